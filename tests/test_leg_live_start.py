"""The Legendre kernels leave phase A (recurrence only) when the first chain of a wave is LIVE: at scale 0 and |value| >= LEG_LIVE = 2^-140
(pixell_amd/csrc/legendre_dev.hpp), not at scale 0 alone.  What that drops is below 2^-100 of the input's largest value; what it must not
do is lose a term that counts, leave scaled-up garbage in a pixel whose true value is tiny, start the two directions of a plan at
different steps, or let a seed recorded at one step be used at another.

Grids (spins 0 and 2 on each): 768 x 1536 Fejer-1 at lmax 767 -- the chains of the polar rings start hundreds of powers of two below
scale 0, and k_small_grid gives short waves (K = 2) -- and 513 x 1024 Clenshaw-Curtis at lmax 511 (pole rings, lone equator ring).  One
batched call of 4 maps per grid runs the FP64-MFMA kernels.

Reference: the long-double oracle (oracle/sht_oracle.py), TOL = 1e-11 as in tests/test_sht_parity.py.  The oracle is O(rings lmax^2) in
Python long double (40 s for one spin-2 synthesis on the larger grid), so it is evaluated the way test_sht_parity.check_large_subset does
at large lmax: on a mirror-symmetric SUBSET of the rings -- the 8 rings next to each pole, every 20th ring or so between them, the equator
-- synthesis ring by ring, and the Legendre analysis as the adjoint synthesis of a Gaussian map supported on those rings (the same
leg_ana kernels, all rings of the wave in flight, the sum over the rings restricted by the data).  analysis_2d itself is checked on
the band-limited map of the synthesis test, where the truth is the input alm.  The single-coefficient case adds every ring within 6
degrees of a pole and every third one up to 24 degrees: that is where its map is tiny (below 2^-100 of its maximum from ~20 degrees on).  Every reference is computed once per session and shared."""
import functools
import numpy as np
import pytest
from pixell_amd import sht
from oracle import sht_oracle as so

TOL = 1e-11
GRIDS = {"F1": ("F1", 768, 1536, 767), "CC": ("CC", 513, 1024, 511)}
CASES = [(g, s) for g in GRIDS for s in (0, 2)]
PHI0 = 0.3

def rel(a, b): return np.max(np.abs(a-b))/max(np.max(np.abs(b)), 1e-300)
def relrms(a, b): return np.sqrt(np.mean(np.abs(a-b)**2))/max(np.sqrt(np.mean(np.abs(b)**2)), 1e-300)

def ring_subset(nt, cap_deg=None, theta=None):
	"""mirror-symmetric ring subset: 8 rings next to each pole, ~20 in between, the middle; cap_deg: every ring within a quarter of that angle of a
	pole and every third one up to it too"""
	idx = [np.arange(0, min(8, nt//2)), np.arange(8, nt//2, max(1, nt//40)), [nt//2, (nt-1)//2]]
	if cap_deg is not None:
		d = np.rad2deg(np.minimum(theta, np.pi-theta))
		idx += [np.nonzero(d < cap_deg/4)[0], np.nonzero(d < cap_deg)[0][::3]]
	idx = np.concatenate([np.asarray(i, int) for i in idx])
	return np.unique(np.concatenate([idx, nt-1-idx]))

def ring_kw(theta, nph, lmax, mmax=None):
	mmax = lmax if mmax is None else mmax
	n = len(theta)
	return dict(theta=theta, nphi=np.full(n, nph, np.uint64), phi0=np.full(n, PHI0), ringstart=np.arange(n, dtype=np.uint64)*nph, lmax=lmax, mmax=mmax,
		mstart=so._tri_mstart(lmax, mmax))

def grid_kw(grid, spin):
	geo, nt, nph, lmax = grid
	return dict(spin=spin, lmax=lmax, mstart=so._tri_mstart(lmax, lmax), geometry=geo, phi0=PHI0)

def single_alm(lmax, spin):
	"""one coefficient: l = lmax, m = lmax // 2, value 1 (spin 2: in E)"""
	nc = 1 if spin == 0 else 2
	m0 = lmax//2
	alm = np.zeros((nc, so.nalm(lmax)), complex); alm[0, int(so._tri_mstart(lmax, lmax)[m0])+lmax] = 1.0
	return alm, m0

@functools.lru_cache(maxsize=None)
def gaussian_case(grid, spin):
	"""Gaussian alm and its oracle map on the ring subset; a Gaussian map supported on the subset and its oracle adjoint synthesis"""
	geo, nt, nph, lmax = grid
	nc = 1 if spin == 0 else 2
	th = np.asarray(so.grid_info(geo, nt)["theta"], np.float64); sub = ring_subset(nt)
	alm = so.rand_alm_simple(lmax, nc, 3, spin=(spin,))
	kw = ring_kw(th[sub], nph, lmax)
	ref = so.synthesis(alm=alm, spin=spin, **kw).reshape(nc, len(sub), nph)
	pix = np.zeros((nc, nt, nph)); pix[:, sub] = np.random.default_rng(5+spin).standard_normal((nc, len(sub), nph))
	ra = so.adjoint_synthesis(map=pix[:, sub].reshape(nc, -1), spin=spin, **kw)
	ra[:, :lmax+1] = ra[:, :lmax+1].real
	for a in (ref, ra): a.setflags(write=False)      # (the inputs go through torch.from_numpy, which wants writable arrays; nothing writes to them)
	return dict(sub=sub, alm=alm, ref=ref, pix=pix, ra=ra)

@functools.lru_cache(maxsize=None)
def single_case(grid, spin, cap_deg=24.0):
	"""the single-coefficient alm and its oracle map on the rings within cap_deg of a pole + the ring subset (oracle with mmax = m0: the rest is zero)"""
	geo, nt, nph, lmax = grid
	nc = 1 if spin == 0 else 2
	th = np.asarray(so.grid_info(geo, nt)["theta"], np.float64); sub = ring_subset(nt, cap_deg, th)
	alm, m0 = single_alm(lmax, spin)
	a_or = np.zeros((nc, so.nalm(lmax, m0)), complex); a_or[0, int(so._tri_mstart(lmax, m0)[m0])+lmax] = 1.0
	ref = so.synthesis(alm=a_or, spin=spin, **ring_kw(th[sub], nph, lmax, mmax=m0)).reshape(nc, len(sub), nph)
	# the oracle alone: finite, and the tiny region is there to be checked (2^-100 of the largest value and far below)
	big = np.max(np.abs(ref))
	assert np.all(np.isfinite(ref)) and big > 0
	ringmax = np.max(np.abs(ref), axis=(0, 2))
	assert np.sum(ringmax < 2.0**-100*big) >= 4 and np.min(ringmax) < 2.0**-300*big, "the case does not reach the range the test is about"
	ref.setflags(write=False)
	return dict(sub=sub, alm=alm, ref=ref)

def check_single(out, c):
	"""a map whose values span hundreds of orders of magnitude: right where it is large, and no scaled-up garbage where it is tiny"""
	ref = c["ref"]; got = out[:, c["sub"]]; big = np.max(np.abs(ref))
	assert np.all(np.isfinite(out))
	e = np.max(np.abs(got-ref))/big
	print("single coefficient: max err / max %.3e, rings of the subset below 2^-100: %d" % (e, int(np.sum(np.max(np.abs(ref), axis=(0, 2)) < 2.0**-100*big))))
	assert e < TOL
	tiny = np.abs(ref) < 2.0**-100*big
	assert tiny.any() and np.max(np.abs(got[tiny])) <= 2.0**-90*big, "%.3e of the largest value where the oracle is below 2^-100 of it" % (np.max(np.abs(got[tiny]))/big)

def alm_dot(a, b, lmax):
	"""real inner product in the triangular layout: m = 0 once, m > 0 twice"""
	w = np.full(a.shape[-1], 2.0); w[:lmax+1] = 1.0
	return float(np.sum((a.real*b.real+a.imag*b.imag)*w))

def body_oracle(grid, spin):
	"""synthesis, adjoint synthesis (the Legendre analysis on Gaussian ring data) and analysis_2d against the oracle"""
	geo, nt, nph, lmax = grid; nc = 1 if spin == 0 else 2
	c = gaussian_case(grid, spin); kw = grid_kw(grid, spin)
	out = np.zeros((nc, nt, nph)); sht.synthesis_2d(alm=c["alm"], map=out, **kw)
	e1 = rel(out[:, c["sub"]], c["ref"])
	oa = np.zeros_like(c["alm"]); sht.adjoint_synthesis_2d(alm=oa, map=c["pix"], **kw)
	e2 = relrms(oa, c["ra"])
	back = np.zeros_like(c["alm"]); sht.analysis_2d(alm=back, map=out, **kw)
	e3 = relrms(back, c["alm"])
	print("%s spin %d: synthesis %.3e  adjoint synthesis %.3e  analysis of the band-limited map %.3e" % (geo, spin, e1, e2, e3))
	assert e1 < TOL, "synthesis_2d"
	assert e2 < TOL, "adjoint_synthesis_2d"
	assert np.max(np.abs(oa-c["ra"])) < 1e-8*np.sqrt(np.mean(np.abs(c["ra"])**2))
	assert e3 < TOL, "analysis_2d"

def body_single(grid, spin):
	geo, nt, nph, lmax = grid; nc = 1 if spin == 0 else 2
	c = single_case(grid, spin)
	out = np.zeros((nc, nt, nph)); sht.synthesis_2d(alm=c["alm"], map=out, **grid_kw(grid, spin))
	check_single(out, c)

def body_dot(grid, spin):
	"""<synthesis(a), x> = <a, adjoint_synthesis(x)> and <analysis(x), a> = <x, adjoint_analysis(a)>, |lhs - rhs| <= 1e-13 ||.|| ||.||
	(random x, not band-limited; the measure of tests/test_baseline_configs.check_adjointness).  Both directions run the same recurrences
	from the same start step, so what is left is rounding: ~1e-15 of the product of the norms."""
	geo, nt, nph, lmax = grid; nc = 1 if spin == 0 else 2
	kw = grid_kw(grid, spin); rng = np.random.default_rng(11+spin)
	x = rng.standard_normal((nc, nt, nph))
	a = so.rand_alm_simple(lmax, nc, 17, spin=(spin,))*(np.arange(so.nalm(lmax)) % 7+1.0)
	nrm = lambda t: float(np.sqrt(np.sum(np.abs(t)**2))); an = np.sqrt(alm_dot(a, a, lmax))
	sa = np.zeros_like(x); sht.synthesis_2d(alm=a, map=sa, **kw)
	sx = np.zeros_like(a); sht.adjoint_synthesis_2d(alm=sx, map=x, **kw)
	lhs, rhs = float(np.sum(sa*x)), alm_dot(a, sx, lmax)
	e1 = abs(lhs-rhs)/max(nrm(sa)*nrm(x), an*np.sqrt(alm_dot(sx, sx, lmax)))
	ax = np.zeros_like(a); sht.analysis_2d(alm=ax, map=x, **kw)
	aa = np.zeros_like(x); sht.adjoint_analysis_2d(alm=a, map=aa, **kw)
	lhs2, rhs2 = alm_dot(ax, a, lmax), float(np.sum(x*aa))
	e2 = abs(lhs2-rhs2)/max(np.sqrt(alm_dot(ax, ax, lmax))*an, nrm(x)*nrm(aa))
	print("%s spin %d: synthesis / adjoint %.3e  analysis / adjoint %.3e" % (geo, spin, e1, e2))
	assert e1 < 1e-13 and e2 < 1e-13
	assert abs(lhs) > 1e-7*nrm(sa)*nrm(x) and abs(lhs2) > 1e-7*nrm(x)*nrm(aa), "degenerate inner products"

def body_seeds(grid, spin, monkeypatch):
	"""a plan with recurrence seeds -- first call (records them at the end of phase A) and second call (loads them) -- against a plan
	without: bit for bit in synthesis (Gaussian alm and the single coefficient)"""
	geo, nt, nph, lmax = grid; nc = 1 if spin == 0 else 2
	kw = grid_kw(grid, spin)
	alms = [gaussian_case(grid, spin)["alm"], single_alm(lmax, spin)[0]]
	def run():
		res = []
		for rep in range(2):
			for alm in alms:
				m = np.zeros((nc, nt, nph)); sht.synthesis_2d(alm=alm, map=m, **kw); res.append(m)
		return res
	monkeypatch.setenv("PXS_SEED_MIN_LMAX", "0"); sht.clear_plans()
	try:
		seeded = run()
		monkeypatch.setenv("PXS_SEED_GB", "0"); sht.clear_plans()
		plain = run()
	finally:
		monkeypatch.delenv("PXS_SEED_GB", raising=False); sht.clear_plans()
	for i, m in enumerate(seeded): assert np.array_equal(m, plain[i % 2]), "call %d with seeds differs from the plan without" % i

def body_ordered(grid, spin):
	"""the ordered analysis (per-wave partial moments from each wave's first row on, summed by reduce_partials) against the default
	(atomic adds): equal to rounding, 1e-14 rms as in test_sht_parity.test_deterministic_mode_gpu; and the ordered one against the oracle"""
	geo, nt, nph, lmax = grid
	c = gaussian_case(grid, spin); kw = grid_kw(grid, spin)
	res = []
	try:
		for det in (True, False):
			sht.set_deterministic(det)
			oa = np.zeros_like(c["alm"]); sht.adjoint_synthesis_2d(alm=oa, map=c["pix"], **kw); res.append(oa)
	finally: sht.set_deterministic(None)
	print("%s spin %d: ordered against default %.3e" % (geo, spin, relrms(res[0], res[1])))
	assert relrms(res[0], res[1]) < 1e-14
	assert relrms(res[0], c["ra"]) < TOL

def body_batched(grid, spin):
	"""4 maps in one call: the FP64-MFMA kernels.  Map 0 is the Gaussian case (against the oracle), map 1 the single coefficient (tiny
	pixels stay tiny), all four against the single-map calls to 1e-13 of the largest value (another summation order)"""
	geo, nt, nph, lmax = grid; nc = 1 if spin == 0 else 2
	c = gaussian_case(grid, spin); s = single_case(grid, spin); kw = grid_kw(grid, spin)
	alm = np.stack([c["alm"], s["alm"]]+[so.rand_alm_simple(lmax, nc, 30+i, spin=(spin,)) for i in range(2)])
	out = np.zeros((4, nc, nt, nph)); sht.synthesis_2d(alm=alm, map=out, **kw)
	assert rel(out[0][:, c["sub"]], c["ref"]) < TOL
	check_single(out[1], s)
	for i in (0, 2):
		one = np.zeros((nc, nt, nph)); sht.synthesis_2d(alm=alm[i], map=one, **kw)
		assert np.abs(one-out[i]).max() < 1e-13*np.abs(one).max()
	pix = np.stack([c["pix"]]+[c["pix"][:, ::-1]*(i+2.0) for i in range(3)])
	oa = np.zeros_like(alm); sht.adjoint_synthesis_2d(alm=oa, map=pix, **kw)
	assert relrms(oa[0], c["ra"]) < TOL
	one = np.zeros_like(alm[0]); sht.adjoint_synthesis_2d(alm=one, map=pix[2], **kw)
	assert relrms(oa[2], one) < 1e-13 and np.abs(oa[2]-one).max() < 1e-12*np.abs(one).max()
	back = np.zeros_like(alm); sht.analysis_2d(alm=back, map=out, **kw)
	assert relrms(back, alm) < TOL

@pytest.mark.gpu
@pytest.mark.parametrize("g,spin", CASES)
def test_oracle_gpu(g, spin): body_oracle(GRIDS[g], spin)

@pytest.mark.gpu
@pytest.mark.parametrize("g,spin", CASES)
def test_single_coefficient_gpu(g, spin): body_single(GRIDS[g], spin)

@pytest.mark.gpu
@pytest.mark.parametrize("g,spin", CASES)
def test_dot_products_gpu(g, spin): body_dot(GRIDS[g], spin)

@pytest.mark.gpu
@pytest.mark.parametrize("g,spin", CASES)
def test_seeded_against_unseeded_gpu(g, spin, monkeypatch): body_seeds(GRIDS[g], spin, monkeypatch)

@pytest.mark.gpu
@pytest.mark.parametrize("g,spin", CASES)
def test_ordered_mode_gpu(g, spin): body_ordered(GRIDS[g], spin)

@pytest.mark.gpu
@pytest.mark.parametrize("g,spin", CASES)
def test_batched_mfma_gpu(g, spin): body_batched(GRIDS[g], spin)
