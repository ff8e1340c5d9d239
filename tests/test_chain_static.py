"""The compile-time-planned chain stage kernels (chain_kernel_static, pixell_amd/csrc/chain_static_table.hpp) against the run-time kernel
they replace for the shapes of the table (chain_kernel): same plan, same input, PXS_CHAIN_STATIC switched per call; against the
oracle; and the table against the FFT engine's own plans.

Grids: 1024 x 2048 with lmax 511 (nm = 512 columns: even) and 900 x 1800 with lmax 750 (nm = 751: the last pair holds one column).
Partial tiles (c.nl < T, or unused slots of a tile of pairs) in these plans, from the stage list PXS_CHAIN_VERBOSE=1 prints:
  1024 x 2048: every line count is a multiple of its T but in StSplit<1> (T = 40 = 20 pairs over 256 pairs: the last tile holds 16);
  900 x 1800: StRingA1 T = 48 over 45 lines, StRingS2 T = 48 over 45, StRingA2 T = 56 = 28 pairs over 450 pairs (the last tile holds 2),
    StFirst T = 32 over 25 and 21 lines, StResize T = 56 over 72 (56 + 16), StSigma T = 32 over 48 (32 + 16), StSplit<1> T = 32 = 16
    pairs over 376 pairs (the last tile holds 8), and the odd last column in StFirst / StSplit.
The oracle's values are fixtures (tests/golden/chain_static/: 8192 sampled pixels of its synthesis_2d and 4096 sampled alm of its
analysis_2d of a white-noise map, per grid and spin; the oracle itself takes minutes at these sizes).

The tests print each measured figure before they assert it.  Measured so far: in the host simulator (1 and 64 lanes per workgroup) the two
paths agree bit for bit, 0.0 in every case; on an MI355X alm2map 0.0 in every case, map2alm 4e-17 ... 2.3e-15, against the oracle 1.2e-14 ... 1.4e-13,
the adjoint pairs 0 ... 1.9e-18."""
import os, numpy as np, pytest
from pixell_amd import sht, _lib
from oracle import sht_oracle as so

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chain_static")
GRIDS = [(1024, 2048, 511), (900, 1800, 750)]
# The two paths run the same operations on the same tables: they differ by the compiler's contraction / reassociation only, a few
# ulp (1.1e-16) per point, far below the transform's own error.  Bound: 1e-13, the bound of the other two-path tests
# (tests/test_theta_line.py) and a hundredth of the 1e-11 the oracle tests allow.
PATH_TOL = 1e-13
ORACLE_TOL = 1e-11

def relrms(a, b): return float(np.sqrt(np.mean(np.abs(a - b)**2)/np.mean(np.abs(b)**2)))

def make_plan(nt, nph, lmax):
	ms = sht.tri_mstart(lmax, lmax)
	return sht.grid_plan("F1", nt, nph, 0.0, (False, False), lmax, lmax, ms, 1)

# ---- 1. the table ------------------------------------------------------------------------------------------------------------
# (stages, static) of the plans the table was made for: every shape but the three left out for their registers
COVER = [((1024, 2048, 512), 12, 12), ((1024, 2048, 511), 12, 12), ((900, 1800, 750), 9, 9), ((5400, 10800, 4000), 12, 11),
	((10800, 21600, 6000), 12, 12), ((21600, 43200, 10000), 11, 10)]

def test_table_agrees_with_the_engine():
	"""every compiled entry's radices and digit reversal are those FftContext::sub plans for its lengths (the library checks and
	throws otherwise); runs on the simulator build here and on the device build there"""
	plan = make_plan(24, 48, 16)
	assert plan.query("chain_static_table") >= 60

@pytest.mark.parametrize("grid,nstage,nstatic", COVER)
def test_table_covers_the_planned_shapes(grid, nstage, nstatic):
	"""T of every entry is what tile_lines_for gives its stage in the plan: the lookup is by (stage, na, nb, T), so a stage whose T
	differed would miss.  The counts come from a dry run of the plan's own calls."""
	plan = make_plan(*grid)
	assert (plan.query("chain_stages"), plan.query("chain_static")) == (nstage, nstatic)

def test_off_table_grid_keeps_the_run_time_kernel():
	plan = make_plan(720, 1440, 700)
	assert plan.query("chain_static") < plan.query("chain_stages")

# ---- 2. static against fallback ------------------------------------------------------------------------------------------------
def both_paths(monkeypatch, fn):
	out = {}
	for on in ("1", "0"):
		monkeypatch.setenv("PXS_CHAIN_STATIC", on)
		out[on] = fn()
	monkeypatch.delenv("PXS_CHAIN_STATIC")
	return out["1"], out["0"]

def run_paths(nt, nph, lmax, spin, monkeypatch, dtype=np.float64, flip=(False, False)):
	nc = 1 if spin == 0 else 2
	ms = sht.tri_mstart(lmax, lmax)
	plan = make_plan(nt, nph, lmax)
	assert plan.query("chain_static") == plan.query("chain_stages") > 0
	kw = dict(spin=spin, lmax=lmax, mmax=lmax, geometry="F1", phi0=0.3, mstart=ms, flip=flip)
	alm = so.rand_alm_simple(lmax, nc, 3, spin=(spin,))
	pix = np.random.default_rng(5).standard_normal((nc, nt, nph)).astype(dtype)
	def syn():
		m = np.zeros((nc, nt, nph), dtype); sht.synthesis_2d(alm=alm, map=m, **kw); return m
	def ana():
		a = np.zeros_like(alm); sht.analysis_2d(alm=a, map=pix, **kw); return a
	m1, m0 = both_paths(monkeypatch, syn)
	a1, a0 = both_paths(monkeypatch, ana)
	ds, da = relrms(m1.astype(np.float64), m0.astype(np.float64)), relrms(a1, a0)
	print("chain static vs run-time %dx%d lmax %d spin %d %s flip %s: alm2map %.3e map2alm %.3e" % (nt, nph, lmax, spin, np.dtype(dtype).name, flip, ds, da))
	assert np.abs(m0).max() > 0 and np.abs(a0).max() > 0
	assert ds < PATH_TOL and da < PATH_TOL, (ds, da)
	return m1, a1

CASES = [(0, np.float64, (False, False)), (2, np.float64, (False, False)), (0, np.float64, (True, True)), (0, np.float32, (False, False))]

@pytest.mark.gpu
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("spin,dtype,flip", CASES)
def test_static_against_run_time_gpu(monkeypatch, grid, spin, dtype, flip):
	m, a = run_paths(*grid, spin, monkeypatch, dtype=dtype, flip=flip)
	if dtype == np.float64 and flip == (False, False): check_oracle(*grid, spin, m, a)      # ---- 3. the static path against the oracle

@pytest.mark.hostsim
@pytest.mark.parametrize("spin", [0, 2])
def test_static_against_run_time_hostsim(monkeypatch, spin):
	"""the reference grid with 4 columns (what the simulator can afford): its four ring stages and its five theta stages (StFirst, StResize twice,
	StSigma, StSplit<0>) keep the shapes of the full plan, hence their static kernels"""
	nt, nph, lmax, mmax = 900, 1800, 750, 3
	nc = 1 if spin == 0 else 2
	ms = sht.tri_mstart(lmax, mmax); nalm = int(ms[-1]) + lmax + 1
	plan = sht.grid_plan("F1", nt, nph, 0.3, (False, False), lmax, mmax, ms, 1)
	assert plan.query("chain_static") == plan.query("chain_stages") == 9
	kw = dict(spin=spin, lmax=lmax, mmax=mmax, geometry="F1", phi0=0.3, mstart=ms)
	rng = np.random.default_rng(2)
	alm = rng.standard_normal((nc, nalm)) + 1j*rng.standard_normal((nc, nalm)); alm[:, :lmax + 1] = alm[:, :lmax + 1].real
	pix = rng.standard_normal((nc, nt, nph))
	def syn():
		m = np.zeros((nc, nt, nph)); sht.synthesis_2d(alm=alm, map=m, **kw); return m
	def ana():
		a = np.zeros_like(alm); sht.analysis_2d(alm=a, map=pix, **kw); return a
	m1, m0 = both_paths(monkeypatch, syn)
	a1, a0 = both_paths(monkeypatch, ana)
	assert np.abs(m0).max() > 0 and np.abs(a0).max() > 0
	assert relrms(m1, m0) < PATH_TOL and relrms(a1, a0) < PATH_TOL, (relrms(m1, m0), relrms(a1, a0))

def check_oracle(nt, nph, lmax, spin, m, a):
	"""sampled pixels of synthesis_2d and sampled alm of analysis_2d of a white-noise (not band-limited) map against the oracle's"""
	fx = np.load(os.path.join(GOLDEN, "oracle_%dx%d_l%d_s%d.npz" % (nt, nph, lmax, spin)))
	nc = 1 if spin == 0 else 2
	alm = so.rand_alm_simple(lmax, nc, 3, spin=(spin,)); pix = np.random.default_rng(5).standard_normal((nc, nt, nph))
	assert np.array_equal(alm.reshape(-1)[:8], fx["alm_check"]) and np.array_equal(pix.reshape(-1)[:8], fx["pix_check"]), "the fixture was made from other inputs"
	es = float(np.abs(m.reshape(-1)[fx["ipix"]] - fx["syn"]).max()/fx["syn_max"])
	ea = float(np.sqrt(np.mean(np.abs(a.reshape(-1)[fx["ialm"]] - fx["ana"])**2))/fx["ana_rms"])
	print("chain static vs oracle %dx%d lmax %d spin %d: synthesis %.3e analysis %.3e" % (nt, nph, lmax, spin, es, ea))
	assert es < ORACLE_TOL and ea < ORACLE_TOL, (es, ea)

# ---- 4. the fallback is still taken, and still right ----------------------------------------------------------------------------
@pytest.mark.gpu
def test_off_table_grid_against_the_oracle_gpu():
	nt, nph, lmax = 720, 1440, 700
	plan = make_plan(nt, nph, lmax)
	assert plan.query("chain_static") < plan.query("chain_stages")
	ms = so._tri_mstart(lmax, lmax); mmax = 24      # (the stage shapes do not depend on mmax but for the widths of the last tiles; the oracle's time does)
	kw = dict(spin=0, lmax=lmax, mmax=mmax, mstart=ms[:mmax + 1], geometry="F1", phi0=0.3)
	alm = so.rand_alm_simple(lmax, 1, 3, spin=(0,))
	ref = np.zeros((1, nt, nph)); so.synthesis_2d(alm=alm, map=ref, **kw)
	out = np.zeros((1, nt, nph)); sht.synthesis_2d(alm=alm, map=out, **kw)
	assert np.abs(out - ref).max() < ORACLE_TOL*np.abs(ref).max()

# ---- 4b. all four theta chains: every transform against its adjoint ------------------------------------------------------------------
# run_paths exercises to_cc and from_cc only.  With PXS_THETA_LINE=0 analysis_2d goes through to_cc and adjoint_analysis_2d through
# to_cc_adjoint on both grids.  Synthesis takes the CC grid only where the map has clearly more rings than it (the thresholds of
# setup_resampling in sht.hip): on 1024 x 2048 with lmax 511 (513 CC rings) synthesis_2d goes through from_cc and adjoint_synthesis_2d
# through from_cc_adjoint; on 900 x 1800 with lmax 750 (757 CC rings) both run on the map's rings and only the ring stages are chain
# stages.  The 900 x 1800 plan has partial tiles in every stage kind it launches and an odd last column (see the list at the top).
# The route is asserted from the plan's own stage list: StSplit<0> (stage 3) ends to_cc / from_cc_adjoint, StSplit<1> (stage 4) ends
# from_cc / to_cc_adjoint.
# Tolerance: 1e-11 of the product of the norms, the bound and the normalisation of the adjoint inner-product test check_adjointness
# (tests/test_baseline_configs.py: test_adjointness_*; tests/test_sht_parity.py pins the same transforms to the oracle with the same TOL = 1e-11).
ADJ_TOL = 1e-11
ADJ_GRIDS = [((900, 1800, 750), False), ((1024, 2048, 511), True)]      # (grid, synthesis through the CC grid)

def alm_dot(a, b, lmax):
	"""real inner product of two alm sets, m = 0 (the first lmax + 1 coefficients) once, m > 0 twice"""
	w = np.full(a.shape[-1], 2.0); w[:lmax + 1] = 1.0
	return float(np.sum((a.real*b.real + a.imag*b.imag)*w))

def planned_stage_ids(plan, monkeypatch, capfd):
	"""stage ids of the chain stages of the plan's analysis and synthesis, from the list the plan prints with PXS_CHAIN_VERBOSE=1"""
	monkeypatch.setenv("PXS_CHAIN_VERBOSE", "1"); capfd.readouterr()
	plan.query("chain_stages")
	monkeypatch.delenv("PXS_CHAIN_VERBOSE")
	return {int(l.split("plan stage ")[1].split(":")[0]) for l in capfd.readouterr().err.splitlines() if "plan stage " in l}

def check_adjoint_pairs(monkeypatch, capfd, grid, via_cc, mmax, spin, static):
	nt, nph, lmax = grid
	nc = 1 if spin == 0 else 2
	monkeypatch.setenv("PXS_THETA_LINE", "0"); monkeypatch.setenv("PXS_CHAIN_STATIC", static)
	ms = sht.tri_mstart(lmax, mmax); nalm = int(ms[-1]) + lmax + 1
	sids = planned_stage_ids(sht.grid_plan("F1", nt, nph, 0.3, (False, False), lmax, mmax, ms, 1), monkeypatch, capfd)
	assert 3 in sids and (4 in sids) == via_cc, sids      # to_cc as the stage chain; from_cc where the synthesis goes through the CC grid
	kw = dict(spin=spin, lmax=lmax, mmax=mmax, geometry="F1", phi0=0.3, mstart=ms)
	rng = np.random.default_rng(21 + spin)
	x = rng.standard_normal((nc, nt, nph))      # (not band-limited)
	a = rng.standard_normal((nc, nalm)) + 1j*rng.standard_normal((nc, nalm)); a[:, :lmax + 1] = a[:, :lmax + 1].real
	l_of = np.concatenate([np.arange(m, lmax + 1) for m in range(mmax + 1)]); a[:, l_of < spin] = 0
	nrm = lambda t: float(np.sqrt(np.sum(t*t))); an = np.sqrt(alm_dot(a, a, lmax)); xn = nrm(x)
	ax = np.zeros_like(a); sht.analysis_2d(alm=ax, map=x, **kw)
	aa = np.zeros_like(x); sht.adjoint_analysis_2d(alm=a, map=aa, **kw)
	lhs, rhs = alm_dot(ax, a, lmax), float(np.sum(x*aa)); n1 = max(np.sqrt(alm_dot(ax, ax, lmax))*an, xn*nrm(aa)); e1 = abs(lhs - rhs)/n1
	sa = np.zeros_like(x); sht.synthesis_2d(alm=a, map=sa, **kw)
	sx = np.zeros_like(a); sht.adjoint_synthesis_2d(alm=sx, map=x, **kw)
	lhs2, rhs2 = float(np.sum(sa*x)), alm_dot(a, sx, lmax); n2 = max(nrm(sa)*xn, an*np.sqrt(alm_dot(sx, sx, lmax))); e2 = abs(lhs2 - rhs2)/n2
	print("chain adjoint pairs %dx%d lmax %d mmax %d spin %d static %s: analysis %.3e synthesis %.3e" % (nt, nph, lmax, mmax, spin, static, e1, e2))
	assert abs(lhs) > 1e-7*n1 and abs(lhs2) > 1e-7*n2, "degenerate inner products"
	assert e1 < ADJ_TOL and e2 < ADJ_TOL, (e1, e2)

@pytest.mark.gpu
@pytest.mark.parametrize("static", ["1", "0"])
@pytest.mark.parametrize("spin", [0, 2])
@pytest.mark.parametrize("grid,via_cc", ADJ_GRIDS)
def test_theta_chains_against_their_adjoints_gpu(monkeypatch, capfd, grid, via_cc, spin, static):
	check_adjoint_pairs(monkeypatch, capfd, grid, via_cc, grid[2], spin, static)

@pytest.mark.hostsim
@pytest.mark.parametrize("static", ["1", "0"])
@pytest.mark.parametrize("spin", [0, 2])
@pytest.mark.parametrize("grid,via_cc", ADJ_GRIDS)
def test_theta_chains_against_their_adjoints_hostsim(monkeypatch, capfd, grid, via_cc, spin, static):
	"""the same grids with 4 columns, as test_static_against_run_time_hostsim"""
	check_adjoint_pairs(monkeypatch, capfd, grid, via_cc, 3, spin, static)

# ---- 5. enmap.fft / ifft ---------------------------------------------------------------------------------------------------------
def fft_round_trip(monkeypatch):
	from pixell_amd import fft as pfft
	rng = np.random.default_rng(12); shp = (2, 150, 240)
	a = rng.standard_normal(shp); ref = np.fft.fftn(a, axes=(-2, -1))
	monkeypatch.setenv("PXS_FFT2_FAST_MINPIX", "0")      # (the chain stages at this size too)
	def run():
		f = pfft.fft(a, axes=[-2, -1]); back = pfft.ifft(f, axes=[-2, -1], normalize=True); return f, back
	(f1, b1), (f0, b0) = both_paths(monkeypatch, run)
	rel = lambda x, y: np.max(np.abs(x - y))/np.max(np.abs(y))
	print("fft2 150x240: static vs numpy %.3e, run-time vs numpy %.3e, round trip %.3e" % (rel(f1, ref), rel(f0, ref), rel(b1.real, a)))
	for f, b in ((f1, b1), (f0, b0)): assert rel(f, ref) < 1e-12 and rel(b, a) < 1e-12      # (the tolerance of tests/test_fft_parity.py)

@pytest.mark.gpu
def test_fft2_round_trip_gpu(monkeypatch): fft_round_trip(monkeypatch)
@pytest.mark.hostsim
def test_fft2_round_trip_hostsim(monkeypatch): fft_round_trip(monkeypatch)

# ---- 6. the timing entry of tools/chain_lab.py ------------------------------------------------------------------------------------
def debug_chain_leaves_the_plan_intact():
	"""pxs_debug_chain on the `tiny` shape of tools/chain_lab.py (F1 90 x 180, lmax 60): every stage group runs and reports a time, an
	unknown group is refused, and the cached plan it ran on (it uses the plan's own scratch) transforms bit for bit as before"""
	import ctypes
	nt, nph, lmax = 90, 180, 60
	lib = _lib.load()
	sht.set_deterministic(True)
	try:
		kw = dict(spin=2, lmax=lmax, geometry="F1", phi0=0.3)
		rng = np.random.default_rng(7); n = (lmax + 1)*(lmax + 2)//2
		alm = rng.standard_normal((2, n)) + 1j*rng.standard_normal((2, n)); alm[:, :lmax + 1] = alm[:, :lmax + 1].real
		pix = rng.standard_normal((2, nt, nph))
		def both():
			m = np.zeros((2, nt, nph)); plan = sht.synthesis_2d(alm=alm, map=m, return_plan=True, **kw)
			a = np.zeros_like(alm); assert sht.analysis_2d(alm=a, map=pix, return_plan=True, **kw) is plan
			return m, a, plan
		m0, a0, plan = both()
		assert np.abs(m0).max() > 0 and np.abs(a0).max() > 0
		ms = ctypes.c_double(-1.0)
		for nc, spin in ((1, 0), (2, 2)):
			for kind in range(5):
				ms.value = -1.0
				assert lib.pxs_debug_chain(plan.handle, kind, nc, spin, 1, ctypes.byref(ms)) == 0, (kind, nc, lib.pxs_last_error())
				print("pxs_debug_chain kind %d nc %d: %.3f ms" % (kind, nc, ms.value))
				assert np.isfinite(ms.value) and ms.value >= 0, (kind, nc, ms.value)
		assert lib.pxs_debug_chain(plan.handle, 5, 1, 0, 1, ctypes.byref(ms)) != 0
		m1, a1, plan1 = both()
		assert plan1 is plan
		assert m1.tobytes() == m0.tobytes() and a1.tobytes() == a0.tobytes()
	finally:
		sht.set_deterministic(None)

@pytest.mark.gpu
def test_debug_chain_leaves_the_plan_intact_gpu(): debug_chain_leaves_the_plan_intact()
@pytest.mark.hostsim
def test_debug_chain_leaves_the_plan_intact_hostsim(): debug_chain_leaves_the_plan_intact()
