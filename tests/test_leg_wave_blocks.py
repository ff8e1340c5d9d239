"""The VALU Legendre kernels deal ring pairs to waves with the padding in wave 0, the polar wave (leg_pair_of, pixell_amd/csrc/legendre_dev.hpp): a wave's
64 K pairs are K blocks of 64 consecutive ones, pole first, and the first wave's leading blocks may hold no pair at all.  What that must not do: lose or
misplace a ring (first wave partly or wholly padding, blocks of padding only), move a wave's polar form or its start step the wrong way, leave scaled-up
garbage in a pixel of a polar block, break the seeds (recorded and loaded under the same map), the ordered analysis (first[]), or the data fetch / sum
reset of a lane that reaches scale 0 long after its wave went live.  (The map itself -- which pair a slot holds, where a wave ends -- is pinned by the
static_asserts next to leg_pair_of.)

Reference: the C port of the long-double oracle (oracle/sht_port.c through oracle/sht_fast.py; pinned to the oracle by tests/test_oracle_port.py),
TOL = 1e-11 as in tests/test_sht_parity.py, evaluated the way test_sht_parity.check_large_subset does: on a mirror-symmetric SUBSET of the rings --
synthesis ring by ring, the Legendre analysis as the adjoint synthesis of a Gaussian map supported on those rings (all rings of the wave in flight).
Every ring set is explicit with nphi = 8, so that the Legendre kernels are all there is.

GPU: lmax + 2 equidistant rings at lmax 2900 = 1451 ring pairs, above k_small_grid's 1400, so the default-K kernels run (leg_syn_s0<4>, leg_ana_s0<8>,
leg_syn_spin<3>, leg_ana_spin<4>); 1451 = 7 192 + 107 = 5 256 + 171 = 2 512 + 427: the first wave is part padding for K = 3, 4 and 8.
Host simulator (PXS_K_SMALL_OFF=1, as test_grid_default_k_hostsim): fewer than 64 pairs (one wave, K - 1 blocks of padding only), 64 K + 5 pairs for
the kernel's K (wave 0 holds 5 pairs), and a ring set crowded towards the poles at lmax 160 whose blocks of 64 pairs go live at different steps.
Both: 768 ring pairs (200 over theta in [0.01, 1.2], 568 over [1.25, pi/2 - 0.005]) under k_small_grid's own rules, the one shape that takes the spin analysis to
K = 3 (the first wave of K = 4 ends at pair 255, not polar-eligible; that of K = 3 at pair 191, eligible), the scalar analysis to K = 4 and both syntheses to
K = 2 between 513 and 1400 pairs: leg_ana_spin<3>, leg_ana_s0<4>, leg_syn_s0<2>, leg_syn_spin<2>.
Every reference is computed once per session and shared."""
import functools
import numpy as np
import pytest
from pixell_amd import sht
from oracle import sht_oracle as so

TOL = 1e-11
NPH = 8
PHI0 = 0.1

def rel(a, b): return np.max(np.abs(a-b))/max(np.max(np.abs(b)), 1e-300)
def relrms(a, b): return np.sqrt(np.mean(np.abs(a-b)**2))/max(np.sqrt(np.mean(np.abs(b)**2)), 1e-300)

def ring_kw(t, lmax):
	n = len(t)
	return dict(theta=t, nphi=np.full(n, NPH, np.uint64), phi0=np.full(n, PHI0), ringstart=np.arange(n, dtype=np.uint64)*NPH, lmax=lmax, mstart=so._tri_mstart(lmax, lmax))

def port_syn(alm, spin, lmax, t):
	"""the port's map [nc, len(t), NPH] on the rings t (ascending, mirror-symmetric)"""
	from oracle import sht_fast as sf
	leg = sf.synth_rings(alm, spin, lmax, t)
	return sf.pixels_on_rings(leg, np.tile(PHI0+2*np.pi*np.arange(NPH)/NPH, (len(t), 1)))

def port_adj(pix, spin, lmax, t):
	"""the port's adjoint synthesis of a map [nc, len(t), NPH] supported on the rings t"""
	from oracle import sht_port
	ms = so._tri_mstart(lmax, lmax)
	L = np.fft.fft(pix, axis=2)[:, :, np.arange(lmax+1) % NPH]*np.exp(-1j*np.arange(lmax+1)*PHI0)[None, None, :]      # sum_x ring e^{-i m phi_x}
	cols = sht_port.leg(spin, lmax, np.arange(lmax+1), t, leg=np.transpose(L, (2, 0, 1)))
	out = np.zeros((pix.shape[0], so.nalm(lmax)), complex)
	for m in range(lmax+1): out[:, int(ms[m])+m:int(ms[m])+lmax+1] = cols[m, :, m:]
	out[:, :lmax+1] = out[:, :lmax+1].real
	return out

def subset(nr, extra=()):
	"""mirror-symmetric ring subset: the 8 rings next to each pole, ~40 in between, the middle, and `extra`"""
	idx = np.concatenate([np.arange(0, min(8, nr//2)), np.arange(8, nr//2, max(1, nr//40)), [nr//2, (nr-1)//2], np.asarray(extra, int)])
	return np.unique(np.concatenate([idx, nr-1-idx]))

def equidistant(nr):
	th = np.arange(nr)*np.pi/(nr-1); th[0] = 1e-4; th[-1] = np.pi-1e-4
	return th

def crowded(npairs, tmin=2e-3):
	"""2 npairs rings, geometrically spaced from tmin to just short of the equator: most of them polar"""
	tn = tmin*((np.pi/2-0.01)/tmin)**(np.arange(npairs)/(npairs-1.0))
	return np.concatenate([tn, (np.pi-tn)[::-1]])

def mid768():
	"""768 ring pairs: 200 over theta in [0.01, 1.2], 568 over [1.25, pi/2 - 0.005], and their mirror images"""
	tn = np.concatenate([np.linspace(0.01, 1.2, 200), np.linspace(1.25, np.pi/2-0.005, 568)])
	return np.concatenate([tn, (np.pi-tn)[::-1]])

def masked_alm(lmax, spin, mmin, seed=6):
	"""Gaussian alm with nothing below m = mmin: its map is tiny on the polar rings"""
	alm = so.rand_alm_simple(lmax, 1 if spin == 0 else 2, seed, spin=(spin,))
	ms = so._tri_mstart(lmax, lmax)
	for m in range(mmin): alm[:, int(ms[m])+m:int(ms[m])+lmax+1] = 0
	return alm

def single_alm(lmax, spin):
	"""one coefficient: l = lmax, m = lmax // 2, value 1 (spin 2: in E)"""
	alm = np.zeros((1 if spin == 0 else 2, so.nalm(lmax)), complex); alm[0, int(so._tri_mstart(lmax, lmax)[lmax//2])+lmax] = 1.0
	return alm

@functools.lru_cache(maxsize=None)
def case(kind, lmax, nr, spin, mmin=0):
	"""ring set, Gaussian alm (nothing below mmin) and its port map on the subset; a Gaussian map supported on the subset and its port adjoint synthesis"""
	nc = 1 if spin == 0 else 2
	th = equidistant(nr) if kind == "eq" else mid768() if kind == "mid" else crowded(nr//2)
	assert len(th) == nr
	sub = subset(nr, extra=np.arange(0, nr//2, 3) if kind == "crowded" else ())
	alm = masked_alm(lmax, spin, mmin)
	ref = port_syn(alm, spin, lmax, th[sub])
	pix = np.zeros((nc, nr, NPH)); pix[:, sub] = np.random.default_rng(5+spin).standard_normal((nc, len(sub), NPH))
	ra = port_adj(pix[:, sub], spin, lmax, th[sub])
	for a in (ref, ra, th): a.setflags(write=False)
	return dict(th=th, sub=sub, alm=alm, ref=ref, pix=pix, ra=ra, lmax=lmax, spin=spin, nc=nc, nr=nr)

def run_syn(c, alm=None):
	return sht.synthesis(alm=c["alm"] if alm is None else alm, spin=c["spin"], **ring_kw(np.array(c["th"]), c["lmax"])).reshape(c["nc"], c["nr"], NPH)
def run_adj(c):
	return sht.adjoint_synthesis(map=c["pix"].reshape(c["nc"], -1), spin=c["spin"], **ring_kw(np.array(c["th"]), c["lmax"]))

def check_case(c, what=("syn", "adj")):
	if "syn" in what:
		out = run_syn(c); e = rel(out[:, c["sub"]], c["ref"])
		print("spin %d, %d rings, lmax %d: synthesis %.3e" % (c["spin"], c["nr"], c["lmax"], e))
		assert np.all(np.isfinite(out)) and e < TOL, "synthesis"
	if "adj" in what:
		oa = run_adj(c); e = relrms(oa, c["ra"])
		print("spin %d, %d rings, lmax %d: adjoint synthesis %.3e" % (c["spin"], c["nr"], c["lmax"], e))
		assert e < TOL, "adjoint synthesis"
		assert np.max(np.abs(oa-c["ra"])) < 1e-8*np.sqrt(np.mean(np.abs(c["ra"])**2))

def check_tiny(out, ref, sub, need):
	"""a map whose values span hundreds of powers of two: right where it is large, no scaled-up garbage where it is tiny.  `need`: the relative size
	below which the reference alone must show at least 4 rings of the subset, or the case does not reach what it is about"""
	big = np.max(np.abs(ref)); ringmax = np.max(np.abs(ref), axis=(0, 2))
	assert np.all(np.isfinite(ref)) and big > 0
	assert np.sum(ringmax < need*big) >= 4, "the case does not reach the range the test is about"
	assert np.all(np.isfinite(out))
	got = out[:, sub]; e = np.max(np.abs(got-ref))/big
	print("max err / max %.3e, rings of the subset below the mark: %d" % (e, int(np.sum(ringmax < need*big))))
	assert e < TOL
	tiny = np.abs(ref) < 2.0**-100*big
	assert tiny.any() and np.max(np.abs(got[tiny])) <= 2.0**-90*big, "%.3e of the largest value where the port is below 2^-100 of it" % (np.max(np.abs(got[tiny]))/big)

# ---- GPU: 1451 ring pairs, the default-K kernels ----
GPU_LMAX = 2900

def body_seeded(spin, ordered, monkeypatch, c=None):
	"""synthesis and adjoint synthesis against the port; the calls repeated on the same plan, so that the first records the seeds and the later ones
	load them (mode 2), and a plan without seeds: as test_sht_parity.check_seeds, bit for bit (the adjoint in the ordered mode; with atomic adds it
	repeats to rounding, 1e-14 rms as test_deterministic_mode_gpu has it)"""
	if c is None: c = case("eq", GPU_LMAX, GPU_LMAX+2, spin)
	def run(): return [(run_syn(c), run_adj(c)) for rep in range(3)]
	monkeypatch.setattr(sht, "_deterministic", ordered); monkeypatch.setenv("PXS_SEED_MIN_LMAX", "0"); sht.clear_plans()
	try:
		res = run()
		monkeypatch.setenv("PXS_SEED_GB", "0"); sht.clear_plans()
		plain = run()
	finally:
		monkeypatch.delenv("PXS_SEED_GB", raising=False); sht.clear_plans()
	e1, e2 = rel(res[0][0][:, c["sub"]], c["ref"]), relrms(res[0][1], c["ra"])
	print("spin %d %s: synthesis %.3e  adjoint synthesis %.3e" % (spin, "ordered" if ordered else "atomic", e1, e2))
	assert e1 < TOL and e2 < TOL
	assert np.max(np.abs(res[0][1]-c["ra"])) < 1e-8*np.sqrt(np.mean(np.abs(c["ra"])**2))
	for m, a in res[1:]+plain:
		assert np.array_equal(m, res[0][0]), "synthesis: a seeded call differs from the recording one or from the plan without seeds"
		if ordered: assert np.array_equal(a, res[0][1]), "ordered adjoint synthesis: the same"
		else: assert relrms(a, res[0][1]) < 1e-14

@pytest.mark.gpu
@pytest.mark.parametrize("spin", [0, 2])
@pytest.mark.parametrize("ordered", [False, True])
def test_padded_first_wave_gpu(spin, ordered, monkeypatch): body_seeded(spin, ordered, monkeypatch)

@functools.lru_cache(maxsize=None)
def single_case(spin):
	"""the single coefficient on the GPU ring set: the port's map on the subset + every third ring within 30 degrees of a pole, where it is below
	2^-100 of its maximum over a wide cap"""
	lmax, nr = GPU_LMAX, GPU_LMAX+2; th = equidistant(nr)
	sub = subset(nr, extra=np.nonzero(th < np.deg2rad(30.0))[0][::3])
	ref = port_syn(single_alm(lmax, spin), spin, lmax, th[sub]); ref.setflags(write=False)
	return sub, ref

@pytest.mark.gpu
@pytest.mark.parametrize("spin", [0, 2])
def test_single_coefficient_gpu(spin):
	c = case("eq", GPU_LMAX, GPU_LMAX+2, spin); sub, ref = single_case(spin)
	check_tiny(run_syn(c, alm=single_alm(GPU_LMAX, spin)), ref, sub, 2.0**-100)

# ---- host simulator: the default-K kernels on small ring sets ----
K_OF = {(0, "syn"): 4, (0, "adj"): 8, (2, "syn"): 3, (2, "adj"): 4}      # K_SYN0, K_ANA0, K_SYNS, K_ANAS (legendre.hip)

@pytest.fixture
def default_k(monkeypatch):
	monkeypatch.setenv("PXS_K_SMALL_OFF", "1"); sht.clear_plans()
	yield
	sht.clear_plans()

@pytest.mark.hostsim
@pytest.mark.parametrize("spin", [0, 2])
def test_one_wave_blocks_of_padding_hostsim(default_k, spin):
	"""30 ring pairs: one wave, its first K - 1 blocks hold no pair at all"""
	check_case(case("eq", 40, 60, spin))

@pytest.mark.hostsim
@pytest.mark.parametrize("spin,what", sorted(K_OF))
def test_five_pairs_in_wave_0_hostsim(default_k, spin, what):
	"""64 K + 5 ring pairs for the kernel's own K: two waves, wave 0 holds the 5 pairs next to the pole (all of them in the subset)"""
	check_case(case("eq", 40, 2*(64*K_OF[(spin, what)]+5), spin), what=(what,))

@pytest.mark.hostsim
@pytest.mark.parametrize("spin", [0, 2])
def test_blocks_go_live_apart_hostsim(default_k, spin):
	"""300 ring pairs crowded towards the poles (theta from 2e-3 on, geometric), lmax 160, nothing below m = 40: sin^m(theta) of the blocks of one
	wave lies hundreds of powers of two apart, so they go live at different steps or never; the port's map alone says that rings below 2^-140 of the
	maximum are there"""
	c = case("crowded", 160, 600, spin, mmin=40)
	check_tiny(run_syn(c), c["ref"], c["sub"], 2.0**-140)
	check_case(c, what=("adj",))

# ---- 768 ring pairs: the mid-grid kernels under k_small_grid's own rules (no PXS_K_SMALL_OFF) ----
def body_mid(spin, ordered, lmax, monkeypatch):
	c = case("mid", lmax, 1536, spin)
	cos2 = np.cos(c["th"][:768])**2
	# K = 4: 3 full waves, wave 0 ends at pair 255, not polar-eligible; K = 3: 4 full waves, wave 0 ends at pair 191, eligible (PXS_POLAR_COS2 = 0.1)
	assert cos2[255] < 0.1 and cos2[191] > 0.1, "the ring set does not take the spin analysis to K = 3"
	monkeypatch.delenv("PXS_K_SMALL_OFF", raising=False); sht.clear_plans()
	body_seeded(spin, ordered, monkeypatch, c)

@pytest.mark.gpu
@pytest.mark.parametrize("spin", [0, 2])
@pytest.mark.parametrize("ordered", [False, True])
def test_mid_grid_kernels_gpu(spin, ordered, monkeypatch): body_mid(spin, ordered, 400, monkeypatch)

@pytest.mark.hostsim
@pytest.mark.parametrize("spin", [0, 2])
@pytest.mark.parametrize("ordered", [False, True])
def test_mid_grid_kernels_hostsim(spin, ordered, monkeypatch): body_mid(spin, ordered, 48, monkeypatch)
