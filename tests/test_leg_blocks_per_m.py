"""The Legendre kernels give an m an ODD number of blocks (leg_blocks_per_m, pixell_amd/csrc/legendre_dev.hpp): where the ring chunks times the maps of a
launch are an even number, one block more, which returns at once.  That block must compute nothing and displace nothing: every chunk of every m and map is
still there, once, under the wave index its seeds, its partial moments and first[] are keyed on.

Ring sets of 1, 2, 3 and 4 chunks for the kernel's own K (64 K (n - 1) + 5 ring pairs: wave 0 holds the 5 pairs next to the pole), both directions, spin 0
and spin 2; two maps in one launch with an odd and with an even chunk count (2 n blocks are even either way: the extra block is the one behind the LAST
map); mmax < lmax; the seeds (a recording call and the calls that load them agree bit for bit) and the ordered analysis (bit for bit from call to call).
Host simulator: PXS_K_SMALL_OFF=1 reaches the default-K kernels (leg_syn_s0<4>, leg_ana_s0<8>, leg_syn_spin<3>, leg_ana_spin<4>), so the counts are
exactly those.  GPU: the same ring sets under k_small_grid's rules (smaller K up to 1400 pairs), which makes other chunk counts of them, odd and even; the
default-K kernels at even and odd counts above 1400 pairs run in tests/test_leg_wave_blocks.py (1451 pairs: 6, 3, 8 and 6 chunks).

Reference and tolerance: those of tests/test_leg_wave_blocks.py (the C port of the long-double oracle on a mirror-symmetric subset of the rings, 1e-11),
whose cases and checks are used as they are."""
import numpy as np
import pytest
from pixell_amd import sht
from oracle import sht_oracle as so
from test_leg_wave_blocks import case, check_case, body_seeded, ring_kw, rel, relrms, K_OF, TOL, NPH

LMAX = 40
COUNTS = [1, 2, 3, 4]
KERNELS = sorted(K_OF)      # (spin, direction)

def rings_for(spin, what, n): return 2*(64*K_OF[(spin, what)]*(n-1)+5)

@pytest.fixture
def default_k(monkeypatch):
	monkeypatch.setenv("PXS_K_SMALL_OFF", "1"); sht.clear_plans()
	yield
	sht.clear_plans()

def body_counts(spin, what, n): check_case(case("eq", LMAX, rings_for(spin, what, n), spin), what=(what,))

@pytest.mark.hostsim
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("spin,what", KERNELS)
def test_chunk_counts_hostsim(default_k, spin, what, n): body_counts(spin, what, n)

@pytest.mark.gpu
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("spin,what", KERNELS)
def test_chunk_counts_gpu(spin, what, n): body_counts(spin, what, n)

def body_two_maps(spin, n):
	"""two maps in one VALU launch (fewer than 4: no MFMA form; no seeds at this lmax, so the launch is not split): each equals its single-map call bit
	for bit in the synthesis and, with atomic sums, to 1e-14 rms in the adjoint, and the first is the oracle's"""
	c = case("eq", LMAX, rings_for(spin, "syn", n), spin); kw = ring_kw(np.array(c["th"]), LMAX)
	alm2 = np.stack([c["alm"], so.rand_alm_simple(LMAX, c["nc"], 11, spin=(spin,))])
	pix2 = np.stack([c["pix"].reshape(c["nc"], -1), np.random.default_rng(12).standard_normal((c["nc"], c["nr"]*NPH))])
	m2 = sht.synthesis(alm=alm2, spin=spin, map=np.zeros(alm2.shape[:-1]+(c["nr"]*NPH,)), **kw)
	a2 = sht.adjoint_synthesis(map=pix2, spin=spin, alm=np.zeros(pix2.shape[:-1]+(so.nalm(LMAX),), complex), **kw)
	for b in range(2):
		assert np.array_equal(m2[b], sht.synthesis(alm=alm2[b], spin=spin, **kw)), "synthesis, map %d of the batch" % b
		assert relrms(a2[b], sht.adjoint_synthesis(map=pix2[b], spin=spin, **kw)) < 1e-14, "adjoint synthesis, map %d of the batch" % b
	e1, e2 = rel(m2[0].reshape(c["nc"], c["nr"], NPH)[:, c["sub"]], c["ref"]), relrms(a2[0], c["ra"])
	print("spin %d, %d chunks, two maps: synthesis %.3e  adjoint synthesis %.3e" % (spin, n, e1, e2))
	assert e1 < TOL and e2 < TOL

@pytest.mark.hostsim
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("spin", [0, 2])
def test_two_maps_hostsim(default_k, spin, n): body_two_maps(spin, n)

@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("spin", [0, 2])
def test_two_maps_gpu(spin, n): body_two_maps(spin, n)

def body_mmax(spin):
	"""mmax = 25 < lmax = 40 on two chunks: the transform of the alm with nothing above mmax (the triangular layout of the first mmax + 1 columns is a
	prefix of the full one)"""
	c = case("eq", LMAX, rings_for(spin, "syn", 2), spin); th = np.array(c["th"]); mmax = 25
	ms = so._tri_mstart(LMAX, LMAX); n = int(ms[mmax])+LMAX+1
	kw = ring_kw(th, LMAX); kws = dict(kw, mmax=mmax, mstart=ms[:mmax+1])
	alm = c["alm"].copy(); alm[:, n:] = 0
	full, cut = sht.synthesis(alm=alm, spin=spin, **kw), sht.synthesis(alm=np.ascontiguousarray(alm[:, :n]), spin=spin, **kws)
	e1 = rel(cut, full)
	pix = c["pix"].reshape(c["nc"], -1)
	afull, acut = sht.adjoint_synthesis(map=pix, spin=spin, **kw), sht.adjoint_synthesis(map=pix, spin=spin, **kws)
	e2 = relrms(acut[:, :n], afull[:, :n])
	print("spin %d, mmax %d: synthesis %.3e  adjoint synthesis %.3e against the full-mmax call" % (spin, mmax, e1, e2))
	assert acut.shape[-1] == n and e1 < TOL and e2 < TOL

@pytest.mark.hostsim
@pytest.mark.parametrize("spin", [0, 2])
def test_mmax_lt_lmax_hostsim(default_k, spin): body_mmax(spin)

@pytest.mark.gpu
@pytest.mark.parametrize("spin", [0, 2])
def test_mmax_lt_lmax_gpu(spin): body_mmax(spin)

def body_repeats(spin, ordered, monkeypatch):
	"""two chunks (an even count): calls repeated on one plan, so that the first records the seeds and the later ones load them, and a plan without seeds:
	the synthesis bit for bit, the adjoint bit for bit in the ordered mode (tests/test_leg_wave_blocks.py::body_seeded)"""
	body_seeded(spin, ordered, monkeypatch, case("eq", LMAX, rings_for(spin, "syn", 2), spin))

@pytest.mark.hostsim
@pytest.mark.parametrize("ordered", [False, True])
@pytest.mark.parametrize("spin", [0, 2])
def test_seeds_and_ordered_sums_hostsim(default_k, spin, ordered, monkeypatch): body_repeats(spin, ordered, monkeypatch)

@pytest.mark.gpu
@pytest.mark.parametrize("ordered", [False, True])
@pytest.mark.parametrize("spin", [0, 2])
def test_seeds_and_ordered_sums_gpu(spin, ordered, monkeypatch): body_repeats(spin, ordered, monkeypatch)
