"""Block starts of the VALU Legendre analysis kernels (legendre_dev.hpp, "Block starts"): a wave holds K blocks of 64 ring pairs and every block runs its
accumulation FMAs only from its own start -- the first 4-step test, counted from the wave's start, at which one of its chains or a chain of a more polar block is
live.  The synthesis kernels were built the same way, measured level and keep one loop for all blocks (profiles/README.md, "Block starts"): their count is pinned
to column (b) of the model here, so that a change of either kind shows.

Ring sets: the rings of a CC grid of N_cc pixels per meridian circle, theta_i = 2 pi i / N_cc, as explicit ring plans with nphi = 8 (the Legendre kernels are all
there is; helpers and the port reference of tests/test_leg_wave_blocks.py):
  full    1602 rings (N_cc 3202, 801 pairs): three waves at K = 6, the polar one part padding
  odd     1601 rings (N_cc 3200): the equator ring is unpaired
  ny      lmax + 1 = 801 rings (N_cc 1600, 401 pairs)
  band    the rings of `full` from pair 268 on (theta >= 30 degrees) and their mirror images: a declination cut, no polar wave
lmax 800, spin 0 and spin 2, synthesis and adjoint synthesis (the Legendre analysis).  The analysis K is forced with the plan option "leg_ana_k": 2, 4, 6 for
spin 2, 4 and 8 for spin 0 (K = 12: leg_ana_s0<12> was built with block starts, passed this test at both shapes -- model counts 14152032 | 11389800 and
172872 | 115044 -- and did not clear the measurement bar against K = 8; the instance is out again, and a K without a compiled kernel raises,
tests/test_leg_ana_blocks.py); the synthesis K is the host's: 2 at these
ring counts (k_small_grid), 4 and 3 in the simulator, which switches that rule off.  Simulator twins at lmax 96 on N_cc 1538 (770 rings, 385 pairs: one pair more than a wave of K = 6 holds) and on its band from pair 130 on (spin 2: at this
lmax the spin-0 synthesis of the band has no block that starts late), K forced the same way.

Each case asserts
 (a) the result against the port at the tolerance of tests/test_leg_ana_blocks.py (1e-11), on a mirror-symmetric subset of the rings;
 (b) that the executed FP64 flops of a seeded analysis launch, plan.profile_flops(executed=True), equal 128 x column (c) of tools/leg_live_count.cpp for the shape, as exact
     integers, and lie strictly below column (b), the count with every block started at the wave's start (which is what the synthesis launch must give, exactly).
     plan.profile_flops() itself keeps reporting the wave count, every block from the wave's start, which tests/test_leg_ana_blocks.py and bench.py pin: column (b).
     A term of 2^-140 is invisible in (a); a block that starts late, or a kernel that does not gate at all, shows in (b);
 (c) that the seeded launch (starts read off the seed tail) gives the same flops as the model and, in the ordered mode, bitwise the output of the recording launch.
MODEL holds (b) and (c) per shape and kernel, FMAs per lane, made with
  g++ -O2 -fopenmp -o leg_live_count tools/leg_live_count.cpp
  ./leg_live_count LMAX NCC 1 KANA0 KANAS KSYN0 KSYNS FIRSTPAIR        (the last lines of its output)
with the arguments given next to each entry."""
import numpy as np
import pytest
from pixell_amd import sht
from test_leg_wave_blocks import ring_kw, rel, relrms, port_syn, port_adj, subset, masked_alm, TOL, NPH

GRIDS = {"full": (3202, 0), "odd": (3200, 0), "ny": (1600, 0), "band": (3202, 268), "sim": (1538, 0), "simband": (1538, 130)}

def thetas(ncc, pair0):
	nr = ncc//2+1; th = 2*np.pi*np.arange(nr)/ncc
	return np.concatenate([th[pair0:(nr+1)//2], th[(nr+1)//2:nr-pair0]])      # (an odd count: the equator ring goes with the northern half)

# (grid, lmax, kernel) -> (column (b), column (c)), FMAs per lane of a seeded launch
MODEL = {
	# ./leg_live_count 800 3202 1 4 2 2 2
	("full", 800, "ana_s0<4>"): (11557200, 10524904), ("full", 800, "ana_spin<2>"): (42372696, 40920400),
	("full", 800, "syn_s0<2>"): (10551456, 10189656), ("full", 800, "syn_spin<2>"): (42372696, 40920400),
	# ./leg_live_count 800 3202 1 8 4 2 2
	("full", 800, "ana_s0<8>"): (13691616, 11236224), ("full", 800, "ana_spin<4>"): (46408080, 42265528),
	# ./leg_live_count 800 3202 1 8 6 2 2
	("full", 800, "ana_spin<6>"): (50092704, 43493688),
	# ./leg_live_count 800 3200 1 8 6 2 2
	("odd", 800, "syn_s0<2>"): (10552740, 10191068), ("odd", 800, "ana_s0<8>"): (13693344, 11237784),
	("odd", 800, "syn_spin<2>"): (42378552, 40925808), ("odd", 800, "ana_spin<6>"): (50101056, 43499928),
	# ./leg_live_count 800 1600 1 8 6 2 2
	("ny", 800, "syn_s0<2>"): (5779128, 5443956), ("ny", 800, "ana_s0<8>"): (7718448, 6090244),
	("ny", 800, "syn_spin<2>"): (23206152, 21861568), ("ny", 800, "ana_spin<6>"): (28437120, 23605176),
	# ./leg_live_count 800 3202 1 8 6 2 2 268
	("band", 800, "syn_s0<2>"): (9076236, 8520808), ("band", 800, "ana_s0<8>"): (13691616, 10059220),
	("band", 800, "syn_spin<2>"): (36361992, 34134088), ("band", 800, "ana_spin<6>"): (44783280, 36941136),
	# ./leg_live_count 96 1538 1 4 2 4 3
	("sim", 96, "syn_s0<4>"): (115248, 95836), ("sim", 96, "ana_s0<4>"): (115248, 95836),
	("sim", 96, "syn_spin<3>"): (350712, 345856), ("sim", 96, "ana_spin<2>"): (347808, 344888),
	# ./leg_live_count 96 1538 1 8 4 4 3
	("sim", 96, "ana_s0<8>"): (115248, 95836), ("sim", 96, "ana_spin<4>"): (456000, 379776),
	# ./leg_live_count 96 1538 1 8 6 4 3
	("sim", 96, "ana_spin<6>"): (359424, 348760),
	# ./leg_live_count 96 1538 1 8 6 4 3 130
	("simband", 96, "syn_spin<3>"): (342000, 266000), ("simband", 96, "ana_spin<6>"): (342000, 266000),
}

def case(grid, lmax, spin):
	ncc, pair0 = GRIDS[grid]; th = thetas(ncc, pair0); nr = len(th); nc = 1 if spin == 0 else 2
	sub = subset(nr)
	alm = masked_alm(lmax, spin, 0)
	ref = port_syn(alm, spin, lmax, th[sub])
	pix = np.zeros((nc, nr, NPH)); pix[:, sub] = np.random.default_rng(15+spin).standard_normal((nc, len(sub), NPH))
	ra = port_adj(pix[:, sub], spin, lmax, th[sub])
	return dict(th=th, sub=sub, alm=alm, ref=ref, pix=pix, ra=ra, lmax=lmax, spin=spin, nc=nc, nr=nr, grid=grid)
_cases = {}
def cached(grid, lmax, spin):
	"""computed once per session and left unchanged"""
	if (grid, lmax, spin) not in _cases:
		c = case(grid, lmax, spin)
		for a in (c["ref"], c["ra"], c["th"], c["pix"], c["alm"]): a.setflags(write=False)
		_cases[(grid, lmax, spin)] = c
	return _cases[(grid, lmax, spin)]

def body(grid, lmax, spin, K, ksyn, monkeypatch):
	c = cached(grid, lmax, spin); kw = ring_kw(np.array(c["th"]), lmax)
	monkeypatch.setattr(sht, "_deterministic", True); monkeypatch.setenv("PXS_SEED_MIN_LMAX", "0"); sht.clear_plans()
	try:
		p = sht.ring_plan(kw["theta"], kw["nphi"], kw["phi0"], kw["ringstart"], lmax, lmax, kw["mstart"], 1, 1); p.set_option("leg_ana_k", K)
		syn = lambda: sht.synthesis(alm=np.array(c["alm"]), spin=spin, **kw).reshape(c["nc"], c["nr"], NPH)
		adj = lambda: sht.adjoint_synthesis(map=np.array(c["pix"]).reshape(c["nc"], -1), spin=spin, **kw)
		m0 = syn(); a0 = adj()      # the recording launches
		assert sht.adjoint_synthesis.last_plan is p and p.query("leg_ana_k") == K
		p.profile(True); p.profile_flops()
		m1 = syn(); wsyn = p.profile_flops(reset=False)[0]; fsyn = p.profile_flops(executed=True)[0]
		a1 = adj(); wana = p.profile_flops(reset=False)[1]; fana = p.profile_flops(executed=True)[1]
		p.profile(False)
	finally:
		sht.clear_plans()
	es, ea = rel(m0[:, c["sub"]], c["ref"]), relrms(a0, c["ra"])
	ks = "s0" if spin == 0 else "spin"
	bs, cs = MODEL[(grid, lmax, "syn_%s<%d>" % (ks, ksyn))]; ba, ca = MODEL[(grid, lmax, "ana_%s<%d>" % (ks, K))]
	print("%s lmax %d spin %d: synthesis K %d %.3e, flops %.0f (model %d, ungated %d); adjoint synthesis K %d %.3e, flops %.0f (model %d, ungated %d)" % (
		grid, lmax, spin, ksyn, es, fsyn, 128*cs, 128*bs, K, ea, fana, 128*ca, 128*ba))
	assert cs < bs and ca < ba, "the shape does not tell the gated kernels from the ungated ones"
	assert np.all(np.isfinite(m0)) and es < TOL, "synthesis"
	assert np.all(np.isfinite(a0)) and ea < TOL, "adjoint synthesis"
	assert fsyn == 128*bs, "synthesis (one loop for all blocks): executed flops against the model's column (b)"
	assert fana == 128*ca and fana < 128*ba, "analysis: executed flops against the model"
	assert wsyn == 128*bs and wana == 128*ba, "the wave counts (every block from the wave's start) against the model's column (b)"
	assert np.array_equal(m1, m0), "synthesis: the seeded launch differs from the recording one"
	assert np.array_equal(a1, a0), "ordered adjoint synthesis: the seeded launch differs from the recording one"

GPU_CASES = [("full", 0, 4), ("full", 0, 8), ("full", 2, 2), ("full", 2, 4), ("full", 2, 6),
	("odd", 0, 8), ("odd", 2, 6), ("ny", 0, 8), ("ny", 2, 6), ("band", 0, 8), ("band", 2, 6)]

@pytest.mark.gpu
@pytest.mark.parametrize("grid,spin,K", GPU_CASES)
def test_block_starts_gpu(grid, spin, K, monkeypatch): body(grid, 800, spin, K, 2, monkeypatch)

@pytest.fixture
def sim(monkeypatch):
	monkeypatch.setenv("PXS_K_SMALL_OFF", "1")

SIM_CASES = [("sim", 0, 4), ("sim", 0, 8), ("sim", 2, 2), ("sim", 2, 4), ("sim", 2, 6), ("simband", 2, 6)]

@pytest.mark.hostsim
@pytest.mark.parametrize("grid,spin,K", SIM_CASES)
def test_block_starts_hostsim(sim, grid, spin, K, monkeypatch): body(grid, 96, spin, K, 4 if spin == 0 else 3, monkeypatch)
