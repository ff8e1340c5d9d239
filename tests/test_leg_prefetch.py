"""Phase C of the spin-0 synthesis reads its step rows with one drain per step pair and the next pair's rows requested right behind it (legendre_dev.hpp, "Row
prefetch"), from the compact tables (a, b) / (a, a + b) that are now built with the plan's tables; the same loop was built for the other three VALU kernels, with
the analysis kernels flushing a full tile at a drain between the two steps of a pair, measured and not kept.  What such a loop must not do, whichever kernel has
it: read a row of the wrong step (the row sets alternate), lose or double a step at the end of an m (0 to 3 steps left after the last full trip), flush a tile at
the wrong row, or hand a transform a table that is still being written.  The cases cover all four kernels, both directions, so that they hold for the loops the
kernels have and for any later attempt.

Legendre-only calls on explicit ring sets with nphi = 8, as tests/test_leg_wave_blocks.py has them, whose cases, reference (the C port of the long-double oracle
on a mirror-symmetric subset of the rings) and tolerance (1e-11, that of tests/test_grid_fuzz.py) are used as they are.
GPU: 3002 equidistant rings = 1501 ring pairs, above k_small_grid's 1400, so the default-K kernels run (leg_syn_s0<4>, leg_ana_s0<8>, leg_syn_spin<3>, leg_ana_spin<4>);
lmax 67 and 200 with mmax = lmax: on this ring set the equatorial waves are live from the first step on, so the steps of an m past phase A are all of them, 1 ... 68
and 1 ... 201 (spin 0: 1 ... 34 and 1 ... 101), every remainder of the trip of four and every position of the 16-step tile among them.  Waves whose most equatorial
ring lies within 71.5 degrees of a pole are polar, the others plain: both forms occur, for every K (asserted).
Host simulator (PXS_K_SMALL_OFF=1): two full waves of the kernel's own K and five pairs more, lmax 67.
One GPU case runs the first transforms of two plans at once on two streams, after both plans' tables have been built."""
import numpy as np
import pytest
from pixell_amd import sht
from oracle import sht_oracle as so
from test_leg_wave_blocks import case, check_case, ring_kw, rel, K_OF, TOL, NPH

NR = 3002
LMAXES = [67, 200]

def forms(nr, K):
	"""(polar waves, plain waves) of an equidistant set of nr rings for K ring pairs per lane: a wave is polar if its most equatorial pair has cos^2 > 0.1"""
	npairs = nr//2; nwave = (npairs+64*K-1)//(64*K); pad = nwave*64*K-npairs
	th = np.arange(nr)*np.pi/(nr-1)
	last = [(w+1)*64*K-1-pad for w in range(nwave)]
	polar = [np.cos(th[p])**2 > 0.1 for p in last]
	return sum(polar), len(polar)-sum(polar)

def test_both_forms_occur():
	for K in sorted(set(K_OF.values())):
		npol, nplain = forms(NR, K)
		assert npol >= 1 and nplain >= 1, (K, npol, nplain)
		npol, nplain = forms(2*(64*K*2+5), K)
		assert npol >= 1 and nplain >= 1, (K, npol, nplain)

@pytest.mark.gpu
@pytest.mark.parametrize("lmax", LMAXES)
@pytest.mark.parametrize("spin", [0, 2])
def test_default_k_kernels_gpu(spin, lmax):
	sht.clear_plans()
	check_case(case("eq", lmax, NR, spin))
	sht.clear_plans()

@pytest.mark.gpu
@pytest.mark.parametrize("spin", [0, 2])
def test_repeats_bitwise_gpu(spin, monkeypatch):
	"""the synthesis of a second call on the plan (seeds loaded where the plan records them) equals the first bit for bit, as does the ordered adjoint"""
	from test_leg_wave_blocks import body_seeded
	body_seeded(spin, True, monkeypatch, case("eq", 200, NR, spin))

@pytest.fixture
def default_k(monkeypatch):
	monkeypatch.setenv("PXS_K_SMALL_OFF", "1"); sht.clear_plans()
	yield
	sht.clear_plans()

@pytest.mark.hostsim
@pytest.mark.parametrize("spin,what", sorted(K_OF))
def test_default_k_kernels_hostsim(default_k, spin, what):
	check_case(case("eq", 67, 2*(64*K_OF[(spin, what)]*2+5), spin), what=(what,))

@pytest.mark.gpu
@pytest.mark.parametrize("spin", [0, 2])
def test_two_plans_two_streams_first_calls_gpu(spin):
	"""two plans (3002 and 3006 rings, lmax 200) with their tables built -- the compact ones, which the spin-0 synthesis reads, among them --, then the first transform
	of each on a stream of its own, neither waiting for the other: each is the port's map"""
	import torch
	sht.clear_plans()
	cs = [case("eq", 200, nr, spin) for nr in (NR, NR+4)]
	kws = [ring_kw(np.array(c["th"]), 200) for c in cs]
	plans = [sht.ring_plan(kw["theta"], kw["nphi"], kw["phi0"], kw["ringstart"], 200, 200, kw["mstart"], 1, 1) for kw in kws]
	for p in plans: p.set_option("build_tables", spin)
	alms = [torch.from_numpy(c["alm"]).cuda() for c in cs]
	outs = [torch.zeros((c["nc"], c["nr"]*NPH), dtype=torch.float64, device="cuda") for c in cs]
	torch.cuda.synchronize()
	for c, kw, alm, out, s in zip(cs, kws, alms, outs, (torch.cuda.Stream(), torch.cuda.Stream())):
		with torch.cuda.stream(s): sht.synthesis(alm=alm, spin=spin, map=out, **kw)
		assert sht.synthesis.last_plan in plans
	torch.cuda.synchronize()
	for c, out in zip(cs, outs):
		e = rel(out.cpu().numpy().reshape(c["nc"], c["nr"], NPH)[:, c["sub"]], c["ref"])
		print("%d rings: synthesis %.3e" % (c["nr"], e))
		assert e < TOL
	sht.clear_plans()
