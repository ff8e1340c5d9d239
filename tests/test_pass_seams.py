"""Split passes against unsplit results at every memory-budget seam.

The library cuts one call into several passes wherever an intermediate would exceed a budget ("Environment switches": the
budgets row).  At the default budgets none of these seams splits below the headline sizes, so here every case runs twice on the same
inputs -- at the default budget and under a budget (or plan option) that forces the split -- and

  1. asserts FROM THE LIBRARY'S REPORT (Plan.passes / sht.fft_passes: counted by the loop that launches, pxs_plan_query "passes_*")
     that the split run took at least 3 passes and that the last one is smaller than the others (assert_split);
  2. compares the two runs: bit for bit wherever the split changes neither the kernel nor the order of a sum; to PATH_TOL = 1e-13 (the
     bound of check_batched and of the other two-path tests) where a pass boundary moves a map between the FP64-MFMA and the
     single-map Legendre kernels, or where the unordered (atomic) Legendre analysis of more than two waves per m is compared;
  3. compares the split run with an independent reference, so that one fault in both runs cannot hide: sht_oracle at TOL = 1e-11
     (tests/test_sht_parity.py) for lmax <= 70, numpy.fft at the 5e-13 of check_lengths for the FFT.

Every case prints the passes the library reported and the measured differences before it asserts.

Where the rule "at least 3 passes, the last one smaller" cannot hold as written, the case says so and asserts what the seam allows:
  - passes of the minimum size (1 map, 1 component, 1 m): every pass has size 1, and there are at least 3 of them;
  - the m ranges of the ordered analysis widen with m (rows per m shrink), so the last one is compared with the one before it;
  - the unfused resamplers never take fewer than 32 lines per pass: the 36 column pairs of F1 78 x 160 go as 32 + 4, two passes (its
    71 columns of the adjoint as 32 + 32 + 7); CC 130 x 300 with lmax 128 (65 pairs: 32 + 32 + 1) is added for the third pass;
  - the ring stage of the analysis takes multiples of T2/2 ring pairs, 52 for rings of 200 pixels on a grid of 97 rings: more than the
    grid has.  The analysis side therefore runs on grids of 260 and 259 rings (T2/2 = 64: 64 + 64 + 2);
  - on CC 130 x 300 with lmax 128 analysis_2d and adjoint_analysis_2d take the unfused route, one map per pass at any budget: the
    equal-passes rule is asserted there for synthesis_2d and adjoint_synthesis_2d, and for all four directions on F1 96 x 200;
  - 6 components in chunks of 4 are 4 + 2, two passes (the chunks of 1 are six);
  - 7 lines of 16384 points under 1 MB are 4 + 3 lines, two passes: the case runs under 0.5 MB as well (2 + 2 + 2 + 1).
No synthesis on rings longer than the LDS line is run: rings whose length the fused ring chain can split (16384 = 128 x 128) never
reach the four-step engine, and a ring length that does was not looked for; seam 6 is covered through pixell_amd.fft alone."""
import re, sys, numpy as np, pytest
from pixell_amd import sht, _lib, fft as pfft
from oracle import sht_oracle as so

ORACLE_TOL = 1e-11      # TOL of tests/test_sht_parity.py
F32_TOL = 1e-6          # ... of its float32 case (check_flips_f32)
PATH_TOL = 1e-13        # check_batched, PATH_TOL of tests/test_chain_static.py
FFT_TOL = 5e-13         # check_lengths of tests/test_fft_parity.py
GB, MB = float(1 << 30), float(1 << 20)

OPS = ("synthesis_2d", "analysis_2d", "adjoint_synthesis_2d", "adjoint_analysis_2d")
TO_MAP = ("synthesis_2d", "adjoint_analysis_2d")      # alm -> map: the Legendre synthesis; the other two run the Legendre analysis

def rel(a, b): return float(np.max(np.abs(a - b))/max(np.max(np.abs(b)), 1e-300))
def relrms(a, b): return float(np.sqrt(np.mean(np.abs(a - b)**2))/max(np.sqrt(np.mean(np.abs(b)**2)), 1e-300))
def diff(op, a, b): return rel(a.astype(np.float64), b.astype(np.float64)) if op in TO_MAP else relrms(a.astype(np.complex128), b.astype(np.complex128))

# ---- inputs and references: made once per shape, shared, never written to -------------------------------------------------------------
_inputs, _oracle = {}, {}
def inputs(geometry, nt, nph, lmax, spin, nb, f32=False):
	"""alm [nb, nc, nalm] and a white-noise (not band-limited) map [nb, nc, nt, nph]"""
	key = (geometry, nt, nph, lmax, spin, nb, f32)
	if key not in _inputs:
		nc = 1 if spin == 0 else 2
		alm = np.stack([so.rand_alm_simple(lmax, nc, 60 + i, spin=(spin,)) for i in range(nb)])
		pix = np.random.default_rng(61 + spin).standard_normal((nb, nc, nt, nph))
		if f32: alm, pix = alm.astype(np.complex64), pix.astype(np.float32)
		_inputs[key] = (alm, pix)
	return _inputs[key]

def call_kw(geometry, lmax, spin, mmax=None, flip=None):
	mmax = lmax if mmax is None else mmax
	kw = dict(spin=spin, lmax=lmax, mmax=mmax, mstart=so._tri_mstart(lmax, lmax)[:mmax + 1], geometry=geometry, phi0=0.3)
	if flip: kw["flip"] = flip
	return kw

def run(op, alm, pix, kw, **extra):
	"""one transform -> (result, plan)"""
	if op == "synthesis_2d": out = np.zeros_like(pix); plan = sht.synthesis_2d(alm=alm, map=out, return_plan=True, **kw)
	elif op == "adjoint_analysis_2d": out = np.zeros_like(pix); plan = sht.adjoint_analysis_2d(alm=alm, map=out, return_plan=True, **kw, **extra)
	elif op == "analysis_2d": out = np.zeros_like(alm); plan = sht.analysis_2d(alm=out, map=pix, return_plan=True, **kw, **extra)
	else: out = np.zeros_like(alm); plan = sht.adjoint_synthesis_2d(alm=out, map=pix, return_plan=True, **kw)
	return out, plan

def oracle_form(kw, nt, nph, analysis):
	"""keywords that make the oracle's analysis restate the form the plan takes (oracle_form of tests/test_sht_parity.py)"""
	f = sht.analysis_form(kw["geometry"], nt, nph, kw["lmax"], analysis=analysis, mmax=kw["mmax"], mstart=kw["mstart"], phi0=kw["phi0"])
	return {"ducc0": dict(fine_cc=f["ncc_circle"]), "weights": dict(weights=True), "interpolant": dict(fine_cc=False)}[f["form"]]

def check_oracle(op, key, alm1, pix1, out1, kw, analysis=None, tol=ORACLE_TOL):
	"""one map of a result against the oracle's (computed once per key).  flip: the oracle works on the flipped map."""
	kw = dict(kw); flip = kw.pop("flip", None)
	fl = (lambda m: np.ascontiguousarray(m[..., ::-1, ::-1])) if flip == (True, True) else (lambda m: m)
	nt, nph = pix1.shape[-2:]
	if (op, key) not in _oracle:
		okw = oracle_form(kw, nt, nph, analysis) if "analysis" in op else {}
		a64, p64 = alm1.astype(np.complex128), fl(pix1.astype(np.float64))
		if op in TO_MAP:
			ref = np.zeros_like(p64); getattr(so, op)(alm=a64, map=ref, **kw, **okw)
		else:
			ref = np.zeros_like(a64); getattr(so, op)(alm=ref, map=p64, **kw, **okw)
			if op == "adjoint_synthesis_2d": ref[:, :kw["lmax"] + 1] = ref[:, :kw["lmax"] + 1].real      # (as check_grid)
		_oracle[(op, key)] = ref
	ref = _oracle[(op, key)]
	d = diff(op, fl(out1) if op in TO_MAP else out1, ref)
	print("    %s against the oracle: %.3e" % (op, d))
	assert d < tol, (op, key, d)

# ---- the two runs -------------------------------------------------------------------------------------------------------------------
def twice(monkeypatch, env, call, fixed=()):
	"""call(split) at the default budgets, then under env (strings); fixed: switches that hold in both runs.  Plans are dropped before,
	between and after, so that each run makes its plans under its own environment."""
	for k, v in dict(fixed).items(): monkeypatch.setenv(k, v)
	sht.clear_plans()
	try:
		whole = call(False)
		sht.clear_plans()
		for k, v in env.items(): monkeypatch.setenv(k, v)
		split = call(True)
	finally:
		for k in list(env) + list(dict(fixed)): monkeypatch.delenv(k, raising=False)
		sht.clear_plans()
	return whole, split

def assert_split(p, label, npass=3, widening=False):
	"""p: a pass report of the split run.  At least npass passes, the last one smaller than the others (widening: than the one before
	it); passes of the minimum size 1 cannot be partial: then every pass has size 1."""
	print("  %s: %d passes, first %d, before the last %d, last %d" % (label, p["n"], p["first"], p["prev"], p["last"]))
	assert p["n"] >= npass, (label, p)
	if p["first"] == 1 and not widening: assert p["prev"] == 1 and p["last"] == 1, (label, p)
	else: assert p["last"] < p["prev"] and (widening or p["last"] < p["first"]), (label, p)

def assert_whole(p, label):
	print("  %s at the default budget: %d passes, last %d" % (label, p["n"], p["last"]))
	assert p["n"] == 1, (label, p)

def compare(op, whole, split, bits, label, why=""):
	d = diff(op, split, whole)
	print("  %s split against whole: %.3e (%s)" % (label, d, "bit for bit" if bits else "to 1e-13: " + why))
	assert np.abs(whole).max() > 0
	if bits: assert np.array_equal(split, whole), (label, d)
	else: assert d < PATH_TOL, (label, d)

def read_err(capfd):
	"""what the library wrote to stderr since the last look; what the test printed so far stays in the captured output"""
	o = capfd.readouterr(); sys.stdout.write(o.out)
	return o.err

def legendre_forms(capfd):
	"""the Legendre kernel that served each map of the call just made, from the launch lists PXS_CHAIN_VERBOSE prints (print_batch_plan),
	in the order of the maps: the lists of the passes of a batched call follow each other"""
	forms = []
	for l in read_err(capfd).splitlines():
		if l.startswith("[pxsht] legendre ") and " maps:" in l:
			for form, b0, b1 in re.findall(r"(VALU|mm8|mm4) \[(\d+),(\d+)\)", l.split(" maps:")[1]): forms += [form]*(int(b1) - int(b0))
	return forms

# ---- 1. maps per pass of a batched call (PXS_BATCH_GB; batch_chunk / run_call) ------------------------------------------------------------
def per_map_bytes(plan, nt, nph, mmax, nc):
	"""scratch of one map of a pass, as batch_chunk counts it: leg + leg on the CC grid (twice) and h"""
	Ncc = plan.query("ncc_circle"); ncc = Ncc//2 + 1 if Ncc > 0 else 0
	return 16*nc*((mmax + 1)*(nt + ncc)*2 + nt*nph)

def check_batch(monkeypatch, capfd, geometry, nt, nph, lmax, spin, nb, per_pass, want, ops=OPS, oracle_maps=()):
	"""nb maps under a budget for per_pass (a real number: between two whole counts) maps per pass; want: the sizes (first, before the last, last)"""
	nc = 1 if spin == 0 else 2
	alm, pix = inputs(geometry, nt, nph, lmax, spin, nb); kw = call_kw(geometry, lmax, spin)
	budget = per_pass*per_map_bytes(sht.grid_plan(geometry, nt, nph, kw["phi0"], (False, False), lmax, lmax, kw["mstart"], 1), nt, nph, lmax, nc)
	for op in ops:
		print("batch passes %s %dx%d lmax %d spin %d, %d maps, %s:" % (geometry, nt, nph, lmax, spin, nb, op))
		def call(split):
			read_err(capfd)
			out, plan = run(op, alm, pix, kw)
			return out, plan.passes("batch"), legendre_forms(capfd)
		(whole, pw, fw), (split, ps, fs) = twice(monkeypatch, {"PXS_BATCH_GB": repr(budget/GB)}, call, fixed={"PXS_CHAIN_VERBOSE": "1"})
		assert_whole(pw, "maps per pass"); assert_split(ps, "maps per pass")
		assert (ps["first"], ps["prev"], ps["last"]) == want, ps
		assert len(fw) == len(fs) == nb, (fw, fs)
		# bit for bit where every map keeps its Legendre kernel and that kernel sums in a fixed order (the Legendre synthesis); to 1e-13
		# where a pass boundary moves maps between the FP64-MFMA and the single-map kernels, or the unordered Legendre analysis ran
		same = fw == fs; ordered = op in TO_MAP
		compare(op, whole, split, same and ordered, op, "maps change their Legendre kernel %s -> %s" % (sorted(set(fw)), sorted(set(fs))) if not same else "the unordered Legendre analysis")
		for i in oracle_maps: check_oracle(op, (geometry, nt, nph, lmax, spin, nb, i), alm[i], pix[i], split[i], kw)

@pytest.mark.hostsim
def test_batch_passes_hostsim(monkeypatch, capfd):
	check_batch(monkeypatch, capfd, "F1", 24, 48, 20, 2, 5, 2.5, (2, 2, 1), oracle_maps=(0, 4))

@pytest.mark.gpu
def test_batch_equal_passes_gpu(monkeypatch, capfd):
	"""(a) the equal-passes rule: 5 spin-2 maps in passes of 2 + 2 + 1.  F1 96 x 200 lmax 30: all four directions, against the oracle.
	CC 130 x 300 lmax 128: the two directions that batch there (see the module docstring); check_batched(5, "CC", 130, 300, 128) of
	test_batched_gpu pins the unsplit run of this shape to the oracle"""
	check_batch(monkeypatch, capfd, "F1", 96, 200, 30, 2, 5, 2.5, (2, 2, 1), oracle_maps=(0, 4))
	check_batch(monkeypatch, capfd, "CC", 130, 300, 128, 2, 5, 2.5, (2, 2, 1), ops=("synthesis_2d", "adjoint_synthesis_2d"))

@pytest.mark.gpu
def test_batch_unbatched_route_gpu(monkeypatch):
	"""... and the two directions that take the unfused route there go one map per pass with or without the budget: bit for bit"""
	alm, pix = inputs("CC", 130, 300, 128, 2, 5); kw = call_kw("CC", 128, 2)
	for op in ("analysis_2d", "adjoint_analysis_2d"):
		def call(split):
			out, plan = run(op, alm, pix, kw); return out, plan.passes("batch")
		(whole, pw), (split, ps) = twice(monkeypatch, {"PXS_BATCH_GB": repr(1e-3)}, call)
		print("batch passes CC 130x300 lmax 128, %s: %s / %s" % (op, pw, ps))
		assert pw == ps == dict(n=5, first=1, prev=1, last=1)
		assert np.array_equal(whole, split)

@pytest.mark.gpu
def test_batch_eight_groups_gpu(monkeypatch, capfd):
	"""(b) the 8-group rule of scalar maps: 19 spin-0 maps under a budget for 12 go as 8 + 8 + 3"""
	check_batch(monkeypatch, capfd, "F1", 96, 200, 30, 0, 19, 12.5, (8, 8, 3), oracle_maps=(18,))
	check_batch(monkeypatch, capfd, "CC", 130, 300, 128, 0, 19, 12.5, (8, 8, 3), ops=("synthesis_2d", "adjoint_synthesis_2d"))

@pytest.mark.gpu
def test_batch_strided_gpu(monkeypatch):
	"""(c) a strided batch: the Q/U group of a [4, 3, ny, nx] stack of T/Q/U maps through curvedsky.alm2map / map2alm, as
	test_batched_gpu builds it, in passes of 1 map.  4 spin-2 maps take the 4-map MFMA kernel in one pass and the single-map kernel
	in passes of 1: to 1e-13.  Against the oracle (lmax 64) as smoke() does."""
	import torch
	from pixell_amd import curvedsky, enmap
	lmax = 64; shape, wcs = enmap.fullsky_geometry(shape=(70, 140))
	alm_h = np.stack([so.rand_alm_simple(lmax, 3, 40 + i, spin=(0, 2)) for i in range(4)]); alm = torch.from_numpy(alm_h).cuda()
	def call(split):
		m = enmap.dmap(torch.zeros((4, 3) + tuple(shape), dtype=torch.float64, device="cuda"), wcs)
		curvedsky.alm2map(alm, m, spin=[0, 2])
		plan = list(sht._plans.d.values())[-1]; p1 = plan.passes("batch")      # (the Q/U group is the last call on the grid's plan)
		back = torch.zeros_like(alm); curvedsky.map2alm(m, alm=back, spin=[0, 2])
		return m.tensor.cpu().numpy(), back.cpu().numpy(), p1, plan.passes("batch")
	(m0, b0, _, _), (m1, b1, p1, p2) = twice(monkeypatch, {"PXS_BATCH_GB": repr(1e-6)}, call)
	print("strided batch 70x140 lmax 64:")
	assert_split(p1, "maps per pass, alm2map"); assert_split(p2, "maps per pass, map2alm")
	assert p1["n"] == p2["n"] == 4
	compare("synthesis_2d", m0, m1, False, "alm2map", "the 4-map MFMA kernel against the single-map kernel")
	compare("analysis_2d", b0, b1, False, "map2alm", "the 4-map MFMA kernel against the single-map kernel")
	mi = curvedsky.analyse_geometry(m1.shape[1:], wcs); ms = so._tri_mstart(lmax, lmax)
	for i in (0, 3):
		ref = np.zeros((3,) + tuple(shape))
		so.synthesis_2d(alm=alm_h[i, :1], map=ref[:1], spin=0, lmax=lmax, mstart=ms, geometry="F1", phi0=mi.phi0)
		so.synthesis_2d(alm=alm_h[i, 1:], map=ref[1:], spin=2, lmax=lmax, mstart=ms, geometry="F1", phi0=mi.phi0)
		d = rel(m1[i], ref[:, ::-1, ::-1]); e = float(np.abs(b1[i] - alm_h[i]).max())      # (the round trip as test_batched_gpu bounds it)
		print("    map %d against the oracle: alm2map %.3e, round trip %.3e" % (i, d, e))
		assert d < ORACLE_TOL and e < ORACLE_TOL

# ---- 2. m ranges of the ordered analysis (PXS_PART_GB; the cuts of leg_analysis_valu, reduce_partials) -------------------------------------
def total_rows(lmax, mmax, spin): return sum((lmax - m)//2 + 1 if spin == 0 else max(0, lmax - max(m, spin) + 1) for m in range(mmax + 1))

def check_m_ranges(monkeypatch, geometry, nt, nph, lmax, spin, nwave, share, mmax=None, oracle=False):
	"""share: the budget holds 1/share of the partial moments of all m (32 bytes per row and wave), None: PXS_PART_GB=0, one m per pass.
	Bit for bit: the ordered sums take every wave's partial moments in wave order, whatever the range an m falls in."""
	mm = lmax if mmax is None else mmax
	(alm, pix), kw = inputs(geometry, nt, nph, lmax, spin, 1), call_kw(geometry, lmax, spin, mmax)
	budget = 0.0 if share is None else total_rows(lmax, mm, spin)*32*nwave/share
	sht.set_deterministic(True)
	try:
		for op in ("analysis_2d", "adjoint_synthesis_2d"):
			print("ordered analysis %s %dx%d lmax %d mmax %d spin %d, budget %d bytes, %s:" % (geometry, nt, nph, lmax, mm, spin, budget, op))
			def call(split):
				out, plan = run(op, alm[0], pix[0], kw); return out, plan.passes("leg_m")
			(whole, pw), (split, ps) = twice(monkeypatch, {"PXS_PART_GB": repr(budget/GB)}, call)
			assert_whole(pw, "m per range")
			if share is None:
				assert_split(ps, "m per range"); assert ps["n"] == mm + 1, ps
			else:
				assert_split(ps, "m per range", widening=True); assert 3 <= ps["n"] <= 6, ps
			compare(op, whole, split, True, op)
			if oracle: check_oracle(op, (geometry, nt, nph, lmax, mm, spin), alm[0], pix[0], split, kw)
	finally:
		sht.set_deterministic(None)

@pytest.mark.hostsim
@pytest.mark.parametrize("spin", [0, 2])
def test_m_ranges_hostsim(monkeypatch, spin):
	check_m_ranges(monkeypatch, "F1", 20, 41, 19, spin, 1, None, oracle=True)
	check_m_ranges(monkeypatch, "F1", 20, 41, 19, spin, 1, 2.2, oracle=True)      # 20 m in ranges of 5 + 8 + 7

# F1 260 x 512 lmax 250 and CC 300 x 520 lmax 255: 130 and 150 ring pairs, two waves per m.  test_grid_gpu of tests/test_sht_parity.py
# pins the unsplit run of ("F1", 260, 512, 250, 0) and of ("CC", 300, 520, 255, 2) to the oracle; the oracle is not run again here.
@pytest.mark.gpu
@pytest.mark.parametrize("spin", [0, 2])
@pytest.mark.parametrize("geometry,nt,nph,lmax", [("F1", 260, 512, 250), ("CC", 300, 520, 255)])
def test_m_ranges_gpu(monkeypatch, geometry, nt, nph, lmax, spin):
	check_m_ranges(monkeypatch, geometry, nt, nph, lmax, spin, 2, 4.0)                # five ranges, e.g. 33 + 39 + 51 + 101 + 27 m
	check_m_ranges(monkeypatch, geometry, nt, nph, lmax, spin, 2, None)               # one m per pass
	check_m_ranges(monkeypatch, geometry, nt, nph, lmax, spin, 2, 4.5, mmax=100)      # mmax < lmax: 18 + 20 + 22 + 25 + 16 m

# ---- 3. components per pass of a theta chain (PXS_CHAIN_SCRATCH_GB; theta_comp_chunk / theta_chunks) ------------------------------------------
# F1 96 x 200 with lmax 30: the map's circle has 192 points, the chains work on 16 column pairs of at most 256 points: 64 KiB per
# component in s1_ and in s2_, in each of the four chains
THETA_COMP_BYTES = 16*16*256
THETA_STAGE = {"analysis_2d": 3, "adjoint_synthesis_2d": 3, "synthesis_2d": 4, "adjoint_analysis_2d": 4}      # StSplit<0> ends to_cc / from_cc_adjoint, StSplit<1> from_cc / to_cc_adjoint

def check_theta_passes(monkeypatch, capfd, chunk):
	"""3 spin-2 maps (6 components) on F1 96 x 200 lmax 30, `chunk` components per pass: synthesis and its adjoint go through the CC grid
	(from_cc, from_cc_adjoint), analysis and its adjoint take the chain (to_cc, to_cc_adjoint); the line engine is off.  Bit for bit:
	every component goes through the same stages with the same tiles, and 48 ring pairs are one wave per m in the Legendre analysis."""
	geometry, nt, nph, lmax, spin, nb = "F1", 96, 200, 30, 2, 3
	alm, pix = inputs(geometry, nt, nph, lmax, spin, nb); kw = call_kw(geometry, lmax, spin)
	budget = 0.0 if chunk == 1 else (chunk + 0.5)*THETA_COMP_BYTES
	for op in OPS:
		print("theta passes F1 96x200 lmax 30 spin 2, 3 maps, %d components per pass, %s:" % (chunk, op))
		def call(split):
			read_err(capfd)
			out, plan = run(op, alm, pix, kw)
			route = [l for l in read_err(capfd).splitlines() if " route " in l]
			return out, plan.passes("theta"), plan.passes("batch"), route
		(whole, pw, bw, rw), (split, ps, bs, rs) = twice(monkeypatch, {"PXS_CHAIN_SCRATCH_GB": repr(budget/GB)}, call, fixed={"PXS_THETA_LINE": "0", "PXS_CHAIN_VERBOSE": "1"})
		print("  " + rs[0])
		assert rw == rs and len(rs) == 1 and ("route chain" in rs[0] if "analysis" in op else "route via-cc" in rs[0]), rs
		assert bw["n"] == bs["n"] == 1      # (one batch pass: the 6 components come to the theta chain together)
		assert_whole(pw, "components per pass"); assert pw["last"] == 6
		assert_split(ps, "components per pass", npass=6 if chunk == 1 else 2)
		if chunk != 1: assert (ps["n"], ps["first"], ps["last"]) == (2, 4, 2), ps      # 4 + 2: the issue's second chunking; two passes are all 6 components allow
		compare(op, whole, split, True, op)
		for i in (0, 2): check_oracle(op, (geometry, nt, nph, lmax, spin, nb, i), alm[i], pix[i], split[i], kw)

@pytest.mark.hostsim
@pytest.mark.parametrize("chunk", [1, 4])
def test_theta_passes_hostsim(monkeypatch, capfd, chunk): check_theta_passes(monkeypatch, capfd, chunk)
@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [1, 4])
def test_theta_passes_gpu(monkeypatch, capfd, chunk): check_theta_passes(monkeypatch, capfd, chunk)

def scratch_budget_per_plan(monkeypatch):
	"""the fractional parser and the per-call reading together: two plans made in one process under different PXS_CHAIN_SCRATCH_GB
	report different pass counts for the same call"""
	alm, pix = inputs("F1", 96, 200, 30, 2, 3); got = {}
	monkeypatch.setenv("PXS_THETA_LINE", "0")
	for gb in (4.5*THETA_COMP_BYTES/GB, 2.5*THETA_COMP_BYTES/GB, 12):
		monkeypatch.setenv("PXS_CHAIN_SCRATCH_GB", repr(gb))
		plan = sht.grid_plan("F1", 96, 200, 0.1*len(got), (False, False), 30, 30, sht.tri_mstart(30), 1)      # (another phi0: another plan)
		out = np.zeros_like(alm); sht.analysis_2d(alm=out, map=pix, spin=2, lmax=30, geometry="F1", phi0=0.1*len(got))
		got[gb] = plan.passes("theta")
	monkeypatch.delenv("PXS_CHAIN_SCRATCH_GB"); monkeypatch.delenv("PXS_THETA_LINE"); sht.clear_plans()
	print("theta passes under three budgets in one process:", got)
	assert [(p["n"], p["first"], p["last"]) for p in got.values()] == [(2, 4, 2), (3, 2, 2), (1, 6, 6)]

@pytest.mark.hostsim
def test_scratch_budget_per_plan_hostsim(monkeypatch): scratch_budget_per_plan(monkeypatch)
@pytest.mark.gpu
def test_scratch_budget_per_plan_gpu(monkeypatch): scratch_budget_per_plan(monkeypatch)

# ---- 4. ring pairs per pass of the ring FFT stages (PXS_RING_CHUNK_MB; ring_chunk in map2leg / h2map) ------------------------------------------
# rings of 200 pixels: the synthesis side splits them 20 x 10 (rows padded to 16 points), the analysis side 10 x 20 (24 points)
RING_BYTES_SYN, RING_BYTES_ANA = 16*20*16, 16*10*24
# synthesis side (h2map): 8 pairs per pass.  CC 97 x 200: 49 ring pairs, the last one a single ring, 6 x 8 + 1.  F1 96 x 200: 48 pairs -- a
# whole number of passes of 8, so 7 pairs per pass there: 6 x 7 + 6.
# analysis side (map2leg): passes of a multiple of T2/2 = 64 pairs on these grids: 130 pairs as 64 + 64 + 2, the last pair of CC 259 x 200 a single ring
RING_CASES = [("CC", 97, 200, 30, 2, TO_MAP, 8.5), ("F1", 96, 200, 30, 0, TO_MAP, 7.5),
	("CC", 259, 200, 30, 2, ("analysis_2d", "adjoint_synthesis_2d"), 8.5), ("F1", 260, 200, 30, 0, ("analysis_2d", "adjoint_synthesis_2d"), 8.5)]

def check_ring_passes(monkeypatch, geometry, nt, nph, lmax, spin, ops, pairs, f32=False, flip=None):
	"""Bit for bit: a ring pair goes through the same two stages whatever pass it is in; the Legendre analysis of these grids has one
	or two waves per m, and two atomic additions commute."""
	nc = 1 if spin == 0 else 2
	(alm, pix), kw = inputs(geometry, nt, nph, lmax, spin, 1, f32), call_kw(geometry, lmax, spin, flip=flip)
	for op in ops:
		print("ring passes %s %dx%d lmax %d spin %d %s flip %s, %s:" % (geometry, nt, nph, lmax, spin, "float32" if f32 else "float64", flip, op))
		budget = pairs*nc*(RING_BYTES_SYN if op in TO_MAP else RING_BYTES_ANA)
		def call(split):
			out, plan = run(op, alm[0], pix[0], kw); return out, plan.passes("ring")
		(whole, pw), (split, ps) = twice(monkeypatch, {"PXS_RING_CHUNK_MB": repr(budget/MB)}, call, fixed={"PXS_RING_LINE": "0"})
		assert_whole(pw, "ring pairs per pass"); assert pw["last"] == (nt + 1)//2
		assert_split(ps, "ring pairs per pass")
		if op in TO_MAP: assert 7 <= ps["first"] <= 10, ps
		else: assert ps["first"] % 52 == 0 or ps["first"] % 64 == 0, ps      # (whole tiles of the second stage; the remainder pass is partial: assert_split)
		compare(op, whole, split, True, op)
		check_oracle(op, (geometry, nt, nph, lmax, spin, f32, flip), alm[0], pix[0], split, kw, tol=F32_TOL if f32 else ORACLE_TOL)

RING_VARIANTS = [(False, None), (True, None), (False, (True, True))]
@pytest.mark.hostsim
@pytest.mark.parametrize("f32,flip", RING_VARIANTS)
@pytest.mark.parametrize("geometry,nt,nph,lmax,spin,ops,pairs", RING_CASES)
def test_ring_passes_hostsim(monkeypatch, geometry, nt, nph, lmax, spin, ops, pairs, f32, flip): check_ring_passes(monkeypatch, geometry, nt, nph, lmax, spin, ops, pairs, f32, flip)
@pytest.mark.gpu
@pytest.mark.parametrize("f32,flip", RING_VARIANTS)
@pytest.mark.parametrize("geometry,nt,nph,lmax,spin,ops,pairs", RING_CASES)
def test_ring_passes_gpu(monkeypatch, geometry, nt, nph, lmax, spin, ops, pairs, f32, flip): check_ring_passes(monkeypatch, geometry, nt, nph, lmax, spin, ops, pairs, f32, flip)

# ---- 5. lines per pass of the unfused theta resamplers (PXS_RESAMPLE_MB, floor of 32; resample_chunk) --------------------------------------------
# (grid, lmax, spin, maps, (passes, first, last) of the column pairs of analysis_2d, ... of the columns of adjoint_analysis_2d)
RESAMPLE_CASES = [("F1", 78, 160, 70, 2, 1, (2, 32, 4), (3, 32, 7)),      # 71 columns: the last pair holds a single column
	("F1", 78, 160, 69, 0, 2, (2, 32, 3), (3, 32, 6)),
	("CC", 130, 300, 128, 2, 1, (3, 32, 1), (5, 32, 1))]      # 129 columns.  lmax > 70: no oracle run here; check_batched(5, "CC", 130, 300, 128) of test_batched_gpu pins the unsplit run of this shape

def check_resample_passes(monkeypatch, capfd, geometry, nt, nph, lmax, spin, nb, want_pairs, want_cols):
	"""PXS_RESAMPLE_MB=0: 32 lines per pass, the floor.  Bit for bit: a column (pair) goes through the same transforms in any pass;
	the rings of these grids are one wave per m in the Legendre analysis."""
	alm, pix = inputs(geometry, nt, nph, lmax, spin, nb); kw = call_kw(geometry, lmax, spin)
	a, x = (alm, pix) if nb > 1 else (alm[0], pix[0])
	for op, extra, fixed, want in (("analysis_2d", {}, {}, want_pairs), ("adjoint_analysis_2d", {}, {}, want_cols),
			("adjoint_analysis_2d", dict(analysis="interpolant"), {"PXS_ADJ_ANA_FUSED": "0"}, want_cols)):
		print("resampler passes %s %dx%d lmax %d spin %d, %d maps, %s %s:" % (geometry, nt, nph, lmax, spin, nb, op, extra))
		def call(split):
			read_err(capfd)
			out, plan = run(op, a, x, kw, **extra)
			route = [l for l in read_err(capfd).splitlines() if " route " in l]
			return out, plan.passes("resample"), route
		(whole, pw, rw), (split, ps, rs) = twice(monkeypatch, {"PXS_RESAMPLE_MB": "0"}, call, fixed=dict(fixed, PXS_CHAIN_VERBOSE="1"))
		print("  " + rs[0])
		assert rw == rs and "route unfused" in rs[0], rs
		assert_whole(pw, "lines per pass"); assert_split(ps, "lines per pass", npass=want[0])
		assert (ps["n"], ps["first"], ps["last"]) == want, ps
		compare(op, whole, split, True, op)
		outs = split if nb > 1 else split[None]
		for i in range(nb if lmax <= 70 else 0): check_oracle(op, (geometry, nt, nph, lmax, spin, nb, i, tuple(extra)), alm[i], pix[i], outs[i], kw, analysis=extra.get("analysis"))

@pytest.mark.hostsim
@pytest.mark.parametrize("geometry,nt,nph,lmax,spin,nb,want_pairs,want_cols", RESAMPLE_CASES[:2])
def test_resample_passes_hostsim(monkeypatch, capfd, geometry, nt, nph, lmax, spin, nb, want_pairs, want_cols): check_resample_passes(monkeypatch, capfd, geometry, nt, nph, lmax, spin, nb, want_pairs, want_cols)
@pytest.mark.gpu
@pytest.mark.parametrize("geometry,nt,nph,lmax,spin,nb,want_pairs,want_cols", RESAMPLE_CASES)
def test_resample_passes_gpu(monkeypatch, capfd, geometry, nt, nph, lmax, spin, nb, want_pairs, want_cols): check_resample_passes(monkeypatch, capfd, geometry, nt, nph, lmax, spin, nb, want_pairs, want_cols)

# ---- 6. lines per pass of the four-step FFT (PXS_FFT_TEMP_MB; lines_budget, o1_per, i_per in FftContext::exec) ------------------------------------
def fft_cases():
	rng = np.random.default_rng(5)
	c = rng.standard_normal((7, 16384)) + 1j*rng.standard_normal((7, 16384))
	r = rng.standard_normal((5, 32768)); rf = np.fft.rfft(r, axis=-1)
	s = rng.standard_normal((3, 11200, 6)) + 1j*rng.standard_normal((3, 11200, 6))
	r2 = rng.standard_normal((3, 20, 16384))
	# name: (transform, numpy's, budget in MB, (passes, first, last) of the lines)
	return {
		"fft [7, 16384], 1 MB": (lambda: pfft.fft(c), lambda: np.fft.fft(c, axis=-1), 1, (2, 4, 3)),      # 4 lines of 256 KB: 4 + 3, two passes
		"fft [7, 16384], 0.5 MB": (lambda: pfft.fft(c), lambda: np.fft.fft(c, axis=-1), 0.5, (4, 2, 1)),
		"ifft [7, 16384], 1 MB": (lambda: pfft.ifft(c), lambda: np.fft.ifft(c, axis=-1)*16384, 1, (2, 4, 3)),
		"ifft [7, 16384], 0.5 MB": (lambda: pfft.ifft(c), lambda: np.fft.ifft(c, axis=-1)*16384, 0.5, (4, 2, 1)),
		"rfft [5, 32768]": (lambda: pfft.rfft(r), lambda: rf, 1, (3, 2, 1)),
		"irfft [5, 32768]": (lambda: pfft.irfft(rf, n=32768, normalize=True), lambda: r, 1, (3, 2, 1)),
		"fft of the strided axis of [3, 11200, 6]": (lambda: pfft.fft(s, axes=[-2]), lambda: np.fft.fft(s, axis=-2), 1, (6, 5, 1)),      # 5 of the 6 lines of a block, then 1
		"2-D rfft of [3, 20, 16384]": (lambda: pfft.rfft(r2, axes=[-2, -1]), lambda: np.fft.rfftn(r2, axes=(-2, -1)), 1.8, (9, 7, 4)),      # the 60 rows in passes of 7 lines (an odd count: a pass boundary inside a pair of rows), 8 x 7 + 4
	}

def check_fft_passes(monkeypatch):
	"""Bit for bit: a line goes through the same two passes whatever chunk it is in"""
	for name, (ours, numpys, mb, want) in fft_cases().items():
		whole = ours(); pw = sht.fft_passes()
		monkeypatch.setenv("PXS_FFT_TEMP_MB", repr(mb))
		try: split = ours(); ps = sht.fft_passes()
		finally: monkeypatch.delenv("PXS_FFT_TEMP_MB")
		print("four-step passes, %s:" % name)
		assert_whole(pw, "lines per pass"); assert_split(ps, "lines per pass", npass=want[0])
		assert (ps["n"], ps["first"], ps["last"]) == want, ps
		d, e = rel(split, whole), rel(split, numpys())
		print("  split against whole %.3e, against numpy %.3e" % (d, e))
		assert np.array_equal(split, whole) and e < FFT_TOL, (name, d, e)

@pytest.mark.hostsim
def test_fft_passes_hostsim(monkeypatch): check_fft_passes(monkeypatch)
@pytest.mark.gpu
def test_fft_passes_gpu(monkeypatch): check_fft_passes(monkeypatch)

# ---- 7. maps per Legendre launch (plan option "leg_max_batch"; leg_max_batch into leg_batch_plan) ------------------------------------------------
def check_launch_cap(monkeypatch, capfd, spin, nb, cap, seam, want, mm_off, ordered=False):
	"""nb maps on F1 96 x 200 lmax 30 with at most `cap` maps (8 cap for the MFMA form) per launch; want: the launches (count, first,
	last) of the form `seam`.  One batch pass in both runs, and the cap moves no map to another kernel (asserted from the launch lists):
	the Legendre synthesis bit for bit, the unordered Legendre analysis bit for bit too -- 48 ring pairs are one wave per m, one addition
	per row -- and the ordered one by construction."""
	geometry, nt, nph, lmax = "F1", 96, 200, 30
	alm, pix = inputs(geometry, nt, nph, lmax, spin, nb); kw = call_kw(geometry, lmax, spin)
	fixed = {"PXS_CHAIN_VERBOSE": "1"}
	if mm_off: fixed.update(PXS_SYN_MM_MIN="0", PXS_ANA_MM_MIN="0")      # (every map through the single-map kernels)
	if ordered: sht.set_deterministic(True)
	try:
		for op in ("analysis_2d",) if ordered else ("synthesis_2d", "analysis_2d"):
			print("launch cap %d, %d spin-%d maps%s, %s:" % (cap, nb, spin, ", ordered" if ordered else "", op))
			def call(split):
				plan = sht.grid_plan(geometry, nt, nph, kw["phi0"], (False, False), lmax, lmax, kw["mstart"], 1)
				plan.set_option("leg_max_batch", cap if split else 0)
				read_err(capfd)
				out, plan2 = run(op, alm, pix, kw); assert plan2 is plan
				return out, plan.passes(seam), plan.passes("batch"), legendre_forms(capfd)
			(whole, pw, bw, fw), (split, ps, bs, fs) = twice(monkeypatch, {}, call, fixed=fixed)
			assert bw["n"] == bs["n"] == 1 and fw == fs and len(fs) == nb, (bw, bs, fw, fs)
			print("  at the default: %d launches, last %d maps" % (pw["n"], pw["last"]))
			assert_split(ps, "maps per %s launch" % seam)
			assert (ps["n"], ps["first"], ps["last"]) == want, ps
			if not ordered: assert pw["n"] < ps["n"], (pw, ps)
			compare(op, whole, split, True, op)
			for i in (0, nb - 1): check_oracle(op, (geometry, nt, nph, lmax, spin, nb, i), alm[i], pix[i], split[i], kw)
	finally:
		sht.set_deterministic(None)

# (spin, maps, cap, the launches looked at, (launches, first, last), single-map kernels only, ordered analysis)
CAP_CASES = [(0, 7, 2, "leg_valu", (4, 2, 1), True, False), (2, 5, 2, "leg_valu", (3, 2, 1), True, False),
	(0, 21, 1, "leg_mm", (3, 8, 5), False, False),      # 8 + 8, then the remainder group of 5
	(2, 5, 2, "leg_valu", (5, 1, 1), False, True)]      # the ordered analysis: one map per launch, with or without the cap
@pytest.mark.hostsim
@pytest.mark.parametrize("spin,nb,cap,seam,want,mm_off,ordered", CAP_CASES)
def test_launch_cap_hostsim(monkeypatch, capfd, spin, nb, cap, seam, want, mm_off, ordered): check_launch_cap(monkeypatch, capfd, spin, nb, cap, seam, want, mm_off, ordered)
@pytest.mark.gpu
@pytest.mark.parametrize("spin,nb,cap,seam,want,mm_off,ordered", CAP_CASES)
def test_launch_cap_gpu(monkeypatch, capfd, spin, nb, cap, seam, want, mm_off, ordered): check_launch_cap(monkeypatch, capfd, spin, nb, cap, seam, want, mm_off, ordered)
