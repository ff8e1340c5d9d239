"""Side streams, several streams at once, and the device-memory arena under them (GPU only: the host simulator has no streams).

Every other GPU test runs on torch's default stream, one call at a time.  Here the same calls run on non-blocking side streams,
two at a time on one cached plan, from two host threads, with a scratch buffer growing or a plan being evicted while earlier work
is still queued -- and must give what the project's own serial path gives (default stream, torch.cuda.synchronize() between the
calls; tests/test_sht_parity.py and the other parity files pin that path to the oracle).  No new tolerances: bitwise equality
(np.array_equal) where the project promises it (synthesis, rotate_alm, FFTs, analysis / adjoint under sht.set_deterministic(True)),
relative rms < 1e-13 for the default-mode analysis (the bound of tests/test_theta_line.py for "same arithmetic, other path").

Overlap is made certain by a gate (class Gate): a bounded run of large matmuls on a third stream, an event behind it, and every
stream of the scenario waiting for that event.  The scenario issues its calls while the gate is closed and then asserts that the
gate event is STILL pending: had it completed, the calls could have run one after the other and the test fails, saying so.
Two places cannot assert after the last call, because a step in them synchronises the device by design, and assert immediately
before that step instead (the work queued up to there is then provably still in flight when the step begins):
  * the first call on a plan (S3): building a plan's recurrence tables ends in hipDeviceSynchronize (csrc/legendre.hip), so the
    gate is over when such a call returns.  The second call of each S3 case runs behind a gate of its own, asserted after issue.
  * the reuse of an arena block released while work was in flight (S5, S6): the arena synchronises the device before it hands
    such a block out (csrc/arena.hip) -- that synchronisation is the fix under test.  The scenarios assert the gate pending right
    before the evicting call and the arena_hits delta after it: the reuse was requested under in-flight work.
  * an S3 case whose call waits for its stream on the host every time (host arrays in or out, a small host table uploaded per call,
    the points plan's check of its positions): the gate is asserted pending right before the second call as well, not after it.
S3 runs each case first on the default stream (the reference), drops the cached plans, and then on the side stream.  The FFT
engine's tables live outside the plan cache, keyed by length: the FFT case runs its side-stream passes BEFORE the reference, on
lengths of its own.

S4 (scratch growth): a buffer that grows gives its old block to the arena and takes a NEW one, so the growing call itself never
aliased the call before it, with or without the ordering of calls inside the library (nothing asks the arena for the old block's
size in that scenario).  What it shares with its neighbours is everything that did not grow, and the grown buffers with the call
AFTER it; the scenario therefore ends with a third call on the first stream.  Reuse of a released block under in-flight work is S5's.

S8 (arena accounting) has no host-simulator twin: the simulator allocates a plan's scratch in the first transform, like the GPU
build, and a transform on a grid whose buffers pass the arena's 32 MB threshold (about 2000 x 1300 spectra) takes minutes there.
"""
import threading
import numpy as np, pytest
from pixell_amd import sht, curvedsky, enmap, fft as pfft

pytestmark = pytest.mark.gpu

MINB = 32 << 20      # the arena's pooling threshold (csrc/arena.hip)

def T():
	import torch
	return torch

def relrms(a, b): return float(np.sqrt(np.mean(np.abs(a - b)**2)/np.mean(np.abs(b)**2)))
def host(x): return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)

# ---- the gate ------------------------------------------------------------------------------------------------------------------------
# Filler: FILLER_REPS float32 matmuls of FILLER_N x FILLER_N on a tensor allocated before the scenario.  Measured on an MI355X
# (test_gate_filler_outlasts_issue prints both figures): see the numbers next to FILLER_REPS.
FILLER_N = 8192
# measured on an MI355X: one filler (64 matmuls) runs 454 ms; issuing four library calls behind a gate from one thread takes 0.59 ms
# (the two-thread scenario adds two thread starts and a barrier, a few ms).  Several hundred times the issue time.
FILLER_REPS = 64

class Gate:
	def __init__(self):
		torch = T()
		self.a = torch.full((FILLER_N, FILLER_N), 1.0/FILLER_N, device="cuda", dtype=torch.float32)
		self.b = torch.empty_like(self.a)
		self.stream = torch.cuda.Stream()
		self.event = None
		with torch.cuda.stream(self.stream): torch.mm(self.a, self.a, out=self.b)      # (the BLAS library's first call: its own setup)
		torch.cuda.synchronize()
	def close(self, streams):
		"""queue the filler and make every stream of `streams` wait for its end"""
		torch = T()
		torch.cuda.synchronize()
		with torch.cuda.stream(self.stream):
			for _ in range(FILLER_REPS): torch.mm(self.a, self.a, out=self.b)
		self.event = torch.cuda.Event(); self.event.record(self.stream)
		for s in streams: s.wait_event(self.event)
	def pending(self, what):
		assert not self.event.query(), ("the gate had already opened %s: the calls of this scenario were not in flight together, "
			"so it proves nothing (filler too short for this machine, or a call synchronised the device)" % what)

@pytest.fixture(scope="module")
def gate():
	return Gate()

@pytest.fixture(autouse=True)
def clean_state():
	torch = T()
	sht.clear_plans(); sht.set_deterministic(None)
	yield
	torch.cuda.synchronize()
	sht.set_deterministic(None); sht.clear_plans()

def streams(n):
	torch = T()
	return [torch.cuda.Stream() for _ in range(n)]

def concurrent(gate, jobs):
	"""jobs: [(stream, fn)], issued in order from this thread behind one gate"""
	torch = T()
	gate.close([s for s, _ in jobs])
	for s, fn in jobs:
		with torch.cuda.stream(s): fn()
	gate.pending("when the last call had been issued")
	torch.cuda.synchronize()

def serial(fns):
	"""the reference: the same calls on the default stream, the device idle between them"""
	torch = T()
	for fn in fns:
		torch.cuda.synchronize(); fn()
	torch.cuda.synchronize()

# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
NT, NPH, LMAX = 2700, 5400, 2000      # F1 grid, fused chains; leg / hbuf = 87 MB per component (above the arena's threshold), a call takes a few ms

def rand_alm(lmax, nc, seed, nb=None):
	rng = np.random.default_rng(seed)
	n = (lmax + 1)*(lmax + 2)//2
	shape = (nc, n) if nb is None else (nb, nc, n)
	a = rng.standard_normal(shape) + 1j*rng.standard_normal(shape)
	a[..., :lmax + 1] = a[..., :lmax + 1].real
	return T().from_numpy(a).cuda()

def rand_map(shape, seed):
	return T().from_numpy(np.random.default_rng(seed).standard_normal(shape)).cuda()

def zeros(shape, complex_=False):
	torch = T()
	return torch.zeros(shape, dtype=torch.complex128 if complex_ else torch.float64, device="cuda")

def kw(lmax=LMAX, geometry="F1", spin=0): return dict(spin=spin, lmax=lmax, geometry=geometry, phi0=0.1)
def nalm(lmax): return (lmax + 1)*(lmax + 2)//2

def test_gate_filler_outlasts_issue(gate):
	"""the figures behind FILLER_REPS: how long the filler runs, how long the host takes to issue four calls on a warm plan"""
	import time
	torch = T()
	alm = rand_alm(LMAX, 1, 1); m = zeros((1, NT, NPH))
	sht.synthesis_2d(alm=alm, map=m, **kw()); torch.cuda.synchronize()
	t0 = time.perf_counter(); gate.close([]); torch.cuda.synchronize(); fill = time.perf_counter() - t0
	s1, s2 = streams(2)
	gate.close([s1, s2])
	t0 = time.perf_counter()
	for s in (s1, s2, s1, s2):
		with torch.cuda.stream(s): sht.synthesis_2d(alm=alm, map=m, **kw())
	issue = time.perf_counter() - t0
	gate.pending("after four calls")
	torch.cuda.synchronize()
	print("gate filler %.1f ms, issue of four calls %.3f ms" % (fill*1e3, issue*1e3))
	assert fill > 20*issue

# ---- S1 / S2: one cached plan, two streams ----------------------------------------------------------------------------------------------
def s1_cases(spin):
	"""[(name, fn_a(out), fn_b(out), make out_a, make out_b)]: a and b run on the same plan"""
	nc = 1 if spin == 0 else 2
	almA, almB = rand_alm(LMAX, nc, 10 + spin), rand_alm(LMAX, nc, 20 + spin)
	mapA, mapB = rand_map((nc, NT, NPH), 30 + spin), rand_map((nc, NT, NPH), 40 + spin)
	k = kw(spin=spin)
	syn = lambda alm: (lambda out: sht.synthesis_2d(alm=alm, map=out, **k))
	ana = lambda m: (lambda out: sht.analysis_2d(alm=out, map=m, **k))
	adj = lambda m: (lambda out: sht.adjoint_synthesis_2d(alm=out, map=m, **k))
	mo = lambda: zeros((nc, NT, NPH)); ao = lambda: zeros((nc, nalm(LMAX)), True)
	return [("alm2map", syn(almA), syn(almB), mo, mo), ("map2alm", ana(mapA), ana(mapB), ao, ao),
		("adjoint_synthesis", adj(mapA), adj(mapB), ao, ao), ("alm2map against map2alm", syn(almA), ana(mapB), mo, ao)]

def run_pair(gate, fa, fb, oa, ob, threads):
	"""two rounds of (a on s1, b on s2); returns ((a1, b1, a2, b2) concurrent, the same serial) as host arrays"""
	torch = T()
	ref = [oa(), ob(), oa(), ob()]; got = [oa(), ob(), oa(), ob()]
	serial([lambda: fa(ref[0]), lambda: fb(ref[1]), lambda: fa(ref[2]), lambda: fb(ref[3])])      # (also: the plan is built and its scratch sized)
	s1, s2 = streams(2)
	if not threads:
		concurrent(gate, [(s1, lambda: fa(got[0])), (s2, lambda: fb(got[1])), (s1, lambda: fa(got[2])), (s2, lambda: fb(got[3]))])
	else:
		gate.close([s1, s2])
		bar = threading.Barrier(2); err = []
		def work(s, f, o1, o2):
			try:
				with torch.cuda.stream(s):
					bar.wait(30); f(o1); f(o2)
			except BaseException as e: err.append(e)
		th = [threading.Thread(target=work, args=(s1, fa, got[0], got[2])), threading.Thread(target=work, args=(s2, fb, got[1], got[3]))]
		for t in th: t.start()
		for t in th: t.join(60)
		assert not any(t.is_alive() for t in th), "a thread is still inside its calls after 60 s"
		gate.pending("when both threads had issued their calls")
		torch.cuda.synchronize()
		assert not err, err
	return [host(x) for x in got], [host(x) for x in ref]

def check_pair(name, got, ref, bitwise):
	for i, (g, r) in enumerate(zip(got, ref)):
		assert np.abs(r).max() > 0
		if bitwise: assert np.array_equal(g, r), "%s, call %d: differs from the serial result (relative rms %.3g)" % (name, i, relrms(g, r))
		else: assert relrms(g, r) < 1e-13, "%s, call %d: relative rms %.3g against the serial result" % (name, i, relrms(g, r))

@pytest.mark.parametrize("spin", [0, 2])
@pytest.mark.parametrize("threads", [False, True], ids=["one_thread", "two_threads"])
def test_s1_s2_same_plan_two_streams(gate, spin, threads):
	"""S1 (one thread) / S2 (two threads, a stream each): two calls at a time on one cached plan, deterministic sums on -> bitwise"""
	sht.set_deterministic(True)
	for name, fa, fb, oa, ob in s1_cases(spin):
		got, ref = run_pair(gate, fa, fb, oa, ob, threads)
		check_pair(name, got, ref, True)
	assert len(sht._plans) == 1      # (one plan served everything)

def test_s1_default_mode_analysis(gate):
	"""S1, default (atomic) analysis sums: the serial result to rounding"""
	name, fa, fb, oa, ob = s1_cases(2)[1]
	got, ref = run_pair(gate, fa, fb, oa, ob, False)
	check_pair(name, got, ref, False)

# ---- S4: a scratch buffer grows while the previous call is in flight ------------------------------------------------------------------
def test_s4_scratch_growth_on_another_stream(gate):
	torch = T()
	k = kw(spin=2)      # (spin 2: the batched spin-0 path builds a table in its first call and waits for it)
	alm1, alm4 = rand_alm(LMAX, 2, 51), rand_alm(LMAX, 2, 52, nb=4)
	ref = [zeros((2, NT, NPH)), zeros((4, 2, NT, NPH)), zeros((2, NT, NPH))]; got = [torch.zeros_like(x) for x in ref]
	calls = lambda out: [lambda: sht.synthesis_2d(alm=alm1, map=out[0], **k), lambda: sht.synthesis_2d(alm=alm4, map=out[1], **k), lambda: sht.synthesis_2d(alm=alm1, map=out[2], **k)]
	serial(calls(ref))
	sht.clear_plans(release=True)      # (an empty arena: the growth below takes new blocks from the driver)
	plan = sht.synthesis_2d(alm=alm1, map=got[0], return_plan=True, **k); torch.cuda.synchronize()      # a fresh plan, sized for one map
	small = plan.info()["scratch_bytes"]; assert small > 2*MINB
	got[0].zero_(); torch.cuda.synchronize()
	before = sht.memory()
	s1, s2 = streams(2)
	c = calls(got)
	# phase 1: the growing call is issued while the call before it is queued.  It may wait for the device itself -- a buffer below the
	# arena's threshold grows through hipFree, which does -- so the gate is looked at before it, not after
	gate.close([s1, s2])
	with torch.cuda.stream(s1): c[0]()
	gate.pending("before the growing call")
	with torch.cuda.stream(s2): c[1]()
	after = sht.memory()
	torch.cuda.synchronize()
	assert plan.info()["scratch_bytes"] > 2*small      # the buffers grew behind the gate ...
	assert after["arena_bytes"] - before["arena_bytes"] > 2*MINB      # ... and their old blocks went to the arena while the first call was queued
	for i in range(2): assert np.array_equal(host(got[i]), host(ref[i])), "phase 1, call %d differs from the serial result (relative rms %.3g)" % (i, relrms(host(got[i]), host(ref[i])))
	# phase 2: four maps on one stream against one map on the other, on the grown buffers
	got[1].zero_()
	concurrent(gate, [(s2, c[1]), (s1, c[2])])
	for i in range(3): assert np.array_equal(host(got[i]), host(ref[i])), "call %d differs from the serial result (relative rms %.3g)" % (i, relrms(host(got[i]), host(ref[i])))

# ---- S5: a plan evicted while its call is in flight, its blocks reused by the next plan ---------------------------------------------
LMAX2 = 1900      # the second geometry: scratch 0.95 x the first one's, inside the arena's reuse window (a block serves requests down to 0.8 of its size)

def test_s5_plan_eviction_in_flight(gate, monkeypatch):
	torch = T()
	monkeypatch.setattr(sht._plans, "cap", 1)
	a1, a2 = rand_alm(LMAX, 2, 61), rand_alm(LMAX2, 2, 62)
	k1, k2 = kw(LMAX, spin=2), kw(LMAX2, spin=2)
	ref1, ref2 = zeros((2, NT, NPH)), zeros((2, NT, NPH)); got1, got2 = torch.zeros_like(ref1), torch.zeros_like(ref2)
	serial([lambda: sht.synthesis_2d(alm=a1, map=ref1, **k1), lambda: sht.synthesis_2d(alm=a2, map=ref2, **k2)])
	sht.clear_plans(release=True)
	sht.synthesis_2d(alm=a1, map=got1, **k1); torch.cuda.synchronize(); got1.zero_(); torch.cuda.synchronize()      # P1 built and warm, the arena empty
	assert len(sht._plans) == 1
	before = sht.memory()
	s1, s2 = streams(2)
	gate.close([s1, s2])
	with torch.cuda.stream(s1): sht.synthesis_2d(alm=a1, map=got1, **k1)      # queued behind the gate
	gate.pending("before the evicting call")
	with torch.cuda.stream(s2): sht.synthesis_2d(alm=a2, map=got2, **k2)      # builds P2: P1 is evicted, its blocks are reused
	after = sht.memory()
	torch.cuda.synchronize()
	assert len(sht._plans) == 1
	assert after["arena_hits"] - before["arena_hits"] >= 2, (before, after)      # (leg and hbuf at least)
	assert np.array_equal(host(got1), host(ref1)), "the evicted plan's call: relative rms %.3g" % relrms(host(got1), host(ref1))
	assert np.array_equal(host(got2), host(ref2)), "the new plan's call: relative rms %.3g" % relrms(host(got2), host(ref2))

# ---- S7: one points plan, synthesis and adjoint on two streams ----------------------------------------------------------------------
def test_s7_points_plan_two_streams(gate):
	torch = T()
	sht.set_deterministic(True)
	lmax, npts = 1000, 200000
	rng = np.random.default_rng(71)
	loc = torch.from_numpy(np.stack([np.arccos(rng.uniform(-1, 1, npts)), rng.uniform(0, 2*np.pi, npts)], 1)).cuda()
	alm = rand_alm(lmax, 1, 72); vals = rand_map((1, npts), 73)
	plan = sht.points_plan(loc, lmax, epsilon=1e-10)
	fs = lambda out: sht.synthesis_general(alm=alm, loc=loc, spin=0, lmax=lmax, map=out, plan=plan)
	fa = lambda out: sht.adjoint_synthesis_general(map=vals, loc=loc, spin=0, lmax=lmax, alm=out, plan=plan)
	mo = lambda: zeros((1, npts)); ao = lambda: zeros((1, nalm(lmax)), True)
	ref = [mo(), ao(), mo(), ao()]; got = [mo(), ao(), mo(), ao()]
	serial([lambda: fs(ref[0]), lambda: fa(ref[1]), lambda: fs(ref[2]), lambda: fa(ref[3])])
	s1, s2 = streams(2)
	with torch.cuda.stream(s1): fs(got[0])      # (the FFT engine keeps scratch per stream: these two streams have theirs before the gate closes)
	with torch.cuda.stream(s2): fa(got[1])
	torch.cuda.synchronize(); got[0].zero_(); got[1].zero_()
	concurrent(gate, [(s1, lambda: fs(got[0])), (s2, lambda: fa(got[1])), (s1, lambda: fs(got[2])), (s2, lambda: fa(got[3]))])
	check_pair("points plan", [host(x) for x in got], [host(x) for x in ref], True)

# ---- S6: FFT scratch tables ----------------------------------------------------------------------------------------------------------
def test_s6_fft_five_streams(gate):
	"""enmap.fft's 2-D engine keeps scratch per stream, four streams per device: the fifth stream evicts the first one's, still in flight"""
	torch = T()
	ny, nx = 2048, 4096      # 128 MB of complex output: the engine's intermediates pass the arena's threshold
	ins = [rand_map((ny, nx), 80 + i) for i in range(5)]
	ref = [zeros((ny, nx), True) for _ in range(5)]; got = [zeros((ny, nx), True) for _ in range(5)]
	serial([(lambda i=i: pfft.fft(ins[i], ref[i], axes=[-2, -1])) for i in range(5)])
	sht.memory(release=True)
	ss = streams(5)
	for i in range(4):
		with torch.cuda.stream(ss[i]): pfft.fft(ins[i], got[i], axes=[-2, -1])      # four streams hold the table's four entries
	torch.cuda.synchronize()
	for g in got: g.zero_()
	before = sht.memory()
	gate.close(ss)
	for i in range(4):
		with torch.cuda.stream(ss[i]): pfft.fft(ins[i], got[i], axes=[-2, -1])
	gate.pending("before the evicting transform")
	with torch.cuda.stream(ss[4]): pfft.fft(ins[4], got[4], axes=[-2, -1])
	after = sht.memory()
	torch.cuda.synchronize()
	assert after["arena_hits"] > before["arena_hits"], (before, after)
	for i in range(5): assert np.array_equal(host(got[i]), host(ref[i])), "stream %d: relative rms %.3g" % (i, relrms(host(got[i]), host(ref[i])))

def test_s6_bluestein_scratch_grows(gate):
	"""a length with a prime factor > 2048 (65537): chirp-z scratch per stream.  Stream 1 has 137 MB (64 lines); behind the gate it
	transforms 64 lines, then 160 lines -- its scratch grows and the old block, which the first transform still reads, goes to the
	arena -- and then stream 2, whose scratch is smaller than that (nothing in this file gives a stream more than 80 MB), transforms
	64 lines of its own: its request is served by that very block (arena_hits), which the arena must not hand over before stream 1's
	first transform has run."""
	torch = T()
	n = 65537
	rng = np.random.default_rng(90)
	mk = lambda lines: torch.from_numpy(rng.standard_normal((lines, n)) + 1j*rng.standard_normal((lines, n))).cuda()
	xa, xb, xc = mk(64), mk(160), mk(64)
	ref = [torch.zeros_like(xa), torch.zeros_like(xb), torch.zeros_like(xc), torch.zeros_like(xa)]; got = [torch.zeros_like(x) for x in ref]
	calls = lambda out: [lambda: pfft.fft(xa, out[0], axes=[-1]), lambda: pfft.fft(xb, out[1], axes=[-1]), lambda: pfft.fft(xc, out[2], axes=[-1]), lambda: pfft.ifft(xa, out[3], axes=[-1])]
	serial(calls(ref))
	sht.memory(release=True)
	s1, s2 = streams(2)
	with torch.cuda.stream(s1): pfft.fft(xa, got[0], axes=[-1])      # stream 1's scratch, sized for 64 lines
	torch.cuda.synchronize(); got[0].zero_()
	before = sht.memory()
	c = calls(got)
	gate.close([s1, s2])
	with torch.cuda.stream(s1): c[0](); c[1]()      # the second grows the scratch: a new block from the driver, the old one to the arena
	grown = sht.memory()
	assert grown["arena_bytes"] - before["arena_bytes"] > 4*MINB and grown["arena_hits"] == before["arena_hits"], (before, grown)
	gate.pending("before the transform that reuses the released block")
	with torch.cuda.stream(s2): c[2]()      # (waits for the device inside the arena: that wait is what keeps stream 1's first transform intact)
	after = sht.memory()
	with torch.cuda.stream(s1): c[3]()
	torch.cuda.synchronize()
	assert after["arena_hits"] > grown["arena_hits"], (grown, after)
	for i in range(4): assert np.array_equal(host(got[i]), host(ref[i])), "transform %d: relative rms %.3g" % (i, relrms(host(got[i]), host(ref[i])))

def test_alm2cl_two_streams(gate):
	"""pxa_alm2cl keeps its partial sums per (device, stream): spectra of two alm on two streams, through the C ABI with device tables
	(curvedsky.alm2cl uploads the alm layout on every call, which waits for the stream), eight calls a stream behind one gate"""
	import ctypes
	from pixell_amd import _lib
	torch = T()
	lmax = 3000
	a = [rand_alm(lmax, 1, 97), rand_alm(lmax, 1, 98)]
	ms = torch.from_numpy(sht.tri_mstart(lmax).astype(np.int64)).cuda()
	lib = _lib.load(); dev = sht.device_index()
	def run(i, out):
		st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
		_lib.check(lib.pxa_alm2cl(lmax, lmax, ms.data_ptr(), 1, a[i].data_ptr(), a[i].data_ptr(), 3, out.data_ptr(), 1, dev, st))
	ref = [zeros((lmax + 1,)) for _ in range(16)]; got = [zeros((lmax + 1,)) for _ in range(16)]
	serial([(lambda k=k: run(k % 2, ref[k])) for k in range(16)])
	ss = streams(2)
	for i in range(2):
		with torch.cuda.stream(ss[i]): run(i, got[i])      # (each stream's scratch exists before the gate closes)
	torch.cuda.synchronize()
	concurrent(gate, [(ss[k % 2], (lambda k=k: run(k % 2, got[k]))) for k in range(16)])
	for k in range(16):
		assert np.abs(host(ref[k])).max() > 0
		assert np.array_equal(host(got[k]), host(ref[k])), "call %d: relative rms %.3g" % (k, relrms(host(got[k]), host(ref[k])))

# ---- S8: arena accounting ------------------------------------------------------------------------------------------------------------
def test_s8_arena_accounting():
	torch = T()
	a1, a2 = rand_alm(LMAX, 2, 95), rand_alm(LMAX2, 2, 96)
	m = zeros((2, NT, NPH))
	def build_run_drop(alm, lmax):
		sht.synthesis_2d(alm=alm, map=m, **kw(lmax, spin=2)); torch.cuda.synchronize(); sht.clear_plans()
		return sht.memory()
	build_run_drop(a1, LMAX); build_run_drop(a2, LMAX2)      # (what the library keeps per process -- FFT tables and the like -- exists from here on)
	sht.clear_plans(release=True)
	m0 = sht.memory()
	assert m0["arena_bytes"] == 0
	m1 = build_run_drop(a1, LMAX)
	assert m1["arena_bytes"] > 2*MINB and m1["live_bytes"] == m0["live_bytes"], (m0, m1)
	m2 = build_run_drop(a2, LMAX2)      # 0.95 of every buffer: served by the first plan's blocks
	assert m2["arena_hits"] - m1["arena_hits"] >= 2, (m1, m2)
	assert m2["arena_bytes"] == m1["arena_bytes"], "the arena holds the same blocks as before, but reports %d bytes after %d" % (m2["arena_bytes"], m1["arena_bytes"])
	assert m2["live_bytes"] == m0["live_bytes"], (m0, m2)
	m3 = sht.memory(release=True)
	assert m3["arena_bytes"] == 0 and m3["live_bytes"] == m0["live_bytes"], (m0, m3)

# ---- S3: a side stream alone, first call on the plan, the default stream busy -----------------------------------------------------------
def _alm_np(lmax, nc, seed):
	return host(rand_alm(lmax, nc, seed))

def s3_cases():
	"""name -> (make inputs, run(inputs) -> result, whether run returns without waiting for its stream once its plans exist).
	run is called as the first use of its plans."""
	torch = T()
	C = {}
	def grid(name, geometry, nt, nph, lmax, spin, line=None):
		nc = 1 if spin == 0 else 2
		k = dict(spin=spin, lmax=lmax, geometry=geometry, phi0=0.0)
		def mk(): return (rand_alm(lmax, nc, 100 + spin), rand_map((nc, nt, nph), 101 + spin))
		def run(inp):
			alm, m = inp
			out_m = zeros((nc, nt, nph)); out_a = zeros((nc, nalm(lmax)), True)
			plan = sht.synthesis_2d(alm=alm, map=out_m, return_plan=True, **k)
			sht.analysis_2d(alm=out_a, map=m, **k)
			if line is not None: assert plan.query("theta_line") == line
			return torch.cat([out_m.flatten(), torch.view_as_real(out_a).flatten()])
		C[name] = (mk, run, True)
	grid("F1 theta line", "F1", 5400, 10800, 4000, 0, line=1)      # the BASELINE C2 grid: the single-kernel theta engine
	grid("F1 chain spin 2", "F1", 512, 1024, 300, 2, line=0)        # the stage chain
	grid("CC", "CC", 1025, 2048, 500, 0)                            # ring weights on the CC grid's own rings
	def band():
		shape, wcs = enmap.band_geometry(np.deg2rad(15.0), shape=None, res=np.pi/2700)
		lmax = 1500
		def mk(): return _alm_np(lmax, 3, 110)
		def run(alm): return np.array(curvedsky.alm2map(alm, enmap.zeros((3,) + tuple(shape[-2:]), wcs), spin=[0, 2]))      # numpy in and out: the host-array route
		C["declination band, host arrays"] = (mk, run, False)      # (a host-array result is complete, downloaded, when its call returns)
	band()
	def healpix():
		nside, lmax = 256, 512
		def mk(): return rand_alm(lmax, 3, 120)
		def run(alm): return curvedsky.alm2map_healpix(alm, zeros((3, 12*nside**2)), spin=[0, 2])      # general ring path: the plan's own side streams
		C["healpix"] = (mk, run, True)
	healpix()
	def pos():
		lmax, npts = 500, 50000
		rng = np.random.default_rng(130)
		def mk():
			loc = torch.from_numpy(np.stack([np.arccos(rng.uniform(-1, 1, npts)), rng.uniform(0, 2*np.pi, npts)], 1)).cuda()
			return loc, rand_alm(lmax, 1, 131), rand_map((1, npts), 132)
		def run(inp):
			loc, alm, vals = inp
			m = curvedsky.alm2map_pos(alm, loc=loc, spin=0)      # device arrays in and out, both directions
			a = curvedsky.alm2map_pos(zeros((1, nalm(lmax)), True), loc=loc, map=vals, spin=0, adjoint=True)
			return torch.cat([m.flatten(), torch.view_as_real(a).flatten()])
		C["alm2map_pos and adjoint"] = (mk, run, False)      # (making the points plan checks the positions on the host: a wait for the stream in every call)
	pos()
	def almops():
		lmax = 600
		def mk(): return rand_alm(lmax, 3, 140)
		C["rotate_alm"] = (mk, lambda alm: curvedsky.rotate_alm(alm, 0.3, 0.7, -1.1), True)
		def run(alm):
			cl = curvedsky.alm2cl(alm)
			f = curvedsky.almxfl(alm, lambda l: 1.0/(1.0 + l))
			return torch.cat([torch.as_tensor(cl).flatten().to(f.device), torch.view_as_real(f).flatten()])
		C["alm2cl, almxfl"] = (mk, run, False)      # (each call uploads a small host table -- the alm layout, the filter -- with a synchronous copy on its stream)
	almops()
	def ffts():
		# The FFT engine's tables are process-wide and keyed by length, not held in the plan cache: for this case the side-stream pass comes
		# BEFORE the default-stream reference (SIDE_FIRST), with lengths nothing else in the test session transforms (1080 x 2100, 4099, 2100)
		ny, nx = 1080, 2100
		def mk(): return rand_map((3, ny, nx), 150), torch.complex(rand_map((600, 4099), 151), rand_map((600, 4099), 152))
		def run(inp):
			m, z = inp
			shape, wcs = enmap.fullsky_geometry(shape=(ny, nx))
			f = pfft.fft(m, zeros((3, ny, nx), True), axes=[-2, -1])                       # real -> complex, the 2-D engine
			b = pfft.ifft(f, zeros((3, ny, nx), True), axes=[-2, -1], normalize=True)      # complex -> complex
			blue = pfft.fft(z, torch.zeros_like(z), axes=[-1])                              # 4099 is prime: Bluestein
			d = pfft.dct(m, torch.zeros_like(m), axes=[-1], type="DCT-II")
			h = enmap.map2harm(enmap.dmap(m, wcs), spin=[0, 2])
			return torch.cat([torch.view_as_real(x).flatten() for x in (f, b, blue, enmap._data(h))] + [d.flatten()])
		C["fft, ifft, Bluestein, DCT, map2harm"] = (mk, run, True)
	ffts()
	return C

S3_NAMES = ["F1 theta line", "F1 chain spin 2", "CC", "declination band, host arrays", "healpix", "alm2map_pos and adjoint", "rotate_alm", "alm2cl, almxfl", "fft, ifft, Bluestein, DCT, map2harm"]
SIDE_FIRST = ("fft, ifft, Bluestein, DCT, map2harm",)      # the reference run comes after the side-stream passes

@pytest.mark.parametrize("name", S3_NAMES)
def test_s3_side_stream_first_call(gate, name):
	torch = T()
	sht.set_deterministic(True)
	mk, run, asynchronous = s3_cases()[name]
	inp = mk(); torch.cuda.synchronize()
	ref = None
	if name not in SIDE_FIRST:
		ref = host(run(inp)); torch.cuda.synchronize()      # default stream, first call on fresh plans
	sht.clear_plans()
	busy = torch.zeros(1 << 24, device="cuda")
	side, = streams(1)
	default = torch.cuda.current_stream()
	gate.close([default]); busy.add_(1.0)      # the default (NULL) stream is held behind the gate
	gate.pending("before the first call")
	with torch.cuda.stream(side): first = run(inp)      # builds its plans (which may wait for the device) and runs on the side stream
	torch.cuda.synchronize()
	gate.close([default, side]); busy.add_(1.0)
	gate.pending("before the second call")
	with torch.cuda.stream(side): second = run(inp)
	if asynchronous: gate.pending("when the second call had been issued")
	torch.cuda.synchronize()
	first, second = host(first), host(second)
	if ref is None: ref = host(run(inp)); torch.cuda.synchronize()
	assert np.abs(ref).max() > 0
	assert np.array_equal(first, ref), "first call on a side stream: relative rms %.3g against the default stream" % relrms(first, ref)
	assert np.array_equal(second, ref), "second call on a side stream: relative rms %.3g against the default stream" % relrms(second, ref)
