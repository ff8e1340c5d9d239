"""`ducc0.sht.experimental`-shaped entry points backed by the HIP kernels (include/pxsht.h).

Same keyword interface as the calls pixell/curvedsky.py makes (curvedsky.py:907-924, 936-960,
1032-1046, 1068-1084, 501): arrays may be numpy (staged through device memory) or torch CUDA
tensors (used in place, no copies).  Output arrays are mutated in place and returned, as ducc does.
Extra keyword `flip=(flip_y, flip_x)` (ours): the map is given in its native pixel order and the
flips of curvedsky.map2buffer/buffer2map (curvedsky.py:1384-1411) are folded into kernel
addressing; phi0 is still that of the flipped map (analyse_geometry().phi0).
"""
import ctypes, os, contextlib, threading
import numpy as np
from . import _lib, _arrays as A
from ._arrays import device_index, current_stream      # (tests and tools call them under these names)

# host-array route (pixell_amd/hostio.py): the Pipeline of the API call in progress ON THIS THREAD, if any.  Per thread: a call on
# another thread must neither see this one's pipeline (its write-backs would complete on a queue this call may already have closed)
# nor be kept from opening its own.
_tls = threading.local()
def _pipe(): return getattr(_tls, "pipe", None)
@contextlib.contextmanager
def host_pipeline(inputs=(), outputs=()):
	"""for the duration of one API call: numpy `inputs` are uploaded by a background thread, in order, starting now; numpy outputs
	of the transforms issued inside are downloaded in the background; everything is complete when the block exits"""
	from . import hostio
	if _pipe() is not None or _lib.is_hostsim() or not any(hostio.eligible(a) for a in list(inputs)+list(outputs)):
		yield; return
	_tls.pipe = hostio.Pipeline(); _tls.pipe.prefetch(inputs)
	try: yield
	finally:
		p = _tls.pipe; _tls.pipe = None; p.close()

class _Buf:
	"""device view of a numpy array or torch tensor (contiguous), with optional write-back.  overwrite: the call writes every
	element (an output whose old content need not travel to the device)"""
	def __init__(self, arr, writeback=False, overwrite=False):
		self.arr = arr; self.writeback = writeback; self.tmp = None; self.keep = None; self.slab = False
		if A.is_tensor(arr):
			A.require_gpu(arr)
			if not arr.is_contiguous():
				if writeback: raise ValueError("output tensors must be contiguous")
				arr = arr.contiguous()
			self.keep = arr; self.ptr = arr.data_ptr()
		else:
			if _lib.is_hostsim():
				if arr.flags.c_contiguous and arr.dtype.isnative: self.keep = arr
				else: self.keep = np.ascontiguousarray(arr); self.tmp = self.keep
				self.ptr = self.keep.ctypes.data
			else:
				torch = A.torch()
				from . import hostio
				pipe = _pipe(); got = pipe.take(arr) if pipe is not None else None
				self.slab = hostio.eligible(arr)
				if got is not None:                      # uploaded in the background since the call began
					self.tmp, ev = got; torch.cuda.current_stream().wait_event(ev)
					self.tmp.record_stream(torch.cuda.current_stream())      # (allocated by the background thread: tell the allocator which stream consumes it)
				elif self.slab and writeback and overwrite:
					self.tmp = A.empty(arr.shape, arr.dtype)
				elif self.slab:
					self.tmp, ev = hostio.upload(arr); torch.cuda.current_stream().wait_event(ev)
				else: self.tmp = A.put(arr)
				self.ptr = self.tmp.data_ptr()
	def finish(self):
		if not self.writeback or self.tmp is None: return
		if _lib.is_hostsim(): self.arr[...] = self.tmp
		elif self.slab:
			from . import hostio
			ev = A.torch().cuda.Event(); ev.record()
			pipe = _pipe()
			if pipe is not None: pipe.writeback(self.tmp, self.arr, ev)      # complete when the host_pipeline block (of this thread) exits
			else: hostio.download(self.tmp, self.arr, after=ev)
		else: self.arr[...] = A.host(self.tmp)

class Plan:
	"""RAII wrapper of pxs_plan"""
	def __init__(self, handle):
		self.handle = handle; self.lock = threading.RLock()      # (option + call pairs on a shared cached plan are atomic per thread)
		self._det_default = int(os.environ.get("PXS_DETERMINISTIC", "0") not in ("", "0"))      # what the library gave the plan when it was made
	def __del__(self):
		try:
			if self.handle: _lib.load().pxs_plan_destroy(self.handle); self.handle = None
		except Exception: pass
	def profile(self, enable=True):
		_lib.check(_lib.load().pxs_profile(self.handle, int(bool(enable))))
	def profile_read(self, reset=True):
		"""{stage: (total ms, launches)} from the hipEvent stage timers (pxsht.h PXS_STAGE_*)"""
		ms = (ctypes.c_double*4)(); cnt = (ctypes.c_int*4)()
		_lib.check(_lib.load().pxs_profile_read(self.handle, ms, cnt, int(bool(reset))))
		names = ["leg_syn", "leg_ana", "ring_fft", "resample"]
		return {n: (ms[i], cnt[i]) for i, n in enumerate(names)}
	def profile_flops(self, reset=True, executed=False):
		"""FP64 flops of the Legendre kernels while profiling was on: (synthesis, analysis).  Default: the wave count of pxs_profile_flops, every block of a wave
		counted from the wave's start.  executed=True: what the kernels executed, the blocks of the analysis kernels counted from their own start (plan query
		"leg_executed_flops_ana"; the synthesis kernels start all blocks with the wave, so their two counts are one)"""
		ana = float(self.query("leg_executed_flops_ana")) if executed else None
		f = (ctypes.c_double*2)()
		_lib.check(_lib.load().pxs_profile_flops(self.handle, f, int(bool(reset))))
		return (f[0], ana) if executed else (f[0], f[1])
	def set_option(self, name, value):
		"""pxs_plan_option: "analysis" = 2 (ducc0's route, the default) | 0 (full theta-interpolant) | 1 (ring weights + adjoint synthesis where ntheta >= 2 lmax + 2);
		"deterministic" = 0 | 1 (ordered, bitwise repeatable analysis sums; see set_deterministic);
		"leg_max_batch" = n (at most n maps per single-map Legendre launch, 8 n per FP64-MFMA launch; 0: the grid limit alone -- for tests);
		"leg_ana_k" = K (ring pairs per lane of the single-map Legendre analysis kernels; 0: the library's rule -- for tests)"""
		_lib.check(_lib.load().pxs_plan_option(self.handle, name.encode(), int(value)))
	def query(self, name):
		"""pxs_plan_query: "analysis_form", "ncc_circle", "ducc_ncc_circle", "theta_line", "chain_stages", "chain_static", "chain_static_table", "leg_ana_k" (ring pairs per lane of the plan's
		most recent single-map Legendre analysis), "passes_<seam>" (see passes) """
		v = ctypes.c_int64()
		_lib.check(_lib.load().pxs_plan_query(self.handle, name.encode(), ctypes.byref(v)))
		return int(v.value)
	def passes(self, seam):
		"""the passes the plan's most recent call took at a memory-budget seam (pxs_plan_query "passes_<seam>", counted by the loop
		that launched them): dict(n=how many, first=, prev=, last= sizes of the first pass, the one before the last and the last).
		seam: "batch" (maps per pass, PXS_BATCH_GB), "leg_m" (m per range of the ordered analysis, PXS_PART_GB), "theta" (components per
		pass of a theta chain, PXS_CHAIN_SCRATCH_GB), "ring" (ring pairs per pass of the ring FFT stages, PXS_RING_CHUNK_MB), "resample"
		(column pairs or columns per pass of an unfused theta resampler, PXS_RESAMPLE_MB), "leg_valu" / "leg_mm" (maps per VALU / MFMA
		Legendre launch, option "leg_max_batch"), "fft" (see fft_passes)"""
		return _passes(self.handle, seam)
	def info(self):
		a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
		_lib.check(_lib.load().pxs_plan_info(self.handle, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
		return dict(nring_syn=a.value, nring_ana=b.value, scratch_bytes=c.value)

def _passes(handle, seam):
	out = {}
	for key, suffix in (("n", ""), ("first", "_first"), ("prev", "_prev"), ("last", "_last")):
		v = ctypes.c_int64()
		_lib.check(_lib.load().pxs_plan_query(handle, ("passes_" + seam + suffix).encode(), ctypes.byref(v)))
		out[key] = int(v.value)
	return out
def fft_passes():
	"""lines per pass of the most recent four-step FFT on the current device (PXS_FFT_TEMP_MB; pxs_plan_query(NULL, "passes_fft")), as
	Plan.passes reports the plan-bound seams"""
	return _passes(None, "fft")

class _PlanCache:
	"""least-recently-used cache of pxs_plan handles: a plan owns device scratch (tens of GB at the largest configurations), so a
	sweep over geometries or band limits must not keep every plan alive.  PIXELL_AMD_MAX_PLANS (default 4) bounds the count; an
	evicted plan is destroyed.  Its kernels may still be queued, on any stream: the library's arena synchronises the device before a
	block of the plan's scratch serves another plan or goes back to the driver (csrc/arena.hip)."""
	def __init__(self):
		import collections
		self.d = collections.OrderedDict()
		self.cap = max(1, int(os.environ.get("PIXELL_AMD_MAX_PLANS", "4")))
	def get(self, key):
		p = self.d.get(key)
		if p is not None: self.d.move_to_end(key)
		return p
	def __setitem__(self, key, plan):
		self.d[key] = plan; self.d.move_to_end(key)
		while len(self.d) > self.cap: self.d.popitem(last=False)
	def clear(self): self.d.clear()
	def __len__(self): return len(self.d)
_plans = _PlanCache()
def clear_plans(release=False):
	"""drop the cached plans.  Their device scratch goes to the library's arena (pxs_memory) for the next plans; release=True returns it to the driver."""
	_plans.clear()
	if release: memory(release=True)

def memory(release=False):
	"""pxs_memory: dict(malloc_ms, malloc_calls, malloc_bytes, arena_hits, arena_bytes, live_bytes); release=True empties the arena first"""
	import gc; gc.collect()      # (plans dropped a moment ago have released their buffers)
	st = (ctypes.c_double*6)()
	_lib.check(_lib.load().pxs_memory(int(bool(release)), st))
	return dict(malloc_ms=st[0], malloc_calls=int(st[1]), malloc_bytes=int(st[2]), arena_hits=int(st[3]), arena_bytes=int(st[4]), live_bytes=int(st[5]))

class PlanPin:
	"""Plans that outlive the cache: an object that transforms on a fixed set of geometries again and again (a wavelet transform: one
	plan per scale group) owns its plans here instead of competing for the PIXELL_AMD_MAX_PLANS slots.  While a pin is active on the
	calling thread (`with pin:`; pins nest, the innermost is used), grid_plan / ring_plan look in it first, then in the cache, and a plan
	they have to build goes into the pin and not into the cache.  With no pin active nothing changes.  The plans (and their device
	scratch) are released with the pin, or by clear()."""
	def __init__(self): self.plans = {}
	def __enter__(self):
		if not hasattr(_tls, "pins"): _tls.pins = []
		_tls.pins.append(self); return self
	def __exit__(self, *exc): _tls.pins.pop(); return False
	def clear(self): self.plans.clear()
	def __len__(self): return len(self.plans)

def _cached_plan(key, make):
	"""the plan of `key`: from the active pin, else from the cache, else make() -- kept by the pin if there is one, by the cache otherwise"""
	pins = getattr(_tls, "pins", None)
	pin = pins[-1] if pins else None
	p = pin.plans.get(key) if pin is not None else None
	if p is None: p = _plans.get(key)
	if p is None:
		p = Plan(make())
		if pin is None: _plans[key] = p
	if pin is not None: pin.plans[key] = p
	return p

_deterministic = None
def set_deterministic(on=True):
	"""Bitwise repeatable transforms (pxs_plan_option "deterministic", include/pxsht.h): by default the Legendre analysis adds the
	contributions of the ring chunks of an m with atomic adds in arrival order, so map2alm / alm2map_adjoint repeat from run to run
	to ~1e-14 only.  on=True applies the ordered sums to every plan used from now on (cached plans included); None restores the
	default (PXS_DETERMINISTIC as the plan was made)."""
	global _deterministic
	_deterministic = None if on is None else bool(on)
def _apply_mode(plan):
	"""the process-wide deterministic switch onto a (cached, shared) plan.  Called with plan.lock held, in the same critical section as the
	transform it applies to (_run_syn / _run_ana): a toggle by another thread cannot land between an option and its call."""
	want = _deterministic
	if want is None and getattr(plan, "_det", None) is not None:      # a cached plan that was switched: back to the default it was made with
		plan.set_option("deterministic", plan._det_default); plan._det = None
	elif want is not None and getattr(plan, "_det", None) != want:
		plan.set_option("deterministic", int(want)); plan._det = want
	return plan

def tri_mstart(lmax, mmax=None):
	if mmax is None: mmax = lmax
	m = np.arange(mmax+1, dtype=np.int64)
	return (m*(2*lmax+1-m)//2).astype(np.uint64)

def grid_plan(geometry, ntheta, nphi, phi0, flip, lmax, mmax, mstart, lstride=1):
	"""cached pxs_plan, shared by every stream of its device (a plan owns its device scratch: the library runs the calls on one plan in
	the order they were issued, whatever their streams -- include/pxsht.h)"""
	ms = np.ascontiguousarray(np.asarray(mstart)[:mmax+1], dtype=np.uint64)
	key = ("g", geometry, int(ntheta), int(nphi), float(phi0), bool(flip[0]), bool(flip[1]), int(lmax), int(mmax), ms.tobytes(), int(lstride), device_index())
	def make():
		h = ctypes.c_void_p()
		_lib.check(_lib.load().pxs_plan_grid2d(ctypes.byref(h), geometry.encode(), int(ntheta), int(nphi), float(phi0),
			int(bool(flip[0])), int(bool(flip[1])), int(lmax), int(mmax), ms.ctypes.data, int(lstride), device_index()))
		return h
	return _cached_plan(key, make)

def ring_plan(theta, nphi, phi0, ringstart, lmax, mmax, mstart, lstride=1, pixstride=1):
	th = np.ascontiguousarray(theta, dtype=np.float64); nph = np.ascontiguousarray(nphi, dtype=np.uint64)
	p0 = np.ascontiguousarray(phi0, dtype=np.float64); rs = np.ascontiguousarray(ringstart, dtype=np.uint64)
	ms = np.ascontiguousarray(np.asarray(mstart)[:mmax+1], dtype=np.uint64)
	key = ("r", th.tobytes(), nph.tobytes(), p0.tobytes(), rs.tobytes(), int(pixstride), int(lmax), int(mmax), ms.tobytes(), int(lstride), device_index())
	def make():
		h = ctypes.c_void_p()
		_lib.check(_lib.load().pxs_plan_rings(ctypes.byref(h), len(th), th.ctypes.data, nph.ctypes.data, p0.ctypes.data, rs.ctypes.data,
			int(pixstride), int(lmax), int(mmax), ms.ctypes.data, int(lstride), device_index()))
		return h
	return _cached_plan(key, make)

def _ncomp(spin, mode):
	"""(alm components, map components) of a call; the one place that refuses an unknown mode"""
	if mode == "DERIV1": return 1, 2
	if mode != "STANDARD": raise ValueError("unknown mode '%s'" % str(mode))
	return (1, 1) if spin == 0 else (2, 2)

def _check_pair(alm, map, spin, mode, pixdims):
	nca, ncm = _ncomp(spin, mode)
	if alm.ndim == 3 and map.ndim == 2+pixdims:          # a batch of independent maps (ours; ducc takes one map per call)
		if alm.shape[0] != map.shape[0]: raise ValueError("batched call: alm and map disagree on the batch size")
		alm, map = alm[0], map[0]
	if alm.ndim != 2 or alm.shape[0] != nca: raise ValueError("alm must have shape [%d,nelem] for spin %d mode %s" % (nca, spin, mode))
	if map.ndim != 1+pixdims or map.shape[0] != ncm: raise ValueError("map must have %d components" % ncm)
	ad, md = A.np_dtype(alm), A.np_dtype(map)
	if ad not in (np.complex64, np.complex128) or md not in (np.float32, np.float64): raise TypeError("alm must be complex, map real")
	return ad, md

class _View:
	"""device pointer + (batch, component) strides of alm [nb?, nc, nelem] / map [nb?, nc, pixels...].  CUDA tensors are used in
	place whenever their inner axes are contiguous (the batch and component axes may be strided views, e.g. one spin group of
	many maps); numpy arrays and other tensors are staged contiguously (and written back for outputs)."""
	def __init__(self, arr, inner_ndim, batched, writeback, overwrite=False):
		self.buf = None
		if A.is_tensor(arr) and (arr.is_cuda or _lib.is_hostsim()):
			st = list(arr.stride()); sh = list(arr.shape)
			inner_ok = all(st[-k] == int(np.prod(sh[len(sh)-k+1:], dtype=np.int64)) for k in range(1, inner_ndim+1))
			if inner_ok:
				self.keep = arr; self.ptr = arr.data_ptr()
				self.cstride = st[-inner_ndim-1]; self.bstride = st[0] if batched else 0
				return
		self.buf = _Buf(arr, writeback=writeback, overwrite=overwrite); self.ptr = self.buf.ptr
		inner = int(np.prod(arr.shape[arr.ndim-inner_ndim:], dtype=np.int64))
		self.cstride = inner; self.bstride = inner*arr.shape[-inner_ndim-1] if batched else 0
	def finish(self):
		if self.buf is not None: self.buf.finish()

def _run_syn(plan, alm, map, spin, mode, adjoint, map_overwrite=False):
	"""alm [nca, nelem], map [ncm, ...] -- or a batch of independent maps alm [nb, nca, nelem], map [nb, ncm, ...] in ONE library call"""
	ad, md = A.np_dtype(alm), A.np_dtype(map)
	batched = alm.ndim == 3
	nb = alm.shape[0] if batched else 1
	av = _View(alm, 1, batched, bool(adjoint)); mv = _View(map, map.ndim-(2 if batched else 1), batched, not adjoint, overwrite=map_overwrite and not adjoint)
	with plan.lock:      # (the adjoint synthesis runs the Legendre analysis: the deterministic option and the call as one step)
		_apply_mode(plan)
		_lib.check(_lib.load().pxs_synthesis(plan.handle, int(spin), 1 if mode == "DERIV1" else 0, int(bool(adjoint)), int(nb),
			av.ptr, A.DT[ad], av.cstride, av.bstride, mv.ptr, A.DT[md], mv.cstride, mv.bstride, current_stream()))
	av.finish(); mv.finish()

ANALYSIS_MODES = {"ducc0": 2, "interpolant": 0, "weights": 1}
def _analysis_mode(analysis):
	"""analysis=None: PIXELL_AMD_ANALYSIS or "ducc0" (the route of ducc0's analysis_2d as published, see include/pxsht.h pxs_plan_option)"""
	if analysis is None: analysis = os.environ.get("PIXELL_AMD_ANALYSIS", "ducc0")
	if analysis not in ANALYSIS_MODES: raise ValueError("analysis must be 'ducc0', 'interpolant' or 'weights', not %r" % (analysis,))
	return ANALYSIS_MODES[analysis]

def analysis_form(geometry, ntheta, nphi, lmax, mmax=None, mstart=None, phi0=0.0, lstride=1, flip=(False, False), analysis=None):
	"""What analysis_2d does on this grid with this option (pxs_plan_query): dict(form="ducc0" (its fine-CC form) | "weights" |
	"interpolant", ncc_circle=N_cc of the Legendre-stage CC grid (0: none), ducc_ncc_circle=ducc0's own N_cc for this lmax)"""
	if mmax is None: mmax = lmax
	if mstart is None: mstart = tri_mstart(lmax, mmax)
	plan = grid_plan(geometry, ntheta, nphi, phi0, flip, lmax, mmax, mstart, lstride)
	plan.set_option("analysis", _analysis_mode(analysis))
	return dict(form={0: "interpolant", 1: "weights", 2: "ducc0"}[plan.query("analysis_form")], ncc_circle=plan.query("ncc_circle"), ducc_ncc_circle=plan.query("ducc_ncc_circle"))

def _run_ana(plan, map, alm, spin, adjoint, analysis=None, alm_dense=False):
	ad, md = A.np_dtype(alm), A.np_dtype(map)
	batched = alm.ndim == 3
	nb = alm.shape[0] if batched else 1
	av = _View(alm, 1, batched, not adjoint, overwrite=alm_dense and not adjoint); mv = _View(map, map.ndim-(2 if batched else 1), batched, bool(adjoint), overwrite=bool(adjoint))      # (a grid plan writes every pixel)
	with plan.lock:      # the options and the call they apply to, as one step: plans are cached and shared between threads
		_apply_mode(plan)
		plan.set_option("analysis", _analysis_mode(analysis))
		_lib.check(_lib.load().pxs_analysis(plan.handle, int(spin), int(bool(adjoint)), int(nb), mv.ptr, A.DT[md], mv.cstride, mv.bstride,
			av.ptr, A.DT[ad], av.cstride, av.bstride, current_stream()))
	av.finish(); mv.finish()

def _grid_args(alm, map, spin, lmax, mmax, mstart, geometry, phi0, lstride, mode, flip):
	_check_pair(alm, map, spin, mode, 2)
	if mmax is None: mmax = lmax
	if mstart is None: mstart = tri_mstart(lmax, mmax)
	nt, nph = map.shape[-2:]
	return grid_plan(geometry, nt, nph, phi0, flip, lmax, mmax, mstart, lstride)

def synthesis_2d(*, alm, map, spin, lmax, geometry, mmax=None, mstart=None, phi0=0.0, nthreads=0, lstride=1, mode="STANDARD", flip=(False, False), return_plan=False):
	"""ducc0.sht.experimental.synthesis_2d as called at curvedsky.py:907-924"""
	plan = _grid_args(alm, map, spin, lmax, mmax, mstart, geometry, phi0, lstride, mode, flip)
	_run_syn(plan, alm, map, spin, mode, False, map_overwrite=True)      # (a grid plan writes every pixel of the map)
	return plan if return_plan else map

def adjoint_synthesis_2d(*, alm, map, spin, lmax, geometry, mmax=None, mstart=None, phi0=0.0, nthreads=0, lstride=1, mode="STANDARD", flip=(False, False), return_plan=False):
	plan = _grid_args(alm, map, spin, lmax, mmax, mstart, geometry, phi0, lstride, mode, flip)
	_run_syn(plan, alm, map, spin, mode, True)
	return plan if return_plan else alm

def analysis_2d(*, alm, map, spin, lmax, geometry, mmax=None, mstart=None, phi0=0.0, nthreads=0, lstride=1, flip=(False, False), return_plan=False, analysis=None):
	"""ducc0.sht.experimental.analysis_2d as called at curvedsky.py:1032-1046.
	analysis (ours): "ducc0" (default): the route ducc0's analysis_2d takes as published -- the theta-interpolant of the rings, low-passed
	to |k| < N_cc where the grid is finer, evaluated on the CC grid of N_cc + 1 rings and integrated with that grid's weights (a CC
	grid with ntheta >= 2 lmax + 2: its own weights directly) | "interpolant": exact quadrature of the full interpolant |
	"weights": ring quadrature weights + adjoint synthesis, the reference's cyl route (curvedsky.py:852-861, 1068-1084), on grids
	with ntheta >= 2 lmax + 2.  The same alm for band-limited maps (include/pxsht.h, pxs_plan_option)."""
	plan = _grid_args(alm, map, spin, lmax, mmax, mstart, geometry, phi0, lstride, "STANDARD", flip)
	# (an alm array that is exactly the triangular layout is written in full: a host array of it need not be uploaded first)
	dense = lstride == 1 and (mmax is None or mmax == lmax) and alm.shape[-1] == (lmax+1)*(lmax+2)//2 and (mstart is None or int(np.asarray(mstart)[-1]) + lmax + 1 == alm.shape[-1])
	_run_ana(plan, map, alm, spin, False, analysis, alm_dense=dense)
	return plan if return_plan else alm

def adjoint_analysis_2d(*, alm, map, spin, lmax, geometry, mmax=None, mstart=None, phi0=0.0, nthreads=0, lstride=1, flip=(False, False), return_plan=False, analysis=None):
	plan = _grid_args(alm, map, spin, lmax, mmax, mstart, geometry, phi0, lstride, "STANDARD", flip)
	_run_ana(plan, map, alm, spin, True, analysis)
	return plan if return_plan else map

def _missing_map(alm, shape):
	"""the map a call without one returns: zeros of the real type of alm, next to it"""
	return A.zeros(shape, np.float32 if A.np_dtype(alm) == np.complex64 else np.float64, like=alm)

def _missing_alm(map, pre, lmax, mstart, lstride):
	"""the alm a call without one returns: zeros [pre..., nelem] of the layout, of the complex type of map, next to it"""
	nelem = int(np.max(np.asarray(mstart).astype(np.int64))+lmax*lstride+1)
	return A.zeros(tuple(pre)+(nelem,), np.complex64 if A.np_dtype(map) == np.float32 else np.complex128, like=map)

def _ring_args(theta, nphi, phi0, ringstart, lmax, mmax, mstart, lstride, pixstride):
	if mmax is None: mmax = lmax
	if mstart is None: mstart = tri_mstart(lmax, mmax)
	return ring_plan(theta, nphi, phi0, ringstart, lmax, mmax, mstart, lstride, pixstride), mstart

def synthesis(*, alm, theta, nphi, phi0, ringstart, lmax, mmax=None, mstart=None, spin=0, map=None, lstride=1, pixstride=1, nthreads=0, mode="STANDARD"):
	"""ducc0.sht.experimental.synthesis as called at curvedsky.py:936-960 (map[nc, npix])"""
	plan, mstart = _ring_args(theta, nphi, phi0, ringstart, lmax, mmax, mstart, lstride, pixstride)
	if map is None:
		rs_ = np.asarray(ringstart).astype(np.int64); last_ = rs_+(np.asarray(nphi).astype(np.int64)-1)*pixstride
		map = _missing_map(alm, (_ncomp(spin, mode)[1], int(max(rs_.max(), last_.max())+1)))
	_check_pair(alm, map, spin, mode, 1)
	_run_syn(plan, alm, map, spin, mode, False)
	synthesis.last_plan = plan
	return map

def adjoint_synthesis(*, map, theta, nphi, phi0, ringstart, lmax, mmax=None, mstart=None, spin=0, alm=None, lstride=1, pixstride=1, nthreads=0, mode="STANDARD"):
	"""ducc0.sht.experimental.adjoint_synthesis as called at curvedsky.py:1068-1084"""
	plan, mstart = _ring_args(theta, nphi, phi0, ringstart, lmax, mmax, mstart, lstride, pixstride)
	if alm is None: alm = _missing_alm(map, (_ncomp(spin, mode)[0],), lmax, mstart, lstride)
	_check_pair(alm, map, spin, mode, 1)
	_run_syn(plan, alm, map, spin, mode, True)
	adjoint_synthesis.last_plan = plan
	return alm

# ---- transforms at arbitrary points (pxs_plan_points; ducc0.sht.experimental.synthesis_general / adjoint_synthesis_general,
# curvedsky.py:993-1016, 1088-1120) ----------------------------------------------------------------------------------------------
EPS_MIN, EPS_MAX = 1e-13, 0.1

def points_grid_shape(lmax, mmax):
	"""(ntheta, nphi) of the Clenshaw-Curtis grid the point transforms synthesise onto: 2 ntheta - 2 and nphi/2 good FFT sizes,
	ntheta >= lmax + 2, nphi >= 2 mmax + 2"""
	g = _lib.load().pxf_fft_good_size
	return int(g(lmax+1))+1, 2*int(g(mmax+1))

def _loc_device(loc):
	"""loc [npts, 2] f64 -> (device array the library reads, npts); ValueError for theta outside [0, pi] or a non-finite phi"""
	tens = A.is_tensor(loc); xp = A.torch() if tens else np
	loc = loc.to(xp.float64).contiguous() if tens else np.ascontiguousarray(loc, dtype=np.float64)
	if loc.ndim != 2 or loc.shape[1] != 2: raise ValueError("loc must have shape [npts, 2]")
	if loc.shape[0] and not bool(((loc[:, 0] >= 0) & (loc[:, 0] <= np.pi) & xp.isfinite(loc[:, 1])).all()):
		raise ValueError("loc: theta must lie in [0, pi] and phi be finite")
	if _lib.is_hostsim() or (tens and loc.is_cuda): return loc, loc.shape[0]
	return A.to_gpu(loc), loc.shape[0]

def points_plan(loc, lmax, mmax=None, mstart=None, lstride=1, epsilon=1e-10):
	"""a pxs_plan of the points loc [npts, 2] (theta, phi) on the cached CC grid plan of (lmax, mmax, layout); not cached itself"""
	if mmax is None: mmax = lmax
	if mstart is None: mstart = tri_mstart(lmax, mmax)
	epsilon = float(epsilon)
	if not (EPS_MIN <= epsilon <= EPS_MAX): raise ValueError("epsilon must lie in [%g, %g], got %g" % (EPS_MIN, EPS_MAX, epsilon))
	nt, nph = points_grid_shape(lmax, mmax)
	grid = grid_plan("CC", nt, nph, 0.0, (False, False), lmax, mmax, mstart, lstride)
	dloc, npts = _loc_device(loc)
	h = ctypes.c_void_p()
	_lib.check(_lib.load().pxs_plan_points(ctypes.byref(h), grid.handle, int(npts), A.ptr(dloc) if npts else None, epsilon, device_index(), current_stream()))
	p = Plan(h); p.grid = grid; p.npts = int(npts)
	return p

def points_profile(plan, enable=True):
	"""stage timers of a point plan (pxs_plan_option "profile"): enable resets them"""
	plan.set_option("profile", int(bool(enable)))

def points_profile_read(plan):
	"""{stage: ms} summed over the calls since points_profile(plan): cc_sht (CC synthesis / its adjoint), fft (2-D FFTs), grid (doubling,
	fold, padding, truncation), interp, spread (spreading + slab gather); plan: host wall time of making the plan"""
	out = {k: plan.query("stage_us_"+k)*1e-3 for k in ("cc_sht", "fft", "grid", "interp", "spread")}
	out["plan"] = plan.query("plan_us")*1e-3
	return out

def _default_eps(epsilon, map_dtype):
	if epsilon is not None: return epsilon
	return 1e-6 if np.dtype(map_dtype) == np.float32 else 1e-10

def _run_points(plan, alm, map, spin, mode, adjoint):
	with plan.grid.lock:      # the grid plan's deterministic option applies to the Legendre stage of this call
		_apply_mode(plan.grid)
		_run_syn(plan, alm, map, spin, mode, adjoint, map_overwrite=True)

def _use_plan(plan, loc, lmax, mmax, mstart, lstride, epsilon, map_dtype):
	"""the point plan of a call: the caller's (made by points_plan for the same loc, band limit, layout and epsilon: the binning and sort
	of the points are then shared by several calls, e.g. the spin groups of one alm2map_pos) or a new one"""
	if plan is not None:
		if plan.npts != int(loc.shape[0]): raise ValueError("plan was made for %d points, loc has %d" % (plan.npts, int(loc.shape[0])))
		return plan
	return points_plan(loc, lmax, mmax, mstart, lstride, _default_eps(epsilon, map_dtype))

def synthesis_general(*, alm, loc, spin, lmax, mmax=None, mstart=None, lstride=1, epsilon=None, mode="STANDARD", map=None, nthreads=0, plan=None):
	"""ducc0.sht.experimental.synthesis_general as called at curvedsky.py:1004, 1098: alm [nca, nelem] (or a batch [nb, nca, nelem]) ->
	map [ncm, npts] (or [nb, ncm, npts]) at loc [npts, 2] = (theta, phi).  numpy in, numpy out; a CUDA tensor stays on its device.
	epsilon: relative L2 accuracy (default 1e-10 for float64 maps, 1e-6 for float32), within [1e-13, 0.1].
	plan (ours): a points_plan of these points to reuse (its epsilon and layout apply)."""
	npts = int(loc.shape[0])
	if map is None: map = _missing_map(alm, tuple(alm.shape[:-2])+(_ncomp(spin, mode)[1], npts))
	_check_pair(alm, map, spin, mode, 1)
	if map.shape[-1] != npts: raise ValueError("map has %d points, loc %d" % (map.shape[-1], npts))
	plan = _use_plan(plan, loc, lmax, mmax, mstart, lstride, epsilon, A.np_dtype(map))
	if npts == 0: return map
	_run_points(plan, alm, map, spin, mode, False)
	return map

def adjoint_synthesis_general(*, map, loc, spin, lmax, mmax=None, mstart=None, lstride=1, epsilon=None, mode="STANDARD", alm=None, nthreads=0, plan=None):
	"""ducc0.sht.experimental.adjoint_synthesis_general as called at curvedsky.py:1104-1115: the exact transpose of synthesis_general,
	map [ncm, npts] -> alm [nca, nelem] (overwritten; allocated when None)"""
	if mmax is None: mmax = lmax
	if mstart is None: mstart = tri_mstart(lmax, mmax)
	npts = int(loc.shape[0])
	if alm is None: alm = _missing_alm(map, tuple(map.shape[:-2])+(_ncomp(spin, mode)[0],), lmax, mstart, lstride)
	_check_pair(alm, map, spin, mode, 1)
	if map.shape[-1] != npts: raise ValueError("map has %d points, loc %d" % (map.shape[-1], npts))
	plan = _use_plan(plan, loc, lmax, mmax, mstart, lstride, epsilon, A.np_dtype(map))
	if npts == 0:      # (no map to read: the transpose of an empty synthesis is zero)
		alm[...] = 0
		return alm
	_run_points(plan, alm, map, spin, mode, True)
	return alm


_gridweights_cache = {}
def rotate_alm(alm, lmax, psi, theta, phi, nthreads=1):
	"""ducc0.sht.rotate_alm as called at curvedsky.py:731: alm[nelem] (or [ncomp, nelem]) of lmax in the triangular layout, rotated
	by the zyz Euler angles psi, theta, phi; returns a new array (numpy in, numpy out; a CUDA tensor stays on its device).
	nthreads is accepted and ignored."""
	from . import almops
	return almops.rotate_alm(alm, lmax, psi, theta, phi, inplace=False)

def get_gridweights(geometry, ntheta):
	"""ducc0.sht.experimental.get_gridweights (curvedsky.py:501, 855); sum = 4 pi.  The last few results are kept: quad_weights asks
	for the same grid on every map2alm of a declination band"""
	key = (str(geometry), int(ntheta))
	out = _gridweights_cache.get(key)
	if out is None:
		out = np.zeros(int(ntheta), np.float64)
		_lib.check(_lib.load().pxs_gridweights(geometry.encode(), int(ntheta), out.ctypes.data))
		if len(_gridweights_cache) >= 8: _gridweights_cache.pop(next(iter(_gridweights_cache)))
		_gridweights_cache[key] = out
	return out.copy()

def grid_maxlmax(geometry, ntheta):
	return int(_lib.load().pxs_grid_maxlmax(geometry.encode(), int(ntheta)))
