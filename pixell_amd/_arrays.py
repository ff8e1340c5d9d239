"""The one place that knows numpy arrays from torch tensors from the simulator.

Every module above the C ABI takes numpy arrays (staged through device memory), torch CUDA tensors (used where they are) and dmaps
(a tensor with a geometry); the simulator build of the library (tests only) reads host pointers, so there numpy arrays stay numpy and
tensors live on the host.  What an array is, where the library reads it and what comes back to the caller is decided here and nowhere
else.  A leaf module: numpy and the loader only."""
import ctypes
import numpy as np
from . import _lib

DT = {np.dtype(np.float32): 0, np.dtype(np.float64): 1, np.dtype(np.complex64): 2, np.dtype(np.complex128): 3}      # the dtype codes of the C ABI

def torch():
	import torch
	return torch

def is_tensor(x):
	return type(x).__module__.startswith("torch")

def unwrap(x):
	"""the tensor of a dmap / dmaps, anything else as it is"""
	return x.tensor if hasattr(x, "tensor") and not is_tensor(x) else x

def np_dtype(x):
	"""the numpy dtype of an array or tensor of any kind"""
	return np.dtype(str(x.dtype).replace("torch.", "")) if is_tensor(x) else np.dtype(x.dtype)

def tdtype(dtype):
	"""the torch dtype of a numpy dtype"""
	return getattr(torch(), np.dtype(dtype).name)

_cuda_ready = False
def device_index():
	if _lib.is_hostsim(): return 0
	t = torch()
	if not t.cuda.is_available():
		raise RuntimeError("pixell_amd needs a ROCm GPU (torch.cuda.is_available() is False); there is no CPU fallback")
	global _cuda_ready
	if not _cuda_ready:
		# make torch create its HIP context before libpxsht.so makes its first runtime call: a process whose first HIP
		# call came from the library (numpy-only callers) got "no ROCm-capable device" from hipSetDevice on the GPU box
		t.cuda.init(); t.zeros(1, device="cuda"); _cuda_ready = True
	return t.cuda.current_device()

def current_stream():
	if _lib.is_hostsim(): return None
	return ctypes.c_void_p(torch().cuda.current_stream().cuda_stream)

def require_gpu(t):
	"""a tensor the library is to read must be on the GPU (anywhere in the simulator)"""
	if not t.is_cuda and not _lib.is_hostsim(): raise ValueError("torch tensors passed to pixell_amd must live on the GPU")
	return t

def ptr(x):
	"""the address the library gets for x (None for None)"""
	x = unwrap(x)
	return None if x is None else (x.data_ptr() if is_tensor(x) else x.ctypes.data)

def device_of(*arrs):
	"""the torch device of the first tensor / dmap among arrs (None: everything lives on the host)"""
	for a in arrs:
		a = unwrap(a)
		if a is not None and is_tensor(a): return require_gpu(a).device
	return None

def is_contiguous(x):
	return x.is_contiguous() if is_tensor(x) else x.flags["C_CONTIGUOUS"]

def astype(x, dtype):
	if np_dtype(x) == np.dtype(dtype): return x
	return x.to(tdtype(dtype)) if is_tensor(x) else np.asarray(x).astype(dtype)

def host(x):
	"""x as a numpy array"""
	x = unwrap(x)
	return x.detach().cpu().numpy() if is_tensor(x) else np.asarray(x)

def to_gpu(x):
	"""a contiguous numpy array or a host tensor -> a tensor on the current GPU"""
	device_index()
	return (x if is_tensor(x) else torch().from_numpy(x)).cuda()

def put(x, dtype=None, device=None):
	"""x as a contiguous array of dtype (None: its own) where the library reads it: tensors on `device` (None: their own), numpy
	arrays as tensors on `device` (None: the current GPU; in the simulator they stay numpy)"""
	x = unwrap(x)
	if is_tensor(x):
		return require_gpu(x).to(device=device if device is not None else x.device, dtype=x.dtype if dtype is None else tdtype(dtype)).contiguous()
	x = np.ascontiguousarray(x, dtype=dtype)
	if device is not None: return torch().from_numpy(x).to(device)
	return x if _lib.is_hostsim() else to_gpu(x)

def _new(make, shape, dtype, like, device):
	if like is not None:
		like = unwrap(like)
		if not is_tensor(like): return getattr(np, make)(tuple(shape), dtype)
		device = like.device
	elif device is None:
		if _lib.is_hostsim(): return getattr(np, make)(tuple(shape), dtype)
		device_index(); device = "cuda"
	return getattr(torch(), make)(tuple(shape), dtype=tdtype(dtype), device=device)

def empty(shape, dtype, like=None, device=None):
	"""an uninitialised array of the kind `like` is (a tensor next to it, or numpy); without `like`, where the library writes: a tensor
	on `device` (None: the current GPU; numpy in the simulator)"""
	return _new("empty", shape, dtype, like, device)

def zeros(shape, dtype, like=None, device=None):
	return _new("zeros", shape, dtype, like, device)

def out_array(given, shape, dtypes, device, name, layout):
	"""the array a kernel writes for the caller's output array `given` (a dmap, tensor or numpy array of one of `dtypes`, of `shape`,
	C-contiguous): itself where the library can write it, a staged copy otherwise (result() brings it back)"""
	data = unwrap(given)
	if np_dtype(data) not in dtypes: raise ValueError("%s must be %s" % (name, " or ".join(np.dtype(t).name for t in dtypes)))
	if tuple(data.shape) != tuple(shape): raise ValueError("%s must be %s" % (name, layout))
	if not is_contiguous(data): raise ValueError("%s must be C-contiguous" % name)
	return put(data, None, device)

def result(work, given):
	"""after the kernel: `given` with what was written into its staged copy `work` (nothing to do when they are one array)"""
	data = unwrap(given)
	if ptr(work) != ptr(data): data[...] = (work if is_tensor(data) else host(work)).reshape(data.shape)
	return given
