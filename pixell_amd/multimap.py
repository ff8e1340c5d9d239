"""A list of maps of different geometries handled as one array (the container of pixell.multimap, with its layout): one array
[..., ntot] holds the maps' pixels concatenated along the last axis, a tuple of geometries beside it says how to cut it.  Wavelet
coefficients (pixell_amd.wavelets) are the main user: arithmetic acts on every scale at once, `.maps[i]` is scale i as a map.

ndmaps is the numpy container; dmaps is its device counterpart around a torch CUDA tensor, as enmap.dmap is to enmap.ndmap: nothing
leaves HBM until `.to_host()`.  The per-map reductions (mean, var, std, min, max) return host arrays [nmap, pre...] for both.
I/O, the position / l tables and the FFT wrappers of the reference's module are not here."""
import numpy as np
from . import enmap, _arrays as A

class Geometry:
	"""(shape, wcs) of one map; unpacks like the pair it stands for"""
	def __init__(self, shape, wcs=None):
		if wcs is None and hasattr(shape, "wcs"): shape, wcs = shape.shape, shape.wcs
		if wcs is None: raise ValueError("Geometry needs a shape and a wcs, or an object with both")
		self.shape, self.wcs = tuple(int(n) for n in shape), wcs
	@property
	def npix(self): return self.shape[-2]*self.shape[-1]
	@property
	def nopre(self): return Geometry(self.shape[-2:], self.wcs)
	def __len__(self): return 2
	def __iter__(self): yield self.shape; yield self.wcs
	def __repr__(self): return "Geometry(%s,%s)" % (str(self.shape), str(self.wcs))

def nopre(geometries):
	"""the geometries without their leading dimensions"""
	return tuple(Geometry(*geo).nopre for geo in geometries)

def _offsets(geometries): return np.concatenate([[0], np.cumsum([geo.npix for geo in geometries])]).astype(int)

class _Common:
	"""what ndmaps and dmaps share: the bookkeeping around an array [..., ntot] and self.geometries"""
	@property
	def pre(self): return tuple(self.shape[:-1])
	@property
	def npixs(self): return [geo.npix for geo in self.geometries]
	@property
	def ntot(self): return int(np.sum(self.npixs))
	@property
	def nmap(self): return len(self.geometries)
	@property
	def maps(self): return _map_view(self)

class ndmaps(_Common, np.ndarray):
	"""numpy array [..., ntot] + geometries"""
	def __new__(cls, arr, geometries):
		obj = np.asarray(arr).view(cls)
		obj.geometries = nopre(geometries)
		return obj
	def __array_finalize__(self, obj):
		if obj is None: return
		self.geometries = getattr(obj, "geometries", None)
	def __repr__(self): return "ndmaps(%s,%s)" % (np.asarray(self), str(self.geometries))
	def __str__(self): return repr(self)
	def copy(self, order="K"): return ndmaps(np.copy(self, order), self.geometries)
	def contig(self): return ndmaps(np.ascontiguousarray(self), self.geometries)

class dmaps(_Common):
	"""device-resident multimap: a torch CUDA tensor [..., ntot] + geometries.  Arithmetic with scalars, tensors, dmaps and (host)
	arrays that broadcast; `.maps[i]` are enmap.dmap views of the tensor."""
	def __init__(self, tensor, geometries): self.tensor = tensor; self.geometries = nopre(geometries)
	@property
	def shape(self): return tuple(self.tensor.shape)
	@property
	def ndim(self): return self.tensor.ndim
	@property
	def dtype(self): return A.np_dtype(self.tensor)
	def copy(self): return dmaps(self.tensor.clone(), self.geometries)
	def contig(self): return dmaps(self.tensor.contiguous(), self.geometries)
	def to_host(self): return ndmaps(self.tensor.cpu().numpy(), self.geometries)
	def __repr__(self): return "dmaps(%s,%s)" % (str(self.tensor), str(self.geometries))
	def __getitem__(self, sel):
		"""indexing the leading axes keeps the geometries; anything that touches the pixel axis returns the bare tensor"""
		res = self.tensor[sel]
		s = sel if isinstance(sel, tuple) else (sel,)
		keeps = res.ndim >= 1 and res.shape[-1] == self.shape[-1] and not any(x is Ellipsis for x in s) and len([x for x in s if x is not None]) < self.ndim
		return dmaps(res, self.geometries) if keeps else res
	def __setitem__(self, sel, val): self.tensor[sel] = _operand(val, self.tensor)
	def _bin(self, other, op, reverse=False):
		o = _operand(other, self.tensor)
		if o is NotImplemented: return NotImplemented
		return dmaps(op(o, self.tensor) if reverse else op(self.tensor, o), self.geometries)
	def _ibin(self, other, op):
		o = _operand(other, self.tensor)
		if o is NotImplemented: return NotImplemented
		op(self.tensor, o); return self
	def __neg__(self): return dmaps(-self.tensor, self.geometries)
	def __pos__(self): return self
	def __abs__(self): return dmaps(abs(self.tensor), self.geometries)

def _operand(x, like):
	"""the other side of an operator as something torch can combine with the tensor `like`"""
	if isinstance(x, dmaps) or isinstance(x, enmap.dmap): return x.tensor
	if A.is_tensor(x) or isinstance(x, (int, float, complex, bool, np.number)): return x
	if isinstance(x, (np.ndarray, list, tuple)): return A.torch().as_tensor(np.ascontiguousarray(x), device=like.device)
	return NotImplemented

import operator as _op
for _name, _fn in [("add", _op.add), ("sub", _op.sub), ("mul", _op.mul), ("truediv", _op.truediv), ("pow", _op.pow)]:
	setattr(dmaps, "__%s__" % _name, (lambda fn: lambda self, other: self._bin(other, fn))(_fn))
	setattr(dmaps, "__r%s__" % _name, (lambda fn: lambda self, other: self._bin(other, fn, reverse=True))(_fn))
for _name, _fn in [("iadd", lambda a, b: a.add_(b)), ("isub", lambda a, b: a.sub_(b)), ("imul", lambda a, b: a.mul_(b)), ("itruediv", lambda a, b: a.div_(b))]:
	setattr(dmaps, "__%s__" % _name, (lambda fn: lambda self, other: self._ibin(other, fn))(_fn))

class _map_view:
	"""`.maps` of a multimap: item i is map i ([pre..., ny, nx], sharing memory), assignable"""
	def __init__(self, mmap):
		self.mmap = mmap; self.offs = _offsets(mmap.geometries)
	def __len__(self): return self.mmap.nmap
	def __iter__(self): return (self[i] for i in range(len(self)))
	def _split(self, sel):
		sel = sel if isinstance(sel, tuple) else (sel,)
		i = int(sel[0])
		if i < 0: i += len(self)
		if not 0 <= i < len(self): raise IndexError("map index out of range")
		return i, sel[1:]
	def _flat(self, i):
		data = self.mmap.tensor if isinstance(self.mmap, dmaps) else np.asarray(self.mmap)
		return data[..., self.offs[i]:self.offs[i+1]]
	def __getitem__(self, sel):
		i, rest = self._split(sel)
		geo = self.mmap.geometries[i]; flat = self._flat(i); shape = self.mmap.pre+geo.shape[-2:]
		if isinstance(self.mmap, dmaps): m = enmap.dmap(flat.unflatten(-1, geo.shape[-2:]), geo.wcs)          # (a view)
		else:
			v = flat.view(); v.shape = shape           # (never a copy: assignments through the result must reach the multimap)
			m = enmap.ndmap(v, geo.wcs)
		return m[rest] if rest else m
	def __setitem__(self, sel, val):
		i, rest = self._split(sel)
		m = self[i]
		if isinstance(val, enmap.dmap): val = val.tensor
		if isinstance(self.mmap, dmaps):
			m.tensor[rest if rest else Ellipsis] = _operand(val, m.tensor)
		else:
			if A.is_tensor(val): val = val.cpu().numpy()
			np.asarray(m)[rest if rest else Ellipsis] = val

def _geo_helper(geometries):
	geometries = [Geometry(*geo) for geo in geometries]
	for i, geo in enumerate(geometries):
		if geo.shape[:-2] != geometries[0].shape[:-2]:
			raise ValueError("Geometry %d has pre-shape %s, incompatible with geometry 0 with %s" % (i, str(geo.shape[:-2]), str(geometries[0].shape[:-2])))
	return geometries, int(sum(geo.npix for geo in geometries))

def _new(geometries, dtype, device, make):
	"""make(shape, dtype) on the host, its torch namesake on `device` (a torch device, or True for the current GPU)"""
	geometries, ntot = _geo_helper(geometries)
	shape = (geometries[0].shape[:-2] if geometries else ())+(ntot,)
	if device is None or device is False: return ndmaps(getattr(np, make)(shape, dtype), geometries)
	dev = "cuda" if device is True else device
	return dmaps(getattr(A.torch(), make)(shape, dtype=A.tdtype(dtype), device=dev), geometries)

def zeros(geometries, dtype=np.float64, device=None):
	"""zero-initialised multimap of the given geometries [(shape, wcs), ...] (the shapes may carry common leading dimensions);
	device: None = numpy ndmaps, True or a torch device = dmaps there"""
	return _new(geometries, dtype, device, "zeros")
def empty(geometries, dtype=np.float64, device=None):
	"""uninitialised multimap"""
	return _new(geometries, dtype, device, "empty")
def full(geometries, val, dtype=None, device=None):
	"""multimap filled with val: a scalar, or an array that broadcasts with pre + (nmap,) to give every map its own constant"""
	val = np.asarray(val)
	geos, _ = _geo_helper(geometries)
	if len(geos) == 0: return empty(geometries, val.dtype if dtype is None else dtype, device)
	pre = geos[0].shape[:-2]; nmap = len(geos)
	val = np.broadcast_to(val, np.broadcast_shapes(val.shape, pre+(nmap,)))
	res = empty([(val.shape[:-1]+geo.shape[-2:], geo.wcs) for geo in geos], val.dtype if dtype is None else dtype, device)
	for i in range(nmap): res.maps[i] = val[..., i][..., None, None]
	return res

def multimap(maps):
	"""the multimap of a list of maps (ndmaps for enmap.ndmap, dmaps for enmap.dmap) with common leading dimensions"""
	if len(maps) == 0: return ndmaps(np.zeros(0), [])
	for i, m in enumerate(maps):
		if tuple(m.shape[:-2]) != tuple(maps[0].shape[:-2]):
			raise ValueError("Map %d in multimaps constructor has pre-shape %s, incompatible with map 0 with %s" % (i, str(m.shape[:-2]), str(maps[0].shape[:-2])))
	geos = [(m.shape, m.wcs) for m in maps]
	if isinstance(maps[0], enmap.dmap):
		return dmaps(A.torch().cat([m.tensor.reshape(m.shape[:-2]+(-1,)) for m in maps], -1), geos)
	return ndmaps(np.concatenate([np.asarray(m).reshape(m.shape[:-2]+(-1,)) for m in maps], -1), geos)

def samegeos(arr, *args):
	"""arr with the geometries of the first multimap among args (sharing arr's memory where possible); arr itself if there is none"""
	for m in args:
		geos = getattr(m, "geometries", None)
		if geos is not None: return dmaps(arr, geos) if A.is_tensor(arr) else ndmaps(arr, geos)
	return arr

def _reduce(mmap, host_fn, dev_fn):
	if isinstance(mmap, dmaps): return np.array([dev_fn(m.tensor).cpu().numpy() for m in mmap.maps])
	return np.array([host_fn(np.asarray(m), (-2, -1)) for m in mmap.maps])

def mean(mmap):
	"""mean over the pixels of every map: host array [nmap, pre...]"""
	return _reduce(mmap, np.mean, lambda t: t.mean((-2, -1)))
def var(mmap):
	"""variance over the pixels of every map (population variance, as numpy's)"""
	return _reduce(mmap, np.var, lambda t: t.var((-2, -1), unbiased=False))
def std(mmap):
	return _reduce(mmap, np.std, lambda t: t.std((-2, -1), unbiased=False))
def min(mmap):
	return _reduce(mmap, np.min, lambda t: t.amin((-2, -1)))
def max(mmap):
	return _reduce(mmap, np.max, lambda t: t.amax((-2, -1)))
