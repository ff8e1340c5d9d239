"""Spline interpolation of maps at arbitrary positions on the device: the reference's utils.interpol / utils.interpolator /
SplineInterpolator (pixell/utils.py:630-783), which sit under enmap.at and enmap.project.

SplineInterpolator is scipy.ndimage.spline_filter(arr[I], order, mode=border) followed by scipy.ndimage.map_coordinates(...,
prefilter=False) there; here the filter is pxm_spline_filter (a chunked recursion along both axes, FP64) and the evaluation pxm_interpol,
one lane per point (csrc/interpol.hip).  The kernel computes pixel coordinates itself from a per-axis affine map, so enmap.at from sky
coordinates and enmap.project between two separable geometries read no coordinate array they were not given.  Orders 0, 1 and 3 over the
last two axes of an array; borders "nearest", "mirror", "constant", "wrap" (scipy's legacy rule, as the reference inherits it) and
"grid-wrap" (a true period of n samples: what an RA axis that goes round the sky wants).

Numpy in gives numpy out; CUDA tensors or a dmap in give tensors out on that device.  The result has the map's dtype for orders 0 and 1
(integer maps become float64 at order 1) and is float64 at order 3, as the filtered array is.  Orders 2, 4, 5 and mode="fourier" raise
NotImplementedError."""
import numpy as np
from . import _lib, _arrays as A

CHUNK = (256, 256)      # samples per workgroup along (y, x) in the filter's passes (csrc/interpol.hip CHUNK): the tests size their cases from it
BORDERS = {"nearest": 0, "mirror": 1, "constant": 2, "wrap": 3, "grid-wrap": 4}      # the border codes of pxm_interpol
_EXTENSION = {"nearest": 1, "mirror": 0, "constant": 0, "wrap": 0, "grid-wrap": 2}   # what the prefilter inverts: 0 mirror, 1 reflect, 2 periodic
_F32, _F64 = np.dtype(np.float32), np.dtype(np.float64)
_DT = {_F32: 0, _F64: 1, np.dtype(np.uint8): 4, np.dtype(np.int32): 5}
IDENTITY = ((0.0, 1.0), (0.0, 1.0))      # the affine map (off, scale) per axis of positions given in pixels
NO_REWIND = ((0.0, 0.0), (0.0, 0.0))     # (ref, per) per axis: per <= 0 skips the rewind

def _ip_get_mode(mode, order):
	"""(mode, order) with the aliases of utils._ip_get_mode (utils.py:760-767)"""
	if   mode in ["nn", "nearest"]: mode, order = "spline", 0
	elif mode in ["lin", "linear"]: mode, order = "spline", 1
	elif mode in ["cub", "cubic"]: mode, order = "spline", 3
	elif mode in ["fft", "nufft", "fourier"]: mode = "fourier"
	if mode not in ["spline", "fourier"]: raise ValueError("Unrecognized interpol mode '%s'" % str(mode))
	if mode == "fourier": raise NotImplementedError("fourier interpolation is not implemented on the device")
	if order not in (0, 1, 3): raise NotImplementedError("spline interpolation of order %s is not implemented on the device (orders 0, 1, 3)" % str(order))
	return mode, int(order)

def _check_border(border):
	"""a border name, or a pair of them (y, x): what reproject.thumbnails reads a map that goes round the sky with"""
	if isinstance(border, (tuple, list)):
		if len(border) != 2: raise ValueError("a border per axis is a pair (y, x)")
		return tuple(_check_border(b) for b in border)
	if border not in BORDERS: raise ValueError("Unrecognized border '%s'" % str(border))
	return border

def _raw(x):
	"""the tensor of a dmap, a tensor as it is, anything else as a plain numpy array"""
	x = A.unwrap(x)
	return x if A.is_tensor(x) else np.asarray(x)

def _filter(d, border):
	"""the cubic B-spline coefficients (float64) of the contiguous float32 / float64 array d [..., ny, nx], lying where the library reads
	it, as an array next to it"""
	ny, nx = int(d.shape[-2]), int(d.shape[-1])
	nmap = int(np.prod(d.shape[:-2], dtype=np.int64))
	tmp, out = A.empty(d.shape, np.float64, like=d), A.empty(d.shape, np.float64, like=d)
	if isinstance(border, tuple):
		_lib.check(_lib.load().pxm_spline_filter_axes(nmap, ny, nx, A.ptr(d), _DT[A.np_dtype(d)], ny*nx, A.ptr(tmp), A.ptr(out), _EXTENSION[border[0]],
			_EXTENSION[border[1]], A.device_index(), A.current_stream()))
		return out
	_lib.check(_lib.load().pxm_spline_filter(nmap, ny, nx, A.ptr(d), _DT[A.np_dtype(d)], ny*nx, A.ptr(tmp), A.ptr(out), _EXTENSION[border],
		A.device_index(), A.current_stream()))
	return out

def _as_kind(work, device):
	"""what the caller gets: a numpy array for host inputs, a tensor on `device` otherwise"""
	if device is None: return A.host(work)
	return work if A.is_tensor(work) else A.torch().from_numpy(work).to(device)

def spline_filter(arr, order=3, border="nearest"):
	"""The B-spline coefficients of arr [..., ny, nx] over its last two axes, float64: scipy.ndimage.spline_filter(arr[I], order,
	mode=border) for every leading index I.  Orders 0 and 1 have no filter: a float64 copy.  A map comes back as a map.  border may be
	a pair (y, x): each axis is then filtered under its own border's extension."""
	_, order = _ip_get_mode("spline", order); border = _check_border(border)
	data = _raw(arr)
	if data.ndim < 2: raise ValueError("spline_filter needs at least two axes")
	device = A.device_of(data)
	d = A.put(data, _F32 if A.np_dtype(data) == _F32 and order > 1 else _F64, device)
	if order > 1: res = _filter(d, border)
	else: res = d.clone() if A.is_tensor(d) else np.array(d)
	res = _as_kind(res, device)
	return type(arr)(res, arr.wcs) if hasattr(arr, "wcs") else res

class SplineInterpolator:
	"""arr [{pre}, ny, nx] prepared for interpolation at many sets of positions: utils.SplineInterpolator (utils.py:696-720).  The
	prefilter (order 3) runs once, here; every call is one launch.  border: a name, or a pair (y, x) for reproject.thumbnails."""
	prefiltered = True
	def __init__(self, arr, npre=0, mode="spline", border="nearest", order=3, cval=0.0):
		self.mode, self.order = _ip_get_mode(mode, order)
		self.border, self.cval = _check_border(border), float(cval)
		data = _raw(arr)
		if data.ndim < 2: raise ValueError("interpolation needs an array of at least two axes")
		self.npre = npre % data.ndim
		if data.ndim-self.npre != 2: raise NotImplementedError("only the last two axes of an array can be interpolated on the device")
		self.device = A.device_of(data)      # None: the caller's array is a numpy array
		dt = A.np_dtype(data)
		if self.order != 0:
			if dt not in (_F32, _F64): dt = _F64      # (utils.asfarray)
		elif dt == np.dtype(bool): dt = np.dtype(np.uint8)
		elif dt not in _DT: raise ValueError("order 0 reads float32, float64, uint8, int32 and bool maps, not %s" % dt.name)
		d = A.put(data, dt, self.device)
		self.arr = _filter(d, self.border) if self.order > 1 else d
	def __call__(self, inds, out=None):
		"""the values at inds [{y,x}, ...] in pixels: [{pre}, ...]"""
		inds = A.unwrap(inds)
		if not A.is_tensor(inds): inds = np.asarray(inds, np.float64)
		if inds.ndim < 1 or inds.shape[0] != 2: raise ValueError("arr.ndim-len(inds) != npre")
		return self.evaluate(tuple(inds.shape[1:]), pts=inds, out=out)
	def evaluate(self, oshape, pts=None, affine=IDENTITY, rewind=NO_REWIND, out=None):
		"""The values [{pre}, oshape] at the points pts [2, oshape] or, without pts, at the pixels of a grid oshape = (ony, onx).  A
		point's pixel coordinate on axis a is affine[a][0] + affine[a][1]*p, rewound into rewind[a][1] pixels around rewind[a][0] where
		that period is positive.  out: an array of the result's shape and dtype to fill."""
		if isinstance(self.border, tuple): raise NotImplementedError("an interpolator with a border per axis is read by reproject.thumbnails only")
		oshape = tuple(int(n) for n in oshape)
		pre = tuple(self.arr.shape[:self.npre]); ny, nx = int(self.arr.shape[-2]), int(self.arr.shape[-1])
		nmap, npts = int(np.prod(pre, dtype=np.int64)), int(np.prod(oshape, dtype=np.int64))
		device = self.device if self.device is not None else A.device_of(pts, out)
		where = A.device_of(self.arr)      # (where the library reads: None in the simulator)
		dt = A.np_dtype(self.arr)
		if out is None: work = A.empty(pre+oshape, dt, like=self.arr)
		else: work = A.out_array(out, pre+oshape, (dt,), where, "out", "[{pre}, ...] as the positions")
		d_pts, ony, onx = None, 0, 1
		if pts is not None: d_pts = A.put(pts.reshape(2, -1), np.float64, where)
		elif len(oshape) != 2: raise ValueError("a grid of points is [ony, onx]")
		else: ony, onx = oshape[0], max(oshape[1], 1)
		(yoff, yscale), (xoff, xscale) = affine; (yref, yper), (xref, xper) = rewind
		_lib.check(_lib.load().pxm_interpol(nmap, ny, nx, A.ptr(self.arr), _DT[dt], ny*nx, npts, A.ptr(d_pts), ony, onx,
			float(yoff), float(yscale), float(xoff), float(xscale), float(yref), float(yper), float(xref), float(xper),
			self.order, BORDERS[self.border], self.cval, A.ptr(work), A.device_index(), A.current_stream()))
		if out is not None: return A.result(work, out)
		return _as_kind(work, device)

def interpolator(arr, npre=0, mode="spline", border="nearest", order=3, cval=0.0):
	"""An object that interpolates arr at many sets of positions: utils.interpolator (utils.py:681-694)"""
	mode, order = _ip_get_mode(mode, order)
	return SplineInterpolator(arr, npre=npre, mode=mode, border=border, order=order, cval=cval)

def interpol(arr, inds, out=None, mode="spline", border="nearest", order=3, cval=0.0, ip=None):
	"""The values of arr [{pre}, ny, nx] at the float pixel positions inds [{y,x}, ...]: [{pre}, ...] (utils.interpol, utils.py:630-679).
	mode "nn" / "lin" / "cub" or ("spline", order 0 / 1 / 3); border "nearest", "wrap", "mirror", "constant" (cval) or "grid-wrap";
	ip: an interpolator(...) of arr to use again (mode, border, order and cval are then its own)."""
	if ip is None:
		nd = 1 if _raw(inds).ndim == 0 else len(inds)
		ip = interpolator(arr, _raw(arr).ndim-nd, mode=mode, border=border, order=order, cval=cval)
	return ip(inds, out=out)
