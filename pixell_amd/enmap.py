"""The few pieces of pixell.enmap the harmonic-transform path touches (host bookkeeping),
plus enmap.fft / enmap.ifft running on the HIP FFT engine.

Mirrors: ndmap (enmap.py:33-163), fullsky_geometry (enmap.py:1713-1740), spin_helper
(enmap.py:3378-3388), area_cyl / pixsize (enmap.py:1032-1036, 1097-1099), fft / ifft
(enmap.py:1307-1337)."""
import threading
import numpy as np
from . import wcs as wcsutils, fft as enfft, _lib, _arrays as A
from .wcs import CarWCS

degree = np.pi/180

class ndmap(np.ndarray):
	"""numpy array + wcs (enmap.ndmap, enmap.py:33)"""
	def __new__(cls, arr, wcs):
		obj = np.asarray(arr).view(cls)
		obj.wcs = wcs
		return obj
	def __array_finalize__(self, obj):
		if obj is None: return
		self.wcs = getattr(obj, "wcs", None)
	def copy(self, order="C"): return ndmap(np.copy(self, order), self.wcs)
	def __getitem__(self, sel):
		"""slicing the two pixel axes moves the wcs with the data (enmap.ndmap.__getitem__, enmap.py:140-163); anything that
		removes or fancy-indexes a pixel axis returns a plain array, which has no geometry"""
		res = np.ndarray.__getitem__(self, sel)
		return _sliced(self, res, sel)
	@property
	def geometry(self): return self.shape, self.wcs
	def pixsize(self): return pixsize(self.shape, self.wcs)
	def area(self): return area(self.shape, self.wcs)

class dmap:
	"""device-resident map: a torch CUDA tensor + wcs, accepted wherever an ndmap is"""
	def __init__(self, tensor, wcs): self.tensor = tensor; self.wcs = wcs
	@property
	def shape(self): return tuple(self.tensor.shape)
	@property
	def ndim(self): return self.tensor.ndim
	@property
	def dtype(self):
		return np.dtype(str(self.tensor.dtype).replace("torch.", ""))      # (any dtype: domains and masks are maps too)
	def __getitem__(self, sel):
		res = _sliced(self, self.tensor[sel], sel)
		if not isinstance(res, dmap): raise IndexError("indexing a pixel axis of a dmap leaves no map geometry: slice the tensor itself")
		return res
	def copy(self):
		"""a dmap of a clone of the tensor, which keeps the strides of a dense permuted tensor (torch.clone preserves the memory format):
		code that computes addresses from the copy asks for a C-contiguous one itself, as harm2map does"""
		return dmap(self.tensor.clone(), self.wcs)
	def pixsize(self): return pixsize(self.shape, self.wcs)

def _sliced(parent, res, sel):
	"""wrap the result of parent[sel] with the geometry it now has (None axes / Ellipsis / leading-axis indexing allowed)"""
	nd = parent.ndim
	if isinstance(parent, ndmap) and not isinstance(res, np.ndarray): return res     # every axis indexed: a numpy scalar stays one
	sel = sel if isinstance(sel, tuple) else (sel,)
	if any(isinstance(x, (list, np.ndarray)) or A.is_tensor(x) for x in sel):
		return np.asarray(res) if isinstance(parent, ndmap) else res          # fancy indexing: no geometry
	nreal = sum(1 for x in sel if x is not None and x is not Ellipsis)
	full = []
	for x in sel:
		if x is Ellipsis: full += [slice(None)]*(nd-nreal)
		elif x is not None: full.append(x)
	full += [slice(None)]*(nd-len(full))
	ysel, xsel = full[nd-2], full[nd-1]
	if not (isinstance(ysel, slice) and isinstance(xsel, slice)):
		return np.asarray(res) if isinstance(parent, ndmap) else res          # a pixel axis was indexed away
	if ysel == slice(None) and xsel == slice(None): wcs = parent.wcs
	else: _, wcs = wcsutils.slice_geometry(parent.shape, parent.wcs, (ysel, xsel))
	return dmap(res, wcs) if isinstance(parent, dmap) else ndmap(res, wcs)

def enmap(arr, wcs=None, dtype=None, copy=True):
	if wcs is None: wcs = getattr(arr, "wcs", None)
	arr = np.array(arr, dtype=dtype, copy=copy) if copy else np.asarray(arr, dtype=dtype)
	return ndmap(arr, wcs)
def samewcs(arr, *args):
	for m in args:
		if hasattr(m, "wcs"): return ndmap(arr, m.wcs)
	return arr
def zeros(shape, wcs=None, dtype=None): return ndmap(np.zeros(shape, dtype=dtype), wcs)
def empty(shape, wcs=None, dtype=None): return ndmap(np.empty(shape, dtype=dtype), wcs)
def ones(shape, wcs=None, dtype=None): return ndmap(np.ones(shape, dtype=dtype), wcs)

# rows a full-sky CAR grid spends ON the poles: Clenshaw-Curtis has a ring on each pole (ny - 1 intervals span pi),
# Fejer-1 keeps half a pixel away from both (ny intervals)
_POLE_ROWS = {"cc": 1, "fejer1": 0}

def fullsky_geometry(res=None, shape=None, dims=(), proj="car", variant="fejer1"):
	"""(shape, wcs) of a CAR map covering the whole sky, from a resolution in radians or a pixel shape (ny, nx): the
	geometry contract of enmap.fullsky_geometry (enmap.py:1713-1740).  Columns run east to west (cdelt_ra < 0) with pixel
	centres half a pixel off RA = 0; rows run south to north with the equator on the row lattice."""
	assert proj == "car", "Only CAR fullsky geometry implemented"
	key = str(variant).lower()
	if key not in _POLE_ROWS: raise ValueError("Unrecognized CAR variant '%s'" % str(variant))
	extra = _POLE_ROWS[key]
	if shape is None:
		dy, dx = np.broadcast_to(np.asarray(res, float), (2,)) if np.ndim(res) else (float(res), float(res))
		ny, nx = int(round(np.pi/dy))+extra, int(round(2*np.pi/dx))
	else:
		ny, nx = int(shape[-2]), int(shape[-1])
		dy, dx = np.pi/(ny-extra), 2*np.pi/nx
	assert abs(dy*(ny-extra)-np.pi) < 1e-8, "Vertical resolution does not evenly divide the sky; this is required for SHTs."
	assert abs(dx*nx-2*np.pi) < 1e-8, "Horizontal resolution does not evenly divide the sky; this is required for SHTs."
	wcs = CarWCS(cdelt=[-360.0/nx, 180.0/(ny-extra)], crval=[0.5*dx/degree, 0.0], crpix=[nx//2+0.5, 0.5*(ny+1)])
	return tuple(dims)+(ny, nx), wcs

def band_geometry(dec_cut, res=None, shape=None, dims=(), proj="car", variant="fejer1"):
	"""the rows of the full-sky geometry whose centres lie within |dec| <= dec_cut (or within [dec_cut[0], dec_cut[1]]), all
	columns kept (enmap.band_geometry, enmap.py:1742-1772)"""
	cut = np.atleast_1d(np.asarray(dec_cut, float))
	lo, hi = (-cut[0], cut[0]) if cut.size == 1 else (cut[0], cut[1])
	fshape, fwcs = fullsky_geometry(res=res, shape=shape, dims=dims, proj=proj, variant=variant)
	rows = [float(wcsutils.world2pix(fwcs, 0, d/degree)[1]) for d in (lo, hi)]
	first, last = max(int(np.round(min(rows))), 0), min(int(np.round(max(rows))), fshape[-2])
	w = fwcs.deepcopy(); w.wcs.crpix[1] -= first
	return tuple(dims)+(last-first, fshape[-1]), w

def thumbnail_geometry(r=None, res=None, shape=None, dims=(), proj="tan"):
	"""(shape, wcs) of a geometry in projection proj ("car" or "tan") centred on (0, 0), which lies exactly on pixel shape//2 of an odd
	shape, cdelt = (-res, res): the geometry of reproject.thumbnails (enmap.thumbnail_geometry, enmap.py:1770-1820).  Two of r (the
	radius from the centre to the edges), res and shape, in radians."""
	proj = str(proj).lower()
	if proj not in ("car", "tan"): raise NotImplementedError("thumbnail_geometry: projections \"car\" and \"tan\", not \"%s\"" % proj)
	make = CarWCS if proj == "car" else wcsutils.TanWCS
	dirs = np.array([1.0, -1.0])
	def odd(shape): return np.rint(np.zeros(2)+np.asarray(shape[-2:], float)).astype(int)//2*2+1
	def rpix(wcs, r):      # |pixel offset| {y,x} of the point (dec, ra) = r from the centre
		x, y = wcs.wcs_world2pix(r[1]/degree, r[0]/degree, 0)
		return np.abs(np.array([float(y), float(x)]))
	def expand(res):
		res = np.atleast_1d(np.asarray(res, float))
		return dirs*res[0] if res.size == 1 else res
	if r is None:
		if res is None or shape is None: raise ValueError("Two of r, res and shape must be given")
		res, shape = expand(res), odd(shape)
		wcs = make(cdelt=res[::-1]/degree, crval=[0, 0], crpix=shape[::-1]//2+1)
	elif shape is None:
		if res is None: raise ValueError("Two of r, res and shape must be given")
		res, r = expand(res), np.zeros(2)+r
		wcs = make(cdelt=res[::-1]/degree, crval=[0, 0], crpix=[1, 1])
		shape = 2*np.rint(rpix(wcs, r)).astype(int)+1
		wcs.wcs.crpix = np.array(shape[::-1]//2+1, float)
	else:
		shape, r = odd(shape), np.zeros(2)+r
		wcs = make(cdelt=[1, 1], crval=[0, 0], crpix=[1, 1])
		ratio = (shape-1)/(2*rpix(wcs, r))*dirs
		wcs.wcs.cdelt = wcs.wcs.cdelt/ratio[::-1]
		wcs.wcs.crpix = np.array(shape[::-1]//2+1, float)
	return tuple(dims)+tuple(int(n) for n in shape), wcs

def spin_helper(spin, n):
	"""Walk the n components of a map / alm stack in spin groups: yields (spin, first, last+1); spin 0 takes one component,
	any other spin a pair; the spin list is cycled (enmap.spin_helper, enmap.py:3378-3388).  IndexError if a pair is cut."""
	import itertools
	first = 0
	for s in itertools.cycle(np.atleast_1d(spin).reshape(-1)):
		if first >= n: return
		width = 1 if s == 0 else 2
		if first+width > n: raise IndexError("Unpaired component in spin transform")
		yield s, first, first+width
		first += width

def pix2sky(shape, wcs, pix):
	"""[{y,x},...] -> [{dec,ra},...] in radians (enmap.pix2sky, enmap.py:483-494, linear CAR)"""
	pix = np.asarray(pix, float)
	ra, dec = wcsutils.pix2world(wcs, pix[1], pix[0])
	return np.array([dec*degree, ra*degree])

def area(shape, wcs):
	"""solid angle of a separable cylindrical map: (sin dec_hi - sin dec_lo) * RA range (enmap.area_cyl, enmap.py:1032-1036)"""
	if not wcsutils.is_separable(wcs): raise NotImplementedError("area: only separable cylindrical geometries")
	lo, hi, _ = _dec_span(shape, wcs)
	return (np.sin(hi)-np.sin(lo))*abs(wcs.wcs.cdelt[0])*degree*shape[-1]
def pixsize(shape, wcs): return area(shape, wcs)/np.prod(shape[-2:])

def pixshapes_cyl(shape, wcs, signed=False):
	"""[{height,width}, ny] of the pixels of each row of a separable cylindrical geometry, radians: a row from dec1 to dec2 is dec2 - dec1
	high and, its pixels having the area dRA (sin dec2 - sin dec1), area/height wide (enmap.pixshapes_cyl, enmap.py:1150-1175)"""
	if not wcsutils.is_separable(wcs): raise NotImplementedError("pixshapes_cyl: only separable cylindrical geometries")
	ny = int(shape[-2])
	dec = np.clip(pix2sky(shape, wcs, [np.arange(ny+1)-0.5, np.zeros(ny+1)])[0], -np.pi/2, np.pi/2)
	heights = dec[1:]-dec[:-1]
	sdec = np.sin(dec)
	res = np.array([heights, wcs.wcs.cdelt[0]*degree*(sdec[1:]-sdec[:-1])/heights])
	return res if signed else np.abs(res)

def pixsizemap(shape, wcs, broadcastable=False):
	"""the area of every pixel in steradians, [ny, nx] (broadcastable: [ny, 1]), a host ndmap: exact per row for separable cylindrical
	geometries (enmap.pixsizemap, enmap.py:1177-1204)"""
	psize = np.prod(pixshapes_cyl(shape, wcs), 0)[:, None]
	if not broadcastable: psize = np.broadcast_to(psize, tuple(shape[-2:]))
	return ndmap(psize, wcs)

def _norm(emap, normalize, sign, dct=False):
	norm = 1.0
	if normalize: norm /= (np.prod(2*np.array(emap.shape[-2:])-1)**0.5 if dct else np.prod(emap.shape[-2:])**0.5)   # (enmap.py:1318,1331)
	if normalize in ["phy", "phys", "physical"]: norm *= emap.pixsize()**(0.5*sign)
	return norm

def fft(emap, omap=None, nthread=0, normalize=True, adjoint_ifft=False, dct=False):
	"""enmap.fft (enmap.py:1307-1323): 2-D FFT over the last two axes, scaling fused into the
	last kernel pass instead of a separate `res *= norm` sweep."""
	norm = _norm(emap, normalize, -1 if adjoint_ifft else +1, dct=dct)
	if dct: return _wrap(enfft.dct(_data(emap), _data(omap) if omap is not None else None, axes=[-2, -1], nthread=nthread, _scale=norm), emap)
	res = enfft.fft(_data(emap), _data(omap) if omap is not None else None, axes=[-2, -1], nthread=nthread, _scale=norm)
	return _wrap(res, emap)

def ifft(emap, omap=None, nthread=0, normalize=True, adjoint_fft=False, dct=False):
	"""enmap.ifft (enmap.py:1325-1337)"""
	norm = _norm(emap, normalize, +1 if adjoint_fft else -1, dct=dct)
	if dct: return _wrap(enfft.idct(_data(emap), _data(omap) if omap is not None else None, axes=[-2, -1], nthread=nthread, normalize=False, _scale=norm), emap)
	res = enfft.ifft(_data(emap), _data(omap) if omap is not None else None, axes=[-2, -1], nthread=nthread, normalize=False, _scale=norm)
	return _wrap(res, emap)

def dct(emap, omap=None, nthread=0, normalize=True): return fft(emap, omap=omap, nthread=nthread, normalize=normalize, dct=True)
def idct(emap, omap=None, nthread=0, normalize=True): return ifft(emap, omap=omap, nthread=nthread, normalize=normalize, dct=True)
def fft_adjoint(emap, omap=None, nthread=0, normalize=True): return ifft(emap, omap=omap, nthread=nthread, normalize=normalize, adjoint_fft=True)
def ifft_adjoint(emap, omap=None, nthread=0, normalize=True): return fft(emap, omap=omap, nthread=nthread, normalize=normalize, adjoint_ifft=True)

def _data(m):
	if m is None: return None
	if isinstance(m, dmap): return m.tensor
	if A.is_tensor(m): return m          # a bare torch tensor
	return np.asarray(m)
def _wrap(res, like):
	if isinstance(like, dmap): return dmap(res, like.wcs)
	return ndmap(res, getattr(like, "wcs", None))

# ---------------------------------------------------------------------------------------
# flat-sky harmonic helpers around fft/ifft.  Geometry arithmetic is host numpy; everything
# that touches an [ny,nx] array runs on the GPU (include/pxsht.h pxm_*).
# ---------------------------------------------------------------------------------------
def _dec_span(shape, wcs):
	"""declinations of the lower and upper map edge (pixel edges, not centres), clipped to the sphere, and the row direction"""
	edges = pix2sky(shape, wcs, [[-0.5, shape[-2]-0.5], [0, 0]])[0]
	sign = 1 if edges[0] <= edges[1] else -1
	lo, hi = np.clip(np.sort(edges), -np.pi/2, np.pi/2)
	return lo, hi, sign

def extent(shape, wcs, signed=False, method="auto"):
	"""[height, width] of the patch in radians (enmap.extent, enmap.py:917-1014).  "cylindrical" (separable geometries): the
	width is the RA range times the mean of cos(dec) over the patch, so that area = height * width holds exactly;
	"intermediate": pixel counts times the WCS increments."""
	if method == "auto": method = "cylindrical" if wcsutils.is_separable(wcs) else "intermediate"
	if method in ("inter", "intermediate"):
		ext = np.array([wcs.wcs.cdelt[1]*shape[-2], wcs.wcs.cdelt[0]*shape[-1]], float)*degree
	elif method in ("cyl", "cylindrical"):
		lo, hi, sign = _dec_span(shape, wcs)
		ext = np.array([sign*(hi-lo), shape[-1]*wcs.wcs.cdelt[0]*degree*(np.sin(hi)-np.sin(lo))/(hi-lo)])
	else: raise NotImplementedError("extent: only the cylindrical and intermediate methods")
	return ext if signed else np.abs(ext)

def laxes(shape, wcs, oversample=1, method="auto", broadcastable=False):
	"""the multipoles (ly[ny], lx[nx]) of the bins of the map's 2-D FFT: 2 pi times the FFT frequencies for the pixel pitch
	extent/shape (enmap.laxes, enmap.py:1275-1294); oversample > 1 describes the finer lattice of a zero-padded transform"""
	os_ = int(oversample)
	pitch = extent(shape, wcs, signed=True, method=method)/np.array(shape[-2:], float)
	axes = [2*np.pi*np.fft.fftfreq(n*os_, d) for n, d in zip(shape[-2:], pitch)]
	if os_ > 1: axes = [l+0.5*l[os_]*(1.0/os_-1) for l in axes]
	ly, lx = axes
	return (ly[:, None], lx[None, :]) if broadcastable else (ly, lx)

def lmap(shape, wcs, oversample=1, method="auto"):
	"""[{ly,lx},ny,nx] multipole of every 2-D FFT bin"""
	ly, lx = laxes(shape, wcs, oversample=oversample, method=method, broadcastable=True)
	return ndmap(np.stack(np.broadcast_arrays(ly, lx)).astype(float), wcs)

def modlmap(shape, wcs, oversample=1, method="auto", min=0):
	"""|l| of every 2-D FFT bin (floored at `min`)"""
	ly, lx = laxes(shape, wcs, oversample=oversample, method=method, broadcastable=True)
	l = np.hypot(ly, lx)
	return ndmap(np.maximum(l, min) if min > 0 else l, wcs)

def lpixshape(shape, wcs, signed=False, method="auto"): return 2*np.pi/extent(shape, wcs, signed=signed, method=method)
def lpixsize(shape, wcs, signed=False, method="auto"): return float(np.prod(lpixshape(shape, wcs, signed=signed, method=method)))

def queb_rotmat(lmap, inverse=False, iau=False, spin=2, wcs=None):
	"""host version of the [2,2,ny,nx] rotation between (Q,U) and (E,B) in flat-sky harmonic space: angle = spin * atan2(+-lx, ly),
	sign flipped by `iau` and by `inverse` (enmap.queb_rotmat, enmap.py:1391-1400).  The transforms below never build it: they rotate
	in place on the GPU (pxm_rotate_queb)."""
	sign = (-1 if iau else 1)*(-1 if inverse else 1)
	ang = spin*np.arctan2(sign*np.asarray(lmap[1]), np.asarray(lmap[0]))
	c, s_ = np.cos(ang), np.sin(ang)
	return samewcs(np.array([[c, -s_], [s_, c]]), lmap)

def _to_device(emap, dtype=None):
	"""(dmap on the GPU, True if the input was a host array)"""
	if isinstance(emap, dmap): return emap, False
	t = A.put(emap, dtype); staged = A.is_tensor(t)
	return (dmap if staged else ndmap)(t, getattr(emap, "wcs", None)), staged
def _to_host(m):
	return ndmap(A.host(m), m.wcs) if isinstance(m, dmap) else m
def _geo_key(shape, wcs):
	"""what the l axes of a map depend on: its pixel shape and the WCS numbers (None: no usable key, do not cache)"""
	try: return (tuple(int(v) for v in shape[-2:]), tuple(np.asarray(wcs.wcs.cdelt, float)), tuple(np.asarray(wcs.wcs.crval, float)), tuple(np.asarray(wcs.wcs.crpix, float)), tuple(wcs.wcs.ctype))
	except Exception: return None
_axes_cache = {}
_cache_lock = threading.Lock()      # (the geometry caches below are shared between threads)
def _dev_axes(shape, wcs, like):
	"""ly, lx as device f64 arrays living next to `like` (kept per geometry and device: a Monte-Carlo loop calls lbin / map2harm on the
	same geometry every realisation, and the upload from pageable memory is a host synchronisation each time)"""
	if _lib.is_hostsim():
		ly, lx = laxes(shape, wcs)
		return np.ascontiguousarray(ly), np.ascontiguousarray(lx)
	key = _geo_key(shape, wcs)
	if key is not None: key = key+(str(like.device),)
	with _cache_lock:      # lookup, fill and eviction as one step; the cached tensors are shared and must not be modified by callers
		hit = _axes_cache.get(key) if key is not None else None
		if hit is None:
			hit = tuple(A.put(l, None, like.device) for l in laxes(shape, wcs))
			A.torch().cuda.current_stream().synchronize()      # (complete before another thread's stream may read them)
			if key is not None:
				if len(_axes_cache) >= 8: _axes_cache.pop(next(iter(_axes_cache)))
				_axes_cache[key] = hit
	return hit

def _rotate_pairs(hmap, spin, iau, inverse):
	"""rotate every spin-s pair of a contiguous complex harmonic map [...,ncomp,ny,nx] in place"""
	data = _data(hmap)
	if data.ndim <= 2: return
	if not A.is_contiguous(data): raise ValueError("_rotate_pairs: the harmonic map must be C-contiguous (component addresses are computed from its shape)")
	ny, nx = data.shape[-2:]; nc = data.shape[-3]
	lib = _lib.load(); dev = A.device_index(); st = A.current_stream()
	dt = A.DT[A.np_dtype(data)]; esz = A.np_dtype(data).itemsize
	ly, lx = _dev_axes(hmap.shape, hmap.wcs, data)
	npre = int(np.prod(data.shape[:-3], dtype=int))
	base = A.ptr(data)
	for s, i1, i2 in spin_helper(spin, nc):
		if s == 0: continue
		sign = (-1 if iau else 1)*(-1 if inverse else 1)
		for p in range(npre):
			a = int(base+((p*nc+int(i1))*ny*nx)*esz); b = int(a+ny*nx*esz)
			_lib.check(lib.pxm_rotate_queb(ny, nx, A.ptr(ly), A.ptr(lx), int(s), 1 if sign < 0 else 0, a, b, dt, dev, st))

def map2harm(emap, nthread=0, normalize=True, iau=False, spin=[0, 2], adjoint_harm2map=False):
	"""2-D FFT + Q/U -> E/B rotation (enmap.map2harm, enmap.py:1358-1375); the rotation runs in place on the GPU"""
	dev, was_host = _to_device(emap)
	res = fft(dev, nthread=nthread, normalize=normalize, adjoint_ifft=adjoint_harm2map)
	if res.ndim > 2: _rotate_pairs(res, spin, iau, inverse=False)
	return _to_host(res) if was_host else res

def harm2map(emap, nthread=0, normalize=True, iau=False, spin=[0, 2], keep_imag=False, adjoint_map2harm=False):
	"""E/B -> Q/U rotation + inverse 2-D FFT (enmap.harm2map, enmap.py:1376-1389)"""
	dev, was_host = _to_device(emap)
	if dev.ndim > 2:
		# the working copy is C-contiguous whatever the caller's strides: _rotate_pairs addresses components from the shape
		d = _data(dev)
		dev = _wrap(d.clone(memory_format=A.torch().contiguous_format) if A.is_tensor(d) else np.array(d, order="C"), dev)
		_rotate_pairs(dev, spin, iau, inverse=True)
	res = ifft(dev, nthread=nthread, normalize=normalize, adjoint_fft=adjoint_map2harm)
	if not keep_imag:
		r = _data(res).real
		res = _wrap(r.contiguous() if hasattr(r, "contiguous") else np.ascontiguousarray(r), res)
	return _to_host(res) if was_host else res

def map2harm_adjoint(emap, nthread=0, normalize=True, iau=False, spin=[0, 2], keep_imag=False):
	return harm2map(emap, nthread=nthread, normalize=normalize, iau=iau, spin=spin, keep_imag=keep_imag, adjoint_map2harm=True)
def harm2map_adjoint(emap, nthread=0, normalize=True, iau=False, spin=[0, 2]):
	return map2harm(emap, nthread=nthread, normalize=normalize, iau=iau, spin=spin, adjoint_harm2map=True)

def calc_ps2d(harm, harm2=None):
	"""2-D (cross) power spectrum Re(harm conj(harm2)) with numpy broadcasting of the leading axes
	(enmap.calc_ps2d, enmap.py:1959-2011); each distinct pair of 2-D maps is computed once."""
	same = harm2 is None or harm2 is harm
	h1, host1 = _to_device(harm); h2, host2 = (h1, host1) if same else _to_device(harm2)
	d1, d2 = _data(h1), _data(h2)
	ct = np.result_type(A.np_dtype(d1), A.np_dtype(d2))
	if ct not in (np.dtype(np.complex64), np.dtype(np.complex128)): raise ValueError("calc_ps2d needs complex harmonic maps")
	d1 = A.put(d1, ct); d2 = d1 if same else A.put(d2, ct)
	ny, nx = d1.shape[-2:]
	pshape = np.broadcast_shapes(tuple(d1.shape[:-2]), tuple(d2.shape[:-2]))
	i1 = np.broadcast_to(np.arange(int(np.prod(d1.shape[:-2], dtype=int))).reshape(d1.shape[:-2]), pshape).reshape(-1)
	i2 = np.broadcast_to(np.arange(int(np.prod(d2.shape[:-2], dtype=int))).reshape(d2.shape[:-2]), pshape).reshape(-1)
	rt = np.dtype(np.float32) if ct == np.dtype(np.complex64) else np.dtype(np.float64)
	out = A.empty(tuple(pshape)+(ny, nx), rt, like=d1)
	lib = _lib.load(); dev = A.device_index(); st = A.current_stream()
	n = ny*nx; done = {}
	flat = out.reshape(-1, ny, nx)
	for i in range(len(i1)):
		key = tuple(sorted((int(i1[i]), int(i2[i])))) if same else (int(i1[i]), int(i2[i]))
		if key in done: flat[i] = flat[done[key]]; continue
		done[key] = i
		_lib.check(lib.pxm_ps2d(n, A.ptr(d1)+int(i1[i])*n*ct.itemsize, A.ptr(d2)+int(i2[i])*n*ct.itemsize, A.DT[ct],
			A.ptr(out)+i*n*rt.itemsize, A.DT[rt], dev, st))
	res = _wrap(out, h1)
	return _to_host(res) if host1 else res

_lbin_cache = {}
def lbin(map, bsize=None, brel=1.0, return_nhit=False, return_bins=False, lop=None):
	"""radial binning of a real fourier-space map in |l| (enmap.lbin / _bin_helper, enmap.py:2526-2556): returns b(l), l"""
	if lop is not None:
		# a transform of |l| (e.g. a logarithm): the bin of a pixel is no longer floor(|l| / bsize) of the kernel above but a table of the geometry,
		# made here as the reference makes it (the default bin width comes from the TRANSFORMED |l|, enmap.py:2528-2530)
		l = np.asarray(lop(np.asarray(modlmap(map.shape, map.wcs))))
		if bsize is None: bsize = min(abs(l[0, 1]), abs(l[1, 0]))
		return _bin_helper(map, l, bsize*brel, return_nhit=return_nhit, return_bins=return_bins)
	gkey = _geo_key(map.shape, map.wcs)
	with _cache_lock:
		geo = _lbin_cache.get((gkey, bsize, brel)) if gkey is not None else None
		if geo is None:
			ly, lx = laxes(map.shape, map.wcs)
			bs = min(abs(lx[1]), abs(ly[1])) if bsize is None else bsize
			bs = float(bs*brel)
			lmax = float(np.sqrt(np.max(ly**2)+np.max(lx**2)))
			geo = dict(bsize=bs, n=int(lmax/bs), lsum=None, nhit=None)
			if gkey is not None:
				if len(_lbin_cache) >= 8: _lbin_cache.pop(next(iter(_lbin_cache)))
				_lbin_cache[(gkey, bsize, brel)] = geo
	bsize, n = geo["bsize"], geo["n"]
	dev_map, was_host = _to_device(map)
	d = _data(dev_map)
	if A.np_dtype(d) not in (np.dtype(np.float32), np.dtype(np.float64)): raise ValueError("lbin needs a real map")
	if hasattr(d, "contiguous"): d = d.contiguous()
	ny, nx = d.shape[-2:]; npre = int(np.prod(d.shape[:-2], dtype=int))
	dly, dlx = _dev_axes(map.shape, map.wcs, d)
	acc = A.zeros((npre+2, max(n, 1)), np.float64, like=d)
	lib = _lib.load(); dev = A.device_index(); st = A.current_stream()
	esz = A.np_dtype(d).itemsize
	# the sums of |l| and the pixel counts per bin depend on the geometry alone: taken with the first map of the first call on a geometry
	# and kept (two of the kernel's three atomic adds per pixel)
	for i in range(npre):
		first = i == 0 and geo["nhit"] is None
		_lib.check(lib.pxm_lbin(ny, nx, A.ptr(dly), A.ptr(dlx), bsize, n, A.ptr(d)+i*ny*nx*esz, A.DT[A.np_dtype(d)],
			A.ptr(acc)+i*max(n, 1)*8, (A.ptr(acc)+npre*max(n, 1)*8) if first else None, (A.ptr(acc)+(npre+1)*max(n, 1)*8) if first else None, dev, st))
	acc = A.host(acc)
	if geo["nhit"] is None and npre > 0:
		with _cache_lock: geo["lsum"], geo["nhit"] = acc[npre, :n].copy(), acc[npre+1, :n].copy()      # (the geometry-only sums: set once, under the lock)
	nhit = geo["nhit"] if geo["nhit"] is not None else acc[npre+1, :n]
	lsum = geo["lsum"] if geo["lsum"] is not None else acc[npre, :n]
	with np.errstate(invalid="ignore", divide="ignore"):
		mout = (acc[:npre, :n]/nhit).reshape(tuple(d.shape[:-2])+(n,))
		orads = lsum/nhit
	if return_bins:
		edges = np.arange(len(orads)+1)*bsize
		orads = np.array([orads, edges[:-1], edges[1:]])
	if return_nhit: return mout, orads, nhit.astype(int)
	return mout, orads

def _bin_helper(map, r, bsize, return_nhit=False, return_bins=False):
	"""means of the map over the bins floor(r / bsize) of a per-pixel coordinate r[ny,nx] (enmap._bin_helper, enmap.py:2533-2556): the bin table,
	the pixel counts and the mean coordinate of every bin are functions of the geometry (host); the sums over the map run on the GPU (pxm_bin_index)"""
	r = np.asarray(r, float)
	n = int(np.max(r/bsize))
	rinds = np.floor(r/bsize).reshape(-1).astype(np.int64)
	nhit = np.bincount(rinds, minlength=n)[:n]
	with np.errstate(invalid="ignore", divide="ignore"): orads = np.bincount(rinds, weights=r.reshape(-1), minlength=n)[:n]/nhit
	dev_map, was_host = _to_device(map)
	d = _data(dev_map)
	if A.np_dtype(d) not in (np.dtype(np.float32), np.dtype(np.float64)): raise ValueError("binning needs a real map")
	if hasattr(d, "contiguous"): d = d.contiguous()
	ny, nx = d.shape[-2:]; npre = int(np.prod(d.shape[:-2], dtype=int))
	if rinds.size != ny*nx: raise ValueError("binning: the coordinate map does not have the map's pixel shape")
	tab = np.where((rinds >= 0) & (rinds < n), rinds, -1).astype(np.int32)
	dtab = A.put(tab, None, A.device_of(d)); acc = A.zeros((npre, max(n, 1)), np.float64, like=d)
	lib = _lib.load(); dev = A.device_index(); st = A.current_stream()
	esz = A.np_dtype(d).itemsize
	for i in range(npre):
		_lib.check(lib.pxm_bin_index(ny*nx, A.ptr(dtab), n, A.ptr(d)+i*ny*nx*esz, A.DT[A.np_dtype(d)], A.ptr(acc)+i*max(n, 1)*8, dev, st))
	acc = A.host(acc)
	with np.errstate(invalid="ignore", divide="ignore"): mout = (acc[:, :n]/nhit).reshape(tuple(d.shape[:-2])+(n,))
	if return_bins:
		edges = np.arange(len(orads)+1)*bsize
		orads = np.array([orads, edges[:-1], edges[1:]])
	if return_nhit: return mout, orads, nhit
	return mout, orads

def posaxes(shape, wcs):
	"""(dec[ny], ra[nx]) of the pixel centres of a separable geometry, radians (enmap.posaxes)"""
	if not wcsutils.is_separable(wcs): raise NotImplementedError("posaxes: only separable cylindrical geometries")
	dec = pix2sky(shape, wcs, [np.arange(shape[-2]), np.zeros(shape[-2])])[0]
	ra  = pix2sky(shape, wcs, [np.zeros(shape[-1]), np.arange(shape[-1])])[1]
	return dec, ra

def posmap(shape, wcs, safe=True, corner=False, separable="auto", dtype=np.float64, device=None):
	"""[{dec,ra},ny,nx] coordinates of every pixel centre (corner: of its lower corner) in radians, for separable cylindrical
	geometries: the outer sum of posaxes (enmap.posmap, enmap.py:435-465).  device: a torch device -> a dmap there, filled by
	broadcasting the two axes on the device.  (lensing.lens_map_curved never makes this map: pxm_deflect takes the axes' numbers.)"""
	if separable == "auto": separable = wcsutils.is_separable(wcs)
	if not separable: raise NotImplementedError("posmap: only separable cylindrical geometries")
	dec, ra = posaxes(shape, wcs)
	if corner:
		w = wcs.wcs; dec = dec-0.5*w.cdelt[1]*degree; ra = ra-0.5*w.cdelt[0]*degree
	ny, nx = int(shape[-2]), int(shape[-1])
	if device is not None:
		torch = A.torch()
		res = A.empty((2, ny, nx), dtype, device=device)
		res[0] = torch.as_tensor(dec, device=device)[:, None]; res[1] = torch.as_tensor(ra, device=device)[None, :]
		return dmap(res, wcs)
	res = np.empty((2, ny, nx), dtype)
	res[0] = dec[:, None]; res[1] = ra[None, :]
	return ndmap(res, wcs)

def _rotate_pairs_by(data, psi, c0, c1, spin):
	"""in place: components (c0, c1) of the contiguous real array data [npre, ncomp, npix...] (numpy in the simulator, a tensor next to
	psi otherwise) rotated by spin*psi, psi f64 [npix...] contiguous -- every pre-dimension entry in one pxm_rotate_pol call"""
	npre, nc = int(data.shape[0]), int(data.shape[1])
	npix = int(np.prod(data.shape[2:], dtype=np.int64))
	dt = A.np_dtype(data)
	lib = _lib.load(); dev = A.device_index(); st = A.current_stream()
	base = A.ptr(data)
	_lib.check(lib.pxm_rotate_pol(npix, npre, base+int(c0)*npix*dt.itemsize, base+int(c1)*npix*dt.itemsize, nc*npix, A.DT[dt], A.ptr(psi), int(spin), dev, st))

def rotate_pol(emap, angle, comps=[-2, -1], spin=2, axis=-3):
	"""A copy of emap with the components `comps` of `axis` rotated by spin*angle (radians): (a, b) -> (c a - s b, s a + c b),
	c + i s = exp(i spin angle) (enmap.rotate_pol, enmap.py:1402-1416).  angle: a scalar or an array (host or device) that broadcasts
	against emap with `axis` removed.  Host arrays, dmaps and CUDA tensors; the rotation runs on the GPU (pxm_rotate_pol), all leading
	entries in one call when the angle does not depend on them."""
	if spin == 0: return emap
	data = _data(emap)
	tens = A.is_tensor(data)
	rdt = A.np_dtype(data)
	if rdt not in (np.dtype(np.float32), np.dtype(np.float64)): raise ValueError("rotate_pol needs a real float32 or float64 map")
	axis %= data.ndim
	nc = int(data.shape[axis]); c0, c1 = int(comps[0]) % nc, int(comps[1]) % nc
	if c0 == c1: raise ValueError("rotate_pol: the two components must differ")
	pre, post = tuple(data.shape[:axis]), tuple(data.shape[axis+1:])
	if tens:
		torch = A.torch()
		work = A.require_gpu(data).clone(memory_format=torch.contiguous_format)
		ang = _data(angle)
		ang = ang.to(device=work.device, dtype=torch.float64) if A.is_tensor(ang) else torch.as_tensor(np.asarray(ang, np.float64), device=work.device)
		full = torch.broadcast_shapes(tuple(ang.shape), pre+post)
	else:
		work = A.put(data)
		if not A.is_tensor(work): work = np.array(work, order="C")      # (in the simulator what put() returns may be the caller's own array, and the rotation is in place)
		ang = np.asarray(A.host(angle), np.float64)
		full = np.broadcast_shapes(ang.shape, pre+post)
		ang = A.put(ang)
	if tuple(full) != pre+post: raise ValueError("rotate_pol: angle of shape %s does not broadcast against the map" % (tuple(ang.shape),))
	lead = tuple(ang.shape)[:max(ang.ndim-len(post), 0)]
	w3 = work.reshape((int(np.prod(pre, dtype=np.int64)), nc)+post)
	if A.is_tensor(ang): spread = lambda a, sh: a.broadcast_to(sh).contiguous()
	else: spread = lambda a, sh: np.ascontiguousarray(np.broadcast_to(a, sh))
	if all(n == 1 for n in lead):
		_rotate_pairs_by(w3, spread(ang.reshape(tuple(ang.shape)[len(lead):]), post), c0, c1, spin)
	else:
		afull = spread(ang, pre+post).reshape((w3.shape[0],)+post)
		for p in range(w3.shape[0]): _rotate_pairs_by(w3[p:p+1], afull[p], c0, c1, spin)
	if not tens: work = A.host(work)
	if isinstance(emap, dmap): return dmap(work, emap.wcs)
	if tens: return work
	return ndmap(work, emap.wcs) if isinstance(emap, ndmap) else work

def center(shape, wcs):
	"""[dec, ra] of the middle of the pixel grid (enmap.center, enmap.py:1254-1256)"""
	return pix2sky(shape, wcs, (np.array(shape[-2:])-1)/2.0)

def modrmap(shape, wcs, ref="center"):
	"""angular distance of every pixel centre from ref = [dec, ra] (radians; "center": the middle of the map) as a host ndmap: geometry only
	(enmap.modrmap, enmap.py:1263-1273, with utils.angdist's Vincenty form, stable at small and at large separations)"""
	if isinstance(ref, str):
		if ref != "center": raise ValueError(ref)
		ref = center(shape, wcs)
	ref = np.asarray(ref, float)
	dec, ra = posaxes(shape, wcs)
	dra = (ra-ref[1])[None, :]
	sd, cd = np.sin(dec)[:, None], np.cos(dec)[:, None]
	sr, cr = np.sin(ref[0]), np.cos(ref[0])
	y = np.hypot(cr*np.sin(dra), cd*sr-sd*cr*np.cos(dra))
	x = sd*sr+cd*cr*np.cos(dra)
	return ndmap(np.arctan2(y, x), wcs)

def shift(map, off, inplace=False, keepwcs=False):
	"""cyclic shift of the pixels: (i, j) -> (i + off[0], j + off[1]) (enmap.shift, enmap.py:3277-3290); unless keepwcs the reference pixel moves along"""
	off = np.atleast_1d(off).astype(int)
	axes = tuple(range(-len(off), 0))
	if isinstance(map, dmap):
		t = A.torch().roll(map.tensor, tuple(int(o) for o in off), axes)
		if inplace: map.tensor.copy_(t); res = map
		else: res = dmap(t, map.wcs)
	else:
		t = np.roll(np.asarray(map), tuple(int(o) for o in off), axes)
		if inplace: map[...] = t; res = map
		else: res = ndmap(t, map.wcs)
	if not keepwcs:
		w = res.wcs.deepcopy(); w.wcs.crpix = np.array(w.wcs.crpix, float); w.wcs.crpix[:len(off)] += off[::-1]; res.wcs = w
	return res

def rbin(map, center=[0, 0], bsize=None, brel=1.0, return_nhit=False, return_bins=False, rop=None):
	"""mean of the map in rings of width bsize (default: the smaller pixel pitch) around center = [dec, ra]: b(r)[..., nbin], r[nbin]
	(enmap.rbin, enmap.py:2512-2524)"""
	r = np.asarray(modrmap(map.shape, map.wcs, ref=center))
	if rop: r = np.asarray(rop(r))
	if bsize is None: bsize = np.min(extent(map.shape, map.wcs)/np.array(map.shape[-2:]))
	return _bin_helper(map, r, bsize*brel, return_nhit=return_nhit, return_bins=return_bins)

for _cls in (ndmap, dmap):
	_cls.extent   = lambda self, **kw: extent(self.shape, self.wcs, **kw)
	_cls.modrmap  = lambda self, **kw: modrmap(self.shape, self.wcs, **kw)
	_cls.rbin     = lambda self, *a, **kw: rbin(self, *a, **kw)
	_cls.pix2sky  = lambda self, pix: pix2sky(self.shape, self.wcs, pix)
	_cls.laxes    = lambda self, **kw: laxes(self.shape, self.wcs, **kw)
	_cls.lmap     = lambda self, **kw: lmap(self.shape, self.wcs, **kw)
	_cls.modlmap  = lambda self, **kw: modlmap(self.shape, self.wcs, **kw)
	_cls.lbin     = lambda self, *a, **kw: lbin(self, *a, **kw)
	_cls.posmap   = lambda self, **kw: posmap(self.shape, self.wcs, **kw)
	_cls.at       = lambda self, pos, **kw: at(self, pos, **kw)
	_cls.project  = lambda self, shape, wcs, **kw: project(self, shape, wcs, **kw)
	_cls.pixsizemap = lambda self, **kw: pixsizemap(self.shape, self.wcs, **kw)

# ---------------------------------------------------------------------------------------
# bounding boxes and pixel sizes of separable CAR geometries (what pixell_amd.wavelets builds its per-scale geometries from)
# ---------------------------------------------------------------------------------------
def _rewind(a, ref, period):
	"""a moved by whole periods into [ref - period/2, ref + period/2)"""
	return ref+(np.asarray(a, float)-ref+period/2.0) % period-period/2.0

def _unwind_middle(a, period, ref=0.0):
	"""the samples a[..., n] of a continuous cyclic coordinate without their period jumps: the middle sample is brought within half a period
	of ref, and every other one is moved by the whole periods that make the sequence continuous from there outwards"""
	a = np.array(_rewind(a, ref, period))
	if a.ndim == 0 or a.shape[-1] < 2: return a
	jumps = np.round((a[..., 1:]-a[..., :-1])/period)
	mid = a.shape[-1]//2
	a[..., mid+1:] -= np.cumsum(jumps[..., mid:], -1)*period
	a[..., :mid] += np.cumsum(jumps[..., mid-1::-1], -1)[..., ::-1]*period
	return a

def corners(shape, wcs, npoint=10, corner=True):
	"""[{bottom left, top right},{dec,ra}] in radians: the outer corners of the first and last pixel (corner=True) or their centres.  The
	RA of both is on the same side of the wrapping cut: the diagonal is sampled at npoint points and followed without 2 pi jumps,
	with the middle sample in [-pi, pi)"""
	off = 0.5 if corner else 0.0
	pix = np.array([np.linspace(-off, shape[-2]-1+off, num=npoint, endpoint=True), np.linspace(-off, shape[-1]-1+off, num=npoint, endpoint=True)])
	ra, dec = wcsutils.pix2world(wcs, pix[1], pix[0])
	return _unwind_middle(np.array([dec, ra])*degree, 2*np.pi).T[[0, -1]]

def skybox2pixbox(shape, wcs, skybox, npoint=10, corner=False, include_direction=False):
	"""pixel box [{from,to},{y,x}] (fractional) of the coordinate box [{from,to},{dec,ra}], the x pixels followed along the diagonal without
	jumps of the sky's period; include_direction appends the sign of the pixel direction of each axis"""
	skybox = np.asarray(skybox, float)
	coords = np.array([np.linspace(skybox[0, 0], skybox[1, 0], num=npoint, endpoint=True), np.linspace(skybox[0, 1], skybox[1, 1], num=npoint, endpoint=True)])/degree
	x, y = wcsutils.world2pix(wcs, coords[1], coords[0])
	wpix = [np.array(x), np.array(y)]
	if corner: wpix = [v+0.5 for v in wpix]
	for i, n in enumerate(shape[-2:][::-1]):
		wpix[i] = _unwind_middle(wpix[i], abs(360.0/wcs.wcs.cdelt[i]), ref=n/2.0+(0.5 if corner else 0.0))
	pix = np.array(wpix[::-1])
	res = pix[:, [0, -1]].T
	if include_direction: res = np.concatenate([res, np.sign(pix[:, 1]-pix[:, 0])[None]], 0)
	return res

def pixshapebounds(shape, wcs, separable="auto"):
	"""[{min,max},{height,width}] of the pixels in radians, separable cylindrical geometries only: a row's pixels are dec_hi - dec_lo high
	and area/height = dRA (sin dec_hi - sin dec_lo)/(dec_hi - dec_lo) wide"""
	if separable is False or not wcsutils.is_separable(wcs): raise NotImplementedError("pixshapebounds: only separable cylindrical geometries")
	ny = shape[-2]
	dec = np.clip(pix2sky(shape, wcs, [np.arange(ny+1)-0.5, np.zeros(ny+1)])[0], -np.pi/2, np.pi/2)
	heights = dec[1:]-dec[:-1]
	sdec = np.sin(dec)
	widths = wcs.wcs.cdelt[0]*degree*(sdec[1:]-sdec[:-1])/heights
	ps = np.abs(np.array([heights, widths]))
	return np.array([np.min(ps, 1), np.max(ps, 1)])

# ---------------------------------------------------------------------------------------
# what pointsrcs.sim_objects needs: object positions in pixels, and the pixel window
# ---------------------------------------------------------------------------------------
def sky2pix(shape, wcs, coords, safe=True, corner=False):
	"""[{dec,ra},...] in radians -> [{y,x},...] (fractional, 0-based; enmap.sky2pix, enmap.py:496-529) for the linear CAR relation of
	wcs.py.  The x of a geometry whose columns go round the sky is not brought into [0, nx): callers that need that wrap themselves."""
	coords = np.asarray(coords, float)
	x, y = wcsutils.world2pix(wcs, coords[1]/degree, coords[0]/degree)
	res = np.array([y, x])
	return res+0.5 if corner else res

# ---------------------------------------------------------------------------------------
# reading a map at positions and on another geometry (enmap.py:561-638, 796-842); the kernels are behind pixell_amd.interpol
# ---------------------------------------------------------------------------------------
def _rewind_of(shape, wcs, safe):
	"""(ref, per) per pixel axis {y,x} of the rewind of the reference's sky2pix(safe=True) (enmap.py:509-519): pixel coordinates are brought
	within half a turn of the sky, |360/cdelt| pixels, of the middle of the map, on both axes; no rewind without safe"""
	if not safe: return ((0.0, 0.0), (0.0, 0.0))
	w = wcs.wcs
	return ((shape[-2]/2.0, abs(360.0/w.cdelt[1])), (shape[-1]/2.0, abs(360.0/w.cdelt[0])))

def _need_separable(wcs, what):
	if not wcsutils.is_separable(wcs): raise NotImplementedError("%s: only separable cylindrical geometries" % what)

def at(map, pos, mode="spline", order=3, border="constant", cval=0.0, unit="coord", safe=True, ip=None):
	"""The values of map [..., ny, nx] at pos [{dec,ra}, ...] in radians (unit="coord") or [{y,x}, ...] in pixels (unit="pix"), interpolated:
	[..., ...] (enmap.at, enmap.py:796-842).  mode, order, border and cval as in interpol.interpol; safe: positions a whole turn of the sky
	away land where they belong.  ip: an interpol.interpolator of the map to use again (the prefilter of order 3 then does not run).  One
	launch: the kernel turns positions into pixels itself.  Host maps give numpy arrays, dmaps tensors."""
	from . import interpol
	if unit not in ("coord", "pix"): raise ValueError("Unrecognized unit '%s'" % str(unit))
	if ip is None: ip = interpol.interpolator(map, npre=map.ndim-2, mode=mode, order=order, border=border, cval=cval)
	pos = _data(pos)
	if not A.is_tensor(pos): pos = np.asarray(pos, np.float64)
	if pos.ndim < 1 or pos.shape[0] != 2: raise ValueError("pos must be [{dec,ra},...] or [{y,x},...]")
	if unit == "pix": return ip.evaluate(tuple(pos.shape[1:]), pts=pos)
	_need_separable(map.wcs, "at")
	w = map.wcs.wcs
	affine = tuple((float(-w.crval[k]/w.cdelt[k]+w.crpix[k]-1), float(1.0/(degree*w.cdelt[k]))) for k in (1, 0))
	return ip.evaluate(tuple(pos.shape[1:]), pts=pos, affine=affine, rewind=_rewind_of(map.shape, map.wcs, safe))

def project(map, shape, wcs, mode="spline", order=3, border="constant", cval=0.0, force=False, safe=True, ip=None):
	"""map [..., ny, nx] on the geometry (shape, wcs), interpolated: [..., shape[-2], shape[-1]] (enmap.project, enmap.py:561-638).  Both
	geometries separable and cylindrical; the whole output is one launch that computes the input pixel of every output pixel itself.
	Equal geometries give a copy (force: interpolate anyway).  The result has the interpolation's dtype: float64 at order 3.  The
	reference's blocks of 1000 output rows, each on an apodised band of the input, are a way to save memory and are not reproduced
	(INTEGRATION.md E)."""
	from . import interpol
	oshape = (int(shape[-2]), int(shape[-1]))
	if not force and ip is None and _geo_key(map.shape, map.wcs) == _geo_key(oshape, wcs) and _geo_key(oshape, wcs) is not None: return map.copy()
	_need_separable(map.wcs, "project"); _need_separable(wcs, "project")
	if ip is None: ip = interpol.interpolator(map, npre=map.ndim-2, mode=mode, order=order, border=border, cval=cval)
	wi, wo = map.wcs.wcs, wcs.wcs
	# output pixel o lies at crval_o + (o + 1 - crpix_o) cdelt_o, which is input pixel (that - crval_i)/cdelt_i + crpix_i - 1
	affine = tuple((float((wo.crval[k]+(1-wo.crpix[k])*wo.cdelt[k]-wi.crval[k])/wi.cdelt[k]+wi.crpix[k]-1), float(wo.cdelt[k]/wi.cdelt[k])) for k in (1, 0))
	res = ip.evaluate(oshape, affine=affine, rewind=_rewind_of(map.shape, map.wcs, safe))
	return dmap(res, wcs) if A.is_tensor(res) else ndmap(res, wcs)

def pixwin_1d(f, order=0):
	"""the pixel window along one axis at the dimensionless frequency f (pixel pitch 1): nearest-neighbour (order 0) or linear (order 1)
	map-making (utils.pixwin_1d, utils.py:856-869)"""
	f = np.asarray(f, float)
	if order is None or order == "none": return f*0+1
	if order == 0 or order == "nn": return np.sinc(f)
	if order == 1 or order == "lin": return np.sinc(f)**2/(1/3*(2+np.cos(2*np.pi*f)))
	raise ValueError("Unsupported pixel window order '%s'" % str(order))

def calc_window(shape, order=0, scale=1):
	"""(wy[ny], wx[nx]): the separable Fourier-space pixel window, window = wy[:,None]*wx[None,:] (enmap.calc_window, enmap.py:1472-1483)"""
	return pixwin_1d(np.fft.fftfreq(shape[-2], scale), order=order), pixwin_1d(np.fft.fftfreq(shape[-1], scale), order=order)

def apply_window(emap, pow=1.0, order=0, scale=1, nofft=False):
	"""A copy of emap with the pixel window to the power pow applied (enmap.apply_window, enmap.py:1485-1496): FFT, one multiplication
	per axis on the device (pxm_mul_axis), inverse FFT.  nofft: emap is a Fourier-space map already.  Host maps, dmaps and CUDA tensors."""
	wy, wx = calc_window(emap.shape, order=order, scale=scale)
	like = emap if isinstance(emap, (dmap, ndmap)) else None
	dev, was_host = _to_device(emap if like is not None else dmap(emap, None) if A.is_tensor(emap) else ndmap(np.asarray(emap), None))
	d = _data(dev)
	rdt = A.np_dtype(d)
	ct = np.result_type(rdt, np.complex64)
	if A.is_tensor(d): work = d.to(A.tdtype(ct), copy=True).contiguous()
	else: work = np.array(d, dtype=ct, order="C")
	wmap = _wrap(work, dev)
	if not nofft: wmap = fft(wmap, normalize=False)
	data = _data(wmap)
	enfft._mul_axis(data, data.ndim-2, wy**pow)
	enfft._mul_axis(data, data.ndim-1, wx**pow)
	if not nofft:
		wmap = ifft(wmap, normalize=False)
		data = _data(wmap)
		data = data.real*(1.0/(data.shape[-2]*data.shape[-1]))
		data = A.put(data if rdt.kind == "c" else A.astype(data, rdt))
	elif rdt.kind != "c": raise ValueError("apply_window(nofft=True) needs a complex Fourier-space map")
	res = _wrap(data, dev)
	if was_host: res = _to_host(res)
	if like is None: return _data(res)
	return res

def unapply_window(emap, pow=1.0, order=0, scale=1, nofft=False):
	"""the inverse of apply_window (enmap.py:1498-1500)"""
	return apply_window(emap, pow=-pow, order=order, scale=scale, nofft=nofft)

# ---------------------------------------------------------------------------------------
# distance transforms and apodisation (enmap.py:2127-2286, 2440-2490); the kernels are behind pixell_amd.distances
# ---------------------------------------------------------------------------------------
_DIST_METHODS = ("cellgrid", "bubble", "simple")
def _check_method(method):
	if method not in _DIST_METHODS: raise ValueError("Unknown method '%s'" % str(method))

def distance_from(shape, wcs, points, omap=None, odomains=None, domains=False, method="cellgrid", rmax=None, step=1024):
	"""The distance of each pixel of the geometry from the nearest of points [{dec,ra}, npoint], [ny, nx]; with domains=True also the index
	of that point (enmap.distance_from, enmap.py:2160-2215).  rmax: beyond it the distance is rmax and the domain -1.  Every method
	("cellgrid", "bubble", "simple") runs the same exact search on the device; step is accepted and not used."""
	from . import distances
	_check_method(method)
	return distances.distance_from_points(shape, wcs, points=points, rmax=rmax, omap=omap, odomains=odomains, domains=domains)

def _planes(m, what):
	"""(the data of map m as [npre, ny, nx], its leading shape)"""
	if not hasattr(m, "wcs"): raise ValueError("%s needs a map with a geometry (ndmap or dmap)" % what)
	d = _data(m)
	if d.ndim < 2: raise ValueError("%s needs at least two axes" % what)
	return d.reshape((-1,)+tuple(d.shape[-2:])), tuple(d.shape[:-2])

def distance_transform(mask, omap=None, rmax=None, method="cellgrid"):
	"""The distance of each pixel from the closest zero pixel of mask [..., ny, nx]; zero inside the zero regions (enmap.distance_transform,
	enmap.py:2127-2138).  The edges of the zero regions are found on the device, searched from as pixel indices, and the mask itself says
	where no search is needed.  A mask without zeros gives rmax (infinity without one)."""
	from . import distances
	_check_method(method)
	md, pre = _planes(mask, "distance_transform")
	if omap is None: od = A.zeros(md.shape, np.float64, like=md)
	else:
		od = _data(omap)
		if tuple(od.shape) != pre+tuple(md.shape[-2:]): raise ValueError("omap must have the shape of the mask")
		od = od.reshape(md.shape)
	for i in range(md.shape[0]):
		m8 = A.astype(md[i] != 0, np.uint8)
		edges = distances.find_edges(m8, flat=True)
		if A.is_tensor(od) or not A.is_tensor(m8): distances.distance_from_points(mask.shape, mask.wcs, pix=edges, rmax=rmax, omap=od[i], skip=m8)
		else: od[i] = _to_host(distances.distance_from_points(mask.shape, mask.wcs, pix=edges, rmax=rmax, skip=m8))      # (a device mask and a host omap)
	if omap is not None: return omap
	return _wrap(od.reshape(pre+tuple(md.shape[-2:])), mask)

def labeled_distance_transform(labels, omap=None, odomains=None, rmax=None, method="cellgrid"):
	"""The distance of each pixel from the closest non-zero pixel of labels [..., ny, nx], and the label of that pixel: (omap, odomains)
	(enmap.labeled_distance_transform, enmap.py:2140-2158).  The distance is zero inside the labelled regions; odomains keeps what it held
	where no labelled pixel is within rmax."""
	from . import distances
	_check_method(method)
	ld, pre = _planes(labels, "labeled_distance_transform")
	ld = A.astype(ld, np.int32)
	full = pre+tuple(ld.shape[-2:])
	od = A.zeros(ld.shape, np.float64, like=ld) if omap is None else _data(omap).reshape(ld.shape)
	dd = A.zeros(ld.shape, np.int32, like=ld) if odomains is None else _data(odomains).reshape(ld.shape)
	if A.is_tensor(ld) != A.is_tensor(od) or A.is_tensor(ld) != A.is_tensor(dd): raise ValueError("labels, omap and odomains must all live on the host or all on the device")
	for i in range(ld.shape[0]):
		lab = ld[i].contiguous() if A.is_tensor(ld) else np.ascontiguousarray(ld[i])
		edges = distances.find_edges_labeled(lab, flat=True)
		_, dom = distances.distance_from_points(labels.shape, labels.wcs, pix=edges, rmax=rmax, omap=od[i], domains=True)
		dom = _data(dom)
		good = dom >= 0
		if int(edges.shape[0]) > 0:
			mapping = lab.reshape(-1)[edges]
			dd[i][good] = A.astype(mapping[A.astype(dom[good], np.int64)], A.np_dtype(dd))
		od[i][lab != 0] = 0
	oo = omap if omap is not None else _wrap(od.reshape(full), labels)
	do = odomains if odomains is not None else _wrap(dd.reshape(full), labels)
	return oo, do

def map_mul(mat, vec):
	"""Elementwise matrix multiplication mat*vec along the last non-pixel axes; the result has the shape of vec (enmap.map_mul,
	enmap.py:1418-1427).  A mat of three axes or fewer is a plain product.  Host maps or device maps (an einsum of torch's there)."""
	m, v = _data(mat), _data(vec)
	like = mat if hasattr(mat, "wcs") else vec
	if not hasattr(m, "ndim"): m = np.asarray(m)
	if m.ndim <= 3: return _wrap(m*v, like) if hasattr(like, "wcs") else m*v
	res = A.torch().einsum("...abyx,...byx->...ayx", m, v) if A.is_tensor(m) else np.einsum("...abyx,...byx->...ayx", m, v)
	return _wrap(res, like) if hasattr(like, "wcs") else res

def _mask_not(mask): return _wrap(_data(mask) == 0, mask)

def grow_mask(mask, r):
	"""Grow the true part of the boolean mask by a distance of r radians (enmap.grow_mask, enmap.py:2280-2282)"""
	d = distance_transform(_mask_not(mask), rmax=r)
	return _wrap(_data(d) < r, mask)

def shrink_mask(mask, r):
	"""Shrink the true part of the boolean mask by a distance of r radians (enmap.shrink_mask, enmap.py:2284-2286)"""
	d = distance_transform(mask, rmax=r)
	return _wrap(_data(d) >= r, mask)

def apod_profile_lin(x): return x
def apod_profile_cos(x):
	"""0.5 (1 - cos(pi x)), of a numpy array or a torch tensor"""
	if isinstance(x, dmap): return dmap(apod_profile_cos(x.tensor), x.wcs)
	return 0.5*(1-(A.torch().cos(np.pi*x) if A.is_tensor(x) else np.cos(np.pi*x)))

def apod_mask(mask, width=1*degree, edge=True, profile=apod_profile_cos):
	"""Given a mask that is 0 in bad regions and 1 in good regions, an apodisation map that is still 0 in the bad regions and goes to 1 over
	`width` radians inside the good ones, as profile(distance/width) (enmap.apod_mask, enmap.py:2479-2490).  edge: what lies outside the
	image counts as bad."""
	if edge:
		md = _data(mask)
		md = md.clone() if A.is_tensor(md) else np.array(md)
		md[..., 0, :] = 0; md[..., :, 0] = 0
		md[..., -1, :] = 0; md[..., :, -1] = 0
		mask = _wrap(md, mask)
	r = distance_transform(mask, rmax=width)
	return _wrap(profile(_data(r)/width), mask)

def _median2(d):
	"""the median over the last two axes, as numpy.median takes it (the mean of the two middle values of an even count)"""
	if not A.is_tensor(d): return np.median(d, (-2, -1))
	s = d.reshape(tuple(d.shape[:-2])+(-1,)).sort(-1).values
	n = s.shape[-1]
	return 0.5*(s[..., (n-1)//2]+s[..., n//2])

def apod(map, width, profile="cos", fill="zero", inplace=False):
	"""Apodise the outermost width [{y,x}] (or one number: both) pixels of each edge of the map (enmap.apod, enmap.py:2440-2474).  fill:
	"zero": towards 0; "mean", "median": towards the mean or median of each [ny, nx] map; "crossfade": towards the opposite edge.
	Slicing only, on the host or on the device wherever the map lives."""
	if fill not in ("zero", "mean", "median", "crossfade"): raise ValueError("Unknown fill '%s'" % str(fill))
	if profile not in ("lin", "cos"): raise ValueError("Unknown apodization profile '%s'" % str(profile))
	width = (np.zeros(2, int)+width).astype(int)
	d = _data(map)
	if not inplace: d = d.clone() if A.is_tensor(d) else np.array(d)
	if fill == "mean": offset = d.mean((-2, -1))[..., None, None]
	elif fill == "median": offset = _median2(d)[..., None, None]
	if fill in ("mean", "median"): d -= offset
	for i, w in enumerate(width):
		w = int(w)
		if w <= 0: continue
		x = np.arange(1, w+1, dtype=float)/((2*w+1) if fill == "crossfade" else (w+1))
		prof = apod_profile_lin(x) if profile == "lin" else apod_profile_cos(x)
		if A.is_tensor(d): prof = A.torch().as_tensor(prof, dtype=d.dtype, device=d.device)
		else: prof = prof.astype(d.dtype, copy=False)
		rev = prof.flip(0) if A.is_tensor(d) else prof[::-1]
		slice1 = (Ellipsis,)+(slice(None),)*i+(slice(0, w),)+(slice(None),)*(1-i)
		slice2 = (Ellipsis,)+(slice(None),)*i+(slice(-w, None),)+(slice(None),)*(1-i)
		broad = (None,)*i+(slice(None),)+(None,)*(1-i)
		if fill == "crossfade":
			m1 = d[slice1].clone() if A.is_tensor(d) else d[slice1].copy()
			m2 = d[slice2].clone() if A.is_tensor(d) else d[slice2].copy()
			d[slice1] = m1*(1-prof).flip(0)[broad]+m2*rev[broad] if A.is_tensor(d) else m1*(1-prof)[::-1][broad]+m2*rev[broad]
			d[slice2] = m2*(1-prof)[broad]+m1*prof[broad]
		else:
			d[slice1] *= prof[broad]
			d[slice2] *= rev[broad]
	if fill in ("mean", "median"): d += offset
	return map if inplace else _wrap(d, map)

for _cls in (ndmap, dmap):
	_cls.distance_transform = lambda self, **kw: distance_transform(self, **kw)
	_cls.labeled_distance_transform = lambda self, **kw: labeled_distance_transform(self, **kw)
	_cls.distance_from = lambda self, points, **kw: distance_from(self.shape, self.wcs, points, **kw)
	_cls.grow_mask    = lambda self, r: grow_mask(self, r)
	_cls.shrink_mask  = lambda self, r: shrink_mask(self, r)
	_cls.apod_mask    = lambda self, **kw: apod_mask(self, **kw)
	_cls.apod         = lambda self, width, **kw: apod(self, width, **kw)
	_cls.label        = lambda self, **kw: _label(self, **kw)

def _label(mask, **kw):
	from . import labels
	return labels.label(mask, **kw)
