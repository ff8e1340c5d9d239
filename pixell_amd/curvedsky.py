"""Drop-in for the spherical-harmonic-transform API of pixell/curvedsky.py on MI355X.

Same function names, argument meaning and error behaviour as the reference for the `2d` and
`cyl` methods and the healpix / profile helpers (curvedsky.py:83-302, 312-403, 510-580, 756-1086, 1170-1446).  Transforms at arbitrary
positions run on the GPU: alm2map_pos, alm2map_raw_general and map2alm_raw_general (curvedsky.py:174-207, 993-1016, 1088-1120; sht.synthesis_general).
The `general` method for whole maps (non-cylindrical pixelisations) is outside the accelerated path and raises NotImplementedError (prof2alm:
without the rotation to `dir`).
rotate_alm (curvedsky.py:714-740) runs on the GPU (almops.rotate_alm, triangular layout).

Differences that matter for speed, not for results:
  * the flipped / padded copies of map2buffer / buffer2map (curvedsky.py:1384-1411) are not
    made: flips are negative strides inside the kernels (sht.*(flip=...));
  * `map` may be an enmap.ndmap (numpy; staged through the GPU) or an enmap.dmap wrapping a torch
    CUDA tensor (transformed in place, nothing leaves HBM); `alm` likewise numpy or tensor.
"""
import os
import numpy as np
from . import enmap, sht, _lib, _arrays as A, wcs as wcsutils

from .geometry import Bunch, degree

def nint(a): return np.round(a).astype(int)
def complex_dtype(dtype): return np.result_type(dtype, 0j)
def real_dtype(dtype): return np.zeros([0], dtype).real.dtype
def nditer(shape):
	for I in np.ndindex(*shape): yield tuple(I)

def nalm2lmax(nalm):
	"""band limit of a full triangular layout with nalm = (lmax+1)(lmax+2)/2 elements"""
	return int((np.sqrt(8.0*nalm+1)-1)/2)-1

# ---------------------------------------------------------------------------------------
# alm layout
# ---------------------------------------------------------------------------------------
def _mstart_triangular(lmax, mmax, stride):
	m = np.arange(mmax+1, dtype=np.int64)
	return stride*((m*(2*lmax+1-m))//2)           # column m starts where l = 0 WOULD be: element (l, m) sits at mstart[m] + l stride
def _mstart_rectangular(lmax, mmax, stride):
	return stride*(lmax+1)*np.arange(mmax+1, dtype=np.int64)
_LAYOUTS = {"triangular": (_mstart_triangular, nalm2lmax), "tri": (_mstart_triangular, nalm2lmax),
	"rectangular": (_mstart_rectangular, lambda nalm: int(np.sqrt(nalm))-1), "rect": (_mstart_rectangular, lambda nalm: int(np.sqrt(nalm))-1)}

class alm_info:
	"""Where element (l, m) of a spherical-harmonic coefficient array lives: index = mstart[m] + l*stride (the contract of
	pixell's curvedsky.alm_info, curvedsky.py:409-476, which the C ABI takes over as `mstart` / `lstride`).
	layout: "triangular" (m-major, no padding; the default), "rectangular" (every m has lmax+1 slots) or an explicit mstart array.
	Either lmax or the element count nalm fixes the size; mmax defaults to lmax."""
	def __init__(self, lmax=None, mmax=None, nalm=None, stride=1, layout="triangular"):
		lmax, mmax, nalm = (None if v is None else int(v) for v in (lmax, mmax, nalm))
		if isinstance(layout, str):
			if layout not in _LAYOUTS: raise ValueError("unknown alm layout: %s" % layout)
			build, lmax_from_count = _LAYOUTS[layout]
			if lmax is None:
				if nalm is None: raise ValueError("alm_info needs lmax or nalm")
				lmax = lmax_from_count(nalm)
			if mmax is None: mmax = lmax
			mstart = build(lmax, mmax, int(stride))
		else:
			mstart = np.asarray(layout)
			if lmax is None or mmax is None: raise ValueError("an explicit mstart needs lmax and mmax")
		self.lmax, self.mmax, self.stride = lmax, mmax, int(stride)
		self.nelem = int(np.max(mstart))+(lmax+1)*self.stride
		self.nreal = lmax*lmax+2*lmax+2
		assert nalm is None or self.nelem == nalm, "lmax must be explicitly specified when lmax != mmax"
		self.mstart = mstart.astype(np.uint64, copy=False)
	nl = property(lambda self: self.lmax+1)
	nm = property(lambda self: self.mmax+1)
	def lm2ind(self, l, m):
		return (self.mstart[m].astype(int, copy=False)+np.asarray(l)*self.stride).astype(int, copy=False)
	def get_map(self):
		raise NotImplementedError
	def alm2cl(self, alm, alm2=None, dtype=None):
		"""cross power spectrum of alm and alm2, which broadcast (curvedsky.py:451-462); e.g.
		cl[{T,E,B},{T,E,B},nl] = ainfo.alm2cl(alm[:,None,:], alm[None,:,:])"""
		from . import almops
		return almops.alm2cl(self, alm, alm2=alm2, cl_dtype=dtype)
	def lmul(self, alm, lmat, out=None):
		"""res[a,lm] = lmat[a,b,l]*alm[b,lm] (or the broadcasting product for lmat[...,l]) (curvedsky.py:463-466)"""
		from . import almops
		return almops.lmul(self, alm, lmat, out=out)
	def bank_split(self, alm, filters, lmaxs, Ls=None):
		"""one filtered, truncated copy of alm per scale, each in the triangular layout of Ls[i] (almops.bank_split)"""
		from . import almops
		return almops.bank_split(self, alm, filters, lmaxs, Ls=Ls)
	def bank_merge(self, alms, filters, lmaxs, Ls=None, out=None, accumulate=False):
		"""the transpose: the filtered sum of the per-scale alms in this layout (almops.bank_merge)"""
		from . import almops
		return almops.bank_merge(self, alms, filters, lmaxs, Ls=Ls, out=out, accumulate=accumulate)
	def __repr__(self):
		return "alm_info(lmax=%s,mmax=%s,mstart=%s)" % (str(self.lmax), str(self.mmax), str(self.mstart))

# ---------------------------------------------------------------------------------------
# geometry analysis: thin names over pixell_amd/geometry.py (the reference's function names, curvedsky.py:478-505, 1170-1353)
# ---------------------------------------------------------------------------------------
from . import geometry as _geo
get_ducc_maxlmax = _geo.grid_maxlmax
def get_ducc_geo(wcs, shape=None, tol=1e-6): return _geo.classify_grid(wcs, shape=shape, tol=tol)
def analyse_geometry(shape, wcs, tol=1e-6): return _geo.analyse(shape, wcs, tol=tol)
def get_method(shape, wcs, minfo=None, pix_tol=1e-6):
	return _geo.method_of((minfo if minfo is not None else _geo.analyse(shape, wcs, tol=pix_tol)).case)
def get_ring_info(shape, wcs, dtype=np.float64): return _geo.ring_tables(shape, wcs, dtype=dtype)
def quad_weights(shape, wcs, pix_tol=1e-6, row_order="reference"):
	"""curvedsky.quad_weights (curvedsky.py:492-505), result for result: the grid's ring weights / nx, SOUTH-first whatever the
	map's row order (the reference reverses the north-first weights for every map).  row_order="map" returns them in the order of
	the map's rows instead -- the two differ only for maps stored north to south."""
	return _geo.ring_weights(shape, wcs, sht.get_gridweights, tol=pix_tol, row_order=row_order)

# ---------------------------------------------------------------------------------------
# array plumbing
# ---------------------------------------------------------------------------------------
def _mdata(map):
	if isinstance(map, enmap.dmap): return map.tensor
	return map if A.is_tensor(map) else np.asarray(map)      # (a bare device tensor stays where it is: alm2map_pos makes one for a tensor alm)

def prepare_alm(alm=None, ainfo=None, lmax=None, pre=(), dtype=np.float64, convert=False, like=None):
	"""(alm, ainfo) ready for a transform of maps of real type `dtype` (the contract of curvedsky.prepare_alm, curvedsky.py:1413-1427):
	a missing alm is allocated (zeros, next to `like`) for ainfo or lmax; an alm of the wrong precision is converted when
	`convert`, refused with ValueError otherwise; a missing ainfo is the triangular layout of the alm's length."""
	want = complex_dtype(dtype)
	if alm is None:
		if ainfo is None and lmax is None: raise ValueError("prepare_alm needs either alm, ainfo or lmax to be specified")
		ainfo = ainfo if ainfo is not None else alm_info(lmax)
		return A.zeros(tuple(pre)+(ainfo.nelem,), want, like), ainfo
	ainfo = ainfo if ainfo is not None else alm_info(nalm=alm.shape[-1])
	have = A.np_dtype(alm)
	if have != want:
		if not convert: raise ValueError("alm had dtype '%s', but expected '%s'" % (str(have), str(want)))
		alm = A.astype(alm, want)
	return alm, ainfo

def _atleast(x, n):
	while x.ndim < n: x = x[None]
	return x

def _contig(x):
	if A.is_tensor(x): return x if x.is_contiguous() else x.contiguous()
	return x

def _copy(x): return None if x is None else (x.clone() if A.is_tensor(x) else x.copy())

def _copy_out(alm, map, copy, alm_is_out):
	"""(alm, map) with the one the call overwrites replaced by a copy of it when `copy` (copy=True of every transform)"""
	if not copy: return alm, map
	return (_copy(alm), map) if alm_is_out else (alm, _copy(map))

def _layout_kwargs(ainfo):
	"""where the library finds element (l, m): the alm layout keywords of every sht call"""
	return dict(lmax=ainfo.lmax, mmax=ainfo.mmax, mstart=ainfo.mstart, lstride=ainfo.stride)

def _check_shapes(alm_full, map_full, deriv, pixdims=2, exc=AssertionError, text=None):
	"""alm [..., ncomp, nelem] and map [..., ncomp, pixels] (deriv: alm [..., nelem], map [..., 2, pixels]) must agree on the leading
	dimensions; raises exc, with `text` for either failure where the caller has one of its own"""
	if deriv and map_full.shape[-pixdims-1] != 2:
		raise exc(text or "map must have shape [...,2,%s] when deriv is True" % ("nloc" if pixdims == 1 else "ny,nx"))
	if tuple(map_full.shape[:map_full.ndim-pixdims-bool(deriv)]) != tuple(alm_full.shape[:-1]):
		raise exc(text or "map and alm must agree on pre-dimensions")

def _weights_like(weights, like):
	"""pixel weights where `like` lives (a scalar stays a scalar)"""
	if np.isscalar(weights) or not A.is_tensor(like): return weights
	return A.torch().as_tensor(np.asarray(weights), device=like.device)

def _dec_sign(like, pixdims):
	"""[-1, 1] along the component axis of a gradient map [2, pixels...]: d/dtheta <-> d/ddec"""
	f = np.array([-1.0, 1.0]).reshape((2,)+(1,)*pixdims)
	return A.torch().as_tensor(f, dtype=like.dtype, device=like.device) if A.is_tensor(like) else f.astype(like.dtype)

def _batched_jobs(spin, alm_full, map_full):
	"""[(spin, alm [nb, nca, nelem], map [nb, ncm, ny, nx])]: the reference loops over the pre-dimensions and the spin groups
	(curvedsky.py:910-924, 1038-1046) with one ducc call each; here every spin group is ONE library call over all pre-dimension
	entries, and a stack of scalar maps (every component a spin-0 group) is one call over its components."""
	nelem = alm_full.shape[-1]; ncomp = alm_full.shape[-2]; ny, nx = map_full.shape[-2:]
	groups = [(int(s), j1, j2) for s, j1, j2 in enmap.spin_helper(spin, ncomp)]
	if int(np.prod(map_full.shape[:-3], dtype=int)) == 0: return []       # empty pre-dimension: nothing to transform
	a3 = _as_view(alm_full, (-1, ncomp, nelem)); m4 = _as_view(map_full, (-1, ncomp, ny, nx))
	if a3 is None or m4 is None:
		# pre-dimensions that cannot be merged without a copy (exotic strides): one call per entry, as the reference does
		return [(s, alm_full[I+(slice(j1, j2),)][None], map_full[I+(slice(j1, j2),)][None]) for I in nditer(map_full.shape[:-3]) for s, j1, j2 in groups]
	if all(s == 0 for s, _, _ in groups) and ncomp > 1:
		return [(0, a3.reshape((-1, 1, nelem)), m4.reshape((-1, 1, ny, nx)))]
	return [(s, a3[:, j1:j2], m4[:, j1:j2]) for s, j1, j2 in groups]

def _as_view(x, shape):
	"""x reshaped WITHOUT copying (results are written through these views), or None"""
	try:
		if A.is_tensor(x): return x.view(shape)
		v = x.view(); v.shape = tuple(int(np.prod(x.shape[:x.ndim-len(shape)+1], dtype=int)) if n == -1 else n for n in shape); return v
	except (RuntimeError, AttributeError): return None

# ---------------------------------------------------------------------------------------
# public API
# ---------------------------------------------------------------------------------------
def _by_method(map, method, pix_tol, funcs):
	"""(funcs[method], minfo) for the map's geometry; "auto" picks the method of the geometry"""
	minfo = analyse_geometry(map.shape, map.wcs, tol=pix_tol)
	if method == "auto": method = get_method(map.shape, map.wcs, minfo=minfo)
	if method in funcs: return funcs[method], minfo
	if method == "general":
		raise NotImplementedError("method 'general' (non-cylindrical pixelisations, ducc synthesis_general) is outside the accelerated path")
	raise ValueError("Unrecognized alm2map method '%s'" % str(method))

def alm2map(alm, map, spin=[0, 2], deriv=False, adjoint=False, copy=False, method="auto", ainfo=None,
		verbose=False, nthread=None, epsilon=1e-6, pix_tol=1e-6, locinfo=None, tweak=False):
	"""Spherical harmonics synthesis (curvedsky.alm2map, curvedsky.py:83-164).  See the reference
	docstring for the argument meaning; `map` is overwritten unless copy=True and returned."""
	func, minfo = _by_method(map, method, pix_tol, {"2d": alm2map_2d, "cyl": alm2map_cyl})
	return func(alm, map, ainfo=ainfo, minfo=minfo, spin=spin, deriv=deriv, copy=copy, verbose=verbose, adjoint=adjoint, nthread=nthread, pix_tol=pix_tol)

def alm2map_adjoint(map, alm=None, spin=[0, 2], deriv=False, copy=False, method="auto", ainfo=None, verbose=False, nthread=None, epsilon=None, pix_tol=1e-6, locinfo=None):
	return alm2map(alm, map, spin=spin, deriv=deriv, adjoint=True, copy=copy, method=method, ainfo=ainfo, verbose=verbose, nthread=nthread, epsilon=epsilon, pix_tol=pix_tol, locinfo=locinfo)

def map2alm(map, alm=None, lmax=None, spin=[0, 2], deriv=False, adjoint=False, copy=False, method="auto", ainfo=None,
		verbose=False, nthread=None, niter=0, epsilon=None, pix_tol=1e-6, weights=None, locinfo=None, tweak=False, analysis=None, weights_order="reference"):
	"""Spherical harmonics analysis (curvedsky.map2alm, curvedsky.py:209-302).
	analysis (ours, method "2d" only): None / "ducc0" = the route ducc0's analysis_2d takes as published; "interpolant" = exact
	quadrature of the full theta-interpolant; "weights" = ring quadrature weights + adjoint synthesis (the reference's cyl route,
	curvedsky.py:852-861) on full grids with ny >= 2 lmax + 2: identical alm for band-limited maps (see pixell_amd.sht.analysis_2d).
	weights_order (ours, method "cyl" only): "reference" (default) applies weights to rows exactly as the reference does, including its
	mirrored pixel areas for maps stored north-to-south off a named grid; "map": weight i belongs to map row i (see map2alm_cyl)."""
	func, minfo = _by_method(map, method, pix_tol, {"2d": map2alm_2d, "cyl": map2alm_cyl})
	more = dict(analysis=analysis) if func is map2alm_2d else dict(niter=niter, weights=weights, weights_order=weights_order)
	return func(map, alm, ainfo=ainfo, minfo=minfo, lmax=lmax, spin=spin, deriv=deriv, copy=copy, verbose=verbose, adjoint=adjoint, nthread=nthread, pix_tol=pix_tol, **more)

def map2alm_adjoint(alm, map, lmax=None, spin=[0, 2], deriv=False, copy=False, method="auto", ainfo=None, verbose=False, nthread=None, niter=0, epsilon=1e-6, pix_tol=1e-6, weights=None, locinfo=None, analysis=None):
	"""curvedsky.map2alm_adjoint (curvedsky.py:304-310); analysis (ours): the form of map2alm whose transpose this is"""
	return map2alm(map=map, alm=alm, lmax=lmax, spin=spin, deriv=deriv, adjoint=True, copy=copy, method=method, ainfo=ainfo, verbose=verbose, nthread=nthread, niter=niter, epsilon=epsilon, pix_tol=pix_tol, weights=weights, locinfo=locinfo, analysis=analysis)

# ---- transform families: what differs between the 2d DERIV1 path, cyl rings, healpix rings and points, and the loops they share ----
class _Family:
	"""One kind of pixelisation as the two drivers below see it.
	syn, adj: the forward and adjoint sht function; kw: their fixed keywords; pixdims: the pixel axes of a map.
	to_lib: a map slice [nc, pixels...] as the library takes it (the solver shapes results back to the slice).
	contig_read: a map slice that the library reads is made contiguous first.
	zeroed_map: the solver's synthesis is handed a zeroed map of the slice's size instead of allocating one (the rings of a theta
	window do not cover the map).
	signed_adjoint: an adjoint DERIV1 call applies the declination sign to a COPY of its input.  Points do: their adjoint is the exact
	transpose of the forward call, which signs its output, and leaves the input alone.  The 2d, cyl and healpix adjoints apply no
	sign.  The reference signs the caller's map after the call; the difference is deliberate."""
	def __init__(self, syn, adj, kw, pixdims, to_lib=lambda m: m, contig_read=False, zeroed_map=False, signed_adjoint=False):
		self.syn, self.adj, self.kw, self.pixdims, self.to_lib = syn, adj, kw, pixdims, to_lib
		self.contig_read, self.zeroed_map, self.signed_adjoint = contig_read, zeroed_map, signed_adjoint

def _groups(pre, spin, ncomp, deriv):
	"""(spin, mode, alm index, map index) of every library call over the pre-dimensions `pre`, as the reference loops
	(curvedsky.py:910-924): with deriv one DERIV1 / spin-1 call per entry (the alm gains its component axis), else its spin groups"""
	for I in nditer(pre):
		if deriv: yield 1, "DERIV1", I+(None,), I
		else:
			for s, j1, j2 in enmap.spin_helper(spin, ncomp):
				yield int(s), "STANDARD", I+(slice(j1, j2),), I+(slice(j1, j2),)

def _full_groups(fam, alm_full, map_full, spin, deriv):
	return _groups(map_full.shape[:map_full.ndim-fam.pixdims-1], spin, None if deriv else alm_full.shape[-2], deriv)

def _direct(fam, alm_full, map_full, spin, deriv, adjoint):
	"""alm -> map (adjoint: map -> alm), one library call per group, written into map_full (alm_full)"""
	func = fam.adj if adjoint else fam.syn
	for s, mode, ai, mi in _full_groups(fam, alm_full, map_full, spin, deriv):
		v = alm_full[ai]; a = _contig(v); m = map_full[mi]
		if adjoint and deriv and fam.signed_adjoint: m = m*_dec_sign(m, fam.pixdims)
		if adjoint and fam.contig_read: m = _contig(m)
		func(alm=a, map=fam.to_lib(m), spin=s, mode=mode, **fam.kw)
		if adjoint:
			if a is not v: v[...] = a             # (the library wrote a contiguous staging copy of a strided alm slice)
		elif deriv: map_full[mi+(0,)] *= -1       # theta derivative -> dec derivative (curvedsky.py:919)

def jacobi_inverse(forward, approx_backward, y, niter=0):
	"""Solve forward(x) = y given an approximate inverse B: x_0 = B y, x_{k+1} = x_k + B (y - forward(x_k))
	(Jacobi / Richardson refinement; what curvedsky.jacobi_inverse, curvedsky.py:1122-1136, does around the ring transforms)"""
	x = approx_backward(y)
	for _ in range(int(niter)):
		x = x+approx_backward(y-forward(x))
	return x

def _operators(fam, s, mode, like, weights):
	"""Y, YT, YTW, WY of one group: synthesis onto a map like `like`, its transpose, and both with the pixel weights"""
	kw = dict(fam.kw, spin=s, mode=mode); shp = tuple(like.shape)
	def Y(a):   return fam.syn(alm=_contig(a), map=A.zeros(shp, A.np_dtype(like), like) if fam.zeroed_map else None, **kw).reshape(shp)
	def YT(m):  return fam.adj(map=fam.to_lib(_contig(m)), **kw)
	def YTW(m): return YT(m*weights)
	def WY(a):  return Y(a)*weights
	return Y, YT, YTW, WY

def _solve(fam, alm_full, map_full, spin, deriv, adjoint, niter, weights):
	"""map -> alm by weighted adjoint synthesis + `niter` Jacobi refinements (curvedsky.py:1067-1084), written into alm_full;
	adjoint: the transpose of that operator, alm -> map_full.  deriv: gradient maps [ddec, dra] through the DERIV1 transforms."""
	for s, mode, ai, mi in _full_groups(fam, alm_full, map_full, spin, deriv):
		m = map_full[mi]
		Y, YT, YTW, WY = _operators(fam, s, mode, m, weights)
		if adjoint:
			res = jacobi_inverse(YT, WY, _contig(alm_full[ai]), niter=niter)
			map_full[mi] = res*_dec_sign(m, fam.pixdims) if deriv else res
		else:
			alm_full[ai] = jacobi_inverse(Y, YTW, m*_dec_sign(m, fam.pixdims) if deriv else m, niter=niter)

# ---- 2d ---------------------------------------------------------------------------------
_NO_PADS = ((0, 0), (0, 0))
def _native_pads(minfo, use_y):
	"""((y_before, y_after), (x_before, x_after)) in the map's own pixel order.  minfo.ypad/xpad are in
	ducc orientation, i.e. after the flips of map2buffer (curvedsky.py:1384-1403)."""
	yp = tuple(int(v) for v in minfo.ypad) if use_y else (0, 0)
	xp = tuple(int(v) for v in minfo.xpad)
	if min(yp+xp) < 0: raise ValueError("map extends beyond the matching full-sky grid")
	if minfo.flip[0]: yp = yp[::-1]
	if minfo.flip[1]: xp = xp[::-1]
	return yp, xp

def _padded_like(map, pads, fill):
	"""zero-padded copy of the map (ndmap, or dmap on the GPU) with the wcs moved accordingly; this is the
	buffer map2buffer builds in the reference (curvedsky.py:1384-1403), without the flipped copy"""
	(y0, y1), (x0, x1) = pads
	mdata = _mdata(map)
	shape = tuple(map.shape[:-2])+(map.shape[-2]+y0+y1, map.shape[-1]+x0+x1)
	w = map.wcs.deepcopy(); w.wcs.crpix[0] += x0; w.wcs.crpix[1] += y0
	buf = A.zeros(shape, A.np_dtype(mdata), mdata)
	if fill: buf[..., y0:y0+map.shape[-2], x0:x0+map.shape[-1]] = mdata
	return (enmap.dmap(buf, w) if isinstance(map, enmap.dmap) else enmap.ndmap(buf, w))

def _on_padded(map, pads, map_is_input, run):
	"""run(pmap) on the map padded to its full grid / full rings, as the reference does (curvedsky.py:766-772, 786-792, 866-871):
	an input map is copied into the padding, an output map is cropped back out of it and returned"""
	(y0, y1), (x0, x1) = pads
	pmap = _padded_like(map, pads, fill=map_is_input)
	res = run(pmap)
	if map_is_input: return res
	_mdata(map)[...] = _mdata(pmap)[..., y0:y0+map.shape[-2], x0:x0+map.shape[-1]]
	return map

def alm2map_2d(alm, map, ainfo=None, minfo=None, spin=[0, 2], deriv=False, copy=False, verbose=False, adjoint=False, nthread=None, pix_tol=1e-6):
	"""curvedsky.alm2map_2d + alm2map_raw_2d (curvedsky.py:756-774, 900-926)"""
	alm, map = _copy_out(alm, map, copy, alm_is_out=adjoint)
	mdata = _mdata(map)
	alm, ainfo = prepare_alm(alm=alm, ainfo=ainfo, pre=map.shape[:-2], dtype=A.np_dtype(mdata), convert=not adjoint, like=mdata)
	if minfo is None: minfo = analyse_geometry(map.shape, map.wcs, tol=pix_tol)
	pads = _native_pads(minfo, use_y=True)
	if pads != _NO_PADS:      # (the padded geometry is case "2d")
		return _on_padded(map, pads, adjoint, lambda pmap: alm2map_2d(alm, pmap, ainfo=ainfo, spin=spin, deriv=deriv, copy=False, verbose=verbose, adjoint=adjoint, nthread=nthread, pix_tol=pix_tol))
	alm_full = _atleast(alm, 2 if deriv else 3)
	map_full = _atleast(mdata, 4)
	_check_shapes(alm_full, map_full, deriv)
	func = sht.adjoint_synthesis_2d if adjoint else sht.synthesis_2d
	kwargs = dict(_layout_kwargs(ainfo), phi0=minfo.phi0, geometry=minfo.ducc_geo.name, flip=minfo.flip)
	if deriv:
		_direct(_Family(sht.synthesis_2d, sht.adjoint_synthesis_2d, kwargs, pixdims=2), alm_full, map_full, spin, True, adjoint)
	else:
		jobs = _batched_jobs(spin, alm_full, map_full)
		# numpy arrays: the inputs of all spin groups start uploading now, outputs come back while the next group runs (pixell_amd/hostio.py).
		# Map -> alm: the group that is cheapest to transform goes LAST (its transform is the only one no upload hides); alm -> map: first.
		if adjoint: jobs = sorted(jobs, key=lambda j: -j[2].shape[-3])
		with sht.host_pipeline([m if adjoint else a for s, a, m in jobs], [a if adjoint else m for s, a, m in jobs]):
			for s, a, m in jobs: func(alm=a, map=m, spin=s, **kwargs)
	return alm if adjoint else map

def map2alm_2d(map, alm=None, ainfo=None, minfo=None, lmax=None, spin=[0, 2], deriv=False, copy=False, verbose=False, adjoint=False, nthread=None, pix_tol=1e-6, analysis=None):
	"""curvedsky.map2alm_2d + map2alm_raw_2d (curvedsky.py:822-841, 1018-1048)"""
	alm, map = _copy_out(alm, map, copy, alm_is_out=not adjoint)
	mdata = _mdata(map)
	alm, ainfo = prepare_alm(alm=alm, ainfo=ainfo, lmax=lmax, pre=map.shape[:-2], dtype=A.np_dtype(mdata), convert=adjoint, like=mdata)
	if minfo is None: minfo = analyse_geometry(map.shape, map.wcs, tol=pix_tol)
	if deriv:
		raise NotImplementedError("ducc does not support derivatives for map2alm operations. Can be worked around if necessary.")
	pads = _native_pads(minfo, use_y=True)
	if pads != _NO_PADS:
		return _on_padded(map, pads, not adjoint, lambda pmap: map2alm_2d(pmap, alm=alm, ainfo=ainfo, lmax=lmax, spin=spin, deriv=deriv, copy=False, verbose=verbose, adjoint=adjoint, nthread=nthread, pix_tol=pix_tol, analysis=analysis))
	alm_full = _atleast(alm, 3)
	map_full = _atleast(mdata, 4)
	_check_shapes(alm_full, map_full, False)
	# Restrict to lmax and mmax that the grid allows. Higher ones are ignored (curvedsky.py:1027-1028)
	l = min(ainfo.lmax, minfo.ducc_geo.lmax)
	m = min(ainfo.mmax, l)
	func = sht.adjoint_analysis_2d if adjoint else sht.analysis_2d
	kwargs = dict(phi0=minfo.phi0, lmax=l, mmax=m, geometry=minfo.ducc_geo.name, mstart=ainfo.mstart[:m+1], lstride=ainfo.stride, flip=minfo.flip, analysis=analysis)
	jobs = _batched_jobs(spin, alm_full, map_full)
	if not adjoint: jobs = sorted(jobs, key=lambda j: -j[2].shape[-3])      # (see alm2map_2d: map -> alm takes the largest group first)
	with sht.host_pipeline([a if adjoint else m for s, a, m in jobs], [m if adjoint else a for s, a, m in jobs]):
		for s, a, m in jobs: func(alm=a, map=m, spin=s, **kwargs)
	return map if adjoint else alm

# ---- cyl --------------------------------------------------------------------------------
def _ring_kwargs(rinfo, ainfo, **more):
	"""the keywords of the ring transforms for the ring tables rinfo (ringstart: their offsets unless given)"""
	return dict(dict(_layout_kwargs(ainfo), theta=rinfo.theta, nphi=rinfo.nphi, phi0=rinfo.phi0, ringstart=rinfo.offsets), **more)

def _flat(m):
	return m.reshape(m.shape[:-2]+(m.shape[-2]*m.shape[-1],))

def _cyl_family(map, minfo, ainfo):
	"""the rows of the map as rings in ducc orientation, with the flips of map2buffer expressed as a descending ringstart / negative
	pixel stride (no copy)"""
	assert not np.any(np.array(minfo.xpad) != 0), "partial-width maps are padded by the callers"
	shape = map.shape; ny, nx = shape[-2:]
	fshape, fwcs = wcsutils.flipped(shape, map.wcs, minfo.flip)
	rows = np.arange(ny)[::-1] if minfo.flip[0] else np.arange(ny)
	start = rows*nx + (nx-1 if minfo.flip[1] else 0)
	kw = _ring_kwargs(get_ring_info(fshape, fwcs), ainfo, ringstart=start.astype(np.uint64), pixstride=-1 if minfo.flip[1] else 1)
	return _Family(sht.synthesis, sht.adjoint_synthesis, kw, pixdims=2, to_lib=_flat)

def alm2map_cyl(alm, map, ainfo=None, minfo=None, spin=[0, 2], deriv=False, copy=False, verbose=False, adjoint=False, nthread=None, pix_tol=1e-6):
	"""curvedsky.alm2map_cyl + alm2map_raw_cyl (curvedsky.py:776-794, 928-962)"""
	alm, map = _copy_out(alm, map, copy, alm_is_out=adjoint)
	mdata = _mdata(map)
	alm, ainfo = prepare_alm(alm=alm, ainfo=ainfo, pre=map.shape[:-2], dtype=A.np_dtype(mdata), convert=not adjoint, like=mdata)
	if minfo is None: minfo = analyse_geometry(map.shape, map.wcs, tol=pix_tol)
	pads = _native_pads(minfo, use_y=False)
	if pads != _NO_PADS:      # partial-width map: the rings are extended to the full circle
		return _on_padded(map, pads, adjoint, lambda pmap: alm2map_cyl(alm, pmap, ainfo=ainfo, spin=spin, deriv=deriv, copy=False, verbose=verbose, adjoint=adjoint, nthread=nthread, pix_tol=pix_tol))
	fam = _cyl_family(map, minfo, ainfo)
	alm_full = _atleast(alm, 2 if deriv else 3)
	map_full = _atleast(mdata, 4)
	_check_shapes(alm_full, map_full, deriv)
	_direct(fam, alm_full, map_full, spin, deriv, adjoint)
	return alm if adjoint else map

def map2alm_cyl(map, alm=None, ainfo=None, minfo=None, lmax=None, spin=[0, 2], weights=None, deriv=False, copy=False, verbose=False, adjoint=False, nthread=None, pix_tol=1e-6, niter=0, weights_order="reference"):
	"""curvedsky.map2alm_cyl + map2alm_raw_cyl (curvedsky.py:843-873, 1050-1086): quadrature
	weights (exact grid weights where available) + Jacobi refinement around the HIP transforms."""
	alm, map = _copy_out(alm, map, copy, alm_is_out=not adjoint)
	mdata = _mdata(map)
	# (with deriv the alm has no component axis; the reference allocates [2,nelem] here and then fails its shape check)
	alm, ainfo = prepare_alm(alm=alm, ainfo=ainfo, lmax=lmax, pre=map.shape[:-3] if deriv else map.shape[:-2], dtype=A.np_dtype(mdata), convert=adjoint, like=mdata)
	if minfo is None: minfo = analyse_geometry(map.shape, map.wcs, tol=pix_tol)
	# Row weights.  The reference applies `weights` to the rows of its flipped buffer (north first: map2buffer, curvedsky.py:866-868),
	# here the rings are the map's rows as stored.  weights_order="reference" (default) reproduces the reference result for result:
	#   caller-supplied weights are taken north-first; default weights of a named grid are the grid's (physically right in both);
	#   default weights off the grid are the pixel areas, which the reference reverses for every map (`if minfo.flip:` on a list,
	#   curvedsky.py:860) -- right for maps stored south to north, mirrored for maps stored north to south.
	# weights_order="map": weight i belongs to map row i, pixel areas unmirrored.
	if weights_order not in ("reference", "map"): raise ValueError("weights_order must be 'reference' or 'map'")
	ref_order = weights_order == "reference"
	if weights is None:
		if minfo.ducc_geo is not None and minfo.ducc_geo.name in _geo.WEIGHTED_GRIDS:
			weights = quad_weights(map.shape, map.wcs, pix_tol=pix_tol, row_order="map")
		else:
			# pixel area of each row (enmap.pixsizemap separable; curvedsky.py:858-860)
			ny, nx = map.shape[-2:]
			dec = enmap.pix2sky(map.shape, map.wcs, [np.concatenate([np.arange(ny)-0.5, [ny-0.5]]), np.zeros(ny+1)])[0]
			dec = np.clip(dec, -np.pi/2, np.pi/2)
			weights = np.abs(np.sin(dec[1:])-np.sin(dec[:-1]))*abs(map.wcs.wcs.cdelt[0])*degree
			if ref_order and not minfo.flip[0]: weights = weights[::-1]
	else:
		weights = np.asarray(weights.cpu() if A.is_tensor(weights) else weights)
		if ref_order and minfo.flip[0]: weights = weights[::-1]
	weights = np.ascontiguousarray(weights, dtype=A.np_dtype(mdata))
	pads = _native_pads(minfo, use_y=False)
	if pads != _NO_PADS:      # partial-width map: the rings are zero-extended to the full circle; weights are per row
		return _on_padded(map, pads, not adjoint, lambda pmap: map2alm_cyl(pmap, alm=alm, ainfo=ainfo, lmax=lmax, spin=spin, weights=weights, deriv=deriv, copy=False, verbose=verbose, adjoint=adjoint, nthread=nthread, pix_tol=pix_tol, niter=niter, weights_order="map"))
	fam = _cyl_family(map, minfo, ainfo)
	alm_full = _atleast(alm, 2 if deriv else 3)
	map_full = _atleast(mdata, 4)
	_check_shapes(alm_full, map_full, deriv)
	_solve(fam, alm_full, map_full, spin, deriv, adjoint, niter, _weights_like(weights, mdata)[:, None])
	return map if adjoint else alm

# ---------------------------------------------------------------------------------------
# The reference's helper entry points around the transforms, by name (curvedsky.py:900-1086, 1236-1250, 1349-1353, 1384-1473).
# pixell stages every map through a flipped, padded copy (map2buffer) and runs the `raw` functions on that buffer; here flips are
# strides inside the kernels, so the `raw` functions are the plain ones restricted to what a buffer is (a complete grid / complete
# rings), and map2buffer / buffer2map exist for callers that want the staged form.
# ---------------------------------------------------------------------------------------
class ShapeError(Exception): pass

def dangerous_dtype(dtype): return np.dtype(dtype).byteorder not in ("=", "|")

def flip2slice(flips):
	"""index expression that reverses the trailing axes whose flag is set"""
	return (Ellipsis,)+tuple(slice(None, None, -1 if f else 1) for f in flips)
def flip_array(arr, flips): return arr[flip2slice(flips)]
def flip_geometry(shape, wcs, flips): return wcsutils.flipped(shape, wcs, flips)
def pad_geometry(shape, wcs, pad):
	"""geometry with pad[0] = (rows, columns) added before and pad[1] after"""
	pad = np.asarray(pad)
	w = wcs.deepcopy(); w.wcs.crpix[0] += pad[0, 1]; w.wcs.crpix[1] += pad[0, 0]
	return tuple(shape[:-2])+(int(pad[0, 0]+shape[-2]+pad[1, 0]), int(pad[0, 1]+shape[-1]+pad[1, 1])), w

def map2buffer(map, flip, pad, obuf=False):
	"""zero-filled map of the flipped, padded geometry holding the flipped map (obuf: left empty, an output buffer)"""
	pad = np.asarray(pad)
	shape, wcs = pad_geometry(*flip_geometry(map.shape, map.wcs, flip), pad)
	buf = enmap.zeros(shape, wcs, np.dtype(map.dtype).newbyteorder("="))
	if not obuf: buf[..., pad[0, 0]:shape[-2]-pad[1, 0], pad[0, 1]:shape[-1]-pad[1, 1]] = flip_array(np.asarray(map), flip)
	return buf
def buffer2map(map, flip, pad):
	"""undo map2buffer: crop the padding, flip back (a view)"""
	pad = np.asarray(pad)
	return flip_array(map[..., pad[0, 0]:map.shape[-2]-pad[1, 0], pad[0, 1]:map.shape[-1]-pad[1, 1]], flip)

def prepare_raw(alm, map, ainfo=None, lmax=None, deriv=False, verbose=False, nthread=None, pixdims=2, convert_alm=False):
	"""(alm_full, map_full, ainfo, nthread): alm [..., ncomp, nelem] and map [..., ncomp, pixels] with agreeing leading dimensions
	(deriv: alm [..., nelem], map [..., 2, pixels]); AssertionError otherwise (curvedsky.py:1429-1446)"""
	mdata = _mdata(map)
	alm, ainfo = prepare_alm(alm, ainfo, lmax=lmax, pre=map.shape[:-pixdims], dtype=A.np_dtype(mdata), convert=convert_alm, like=mdata)
	alm_full = _atleast(alm, 2 if deriv else 3); map_full = _atleast(mdata, pixdims+2)
	_check_shapes(alm_full, map_full, deriv, pixdims)
	env = os.environ.get("OMP_NUM_THREADS")
	return alm_full, map_full, ainfo, int(env) if env else int(nthread or 0)

def _require_case(map, minfo, cases, what):
	minfo = analyse_geometry(map.shape, map.wcs) if minfo is None else minfo
	if minfo.case not in cases or (minfo.case == "cyl" and cases == ("2d",)): raise ValueError("%s needs %s (got case '%s'): use the function without _raw, which pads" % (what, " or ".join(cases), minfo.case))
	return minfo

def alm2map_raw_2d(alm, map, ainfo=None, spin=[0, 2], deriv=False, copy=False, verbose=False, adjoint=False, nthread=None):
	"""synthesis_2d / adjoint_synthesis_2d on a map that IS a complete named grid (curvedsky.py:900-926)"""
	return alm2map_2d(alm, map, ainfo=ainfo, minfo=_require_case(map, None, ("2d",), "alm2map_raw_2d"), spin=spin, deriv=deriv, copy=copy, verbose=verbose, adjoint=adjoint, nthread=nthread)
def map2alm_raw_2d(map, alm=None, ainfo=None, lmax=None, spin=[0, 2], deriv=False, copy=False, verbose=False, adjoint=False, nthread=None):
	"""analysis_2d / adjoint_analysis_2d on a map that IS a complete named grid (curvedsky.py:1018-1048)"""
	return map2alm_2d(map, alm=alm, ainfo=ainfo, minfo=_require_case(map, None, ("2d",), "map2alm_raw_2d"), lmax=lmax, spin=spin, deriv=deriv, copy=copy, verbose=verbose, adjoint=adjoint, nthread=nthread)
def alm2map_raw_cyl(alm, map, ainfo=None, minfo=None, spin=[0, 2], deriv=False, copy=False, verbose=False, adjoint=False, nthread=None):
	"""synthesis / adjoint_synthesis on the rows of a map whose rings close the circle (curvedsky.py:928-962)"""
	return alm2map_cyl(alm, map, ainfo=ainfo, minfo=_require_case(map, minfo, ("2d", "cyl"), "alm2map_raw_cyl"), spin=spin, deriv=deriv, copy=copy, verbose=verbose, adjoint=adjoint, nthread=nthread)
def map2alm_raw_cyl(map, alm=None, ainfo=None, lmax=None, spin=[0, 2], weights=None, deriv=False, copy=False, verbose=False, adjoint=False, niter=0, nthread=None):
	"""weighted adjoint_synthesis + Jacobi refinement on the rows of a map whose rings close the circle (curvedsky.py:1050-1086)"""
	return map2alm_cyl(map, alm=alm, ainfo=ainfo, minfo=_require_case(map, None, ("2d", "cyl"), "map2alm_raw_cyl"), lmax=lmax, spin=spin, weights=weights, deriv=deriv, copy=copy, verbose=verbose, adjoint=adjoint, nthread=nthread, niter=niter, weights_order="map")      # (raw: weight i multiplies row i of the array handed in, curvedsky.py:1064-1065)

def alm_complex2real(alm, ainfo=None):
	"""complex alm (m >= 0 storage) -> real vector of the same information with unit Jacobian: the m = 0 block keeps its real
	parts, every m > 0 coefficient becomes sqrt(2) (Re, Im) (curvedsky.py:1451-1456)"""
	alm = np.asarray(alm)
	ainfo = alm_info(nalm=alm.shape[-1]) if ainfo is None else ainfo
	n0 = int(ainfo.mstart[1])+1
	return np.concatenate([alm[..., :n0].real, np.sqrt(2.0)*np.ascontiguousarray(alm[..., n0:]).view(real_dtype(alm.dtype))], -1)
def alm_real2complex(ralm, ainfo=None):
	"""inverse of alm_complex2real; without ainfo the triangular layout with (lmax+1)^2 = len is assumed"""
	ralm = np.asarray(ralm)
	if ainfo is None: ainfo = alm_info(lmax=nint((ralm.shape[-1]-1)**0.5)-1)       # length = lmax^2 + 2 lmax + 2 (a_00's zero slot included)
	n0 = int(ainfo.mstart[1])+1
	out = np.zeros(ralm.shape[:-1]+(ainfo.nelem,), complex_dtype(ralm.dtype))
	out[..., :n0] = ralm[..., :n0]
	out[..., n0:] = np.ascontiguousarray(ralm[..., n0:]).view(out.dtype)/np.sqrt(2.0)
	return out

# ---------------------------------------------------------------------------------------
# healpix maps: the same ring transforms on ring tables with per-ring nphi / phi0 (the general ring path of sht_general.hip)
# ---------------------------------------------------------------------------------------
def npix2nside(npix): return nint((npix/12)**0.5)
def get_ring_info_healpix(nside, rings=None): return _geo.healpix_rings(nside, rings)
def get_ring_info_radial(r): return _geo.radial_rings(r)
def apply_minfo_theta_lim(minfo, theta_min=None, theta_max=None): return _geo.theta_window(minfo, theta_min, theta_max)
def prepare_healmap(healmap, nside=None, pre=(), dtype=np.float64, like=None):
	if healmap is not None: return healmap
	return A.zeros(tuple(pre)+(12*int(nside)**2,), dtype, like)

def _healpix_family(npix, ainfo, theta_min, theta_max):
	"""(ring tables, family) of a healpix map of npix pixels in RING order, restricted to the rings of the theta window"""
	rinfo = apply_minfo_theta_lim(get_ring_info_healpix(npix2nside(npix)), theta_min, theta_max)
	return rinfo, _Family(sht.synthesis, sht.adjoint_synthesis, _ring_kwargs(rinfo, ainfo), pixdims=1, zeroed_map=True)

def alm2map_healpix(alm, healmap=None, spin=[0, 2], deriv=False, adjoint=False, copy=False, ainfo=None, nside=None, theta_min=None, theta_max=None, nthread=None):
	"""alm[..., ncomp, nelem] -> healpix map[..., ncomp, 12 nside^2] in RING order (curvedsky.alm2map_healpix, curvedsky.py:312-351);
	adjoint: the transpose, map -> alm.  With deriv the map is [..., 2, npix] = (d/ddec, d/dra / cos dec)."""
	alm, healmap = _copy_out(alm, healmap, copy, alm_is_out=adjoint)
	rdt = real_dtype(A.np_dtype(alm))
	alm, ainfo = prepare_alm(alm, ainfo, dtype=rdt, convert=not adjoint, like=alm)
	healmap = prepare_healmap(healmap, nside, alm.shape[:-2]+(2,) if deriv else alm.shape[:-1], rdt, like=alm)
	alm_full = _atleast(alm, 2 if deriv else 3); map_full = _atleast(healmap, 3)
	_check_shapes(alm_full, map_full, deriv, 1, ValueError, "When deriv is True, alm must have shape [...,nelem] and map shape [...,2,npix]" if deriv
		else "alm must have shape [...,[ncomp,]nelem] and map shape [...,[ncomp,]npix]")
	rinfo, fam = _healpix_family(map_full.shape[-1], ainfo, theta_min, theta_max)
	if (theta_min is not None or theta_max is not None) and not adjoint: map_full[...] = 0     # rings outside the window are not written
	_direct(fam, alm_full, map_full, spin, deriv, adjoint)
	return alm if adjoint else healmap

def map2alm_healpix(healmap, alm=None, ainfo=None, lmax=None, spin=[0, 2], weights=None, deriv=False, copy=False, verbose=False, adjoint=False, niter=0, theta_min=None, theta_max=None, nthread=None):
	"""healpix map -> alm with pixel-area weights 4 pi / npix (or `weights`) and `niter` Jacobi refinements
	(curvedsky.map2alm_healpix, curvedsky.py:353-403; like healpy.map2alm).  adjoint: the transpose of that operator, alm -> map."""
	alm, healmap = _copy_out(alm, healmap, copy, alm_is_out=not adjoint)
	if deriv: raise NotImplementedError("map2alm_healpix with deriv=True is broken")          # (as in the reference, curvedsky.py:378)
	alm, ainfo = prepare_alm(alm=alm, ainfo=ainfo, lmax=lmax, pre=healmap.shape[:-1], dtype=A.np_dtype(healmap), convert=adjoint, like=healmap)
	alm_full = _atleast(alm, 3); map_full = _atleast(healmap, 3)
	rinfo, fam = _healpix_family(map_full.shape[-1], ainfo, theta_min, theta_max)
	if weights is None: weights = 4*np.pi/rinfo.npix
	_solve(fam, alm_full, map_full, spin, False, adjoint, niter, _weights_like(weights, healmap))
	return healmap if adjoint else alm

# ---------------------------------------------------------------------------------------
# arbitrary positions: the point transforms of sht.synthesis_general (curvedsky.py:174-207, 993-1016, 1088-1120)
# ---------------------------------------------------------------------------------------
def _loc_from_pos(pos):
	"""pos [{dec,ra}, ...] -> loc [..., {codec, ra}] with ra made positive (curvedsky.py:185-193)"""
	if A.is_tensor(pos):
		loc = pos.movedim(0, -1).to(A.torch().float64).clone()
		loc[..., 0] = np.pi/2 - loc[..., 0]
		loc[..., 1] = A.torch().where(loc[..., 1] < 0, loc[..., 1]+2*np.pi, loc[..., 1])
		return loc
	loc = np.moveaxis(np.asarray(pos, np.float64), 0, -1).copy(order="C")
	loc[..., 0] *= -1; loc[..., 0] += np.pi/2
	loc[loc[..., 1] < 0, 1] += 2*np.pi
	return loc

def alm2map_pos(alm, pos=None, loc=None, ainfo=None, map=None, spin=[0, 2], deriv=False, copy=False, verbose=False, adjoint=False, nthread=None, epsilon=None):
	"""alm -> values at arbitrary positions (curvedsky.alm2map_pos, curvedsky.py:174-207).  pos: [{dec,ra}, ...] in radians, or
	loc: [..., {codec,ra}].  The pre-dimensions of pos / loc come back as trailing dimensions of the map: alm [..., nelem] ->
	map [..., npts...] (deriv: [..., 2, npts...], the declination derivative first).  adjoint: map -> alm, returns alm (with deriv
	the exact transpose: the sign of the declination component is applied before the transform and the input is left alone)."""
	alm, map = _copy_out(alm, map, copy, alm_is_out=adjoint)
	if loc is None: loc = _loc_from_pos(pos)
	lpre = tuple(loc.shape[:-1])
	loc = loc.reshape(-1, 2)
	npts = int(loc.shape[0])
	if map is None:
		oshape = tuple(alm.shape[:-1])+((2, npts) if deriv else (npts,))
		mflat = A.zeros(oshape, real_dtype(A.np_dtype(alm)), alm)
	else: mflat = map.reshape(tuple(map.shape[:map.ndim-len(lpre)])+(npts,))
	res = alm2map_raw_general(alm, mflat, loc, ainfo=ainfo, spin=spin, deriv=deriv, nthread=nthread, verbose=verbose, epsilon=epsilon, adjoint=adjoint)
	if adjoint: return res
	return mflat.reshape(tuple(mflat.shape[:-1])+lpre)

def _points_family(loc, ainfo, epsilon, map_dtype):
	"""the points loc [npts, 2] with ONE binning of them (sht.points_plan) for every spin group and Jacobi step"""
	if epsilon is None: epsilon = 1e-10 if map_dtype == np.float64 else 1e-6
	kw = dict(_layout_kwargs(ainfo), loc=loc, epsilon=epsilon, plan=sht.points_plan(loc, ainfo.lmax, ainfo.mmax, ainfo.mstart, ainfo.stride, epsilon))
	return _Family(sht.synthesis_general, sht.adjoint_synthesis_general, kw, pixdims=1, contig_read=True, signed_adjoint=True)

def alm2map_raw_general(alm, map, loc, ainfo=None, spin=[0, 2], deriv=False, copy=False, verbose=False, adjoint=False, nthread=None, epsilon=None):
	"""alm [..., ncomp, nelem] -> map [..., ncomp, npts] at loc [npts, 2] (curvedsky.alm2map_raw_general, curvedsky.py:993-1016); adjoint: the
	transpose.  deriv: alm [..., nelem] -> map [..., 2, npts] = (d/ddec, d/dra / cos dec)."""
	alm, map = _copy_out(alm, map, copy, alm_is_out=adjoint)
	alm_full, map_full, ainfo, nthread = prepare_raw(alm, map, ainfo=ainfo, deriv=deriv, nthread=nthread, pixdims=1, convert_alm=not adjoint)
	_direct(_points_family(loc, ainfo, epsilon, A.np_dtype(map_full)), alm_full, map_full, spin, deriv, adjoint)
	return alm if adjoint else map

def map2alm_raw_general(map, loc, alm=None, ainfo=None, lmax=None, spin=[0, 2], weights=None, deriv=False, copy=False, verbose=False, adjoint=False, nthread=None, niter=0, epsilon=None):
	"""values at loc [npts, 2] -> alm: weighted adjoint synthesis (pixel weights `weights`, default 1) with `niter` Jacobi refinements
	(curvedsky.map2alm_raw_general, curvedsky.py:1088-1120).  adjoint: the transpose of that operator, alm -> map."""
	alm, map = _copy_out(alm, map, copy, alm_is_out=not adjoint)
	alm_full, map_full, ainfo, nthread = prepare_raw(alm, map, ainfo=ainfo, lmax=lmax, deriv=deriv, nthread=nthread, pixdims=1, convert_alm=adjoint)
	fam = _points_family(loc, ainfo, epsilon, A.np_dtype(map_full))
	_solve(fam, alm_full, map_full, spin, deriv, adjoint, niter, _weights_like(1.0 if weights is None else weights, map_full))
	return map if adjoint else alm

# ---------------------------------------------------------------------------------------
# 1-D transforms: radial profiles <-> functions of l, as m = 0 transforms on rings of one pixel (curvedsky.py:510-554)
# ---------------------------------------------------------------------------------------
def _m0_kwargs(theta, lmax):
	return _ring_kwargs(get_ring_info_radial(theta), alm_info(lmax=lmax, mmax=0), spin=0)

def profile2harm(br, r, lmax=None, oversample=1, left=None, right=None):
	"""br[..., nr] sampled at ascending radii r (radians) -> bl[..., lmax+1] with b(r) = sum_l (2l+1)/(4 pi) b_l P_l(cos r): the
	profile is interpolated linearly onto the Clenshaw-Curtis nodes of spacing ~dr that cover [0, r_max], weighted with the CC ring
	weights and analysed with one m = 0 adjoint synthesis (the contract of curvedsky.profile2harm, curvedsky.py:510-541)"""
	br = np.asarray(br); r = np.asarray(r)
	step = (r[-1]-r[0])/(len(r)-1)
	nfull = nint(np.pi/step)+1; step = np.pi/(nfull-1)          # nodes k pi/(nfull-1) of the full circle, of which the first ncut reach r_max
	ncut = int(np.ceil(r[-1]/step))
	if lmax is None: lmax = int(nfull//2-1)
	theta = np.arange(ncut)*step
	kw = _m0_kwargs(theta, lmax)
	w = sht.get_gridweights("CC", nfull)[:ncut]
	norm = np.sqrt(4*np.pi/(2*np.arange(lmax+1)+1))
	out = np.zeros(br.shape[:-1]+(lmax+1,), br.dtype)
	for I in nditer(br.shape[:-1]):
		ring = np.interp(theta, r, br[I], left=left, right=right)[None]*w
		out[I] = sht.adjoint_synthesis(map=np.ascontiguousarray(ring, dtype=np.float64), **kw)[0].real*norm
	return out

def harm2profile(bl, r):
	"""bl[..., nl] -> b(r)[..., nr] = sum_l (2l+1)/(4 pi) b_l P_l(cos r): one m = 0 synthesis on rings of one pixel at
	colatitudes r (curvedsky.harm2profile, curvedsky.py:543-554)"""
	bl = np.asarray(bl); r = np.asarray(r)
	nl = bl.shape[-1]
	kw = _m0_kwargs(r.reshape(-1), nl-1)
	alm = bl*np.sqrt((2*np.arange(nl)+1)/(4*np.pi))+0j
	out = np.zeros(bl.shape[:-1]+(r.size,), bl.dtype)
	for I in nditer(bl.shape[:-1]):
		out[I] = sht.synthesis(alm=np.ascontiguousarray(alm[I][None], dtype=np.complex128), **kw)[0]
	return out

def prof2alm(profile, dir=[0, np.pi/2], spin=0, geometry="CC", nthread=None, norot=False):
	"""alm of a 1-D profile[..., n] sampled on the rings of `geometry` (an azimuthally symmetric field around the pole): one m = 0 analysis_2d of the
	profile as a map one pixel wide, band limit get_ducc_maxlmax(geometry, n) (curvedsky.prof2alm, curvedsky.py:556-580).  norot: the m = 0 layout
	as it is; otherwise expanded to the full triangular layout.  The reference then rotates the pole to dir = [ra, dec] with ducc0.sht.rotate_alm
	(out of this path's scope): only the default direction -- the pole itself, the identity rotation -- is accepted."""
	profile = np.asarray(profile)
	lmax = get_ducc_maxlmax(geometry, profile.shape[-1])
	iainfo = alm_info(lmax=lmax, mmax=0)
	oainfo = alm_info(lmax=lmax, mmax=lmax if not norot else 0)
	if not norot and not (float(dir[0]) == 0.0 and float(dir[1]) == np.pi/2):
		raise NotImplementedError("prof2alm: rotating the profile to dir needs rotate_alm, which is outside the accelerated path")
	ctype = complex_dtype(profile.dtype)
	oalm = np.zeros(profile.shape[:-1]+(oainfo.nelem,), ctype)
	pre = profile.shape[:-1]
	jobs = [(0, (None,))] if len(pre) == 0 else [(s, Ipre+(slice(i1, i2),)) for Ipre in nditer(pre[:-1]) for s, i1, i2 in enmap.spin_helper(spin, pre[-1])]
	for s, I in jobs:
		prof = np.ascontiguousarray(profile[I][..., None])
		alm = np.zeros(prof.shape[:-2]+(iainfo.nelem,), ctype)
		sht.analysis_2d(alm=alm, map=prof, spin=int(s), lmax=lmax, mmax=0, geometry=geometry)
		if not norot: alm = transfer_alm(iainfo, alm, oainfo)
		oalm[I] = alm
	return oalm

# ---------------------------------------------------------------------------------------
# alm post-processing either side of the transforms: almxfl, alm2cl, rand_alm.
# The per-element arithmetic (lmul, alm2cl) runs on the GPU (almops.py -> pxa_*); the random
# numbers come from numpy's legacy global RNG exactly as in the reference, so that a seed gives the
# same alm as pixell (curvedsky.py:61-79, 600-628).
# ---------------------------------------------------------------------------------------
def almxfl(alm, lfilter=None, ainfo=None, out=None):
	"""a_lm * lfilter(l); lfilter is an array starting at l=0 or a function of l (curvedsky.py:630-652)"""
	if not A.is_tensor(alm): alm = np.asarray(alm)
	ainfo = alm_info(nalm=alm.shape[-1]) if ainfo is None else ainfo
	if callable(lfilter):
		l = np.arange(ainfo.lmax+1.0)
		lfilter = lfilter(l)
	return ainfo.lmul(alm, lfilter, out=out)

def alm2cl(alm, alm2=None, ainfo=None, dtype=None):
	"""(cross) power spectrum of alm (and alm2, which must broadcast) (curvedsky.py:674-712)"""
	if not A.is_tensor(alm): alm = np.asarray(alm)
	ainfo = alm_info(nalm=alm.shape[-1]) if ainfo is None else ainfo
	return ainfo.alm2cl(alm, alm2=alm2, dtype=dtype)

def pad_spectrum(ps, lmax):
	ps = np.asarray(ps)
	ops = np.zeros(ps.shape[:-1]+(lmax+1,), ps.dtype)
	ops[..., :ps.shape[-1]] = ps[..., :ps.shape[-1]]
	return ops

def _sym_expand_diag(ps):
	"""powspec.sym_expand(ps, scheme="diag") (powspec.py:22-36, 53-100): [nspec,nl] -> [ncomp,ncomp,nl],
	healpy order: main diagonal first, then successive off-diagonals"""
	n = ps.shape[0]
	ncomp = int(np.ceil((np.sqrt(8*n+1)-1)/2))   # a truncated list: the smallest ncomp whose full list covers it
	which = [(i, i+d) for d in range(ncomp) for i in range(ncomp-d)][:n]
	res = np.zeros((ncomp, ncomp)+ps.shape[1:], ps.dtype)
	for v, (i, j) in zip(ps, which):
		res[i, j] = v; res[j, i] = v
	return res

def prepare_ps(ps, ainfo=None, lmax=None):
	ps = np.asarray(ps)
	if ainfo is None:
		if lmax is None: lmax = ps.shape[-1]-1
		if lmax > ps.shape[-1]-1: ps = pad_spectrum(ps, lmax)
		ainfo = alm_info(lmax)
	if   ps.ndim == 1: wps = ps[None, None]
	elif ps.ndim == 2: wps = _sym_expand_diag(ps)
	elif ps.ndim == 3: wps = ps
	else: raise ValueError("power spectrum must be [nl], [nspec,nl] or [ncomp,ncomp,nl]")
	return wps, ainfo

def _multi_sqrt(wps):
	"""enmap.multi_pow(wps, 0.5) (enmap.py:2021-2024 -> utils.eigpow): matrix square root of each
	[ncomp,ncomp] slice through its eigen-decomposition, negative eigenvalues set to zero.  The power and the product are taken in
	the reference's order of operations (E**0.5, then (V E) V^T), so that the coloured alm of a seed are the reference's bit for bit"""
	A = np.moveaxis(np.asarray(wps, dtype=np.float64), (0, 1), (-2, -1))
	E, V = np.linalg.eigh(A)
	neg = E < 0
	E[~neg] **= 0.5; E[neg] = 0
	res = np.einsum("...ij,...kj->...ik", V*E[..., None, :], V)
	return np.moveaxis(res, (-2, -1), (0, 1))

def fill_gauss(arr, bsize=0x10000):
	rtype = real_dtype(arr.dtype)
	arr = arr.reshape(-1).view(rtype)
	for i in range(0, arr.size, bsize):
		arr[i:i+bsize] = np.random.standard_normal(min(bsize, arr.size-i))

def _transpose_index(ainfo, device=None):
	"""Source and destination positions of alm_info.transpose_alm (cmisc_core.c:116-135): the k-th
	element in storage order (m-major) moves to the k-th (l,m) pair in l-major order.  With `device` the index arrays are built
	there with torch (50 M entries at lmax 10^4: 0.6 s with numpy on the host)."""
	lmax, mmax = ainfo.lmax, ainfo.mmax
	if device is None:
		arange, repeat, cumsum, cat, minimum = np.arange, np.repeat, np.cumsum, np.concatenate, np.minimum
		ms = ainfo.mstart.astype(np.int64); zero = np.zeros(1, np.int64)
	else:
		torch = A.torch()
		arange = lambda n: torch.arange(n, device=device, dtype=torch.int64)
		repeat, cumsum, cat = torch.repeat_interleave, (lambda x: torch.cumsum(x, 0)), torch.cat
		minimum = lambda a, b: torch.clamp(a, max=b)
		ms = torch.as_tensor(ainfo.mstart.astype(np.int64), device=device); zero = torch.zeros(1, device=device, dtype=torch.int64)
	per_m = lmax+1-arange(mmax+1)                                   # number of l per m
	m_src = repeat(arange(mmax+1), per_m)
	l_src = arange(len(m_src))-repeat(cat([zero, cumsum(per_m)[:-1]]), per_m)+m_src
	per_l = minimum(arange(lmax+1), mmax)+1                         # number of m per l
	l_dst = repeat(arange(lmax+1), per_l)
	m_dst = arange(len(l_dst))-repeat(cat([zero, cumsum(per_l)[:-1]]), per_l)
	return ms[m_src]+l_src*ainfo.stride, ms[m_dst]+l_dst*ainfo.stride

def transpose_alm(ainfo, alm, out=None):
	"""alm_info.transpose_alm (curvedsky.py:443-451): reorder numbers generated in l-major order into
	the m-major layout.  alm is out is allowed."""
	if A.is_tensor(alm):
		src, dst = _transpose_index(ainfo, alm.device)
		if out is None: out = alm.clone()
	else:
		src, dst = _transpose_index(ainfo)
		if out is None: out = alm.copy()
	vals = alm[..., src]
	out[..., dst] = vals
	return out
alm_info.transpose_alm = lambda self, alm, out=None: transpose_alm(self, alm, out=out)

def rand_alm_white(ainfo, pre=None, alm=None, seed=None, dtype=np.complex128, m_major=True, rng="numpy"):
	"""unit-variance complex Gaussian numbers for every alm slot.  To give the same alm as pixell for a seed (curvedsky.py:602-628)
	the numbers come from numpy's legacy global RNG, are drawn in l-major order ((l,m) = (0,0), (1,0), (1,1), ...) and are
	then moved to the m-major layout unless m_major is False.
	rng="device" (ours, for throughput: Monte-Carlo loops spend 1.4 s per lmax-10^4 realisation in the host generator): the numbers
	are drawn on the GPU (torch's Philox generator seeded with `seed`) straight into the m-major layout and stay there (a CUDA
	tensor is returned) -- same distribution, NOT the reference's numbers for a seed."""
	if rng == "device":
		torch = A.torch()
		if alm is not None: raise ValueError("rng='device' allocates its own (device) alm")
		g = torch.Generator(device="cuda")
		if seed is not None: g.manual_seed(int(seed))
		else: g.seed()
		shape = (tuple(pre) if pre is not None else ())+(ainfo.nelem, 2)
		rt = torch.float32 if np.dtype(dtype) == np.dtype(np.complex64) else torch.float64
		return torch.view_as_complex(torch.randn(shape, generator=g, dtype=rt, device="cuda"))
	if rng != "numpy": raise ValueError("rng must be 'numpy' or 'device'")
	if seed is not None: np.random.seed(seed)
	if alm is None: alm = np.empty((tuple(pre) if pre is not None else ())+(ainfo.nelem,), dtype)
	fill_gauss(alm)
	if not m_major: return alm
	if not _lib.is_hostsim() and alm.nbytes >= (1 << 24):     # large alm: the reordering as one gather on the GPU (0.6 s of host indexing at lmax 10^4)
		alm[...] = A.host(ainfo.transpose_alm(A.to_gpu(alm)))
		return alm
	return ainfo.transpose_alm(alm, alm)

def rand_alm(ps, ainfo=None, lmax=None, seed=None, dtype=np.complex128, m_major=True, return_ainfo=False, rng="numpy"):
	"""Gaussian alm with (cross) spectrum ps [nl], [nspec,nl] or [ncomp,ncomp,nl] (curvedsky.rand_alm, curvedsky.py:61-79):
	white numbers (rand_alm_white), coloured by the matrix square root of the spectrum on the GPU (alm_info.lmul); the factor
	1/sqrt(2) shares the variance between real and imaginary parts, m = 0 is made real with the full variance.
	rng="device": see rand_alm_white (device-resident result, device generator)."""
	ps = np.asarray(ps)
	wps, ainfo = prepare_ps(ps, ainfo=ainfo, lmax=lmax)
	white = rand_alm_white(ainfo, pre=[wps.shape[0]], seed=seed, dtype=dtype, m_major=m_major, rng=rng)
	colour = (_multi_sqrt(wps)/np.sqrt(2.0)).astype(real_dtype(dtype), copy=False)
	alm = ainfo.lmul(white, colour)
	if A.is_tensor(alm):
		alm[:, :ainfo.lmax+1] = (alm[:, :ainfo.lmax+1].real*np.sqrt(2.0)).to(alm.dtype)
	else:
		m0 = alm[:, :ainfo.lmax+1]                        # the m = 0 column comes first in the m-major layout
		m0.imag = 0; m0.real *= 2**0.5      # (a Python float: single precision alm are scaled in single precision, as the reference's are)
	alm = alm[0] if ps.ndim == 1 else alm
	return (alm, ainfo) if return_ainfo else alm

euler_angs = {}
euler_angs[("gal", "equ")] = np.array([57.06793215, 62.87115487, -167.14056929])*degree
euler_angs[("equ", "gal")] = -euler_angs[("gal", "equ")][::-1]

def rotate_alm(alm, psi, theta, phi, lmax=None, method="auto", nthread=None, inplace=False):
	"""Rotate alm[..., nelem] by the zyz Euler angles psi, theta, phi (curvedsky.py:717-740; see euler_angs): the field f becomes
	f'(n) = f(R^-1 n), R = R_z(phi) R_y(theta) R_z(psi).  Triangular layout (mmax = lmax) only.  Every leading component goes through
	one launch sequence on the GPU (almops.rotate_alm -> pxa_rotate_alm); "auto", "ducc0" and "healpy" all name that same rotation,
	nthread is accepted and ignored.  inplace: alm is overwritten and returned; otherwise it is left as it is."""
	if method is None: raise ValueError("No rotate_alm implementations found")
	if method not in ("auto", "ducc0", "healpy"): raise ValueError("Unrecognized rotate_alm implementation '%s'" % str(method))
	if not A.is_tensor(alm): alm = np.asarray(alm)
	nalm = alm.shape[-1] if alm.ndim else 0
	if lmax is None:
		lmax = nalm2lmax(nalm)
		if (lmax+1)*(lmax+2)//2 != nalm: raise ValueError("rotate_alm: %d elements are not a triangular alm layout" % nalm)
	from . import almops
	return almops.rotate_alm(alm, lmax, psi, theta, phi, inplace=inplace)

def transfer_alm(iainfo, ialm, oainfo, oalm=None, op=lambda a, b: b):
	"""Copy alm between layouts / band limits (curvedsky.py:744-750 -> cmisc.pyx:131-151): for every (l,m) both
	layouts hold, oalm = op(oalm, ialm).  Works on numpy arrays and on torch CUDA tensors (one gather/scatter)."""
	tens = A.is_tensor(ialm)
	if oalm is None:
		oalm = A.zeros(tuple(ialm.shape[:-1])+(oainfo.nelem,), A.np_dtype(ialm), ialm)
	if tuple(ialm.shape[:-1]) != tuple(oalm.shape[:-1]):
		raise ValueError("ialm and oalm must agree on pre-dimensions")
	lmax = min(iainfo.lmax, oainfo.lmax); mmax = min(iainfo.mmax, oainfo.mmax)
	m = np.repeat(np.arange(mmax+1), lmax+1-np.arange(mmax+1))
	first = np.concatenate([[0], np.cumsum(lmax+1-np.arange(mmax+1))[:-1]])
	l = np.arange(len(m))-np.repeat(first, lmax+1-np.arange(mmax+1))+m
	src = iainfo.mstart.astype(np.int64)[m]+l*iainfo.stride
	dst = oainfo.mstart.astype(np.int64)[m]+l*oainfo.stride
	if tens:
		torch = A.torch()
		src = torch.as_tensor(src, device=ialm.device); dst = torch.as_tensor(dst, device=oalm.device)
	oalm[..., dst] = op(oalm[..., dst], ialm[..., src])
	return oalm

def rand_map(shape, wcs, ps, lmax=None, dtype=np.float64, seed=None, spin=[0, 2], method="auto", verbose=False):
	"""Gaussian realisation of the (cross) spectrum ps on the given geometry (curvedsky.rand_map, curvedsky.py:17-37).
	The reference draws its alm with healpy.synalm (healpy is absent here); this uses rand_alm, i.e. the same
	distribution but pixell's own random-number order (SURVEY: 'replace by rand_alm semantics')."""
	ps = np.asarray(ps)
	while ps.ndim < 3: ps = ps[None]
	if ps.shape[0] != ps.shape[1]: raise ValueError("ps must be [ncomp,ncomp,nl] or [nl]")
	if len(shape) not in (2, 3): raise ValueError("shape must be (ncomp,ny,nx) or (ny,nx)")
	ncomp = 1 if len(shape) == 2 else shape[-3]
	ps = ps[:ncomp, :ncomp]
	ctype = np.result_type(dtype, 0j)
	alm = rand_alm(ps, lmax=lmax, seed=seed, dtype=ctype)
	map = enmap.empty((ncomp,)+tuple(shape[-2:]), wcs, dtype=dtype)
	alm2map(alm, map, spin=spin, method=method, verbose=verbose)
	if len(shape) == 2: map = map[0]
	return map

def filter(imap, lfilter, ainfo=None, lmax=None):
	"""alm2map(almxfl(map2alm(imap), lfilter)): isotropic filtering of a map (curvedsky.filter, curvedsky.py:654-671)"""
	alm = map2alm(imap, ainfo=ainfo, lmax=lmax, spin=0)
	alm = almxfl(alm, lfilter=lfilter, ainfo=ainfo)
	out = enmap.dmap(A.torch().empty_like(imap.tensor), imap.wcs) if isinstance(imap, enmap.dmap) else enmap.empty(imap.shape, imap.wcs, dtype=imap.dtype)
	return alm2map(alm, out, spin=0, ainfo=ainfo)
