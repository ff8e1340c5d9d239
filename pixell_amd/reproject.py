"""Reprojection on the device: catalogue cut-outs (thumbnails / thumbnails_ivar, pixell/reproject.py:10-116) and healpix <-> CAR
(map2healpix / healpix2map with rot2euler, inv_euler and restrict_nside, pixell/reproject.py:118-417).

healpix <-> CAR.  method="harm" composes curvedsky.map2alm / map2alm_healpix, rotate_alm(inplace=True) and alm2map_healpix / alm2map; the
alm is made, rotated and read on the device, for host maps too.  method="spline" is one fused launch per leading index of the map
(csrc/healpix.hip): pxm_map2healpix turns every healpix pixel into its centre, rotates it, finds the CAR pixel, gathers the spline taps
of all components and rotates every spin pair by the closed-form angle; pxm_healpix2map does the same from every CAR pixel into the
healpix map (containing pixel or ring-bilinear value, pixell_amd.healpix).  No position array and no angle array is made, so the
reference's bsize batching has nothing to do here: bsize and verbose are accepted and ignored.  The spline route needs a separable CAR
geometry.  healpy is not used; the healpix definitions are those of pixell_amd.healpix.

Catalogue cut-outs.  For every object of a catalogue a small map on a geometry centred on (0, 0), with the object moved to that centre and Q/U
rotated to the local north there: one launch of pxm_thumbnails (csrc/thumbs.hip) for the whole catalogue, which turns every thumbnail
pixel into a direction, rotates it onto the object, finds the input pixel, gathers the spline taps of all components and rotates Q/U
by the analytic parallactic angle.  No position map and no angle map is made, on the host or on the device.

What the result is (and where it differs from the reference on purpose): the reference cuts an apodised, median-filled
box out of the map for every object and interpolates that (by default after oversampling it by FFT); here the WHOLE map is prefiltered
once and every thumbnail reads it directly:
    utils.interpol(map, map.sky2pix(ipos)), ipos, ang = coordinates.transform("cel", ["cel", [[0, 0, ra, dec], False]], posmap(oshape, owcs)[::-1], pol=pol)
followed by enmap.rotate_pol(., -ang).  `apod` is accepted and has no effect.  The RA axis of a map that goes round the sky
(nx |cdelt_x| = 360 degrees) is read with border "grid-wrap" on coefficients that are periodic along x; every other axis with border
"constant", cval 0.  Thumbnail geometries are CAR or TAN (wcs.TanWCS) centred on (0, 0)."""
import ctypes
import numpy as np
from . import _lib, _arrays as A, curvedsky, enmap, healpix, interpol, wcs as wcsutils

degree = np.pi/180
arcmin = degree/60
_PROJ = {"car": 0, "tan": 1}

def _refuse(method, oversample, filter, pixwin):
	"""the options of the reference that act on its per-object cut-outs, which do not exist here"""
	if method not in ("spline", "mixed", "nufft"): raise ValueError("Unrecognized method '%s'" % str(method))
	if method == "nufft": raise NotImplementedError("thumbnails: method=\"nufft\" is not implemented on the device; pass method=\"spline\"")
	if method == "mixed" and oversample > 1:
		raise NotImplementedError("thumbnails: method=\"mixed\" oversamples every cut-out by FFT, which is not implemented on the device; pass method=\"spline\" (or oversample=1)")
	if filter is not None: raise NotImplementedError("thumbnails: filter= acts on the reference's per-object cut-outs, which are not made here; filter the map before the call and pass filter=None")
	if pixwin: raise NotImplementedError("thumbnails: pixwin=True deconvolves the window of every cut-out; call enmap.unapply_window on the map before and pass pixwin=False")

def borders(shape, wcs):
	"""the borders (y, x) a map of this geometry is read with: "grid-wrap" along x if the columns go round the sky, "constant" otherwise"""
	wrap = abs(int(shape[-1])*abs(float(wcs.wcs.cdelt[0]))-360.0) < 1e-9
	return ("constant", "grid-wrap" if wrap else "constant")

def _divided(imap, psize):
	"""imap divided (or, with 1/psize, multiplied) by the host array psize [ny, 1], where imap lives"""
	data = interpol._raw(imap)
	dt = A.np_dtype(data)
	if dt not in (np.dtype(np.float32), np.dtype(np.float64)): dt = np.dtype(np.float64)
	psize = np.asarray(psize, np.float64).astype(dt)
	if A.is_tensor(data): return data.to(A.tdtype(dt))/A.torch().from_numpy(psize).to(data.device)
	return data.astype(dt)/psize

def interpolator(imap, order=3, extensive=False):
	"""The interpol.interpolator thumbnails makes of imap [..., ny, nx] when it is given none: the borders of borders(), cval 0, the
	prefilter (order 3) along x periodic if the columns go round the sky; extensive: of the map divided by its pixel areas.  Make it
	once and pass it as ip= to read a long catalogue in chunks."""
	enmap._need_separable(imap.wcs, "thumbnails")
	data = _divided(imap, enmap.pixsizemap(imap.shape, imap.wcs, broadcastable=True)) if extensive else imap
	return interpol.interpolator(data, npre=imap.ndim-2, order=order, border=borders(imap.shape, imap.wcs), cval=0.0)

def _launch(ip, d_obj, nobj, affine, rewind, oshape, owcs, pol, out, first, nmap):
	"""maps first .. first + nmap - 1 of ip's array -> out [nobj, nmap, oy, ox]; pol: the last two of them are Q, U"""
	ny, nx = int(ip.arr.shape[-2]), int(ip.arr.shape[-1])
	dt = A.np_dtype(ip.arr)
	by, bx = ip.border if isinstance(ip.border, tuple) else (ip.border, ip.border)
	(yoff, yscale), (xoff, xscale) = affine; (yref, yper), (xref, xper) = rewind
	w = owcs.wcs
	_lib.check(_lib.load().pxm_thumbnails(nmap, ny, nx, A.ptr(ip.arr)+first*ny*nx*dt.itemsize, interpol._DT[dt], ny*nx,
		float(yoff), float(yscale), float(xoff), float(xscale), float(yref), float(yper), float(xref), float(xper),
		nobj, A.ptr(d_obj), int(oshape[0]), int(oshape[1]), _PROJ[wcsutils.get_proj(owcs)], float(w.cdelt[1]), float(w.crpix[1]), float(w.cdelt[0]), float(w.crpix[0]),
		ip.order, interpol.BORDERS[by], interpol.BORDERS[bx], ip.cval, int(bool(pol)), nmap-2 if pol else 0, nmap-1 if pol else 0,
		A.ptr(out), A.device_index(), A.current_stream()))

def thumbnails(imap, coords, r=5*arcmin, res=None, proj=None, apod=2*arcmin, method="spline", order=3, oversample=4, pol=None, oshape=None, owcs=None,
		extensive=False, verbose=False, filter=None, pixwin=False, pixwin_order=0, ip=None):
	"""Thumbnails [..., {pre}, oy, ox] of imap [{pre}, ny, nx] (an ndmap or a dmap on a separable CAR geometry) centred on the positions
	coords [..., {dec,ra}] in radians (host or device): reproject.thumbnails (reproject.py:10-105), the whole catalogue in one launch.
	oshape, owcs: the thumbnails' geometry, centred on (0, 0) (enmap.thumbnail_geometry); without them a geometry in projection proj
	("car", the default as in the reference, or "tan") of radius r and resolution res (default: half the map's smallest pixel pitch).
	order 0, 1 or 3.  pol: rotate Q, U (the last two of three components) to the local north of the thumbnail; the default is to do
	so where imap.shape[-3] == 3.  extensive: the map holds a quantity per pixel (it is divided by its pixel areas before and
	multiplied by the thumbnails' after; CAR thumbnails only).  ip: an interpolator(imap, ...) of this module to use again (the
	prefilter then does not run; with extensive it must have been made with extensive=True).  The result is float64 at order 3 and has
	the map's dtype otherwise; numpy arrays for host maps and host coords, tensors otherwise, wrapped as an ndmap / a dmap with owcs.
	Every thumbnail interpolates the whole prefiltered map (the module's docstring); apod has no effect, and method="mixed" with
	oversample > 1, method="nufft", filter= and pixwin=True raise NotImplementedError."""
	_refuse(method, oversample, filter, pixwin)
	if proj is None: proj = "car"
	enmap._need_separable(imap.wcs, "thumbnails")
	cdata = interpol._raw(coords)
	if cdata.ndim < 1 or cdata.shape[-1] != 2: raise ValueError("coords must be [..., {dec,ra}]")
	ishape = tuple(int(n) for n in cdata.shape[:-1])
	if oshape is None:
		if res is None: res = min(np.abs(imap.wcs.wcs.cdelt))*degree/2
		oshape, owcs = enmap.thumbnail_geometry(r=r, res=res, proj=proj)
	oshape = (int(oshape[-2]), int(oshape[-1]))
	oproj = wcsutils.get_proj(owcs)
	if oproj not in _PROJ: raise NotImplementedError("thumbnails: thumbnail geometries are CAR or TAN, not \"%s\"" % oproj)
	if np.any(np.asarray(owcs.wcs.crval, float) != 0): raise ValueError("thumbnails: the thumbnail geometry must be centred on (0, 0)")
	if extensive and oproj != "car":
		raise NotImplementedError("thumbnails: extensive=True needs the pixel areas of the thumbnail geometry, which are exact for proj=\"car\" only (the reference's are wrong for \"tan\"); pass proj=\"car\"")
	pol_compat = imap.ndim >= 3 and imap.shape[-3] == 3
	if pol is None: pol = pol_compat
	if pol and not pol_compat: raise ValueError("Polarization rotation requested, but can't interpret map shape %s as IQU map" % (str(tuple(imap.shape))))
	pre = tuple(int(n) for n in imap.shape[:-2])
	if ip is None: ip = interpolator(imap, order=order, extensive=extensive)
	elif tuple(ip.arr.shape) != tuple(imap.shape) or ip.npre != len(pre): raise ValueError("ip is not an interpolator of this map")
	nobj = int(np.prod(ishape, dtype=np.int64))
	if verbose: print("Extracting %d %dx%d thumbnails from %s map" % (nobj, oshape[0], oshape[1], str(tuple(imap.shape))))
	device = ip.device if ip.device is not None else A.device_of(cdata)
	d_obj = A.put(cdata.reshape(-1, 2), np.float64, A.device_of(ip.arr))
	w = imap.wcs.wcs
	affine = tuple((float(-w.crval[k]/w.cdelt[k]+w.crpix[k]-1), float(1.0/(degree*w.cdelt[k]))) for k in (1, 0))
	rewind = enmap._rewind_of(imap.shape, imap.wcs, True)
	nmap = int(np.prod(pre, dtype=np.int64))
	dt = A.np_dtype(ip.arr)
	if not pol or len(pre) == 1:
		work = A.empty((nobj,)+pre+oshape, dt, like=ip.arr)
		_launch(ip, d_obj, nobj, affine, rewind, oshape, owcs, pol, work, 0, nmap)
	else:      # [{lead}, 3, ny, nx]: one launch per leading entry, each rotating its own Q, U
		lead = nmap//3
		parts = [A.empty((nobj, 3)+oshape, dt, like=ip.arr) for _ in range(lead)]
		for k, part in enumerate(parts): _launch(ip, d_obj, nobj, affine, rewind, oshape, owcs, True, part, 3*k, 3)
		work = (A.torch().stack(parts, 1) if A.is_tensor(parts[0]) else np.stack(parts, 1)).reshape((nobj,)+pre+oshape)
	if extensive: work = _divided(work, 1.0/np.asarray(enmap.pixsizemap(oshape, owcs, broadcastable=True)))
	work = interpol._as_kind(work.reshape(ishape+pre+oshape), device)
	return enmap.dmap(work, owcs) if A.is_tensor(work) else enmap.ndmap(work, owcs)

def thumbnails_ivar(imap, coords, r=5*arcmin, res=None, proj=None, oshape=None, owcs=None, order=1, extensive=True, verbose=False):
	"""thumbnails for hit counts, inverse variances, masks and other quantities that should stay positive and local: linear interpolation,
	no polarisation rotation, extensive by default (reproject.thumbnails_ivar, reproject.py:107-116)"""
	return thumbnails(imap, coords, r=r, res=res, proj=proj, oshape=oshape, owcs=owcs, order=order, oversample=1, pol=False, extensive=extensive,
		verbose=verbose, pixwin=False)

# ---- healpix <-> CAR (reproject.py:118-417) ---------------------------------------------------------------------------------------------
_F32, _F64 = np.dtype(np.float32), np.dtype(np.float64)
_gal2cel = np.array([57.06793215, 62.87115487, -167.14056929])*degree

def rot2euler(rot):
	"""the zyz Euler angles of a rotation given as those angles or as a string "isys,osys" of "cel" / "equ" / "gal" (reproject.py:363-384)"""
	if isinstance(rot, str):
		from scipy.spatial.transform import Rotation
		try: isys, osys = rot.split(",")
		except ValueError: raise ValueError("Rotation string must be of form 'isys,osys', but got '%s'" % str(rot))
		R = Rotation.identity()
		if isys in ["cel", "equ"]: pass
		elif isys == "gal": R *= Rotation.from_euler("zyz", _gal2cel)
		else: raise ValueError("Unrecognized system '%s'" % isys)
		if osys in ["cel", "equ"]: pass
		elif osys == "gal": R *= Rotation.from_euler("zyz", _gal2cel).inv()
		else: raise ValueError("Unrecognized system '%s'" % osys)
		return R.as_euler("zyz")
	return np.asarray(rot, dtype=np.float64)

def inv_euler(euler): return [-euler[2], -euler[1], -euler[0]]

def restrict_nside(nside, mode="mul32", round="ceil"):
	"""nside restricted to a power of two ("pow2"), to a multiple of 32 unless 12 nside^2 <= 1024 ("mul32"), or just rounded ("any"); at
	least 1 (reproject.py:388-417)"""
	if isinstance(round, str): round = {"floor": np.floor, "round": np.round, "ceil": np.ceil}[round]
	if mode == "any": nside = round(nside)
	elif mode == "mul32":
		if 12*nside**2 > 1024: nside = round(nside/32)*32
	elif mode == "pow2": nside = 2**round(np.log2(nside))
	else: raise ValueError("Unrecognized nside mode '%s'" % str(mode))
	return max(1, int(nside))

def _rotmat(rot):
	"""The matrix M that takes the direction of an output pixel to where the input is read, or None: what
	coordinates.transform_euler(inv_euler(rot2euler(rot))[::-1], pos) applies, M = Rz(a) Ry(b) Rz(c) for those angles [a, b, c]
	(coordinates.euler_mat)"""
	if rot is None: return None
	a, b, c = inv_euler(rot2euler(rot))[::-1]
	def Rz(t): return np.array([[np.cos(t), -np.sin(t), 0], [np.sin(t), np.cos(t), 0], [0, 0, 1]])
	def Ry(t): return np.array([[np.cos(t), 0, np.sin(t)], [0, 1, 0], [-np.sin(t), 0, np.cos(t)]])
	return Rz(a).dot(Ry(b)).dot(Rz(c))

def _c_rot(M): return None if M is None else (ctypes.c_double*9)(*[float(v) for v in np.asarray(M).reshape(-1)])
def _c_pairs(spin, ncomp, stokes):
	"""(npair, int [npair][2] = (first component, spin)) of the spin pairs among the ncomp components of a Stokes axis"""
	flat = [int(v) for s, c1, c2 in (enmap.spin_helper(spin, ncomp) if stokes else ()) if s != 0 for v in (c1, s)]
	return len(flat)//2, ((ctypes.c_int*len(flat))(*flat) if flat else None)

def _float_data(x):
	"""the raw array of a map or healpix map with a dtype the kernels read: float32 stays, everything else becomes float64"""
	data = interpol._raw(x)
	return data if A.np_dtype(data) in (_F32, _F64) else A.astype(data, _F64)

def _check_out(out, shape, dt, device, what):
	odata = interpol._raw(out)
	if A.device_of(odata) != device: raise ValueError("%s: the input and out live on different devices" % what)
	if tuple(odata.shape) != tuple(shape) or A.np_dtype(odata) != dt: raise ValueError("%s: out must be %s of shape %s" % (what, np.dtype(dt).name, str(tuple(shape))))
	return odata

def _deliver(work, odata, out, device):
	"""what the caller gets of the array `work` the kernels wrote: `out` filled, or a new array of the caller's kind"""
	if out is None: return interpol._as_kind(work, device)
	if A.ptr(work) != A.ptr(odata): odata[...] = work if A.is_tensor(odata) else A.host(work)
	return out

def _stokes_launches(pre):
	"""(components per launch, launches) of a map with the leading shape pre: the last leading axis is the Stokes axis"""
	ncomp = int(pre[-1]) if pre else 1
	if ncomp > 32: raise NotImplementedError("at most 32 components along the Stokes axis")
	return ncomp, int(np.prod(pre[:-1], dtype=np.int64))

def _harm(alm, rot):
	"""the alm as the output's transform reads it: rotated in place, where it lies"""
	if rot is not None: curvedsky.rotate_alm(alm, *rot2euler(rot), inplace=True)
	return alm

def _harm_map2alm(data, wcs, lmax, spin, niter):
	"""the alm of a map [..., ny, nx] (a raw host or device array): made on the device, and it stays there"""
	d = A.put(data)
	return curvedsky.map2alm(enmap.dmap(d, wcs) if A.is_tensor(d) else enmap.ndmap(d, wcs), lmax=lmax, spin=spin, niter=niter)

def _harm_heal2alm(data, lmax, spin, niter):
	"""the alm of a healpix map [..., npix]: made on the device, and it stays there"""
	return curvedsky.map2alm_healpix(A.put(data), lmax=lmax, spin=spin, niter=niter)

def _bad_method(method): return ValueError("Map reprojection method '%s' not recognized" % str(method))

def map2healpix(imap, nside=None, lmax=None, out=None, rot=None, spin=[0,2], method="harm", order=1, extensive=False, bsize=100000, nside_mode="pow2",
		boundary="constant", verbose=False, niter=0):
	"""The healpix map [..., npix] (RING) of imap [..., ny, nx], an ndmap or a dmap with Stokes along its third-last axis: reproject.map2healpix
	(reproject.py:118-247).  nside: of the result (default: the map's resolution, restricted by nside_mode "pow2" | "mul32" | "any");
	out: an array [..., npix] of the map's dtype where the map lives, filled and returned.  rot: None, "isys,osys" of "cel" / "equ" /
	"gal", or three zyz Euler angles.  spin: of the entries of the Stokes axis ([0] to treat none as a pair).  method "harm" (lmax: default
	the map's Nyquist limit; niter) or "spline" (order 0, 1 or 3; boundary: a border of interpol.BORDERS; separable CAR geometries only).
	extensive: the map holds a quantity per pixel.  The result has the map's dtype (order 3 is computed in float64 and cast at the store):
	a numpy array for an ndmap, a tensor on its device for a dmap.  bsize and verbose are accepted and ignored."""
	if method not in ("harm", "harmonic", "spline"): raise _bad_method(method)
	data = _float_data(imap)
	dt, device = A.np_dtype(data), A.device_of(data)
	pre = tuple(int(n) for n in data.shape[:-2])
	ires = np.mean(np.abs(imap.wcs.wcs.cdelt))*degree
	if out is None:
		if nside is None: nside = restrict_nside(((4*np.pi/ires**2)/12)**0.5, nside_mode)
		npix, odata = healpix.nside2npix(nside), None
	else:
		npix = int(out.shape[-1])
		odata = _check_out(out, pre+(npix,), dt, device, "map2healpix")
	nside = healpix.npix2nside(npix)
	opixsize = 4*np.pi/npix
	if method != "spline":
		if lmax is None: lmax = np.pi/ires
		if extensive: data = _divided(data, np.asarray(enmap.pixsizemap(imap.shape, imap.wcs, broadcastable=True))/opixsize)
		alm = _harm(_harm_map2alm(data, imap.wcs, int(lmax), spin, niter), rot)
		work = A.put(odata) if odata is not None and A.is_contiguous(odata) else A.zeros(pre+(npix,), dt, like=alm)
		curvedsky.alm2map_healpix(alm, work, spin=spin)
		return _deliver(work, odata, out, device)
	if boundary not in interpol.BORDERS: raise ValueError("Unrecognized border '%s'" % str(boundary))
	enmap._need_separable(imap.wcs, "map2healpix(method=\"spline\")")
	ncomp, lead = _stokes_launches(pre)
	src = _divided(data, enmap.pixsizemap(imap.shape, imap.wcs, broadcastable=True)) if extensive else data      # (times opixsize: the kernel's scalar)
	ip = interpol.interpolator(src, npre=len(pre), order=order, border=boundary, cval=0.0)
	ny, nx = int(data.shape[-2]), int(data.shape[-1])
	cdt = A.np_dtype(ip.arr)
	work = A.put(odata) if odata is not None and A.is_contiguous(odata) else A.empty(pre+(npix,), dt, like=ip.arr)
	w = imap.wcs.wcs
	(yoff, yscale), (xoff, xscale) = tuple((float(-w.crval[k]/w.cdelt[k]+w.crpix[k]-1), float(1.0/(degree*w.cdelt[k]))) for k in (1, 0))
	(yref, yper), (xref, xper) = enmap._rewind_of(imap.shape, imap.wcs, True)
	M = _c_rot(_rotmat(rot))
	npair, pairs = _c_pairs(spin, ncomp, len(pre) > 0)
	lib, dev, st = _lib.load(), A.device_index(), A.current_stream()
	for k in range(lead):
		_lib.check(lib.pxm_map2healpix(ncomp, ny, nx, A.ptr(ip.arr)+k*ncomp*ny*nx*cdt.itemsize, interpol._DT[cdt], ny*nx,
			yoff, yscale, xoff, xscale, float(yref), float(yper), float(xref), float(xper), ip.order, interpol.BORDERS[boundary], interpol.BORDERS[boundary], 0.0,
			nside, 0, npix, M, npair, pairs, float(opixsize) if extensive else 1.0, A.ptr(work)+k*ncomp*npix*dt.itemsize, interpol._DT[dt], npix, dev, st))
	return _deliver(work, odata, out, device)

def healpix2map(iheal, shape=None, wcs=None, lmax=None, out=None, rot=None, spin=[0,2], method="harm", order=1, extensive=False, bsize=100000, verbose=False, niter=0):
	"""The map [..., ny, nx] on the geometry (shape, wcs), or filling the map out, of the healpix map iheal [..., npix] (RING, Stokes along its
	second-last axis; a numpy array or a tensor): reproject.healpix2map (reproject.py:249-361).  rot, spin, extensive, niter: as in
	map2healpix.  method "harm" (lmax: default 3 nside) or "spline" (order 0: the pixel that holds the direction, 1: the ring-bilinear value
	of pixell_amd.healpix; separable CAR geometries only).  An ndmap for host input, a dmap on its device for a tensor; bsize and verbose
	are accepted and ignored."""
	if method not in ("harm", "harmonic", "spline"): raise _bad_method(method)
	data = _float_data(iheal)
	dt, device = A.np_dtype(data), A.device_of(data)
	pre = tuple(int(n) for n in data.shape[:-1])
	npix = int(data.shape[-1])
	nside = healpix.npix2nside(npix)
	ipixsize = 4*np.pi/npix
	if out is None:
		if shape is None or wcs is None: raise ValueError("healpix2map needs shape and wcs, or out")
		oshape, odata = pre+(int(shape[-2]), int(shape[-1])), None
	else:
		wcs, oshape = out.wcs, pre+tuple(int(n) for n in out.shape[-2:])
		odata = _check_out(out, oshape, dt, device, "healpix2map")
	rowfac = np.asarray(enmap.pixsizemap(oshape, wcs, broadcastable=True), np.float64)[:, 0]/ipixsize if extensive else None
	def wrap(res): return out if out is not None else (enmap.dmap(res, wcs) if A.is_tensor(res) else enmap.ndmap(res, wcs))
	if method != "spline":
		if lmax is None: lmax = 3*nside
		alm = _harm(_harm_heal2alm(data, int(lmax), spin, niter), rot)
		work = A.put(odata) if odata is not None and A.is_contiguous(odata) else A.zeros(oshape, dt, like=alm)
		curvedsky.alm2map(alm, enmap.dmap(work, wcs) if A.is_tensor(work) else enmap.ndmap(work, wcs), spin=spin)
		if extensive: work *= A.torch().as_tensor(rowfac.astype(dt), device=work.device)[:, None] if A.is_tensor(work) else rowfac.astype(dt)[:, None]
		return wrap(_deliver(work, odata, out, device))
	if order > 1: raise ValueError("Only order 0 and order 1 spline interpolation supported from healpix maps")
	ny, nx, dec0, ddec, ra0, dra = wcsutils.separable_geometry(oshape, wcs)
	ncomp, lead = _stokes_launches(pre)
	d = A.put(data, dt, device)
	work = A.put(odata) if odata is not None and A.is_contiguous(odata) else A.empty(oshape, dt, like=d)
	d_fac = None if rowfac is None else A.put(rowfac, np.float64, A.device_of(d))
	M = _c_rot(_rotmat(rot))
	npair, pairs = _c_pairs(spin, ncomp, len(pre) > 0)
	lib, dev, st = _lib.load(), A.device_index(), A.current_stream()
	for k in range(lead):
		_lib.check(lib.pxm_healpix2map(ncomp, nside, A.ptr(d)+k*ncomp*npix*dt.itemsize, interpol._DT[dt], npix, ny, nx, dec0, ddec, ra0, dra, int(order), M, npair, pairs,
			A.ptr(d_fac), A.ptr(work)+k*ncomp*ny*nx*dt.itemsize, dev, st))
	return wrap(_deliver(work, odata, out, device))
