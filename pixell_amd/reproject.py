"""Catalogue cut-outs on the device: the reference's reproject.thumbnails / thumbnails_ivar (pixell/reproject.py:10-116), the first step of
stacking.  For every object of a catalogue a small map on a geometry centred on (0, 0), with the object moved to that centre and Q/U
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
import numpy as np
from . import _lib, _arrays as A, enmap, interpol, wcs as wcsutils

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
