"""Point sources and other radially symmetric objects on the device: the call signatures of pixell.pointsrcs (pointsrcs.py:35-250, 375-388).

sim_objects paints a catalogue into a map, radial_sum / radial_bin read radial profiles back out around one; both are HIP kernels
(pxm_sim_objects, pxm_radial_sum, csrc/srcsim.hip) that compute the pixel coordinates of a separable cylindrical geometry themselves,
so no position map is made and a device-resident map never leaves the device.  Numpy in gives ndmaps / arrays out; CUDA tensors or a
dmap in give a dmap / tensors out on that device; an omap that is passed in is updated in place.

Where this differs from the reference on purpose: an object is painted on the disc r <= rcut, not on every pixel of
the 8 x 8 cells its bounding box touches; rcut reaches one profile sample further, so that what is left out is below vmin; every radial
bin is complete, the last one included; `op` is honoured; maps may be float64.

Not here: sim_srcs(method="python"), sim_srcs_dist_transform, the catalogue readers and crossmatch."""
import time
import numpy as np
from . import enmap, _lib, _arrays as A, wcs as wcsutils

degree = np.pi/180
_OPS = {"add": 0, "max": 1, "min": 2}
_REAL = (np.dtype(np.float32), np.dtype(np.float64))

def is_equi(r):
	"""whether r[:] = arange(n)*delta, which allows index arithmetic instead of a search (pointsrcs.is_equi, pointsrcs.py:124-128)"""
	r = A.host(r)
	return bool(len(r) > 1 and r[0] == 0 and np.allclose(r[-1], (len(r)-1)*r[1]))

def _profile_tables(profile):
	"""profile [2, n] or a list of such -> (list of float32 [2, n], offsets int32 [nprof+1], rs, vs, vmax float32 [nsamp]);
	vmax[k] = max |vs[j]| over the samples j >= k of the same profile"""
	try: profile[0][0][0]
	except (TypeError, IndexError): profile = [profile]
	profs = [np.ascontiguousarray(A.host(p), dtype=np.float32) for p in profile]
	for p in profs:
		if p.ndim != 2 or p.shape[0] != 2 or p.shape[1] < 1: raise ValueError("a profile must be [{r,b(r)}, nsamp]")
		if np.any(np.diff(p[0]) <= 0): raise ValueError("the radii of a profile must increase")
	off = np.concatenate([[0], np.cumsum([p.shape[1] for p in profs])]).astype(np.int32)
	rs = np.concatenate([p[0] for p in profs]); vs = np.concatenate([p[1] for p in profs])
	vmax = np.concatenate([np.maximum.accumulate(np.abs(p[1])[::-1])[::-1] for p in profs]).astype(np.float32)
	return profs, off, rs, vs, vmax

def sim_objects(shape, wcs, poss, amps, profile, prof_ids=None, omap=None, vmin=None, rmax=None,
		op="add", pixwin=False, pixwin_order=0, separable="auto", transpose=False, prof_equi="auto", cache=None,
		return_times=False):
	"""Paint radially symmetric objects (pointsrcs.sim_objects, pointsrcs.py:35-122).
	shape, wcs: the geometry (separable cylindrical; only shape[-2:] counts); poss [{dec,ra}, nobj] in radians; amps [..., nobj], the
	central amplitudes, whose leading axes are those of the map; profile [{r,b(r)}, nsamp] or a list of such, with prof_ids [nobj]
	choosing one per object (default: the first).  omap: add into (max, min with) this float32 or float64 C-contiguous map [..., ny, nx]
	instead of a new float32 one.  vmin: how faint a value is still worth painting, in map units (default min|amps|*1e-3): object i is
	painted out to rcut_i = r[k+1], k the last profile sample with |b| >= vmin/max|amps[..., i]|, and no further than rmax > 0.
	op: "add" | "max" | "min".  pixwin: apply the pixel window of order pixwin_order afterwards (periodic: wrong at the edges of a patch).
	transpose=True: the transpose of op="add": amps[..., i] += sum over the disc of omap * profile, in place in amps (a float32
	C-contiguous array or tensor; vmin must be given, since rcut follows from the incoming amps); returns omap.
	cache is accepted and not used (no position map is made).  return_times: also return [seconds spent in the call]."""
	t0 = time.time()
	ny, nx, dec0, ddec, ra0, dra = wcsutils.separable_geometry(shape, wcs, separable)
	if op not in _OPS: raise ValueError("op must be one of 'add', 'max', 'min', not %s" % repr(op))
	amps = A.unwrap(amps)
	if transpose:
		if not (A.is_tensor(amps) or isinstance(amps, np.ndarray)): raise ValueError("transpose=True adds into amps in place: it must be an array or tensor")
		if vmin is None: raise ValueError("transpose=True needs vmin: the cut radii follow from the amplitudes that come in")
		if op != "add": raise ValueError("transpose=True is the transpose of op='add'")
		if omap is None: raise ValueError("transpose=True reads omap")
	device = A.device_of(omap, amps, poss)
	pre = tuple(amps.shape[:-1]) if A.is_tensor(amps) else np.shape(amps)[:-1]
	nobj = int(amps.shape[-1]) if A.is_tensor(amps) else int(np.shape(amps)[-1])
	ncomp = int(np.prod(pre, dtype=np.int64))
	d_amps = (A.out_array(amps, amps.shape, _REAL[:1], device, "amps", "") if transpose else A.put(amps, np.float32, device)).reshape(ncomp, nobj)
	poss = A.unwrap(poss)
	if not A.is_tensor(poss): poss = np.asarray(poss)
	if tuple(poss.shape) != (2, nobj): raise ValueError("poss must be [{dec,ra},nobj]")
	d_dec, d_ra = A.put(poss[0], np.float32, device), A.put(poss[1], np.float32, device)
	profs, off, rs, vs, vmax = _profile_tables(profile)
	if prof_ids is not None and not A.is_tensor(prof_ids) and nobj > 0:
		ids = np.asarray(prof_ids)
		if ids.shape != (nobj,) or ids.min() < 0 or ids.max() >= len(profs): raise ValueError("prof_ids must be [nobj] indices into the profile list")
	d_ids = None if prof_ids is None else A.put(prof_ids, np.int32, device)
	if prof_equi == "auto": prof_equi = all(is_equi(p[0]) for p in profs)
	if vmin is None:
		vmin = 0.0 if nobj == 0 or ncomp == 0 else float(abs(d_amps).min())*1e-3
	if rmax is None: rmax = 0
	# the map the kernel works on
	pixshape = (ny, nx)
	if omap is None: work = A.zeros((ncomp,)+pixshape, np.float32, device=device)
	else: work = A.out_array(omap, tuple(pre)+pixshape, _REAL, device, "omap", "[...,ny,nx], where [ny,nx] agrees with shape, and ... agrees with amps").reshape((ncomp,)+pixshape)
	tabs = [A.put(t, t.dtype, device) for t in (off, rs, vs, vmax)]
	_lib.check(_lib.load().pxm_sim_objects(ny, nx, dec0, ddec, ra0, dra, A.ptr(work), A.DT[A.np_dtype(work)], ncomp, ny*nx,
		nobj, A.ptr(d_dec), A.ptr(d_ra), A.ptr(d_amps), nobj, A.ptr(d_ids), len(profs), A.ptr(tabs[0]), len(rs), A.ptr(tabs[1]), A.ptr(tabs[2]), A.ptr(tabs[3]),
		int(bool(prof_equi)), float(vmin), float(rmax), _OPS[op], int(bool(transpose)), A.device_index(), A.current_stream()))
	if transpose: A.result(d_amps, amps); res = omap
	elif omap is not None: res = A.result(work, omap)
	else:
		full = work.reshape(tuple(pre)+pixshape)
		res = enmap.dmap(full, wcs) if device is not None else enmap.ndmap(A.host(full), wcs)
	# NB! Since we're not padding, this fourier operation will have problems at the edges (the reference's remark)
	if pixwin and not transpose: res = enmap.apply_window(res, order=pixwin_order)
	return (res, np.array([time.time()-t0])) if return_times else res

def radial_sum(map, poss, bins, oprofs=None, separable="auto", prof_equi="auto", cache=None, return_times=False):
	"""Sums of the map [..., ny, nx] in the radial bins bins[k] <= r < bins[k+1] (bins [nbin+1], radians, ascending) around the objects at
	poss [{dec,ra}, nobj]: [nobj, ..., nbin], float32 (pointsrcs.radial_sum, pointsrcs.py:130-176).  oprofs: add to this float32
	C-contiguous array instead.  Every bin is complete, the last one too."""
	t0 = time.time()
	if not hasattr(map, "wcs"): raise ValueError("radial_sum needs a map with a geometry (ndmap or dmap)")
	ny, nx, dec0, ddec, ra0, dra = wcsutils.separable_geometry(map.shape, map.wcs, separable)
	mdata = map.tensor if isinstance(map, enmap.dmap) else np.asarray(map)
	poss = A.unwrap(poss)
	device = A.device_of(mdata, poss, oprofs)
	if A.np_dtype(mdata) not in _REAL: mdata = A.astype(mdata, np.float64)
	pre = tuple(mdata.shape[:-2]); ncomp = int(np.prod(pre, dtype=np.int64))
	nobj = int(poss.shape[1])
	hbins = np.ascontiguousarray(A.host(bins), dtype=np.float32)
	nbin = len(hbins)-1
	if nbin < 1 or np.any(np.diff(hbins) < 0): raise ValueError("bins must be at least two ascending edges")
	if prof_equi == "auto": prof_equi = is_equi(hbins)
	d_map = A.put(mdata, None, device).reshape((ncomp, ny, nx))
	d_dec, d_ra = A.put(poss[0], np.float32, device), A.put(poss[1], np.float32, device)
	d_bins = A.put(hbins, np.float32, device)
	if oprofs is None: acc = A.zeros((nobj, ncomp, nbin), np.float32, device=device)
	else: acc = A.out_array(oprofs, (nobj,)+pre+(nbin,), _REAL[:1], device, "oprofs", "[nobj,...,nbin]")
	_lib.check(_lib.load().pxm_radial_sum(ny, nx, dec0, ddec, ra0, dra, A.ptr(d_map), A.DT[A.np_dtype(d_map)], ncomp, ny*nx,
		nobj, A.ptr(d_dec), A.ptr(d_ra), nbin, A.ptr(d_bins), float(hbins[-1]), int(bool(prof_equi)), A.ptr(acc), A.device_index(), A.current_stream()))
	if oprofs is not None: res = A.result(acc, oprofs)
	else:
		res = acc.reshape((nobj,)+pre+(nbin,))
		if device is None: res = A.host(res)
	return (res, np.array([time.time()-t0])) if return_times else res

def radial_bin(map, poss, bins, weights=None, separable="auto", prof_equi="auto", cache=None, return_times=False):
	"""Means of the map in radial bins around the objects, [nobj, ..., nbin]: radial_sum of map*weights over radial_sum of the weights
	(default: ones) (pointsrcs.radial_bin, pointsrcs.py:178-210)"""
	mdata = map.tensor if isinstance(map, enmap.dmap) else np.asarray(map)
	if weights is not None:
		wdata = weights.tensor if isinstance(weights, enmap.dmap) else weights
		if A.is_tensor(mdata) and not A.is_tensor(wdata): wdata = A.torch().as_tensor(np.asarray(wdata), device=mdata.device)
		prod = mdata*wdata
		map = enmap.dmap(prod, map.wcs) if A.is_tensor(prod) else enmap.ndmap(prod, map.wcs)
		wmap = enmap.dmap(wdata, map.wcs) if A.is_tensor(wdata) else enmap.ndmap(np.asarray(wdata), map.wcs)
	elif A.is_tensor(mdata): wmap = enmap.dmap(A.torch().ones(tuple(mdata.shape[-2:]), dtype=mdata.dtype, device=mdata.device), map.wcs)
	else: wmap = enmap.ones(mdata.shape[-2:], map.wcs, mdata.dtype)
	profs, times1 = radial_sum(map, poss, bins, separable=separable, prof_equi=prof_equi, return_times=True)
	div, times2 = radial_sum(wmap, poss, bins, separable=separable, prof_equi=prof_equi, return_times=True)
	# leading axes of the weights broadcast against those of the map
	div = div.reshape(tuple(profs.shape[:1])+(1,)*(profs.ndim-div.ndim)+tuple(profs.shape[-1:])) if div.ndim < profs.ndim else div
	if A.is_tensor(profs): profs /= div
	else:
		with np.errstate(invalid="ignore", divide="ignore"): profs /= div
	return (profs, np.concatenate([times1, times2])) if return_times else profs

def sim_srcs(shape, wcs, srcs, beam, omap=None, dtype=None, nsigma=5, rmax=None, vmin=None, smul=1,
		return_padded=False, pixwin=False, pixwin_order=0, op=np.add, wrap="auto", verbose=False, cache=None,
		separable="auto", method="c"):
	"""The old interface to sim_objects (pointsrcs.sim_srcs with method="c", pointsrcs.py:212-250): srcs [nsrc, {dec,ra,amps...}], beam a
	Gaussian sigma in radians or a profile [{r,b(r)}, n].  float32 maps, smul = 1, no padding; op: add, max or min."""
	if method == "python": raise NotImplementedError("sim_srcs: method 'python' is not implemented; use method='c'")
	if method not in ["c", "C"]: raise ValueError("method must be 'c' or 'python'")
	if not (dtype is None or np.dtype(dtype) == np.float32): raise ValueError("method 'c' only supports float32")
	if smul != 1: raise ValueError("method 'c' does not support smul != 1")
	if vmin is None: vmin = np.exp(-0.5*nsigma**2)
	if op is np.add or op == "add" or op is getattr(np.ndarray, "__iadd__", None): op_ = "add"
	elif op is np.max or op is np.maximum or op == "max": op_ = "max"
	elif op is np.min or op is np.minimum or op == "min": op_ = "min"
	else: raise ValueError("method 'c' only supports op add, max or min")
	if return_padded: raise ValueError("method 'c' does not support return_padded")
	srcs = A.host(srcs)
	ncomp = int(np.prod(shape[:-2], dtype=int))
	nobj = len(srcs)
	poss = srcs.T[:2]
	amps = np.zeros((ncomp, nobj), np.float32)
	amps[:srcs.shape[1]-2] = srcs.T[2:2+ncomp]
	amps = amps.reshape(tuple(shape[:-2])+(nobj,))
	beam = expand_beam(beam, nsigma, rmax)
	return sim_objects(shape, wcs, poss, amps, beam, omap=omap, vmin=vmin, rmax=rmax, op=op_, pixwin=pixwin, pixwin_order=pixwin_order, separable=separable, cache=cache)

def expand_beam(beam, nsigma=5, rmax=None, nper=400):
	"""a Gaussian sigma -> the profile [{r,b(r)}, nsigma*nper] out to rmax (default nsigma sigma); a profile passes through (pointsrcs.py:375-385)"""
	beam = np.asarray(A.host(beam))
	if beam.ndim == 0:
		sigma = beam.reshape(-1)[0]
		if rmax is None: rmax = sigma*nsigma
		r = np.linspace(0, rmax, nsigma*nper)
		return np.array([r, np.exp(-0.5*(r/sigma)**2)])
	elif beam.ndim == 2: return beam
	else: raise ValueError("a beam is a Gaussian sigma or a profile [{r,b(r)},n]")

def nsigma2rmax(beam, nsigma):
	"""the radius at which the profile last reaches exp(-nsigma^2/2) (pointsrcs.py:387-388)"""
	return beam[0, np.where(beam[1] >= np.exp(-0.5*nsigma**2))[0][-1]]
