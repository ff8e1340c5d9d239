"""Distances from points and the edges of masks on the device: what the reference's pixell.distances (cython/distances.pyx over
distances_core.c) gives enmap.distance_from, distance_transform and labeled_distance_transform.

find_edges / find_edges_labeled list the edge pixels of a mask or a label map; distance_from_points gives every pixel of a separable
cylindrical geometry its distance from the nearest of a set of points, and the index of that point.  Both are HIP kernels (pxm_find_edges,
pxm_distance_from, csrc/distance.hip) that compute pixel coordinates themselves in FP64, so no position map is made and a device-resident
mask never leaves the device.  Numpy in gives numpy arrays / ndmaps out; CUDA tensors or a dmap in give tensors / a dmap out on that
device; an omap or odomains that is passed in is filled in place.

Where this differs from the reference on purpose: the distances are exact for every `method` (the reference's default
"cellgrid" propagates a front from pixel to pixel and is not), edges come in ascending order and each once, and points may lie anywhere."""
import ctypes
import numpy as np
from . import enmap, sht
from .sht import _is_tensor, _np_dtype
from .pointsrcs import _geometry, _device_of, _put, _host, _ptr

TILE = 16      # the kernel's tile: return_stats counts visits per TILE x TILE pixels

def _new(shape, dtype, device):
	"""an uninitialised array where the library writes: numpy in the simulator when nothing came as a tensor, a tensor otherwise"""
	if device is None and sht._lib.is_hostsim(): return np.empty(shape, dtype)
	torch = sht._torch()
	if device is None: sht.device_index()
	return torch.empty(tuple(shape), dtype=getattr(torch, np.dtype(dtype).name), device=device if device is not None else "cuda")

def _edges(arr, labeled, flat):
	if isinstance(arr, enmap.dmap): arr = arr.tensor
	if not _is_tensor(arr): arr = np.asarray(arr)
	if arr.ndim != 2: raise ValueError("find_edges needs a 2-D array")
	device = _device_of(arr)
	ny, nx = int(arr.shape[0]), int(arr.shape[1])
	if labeled: d = _put(arr, np.int32, device)
	else: d = _put(arr if enmap._np_any(arr) in (np.dtype(np.uint8), np.dtype(bool)) else (arr != 0), np.uint8, device)
	lib = sht._lib.load(); dev = sht.device_index(); st = sht.current_stream()
	n = ctypes.c_int64(0)
	sht._lib.check(lib.pxm_find_edges(ny, nx, _ptr(d), int(labeled), None, 0, ctypes.byref(n), dev, st))
	out = _new((n.value,), np.int64, device)
	if n.value > 0: sht._lib.check(lib.pxm_find_edges(ny, nx, _ptr(d), int(labeled), _ptr(out), n.value, None, dev, st))
	if device is None: out = _host(out)
	if flat: return out
	return (out//nx, out % nx)

def find_edges(mask, flat=False):
	"""The pixels at the edge of the zero regions of mask [ny, nx]: value 0, and on the border of the array or with a non-zero 4-neighbour
	(distances.find_edges, distances.pyx:275-303).  flat: ascending indices into the flattened mask (int64); otherwise (y[:], x[:]) in
	that order.  Each edge pixel comes once (the reference lists three of the corners twice, and the border first)."""
	return _edges(mask, False, flat)

def find_edges_labeled(labels, flat=False):
	"""The pixels at the edge of the regions of constant non-zero value of labels [ny, nx] (int32): non-zero, and on the border or with a
	4-neighbour of another value (distances.find_edges_labeled, distances.pyx:305-333); the output as for find_edges."""
	return _edges(labels, True, flat)

def distance_from_points(shape, wcs, points=None, pix=None, rmax=None, omap=None, odomains=None, domains=False, skip=None, return_stats=False):
	"""The distance (radians) of every pixel of the separable cylindrical geometry (shape, wcs) from the nearest of the points, exact,
	[ny, nx] float64 unless omap says otherwise.  points [{dec,ra}, npoint] in radians, anywhere on the sphere, or pix [npoint]: flat pixel
	indices of this geometry (int64; no coordinate list is made).  rmax: pixels further away than this get rmax and domain -1.  omap: a
	float32 or float64 C-contiguous [ny, nx] map to fill; odomains: an int32 one; domains: also return the index of the nearest point (the
	lowest among equals).  skip: a [ny, nx] map; pixels where it is 0 get distance 0 and domain -1 without a search.  return_stats: also
	return int32 [ceil(ny/16), ceil(nx/16)]: the number of points each 16 x 16 pixel tile looked at.
	Returns omap[, odomains][, stats]."""
	ny, nx, dec0, ddec, ra0, dra = _geometry(shape, wcs, "auto")
	if (points is None) == (pix is None): raise ValueError("distance_from_points needs either points or pix")
	if isinstance(points, enmap.dmap): points = points.tensor
	if isinstance(skip, enmap.dmap): skip = skip.tensor
	device = _device_of(omap, odomains, points, pix, skip)
	d_dec = d_ra = d_pix = None
	if pix is not None:
		if not _is_tensor(pix): pix = np.asarray(pix)
		d_pix = _put(pix.reshape(-1), np.int64, device); npoint = int(d_pix.shape[0])
	else:
		if not _is_tensor(points): points = np.asarray(points, float)
		if points.ndim == 1: points = points[:, None]
		if points.ndim != 2 or points.shape[0] != 2: raise ValueError("points must be [{dec,ra},npoint]")
		d_dec, d_ra = _put(points[0], np.float64, device), _put(points[1], np.float64, device); npoint = int(points.shape[1])
	d_skip = None
	if skip is not None:
		if tuple(skip.shape) != (ny, nx): raise ValueError("skip must be [ny,nx]")
		d_skip = _put(skip if enmap._np_any(skip) in (np.dtype(np.uint8), np.dtype(bool)) else (skip != 0), np.uint8, device)
	def out_array(given, dtypes, default, name):
		"""(the array the kernel writes, the caller's array or None)"""
		if given is None: return _new((ny, nx), default, device), None
		data = given.tensor if isinstance(given, enmap.dmap) else given
		dt = enmap._np_any(data)
		if dt not in dtypes: raise ValueError("%s must be %s" % (name, " or ".join(np.dtype(t).name for t in dtypes)))
		if tuple(data.shape) != (ny, nx): raise ValueError("%s must be [ny,nx], as the geometry" % name)
		if not (data.is_contiguous() if _is_tensor(data) else data.flags["C_CONTIGUOUS"]): raise ValueError("%s must be C-contiguous" % name)
		return (data if _is_tensor(data) else _put(data, dt, device)), given
	work, given_map = out_array(omap, (np.dtype(np.float32), np.dtype(np.float64)), np.float64, "omap")
	want_dom = domains or odomains is not None
	dom, given_dom = out_array(odomains, (np.dtype(np.int32),), np.int32, "odomains") if want_dom else (None, None)
	stats = _new(((ny+TILE-1)//TILE, (nx+TILE-1)//TILE), np.int32, device) if return_stats else None
	sht._lib.check(sht._lib.load().pxm_distance_from(ny, nx, dec0, ddec, ra0, dra, npoint, _ptr(d_dec), _ptr(d_ra), _ptr(d_pix),
		0.0 if rmax is None else float(rmax), _ptr(d_skip), _ptr(work), sht._DT[_np_dtype(work)], _ptr(dom), _ptr(stats), sht.device_index(), sht.current_stream()))
	def result(arr, given):
		if given is not None:
			gdata = given.tensor if isinstance(given, enmap.dmap) else given
			if not _is_tensor(gdata) and _ptr(arr) != _ptr(gdata): gdata[...] = _host(arr)
			return given
		return enmap.dmap(arr, wcs) if device is not None else enmap.ndmap(_host(arr), wcs)
	res = (result(work, given_map),)
	if domains: res += (result(dom, given_dom),)
	elif given_dom is not None: result(dom, given_dom)
	if return_stats: res += (stats if device is not None else _host(stats),)
	return res if len(res) > 1 else res[0]
