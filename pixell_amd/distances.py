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
from . import enmap, _lib, _arrays as A, wcs as wcsutils

TILE = 16      # the kernel's tile: return_stats counts visits per TILE x TILE pixels
_MASK = (np.dtype(np.uint8), np.dtype(bool))

def _mask8(x, device):
	"""a mask of any dtype as the uint8 array the kernels read: non-zero is set"""
	return A.put(x if A.np_dtype(x) in _MASK else (x != 0), np.uint8, device)

def _edges(arr, labeled, flat):
	arr = A.unwrap(arr)
	if not A.is_tensor(arr): arr = np.asarray(arr)
	if arr.ndim != 2: raise ValueError("find_edges needs a 2-D array")
	device = A.device_of(arr)
	ny, nx = int(arr.shape[0]), int(arr.shape[1])
	if labeled: d = A.put(arr, np.int32, device)
	else: d = _mask8(arr, device)
	lib = _lib.load(); dev = A.device_index(); st = A.current_stream()
	n = ctypes.c_int64(0)
	_lib.check(lib.pxm_find_edges(ny, nx, A.ptr(d), int(labeled), None, 0, ctypes.byref(n), dev, st))
	out = A.empty((n.value,), np.int64, device=device)
	if n.value > 0: _lib.check(lib.pxm_find_edges(ny, nx, A.ptr(d), int(labeled), A.ptr(out), n.value, None, dev, st))
	if device is None: out = A.host(out)
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
	ny, nx, dec0, ddec, ra0, dra = wcsutils.separable_geometry(shape, wcs)
	if (points is None) == (pix is None): raise ValueError("distance_from_points needs either points or pix")
	points, skip = A.unwrap(points), A.unwrap(skip)
	device = A.device_of(omap, odomains, points, pix, skip)
	d_dec = d_ra = d_pix = None
	if pix is not None:
		if not A.is_tensor(pix): pix = np.asarray(pix)
		d_pix = A.put(pix.reshape(-1), np.int64, device); npoint = int(d_pix.shape[0])
	else:
		if not A.is_tensor(points): points = np.asarray(points, float)
		if points.ndim == 1: points = points[:, None]
		if points.ndim != 2 or points.shape[0] != 2: raise ValueError("points must be [{dec,ra},npoint]")
		d_dec, d_ra = A.put(points[0], np.float64, device), A.put(points[1], np.float64, device); npoint = int(points.shape[1])
	d_skip = None
	if skip is not None:
		if tuple(skip.shape) != (ny, nx): raise ValueError("skip must be [ny,nx]")
		d_skip = _mask8(skip, device)
	def out_array(given, dtypes, name):
		"""the array the kernel writes: the caller's (or a staged copy of it), else a new one of the last of dtypes"""
		if given is None: return A.empty((ny, nx), dtypes[-1], device=device)
		return A.out_array(given, (ny, nx), dtypes, device, name, "[ny,nx], as the geometry")
	work = out_array(omap, (np.dtype(np.float32), np.dtype(np.float64)), "omap")
	dom = out_array(odomains, (np.dtype(np.int32),), "odomains") if domains or odomains is not None else None
	stats = A.empty(((ny+TILE-1)//TILE, (nx+TILE-1)//TILE), np.int32, device=device) if return_stats else None
	_lib.check(_lib.load().pxm_distance_from(ny, nx, dec0, ddec, ra0, dra, npoint, A.ptr(d_dec), A.ptr(d_ra), A.ptr(d_pix),
		0.0 if rmax is None else float(rmax), A.ptr(d_skip), A.ptr(work), A.DT[A.np_dtype(work)], A.ptr(dom), A.ptr(stats), A.device_index(), A.current_stream()))
	def result(arr, given):
		if given is not None: return A.result(arr, given)
		return enmap.dmap(arr, wcs) if device is not None else enmap.ndmap(A.host(arr), wcs)
	res = (result(work, omap),)
	if domains: res += (result(dom, odomains),)
	elif odomains is not None: A.result(dom, odomains)
	if return_stats: res += (stats if device is not None else A.host(stats),)
	return res if len(res) > 1 else res[0]
