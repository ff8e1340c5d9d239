"""healpy-shaped pixel arithmetic on the device, RING ordering only: what reproject.map2healpix / healpix2map need of healpy
(pix2ang, ang2pix, get_interp_weights, get_interp_val), as kernels (csrc/healpix.hip: pxm_healpix_index, pxm_healpix_interp).

nside is any integer >= 1 (reproject.restrict_nside(mode="any")); pixel indices are int64.  theta is the colatitude and phi the
longitude in radians, phi taken modulo 2 pi.  The definitions are those of the published pixelisation (Gorski et al. 2005) and of the
HEALPix C++ get_interpol, written out in csrc/healpix.hip; the pixel centres are those of geometry.healpix_rings.  healpy is not a
dependency, and parity with it is not pinned by any test.

Numpy in gives numpy out; CUDA tensors in give tensors out on their device."""
import numpy as np
from . import _lib, _arrays as A

_F32, _F64 = np.dtype(np.float32), np.dtype(np.float64)

def nside2npix(nside): return 12*int(nside)**2

def npix2nside(npix):
	nside = int(round((int(npix)/12.0)**0.5))
	if nside < 1 or 12*nside**2 != int(npix): raise ValueError("Wrong pixel number (it is not 12*nside**2)")
	return nside

def _raw(x):
	x = A.unwrap(x)
	return x if A.is_tensor(x) else np.asarray(x)

def _as_kind(work, device, shape):
	work = work.reshape(shape)
	if device is None: return A.host(work)
	return work if A.is_tensor(work) else A.torch().from_numpy(work).to(device)

def _angles(theta, phi):
	"""theta and phi broadcast against each other -> (their common shape, the caller's device, the flat float64 arrays the library reads)"""
	theta, phi = _raw(theta), _raw(phi)
	device = A.device_of(theta, phi)
	if device is not None:
		torch = A.torch()
		theta, phi = (a.to(device=device, dtype=torch.float64) if A.is_tensor(a) else torch.as_tensor(np.asarray(a, np.float64), device=device) for a in (theta, phi))
		theta, phi = torch.broadcast_tensors(theta, phi)
	else: theta, phi = np.broadcast_arrays(np.asarray(theta, np.float64), np.asarray(phi, np.float64))
	shape = tuple(int(n) for n in theta.shape)
	return shape, device, A.put(theta.reshape(-1), np.float64, device), A.put(phi.reshape(-1), np.float64, device)

def _index(mode, nside, n, pin, theta, phi, pout, out):
	_lib.check(_lib.load().pxm_healpix_index(mode, int(nside), int(n), A.ptr(pin), A.ptr(theta), A.ptr(phi), A.ptr(pout), A.ptr(out), A.device_index(), A.current_stream()))

def _nside(nside):
	if int(nside) != nside or int(nside) < 1: raise ValueError("nside must be an integer >= 1")
	return int(nside)

def pix2ang(nside, ipix):
	"""(theta, phi) of the centres of the pixels ipix (healpy.pix2ang, RING).  A pixel outside [0, 12 nside^2) raises ValueError
	for host input and gives not-a-number for device input (checking would wait for the device)."""
	nside = _nside(nside)
	ipix = _raw(ipix)
	device = A.device_of(ipix)
	if device is None and ipix.size and (ipix.min() < 0 or ipix.max() >= nside2npix(nside)): raise ValueError("pix2ang: a pixel index outside the map")
	shape = tuple(int(n) for n in ipix.shape)
	d = A.put(ipix.reshape(-1), np.int64, device)
	out = A.empty((2, int(d.shape[0])), np.float64, like=d)
	_index(0, nside, d.shape[0], d, None, None, None, out)
	return _as_kind(out[0], device, shape), _as_kind(out[1], device, shape)

def ang2pix(nside, theta, phi):
	"""the pixel (int64) that holds each direction (healpy.ang2pix, RING); -1 where theta or phi is not a number"""
	nside = _nside(nside)
	shape, device, t, f = _angles(theta, phi)
	out = A.empty((int(t.shape[0]),), np.int64, like=t)
	_index(1, nside, t.shape[0], None, t, f, out, None)
	return _as_kind(out, device, shape)

def get_interp_weights(nside, theta, phi):
	"""(pix [4, ...] int64, w [4, ...]): the four pixels and weights of the ring-bilinear value at each direction (healpy.get_interp_weights,
	RING): two pixels on the ring above and two on the ring below; beyond the first or last ring that ring's four pixels share the polar
	part.  The weights are >= 0 and sum to 1."""
	nside = _nside(nside)
	shape, device, t, f = _angles(theta, phi)
	n = int(t.shape[0])
	pix, w = A.empty((4, n), np.int64, like=t), A.empty((4, n), np.float64, like=t)
	_index(2, nside, n, None, t, f, pix, w)
	return _as_kind(pix, device, (4,)+shape), _as_kind(w, device, (4,)+shape)

def _maps(m):
	"""m [..., npix] -> (nside, its leading shape, the caller's device, the contiguous float32 / float64 array the library reads)"""
	m = _raw(m)
	if m.ndim < 1: raise ValueError("a healpix map is [..., npix]")
	nside = npix2nside(m.shape[-1])
	dt = A.np_dtype(m)
	if dt not in (_F32, _F64): dt = _F64
	device = A.device_of(m)
	return nside, tuple(int(n) for n in m.shape[:-1]), device, A.put(m, dt, device)

def get_interp_val(m, theta, phi, order=1):
	"""The values [..., {points}] of the healpix maps m [..., npix] (RING) at the directions (theta, phi): the ring-bilinear value
	(healpy.get_interp_val), or with order=0 the value of the pixel that holds the direction.  In the maps' dtype."""
	if order not in (0, 1): raise ValueError("Only order 0 and order 1 spline interpolation supported from healpix maps")
	nside, pre, device, d = _maps(m)
	shape, pdev, t, f = _angles(theta, phi)
	if device is not None and pdev is not None and device != pdev: raise ValueError("get_interp_val: the map and the directions are on different devices")
	where = A.device_of(d)
	if where is not None: t, f = A.put(t, None, where), A.put(f, None, where)
	ncomp, n = int(np.prod(pre, dtype=np.int64)), int(t.shape[0])
	out = A.empty((ncomp, n), A.np_dtype(d), like=d)
	_lib.check(_lib.load().pxm_healpix_interp(nside, ncomp, A.ptr(d), A.DT[A.np_dtype(d)], 12*nside**2, n, A.ptr(t), A.ptr(f), int(order), A.ptr(out),
		A.device_index(), A.current_stream()))
	return _as_kind(out, device if device is not None else pdev, pre+shape)
