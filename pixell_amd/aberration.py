"""Doppler boost of maps on the device: the call signatures of pixell.aberration (aberration.py:10-378).

boost_map is aberration followed by modulation.  The aberration of a map is: the boost's deflection field (a tiny spin-1 alm,
calc_boost_field) synthesised on the map's pixels (curvedsky.alm2map), the pixels moved along it and the rotation of the polarisation
basis that comes with the move (pxm_deflect, the kernel lensing uses), the map's values at the moved pixels (pxm_plan_map_points /
pxm_map_points: the map's own trigonometric interpolant, evaluated as a type-2 non-uniform FFT) and the rotation (pxm_rotate_pol).  The
modulation is one pass of Planck-law arithmetic per pixel (pxm_modulate).  An Aberrator keeps the sorted points and the rotation
angle on the device, a Modulator the modulation map; nothing of a map's size goes to the host.

dmaps or CUDA tensors in, dmaps out; ndmaps in, ndmaps out.  Only separable cylindrical geometries."""
import ctypes, warnings
import numpy as np
from . import enmap, curvedsky, sht, _lib, _arrays as A, wcs as wcsutils

beta    = 0.001235
dir_equ = np.array([167.919, -6.936])*np.pi/180
dir_gal = np.array([263.986, 48.247])*np.pi/180
dir_ecl = np.array([171.640, -11.154])*np.pi/180
T_cmb = 2.72548      # utils.T_cmb

_MODES = {None: 0, "none": 0, "plain": 1, "T2T": 1, "T2lin": 2, "lin2T": 3, "lin2lin": 4}      # PXM_MOD_*

def boost_map(map, dir=dir_equ, beta=beta, modulation="T2lin", T0=T_cmb, freq=150e9, return_modulation=False, dipole=False,
		map_unit=1e-6, spin=[0, 2], aberrate=True, modulate=True, nthread=None, coord_dtype=None, boundary="auto"):
	"""Doppler-boost (aberrate, then modulate) map [..., ny, nx] for a motion towards dir = [ra, dec] at speed beta (aberration.boost_map,
	aberration.py:10-55).  spin: how the third last axis reads ([0, 2]: T, then Q and U).  modulation: None | "plain" = "T2T" | "T2lin" |
	"lin2T" | "lin2lin"; dipole: keep the monopole's own boost (the CMB dipole) in the scalar components.  boundary: what lies past the
	map's first and last row -- "periodic": the other end of the map, "fullsky": the same rows half a turn away, "auto": "fullsky" when the
	rows cover the sky.  The columns always wrap.  return_modulation: (map, A).  A map given on the device is returned on the device; the
	input is left as it is unless aberrate is False (the modulation works in place, as the reference's does)."""
	if return_modulation: assert modulate, "Can't return modulation of modulation is disabled"
	if aberrate:
		map = aberrate_map(map, dir=dir, beta=beta, spin=spin, nthread=nthread, boundary=boundary)
	if modulate:
		map, mod = modulate_map(map, dir=dir, beta=beta, spin=spin, nthread=nthread, dipole=dipole, modulation=modulation, T0=T0, freq=freq,
			map_unit=map_unit, return_modulation=True)
	return (map, mod) if return_modulation else map

def deboost_map(map, dir=dir_equ, beta=beta, modulation="lin2T", T0=T_cmb, freq=150e9, return_modulation=False, dipole=False,
		map_unit=1e-6, spin=[0, 2], aberrate=True, modulate=True, nthread=None, coord_dtype=None, boundary="auto"):
	"""boost_map with the sign of beta flipped and "lin2T" as the default modulation"""
	return boost_map(map, dir=dir, beta=-beta, modulation=modulation, T0=T0, freq=freq, return_modulation=return_modulation, dipole=dipole,
		map_unit=map_unit, spin=spin, aberrate=aberrate, modulate=modulate, nthread=nthread, coord_dtype=coord_dtype, boundary=boundary)

def aberrate_map(map, dir=dir_equ, beta=beta, spin=[0, 2], nthread=None, coord_dtype=None, boundary="auto"):
	"""the aberration part of boost_map"""
	return Aberrator(map.shape, map.wcs, dir=dir, beta=beta, spin=spin, nthread=nthread, coord_dtype=coord_dtype, boundary=boundary,
		dtype=map.dtype)(map)

def deaberrate_map(map, dir=dir_equ, beta=beta, spin=[0, 2], nthread=None, coord_dtype=None, boundary="auto"):
	return aberrate_map(map, dir=dir, beta=-beta, spin=spin, nthread=nthread, coord_dtype=coord_dtype, boundary=boundary)

def modulate_map(map, dir=dir_equ, beta=beta, modulation="T2lin", T0=T_cmb, freq=150e9, return_modulation=False, dipole=False,
		map_unit=1e-6, spin=[0, 2], nthread=None):
	"""the modulation part of boost_map, in place"""
	modulator = Modulator(map.shape, map.wcs, dir=dir, beta=beta, spin=spin, modulation=modulation, T0=T0, freq=freq, dipole=dipole,
		map_unit=map_unit, nthread=nthread, dtype=map.dtype, _like=map)
	map = modulator(map)
	return (map, modulator.A) if return_modulation else map

def demodulate_map(map, dir=dir_equ, beta=beta, modulation="lin2T", T0=T_cmb, freq=150e9, return_modulation=False, dipole=False,
		map_unit=1e-6, spin=[0, 2], nthread=None):
	return modulate_map(map, dir=dir, beta=-beta, modulation=modulation, T0=T0, freq=freq, return_modulation=return_modulation,
		dipole=dipole, map_unit=map_unit, spin=spin, nthread=nthread)

# ---- arrays ------------------------------------------------------------------------------------------------------------------
def _real_dtype(dtype):
	dtype = np.dtype(dtype)
	if dtype not in (np.dtype(np.float32), np.dtype(np.float64)): raise ValueError("maps must be float32 or float64, not %s" % dtype)
	return dtype

def _planes(data, ny, nx):
	"""the maps of data [..., ny, nx] where the library reads them, as [n, ny, nx] with every map's pixels contiguous, and the distance
	between the maps in elements.  Device arrays keep their strides where they can."""
	if A.is_tensor(data):
		m = A.require_gpu(data).reshape(-1, ny, nx)
		if not m[0].is_contiguous(): m = m.contiguous()
		return m, (int(m.stride(0)) if m.shape[0] > 1 else ny*nx)
	return A.put(data).reshape(-1, ny, nx), ny*nx

def _work_map(pre, shape, wcs, dtype):
	"""a map for alm2map to fill on the device (an ndmap in the simulator)"""
	shp = tuple(pre)+tuple(shape[-2:])
	return enmap.zeros(shp, wcs, dtype) if _lib.is_hostsim() else enmap.dmap(A.zeros(shp, dtype), wcs)

def _wrap_like(res, given, wcs):
	"""res (a device array) as what the caller of `given` expects: a dmap for device input, an ndmap for numpy input"""
	if A.is_tensor(A.unwrap(given)): return enmap.dmap(res, wcs)
	return enmap.ndmap(A.host(res), wcs)

# ---- interpolation -------------------------------------------------------------------------------------------------------------
class _MapPoints:
	"""pxm_plan_map_points: the points pix [2, npts] = (y, x) in pixels (a device array, float64, contiguous) of maps [ny][nx], sorted
	once; calls interpolate any number of maps there"""
	def __init__(self, ny, nx, pix, epsilon, ydouble):
		epsilon = float(epsilon)
		if not (sht.EPS_MIN <= epsilon <= sht.EPS_MAX): raise ValueError("epsilon must lie in [%g, %g], got %g" % (sht.EPS_MIN, sht.EPS_MAX, epsilon))
		self.ny, self.nx, self.npts, self.ydouble = int(ny), int(nx), int(pix.shape[1]), bool(ydouble)
		h = ctypes.c_void_p()
		_lib.check(_lib.load().pxm_plan_map_points(ctypes.byref(h), self.ny, self.nx, int(self.ydouble), self.npts, A.ptr(pix) if self.npts else None,
			epsilon, A.device_index(), A.current_stream()))
		self.plan = sht.Plan(h)
	def __call__(self, maps, cstride):
		"""maps [n, ny, nx] (float32 | float64, cstride elements apart) -> [n, npts] of the same kind"""
		dt = _real_dtype(A.np_dtype(maps))
		out = A.empty((int(maps.shape[0]), self.npts), dt, like=maps)
		if self.npts == 0: return out
		_lib.check(_lib.load().pxm_map_points(self.plan.handle, int(maps.shape[0]), A.ptr(maps), A.DT[dt], int(cstride), A.ptr(out), A.DT[dt],
			self.npts, A.current_stream()))
		return out

def interpol_map(imap, pixs, epsilon=None, ydouble=False, nthread=None):
	"""The values of imap [..., ny, nx] at the pixel coordinates pixs [{y, x}, ...] -> [..., npts]: the map's trigonometric interpolant,
	periodic in both directions; ydouble: continued over the pole instead, row ny being row ny - 1 half a turn away
	(aberration.interpol_map, aberration.py:246-270).  epsilon: relative accuracy, by default 1e-5 for float32 and 1e-12 for float64.
	Coordinates are read as float64 and may be any finite numbers.  Device arrays in, a device array out; numpy in, numpy out."""
	data, pix = A.unwrap(imap), A.unwrap(pixs)
	ny, nx = (int(n) for n in data.shape[-2:])
	dt = _real_dtype(A.np_dtype(data))
	if epsilon is None: epsilon = 1e-5 if dt == np.float32 else 1e-12
	on_host = not A.is_tensor(data)
	maps, cstride = _planes(data, ny, nx)
	dpix = A.put(pix, np.float64, device=maps.device if A.is_tensor(maps) else None).reshape(2, -1)
	out = _MapPoints(ny, nx, dpix, epsilon, ydouble)(maps, cstride).reshape(tuple(data.shape[:-2])+(-1,))
	return A.host(out) if on_host else out

# ---- repeated use ----------------------------------------------------------------------------------------------------------------
def _boundary(boundary, shape, wcs):
	if boundary == "auto": boundary = "fullsky" if fully(shape, wcs) else "periodic"
	if boundary not in ("periodic", "fullsky"): raise ValueError("Unrecognized boundary '%s'" % str(boundary))
	return boundary

class Aberrator:
	def __init__(self, shape, wcs, dir=dir_equ, beta=beta, spin=[0, 2], nthread=None, coord_dtype=np.float64, boundary="auto", dtype=np.float64, epsilon=None):
		"""Everything of the aberration that does not depend on the map's values (aberration.Aberrator, aberration.py:101-162):

		  aberrator = Aberrator(shape, wcs)
		  for map in maps: omap = aberrator(map)

		Kept on the device: the moved pixels, sorted for the interpolation (24 bytes per pixel), and the rotation angle (8).  dtype: the
		maps' (it sets the default accuracy of the interpolation, epsilon); coord_dtype is accepted and ignored, coordinates are float64."""
		boundary = _boundary(boundary, shape, wcs)
		geo = wcsutils.separable_geometry(shape, wcs)      # (raises NotImplementedError for anything else)
		ny, nx, dec0, ddec, ra0, dra = geo
		if epsilon is None: epsilon = 1e-5 if _real_dtype(dtype) == np.float32 else 1e-12
		from . import lensing
		# 1. the deflection field: a tiny spin-1 alm, synthesised on the map's pixels as (e_theta, e_phi) components
		alm_dpos = calc_boost_field(-beta, dir, nthread=nthread)
		deflect = _work_map(alm_dpos.shape[:-1], shape, wcs, np.float64)
		curvedsky.alm2map(A.put(np.ascontiguousarray(alm_dpos, np.complex128)), deflect, spin=1)
		grad = A.unwrap(deflect)
		grad[0] *= -1      # pxm_deflect takes (d/ddec, (d/dra)/cos dec): the first component points north, e_theta south
		# 2. the moved pixels and the rotation of the basis along the move
		loc, psi = lensing.offset_by_grad(None, grad, geodesic=True, pol=True, _loc=True, _geometry=(tuple(shape[-2:]), wcs))
		del deflect, grad
		# 3. ... in pixel coordinates (any period off: the plan wraps them)
		pix = A.empty((2, ny*nx), np.float64, like=loc)
		pix[0] = (np.pi/2-dec0-loc[:, 0])/ddec
		pix[1] = (loc[:, 1]-ra0)/dra
		turn = 2*np.pi/abs(dra)      # ra comes back in [0, 2 pi): the column within half a turn of the map's middle
		pix[1] -= ((pix[1]-0.5*nx)/turn).round()*turn
		del loc
		self.points = _MapPoints(ny, nx, pix, epsilon, boundary == "fullsky")
		del pix
		# pxm_deflect's psi is the spin-2 phase, twice the angle the basis turns by
		psi *= 0.5
		self.gamma = psi
		self.shape, self.wcs, self.spin, self.boundary, self.nthread = tuple(shape[-2:]), wcs, spin, boundary, nthread
	def __call__(self, map, spin=None, nthread=None):
		if spin is None: spin = self.spin
		data = A.unwrap(map)
		ny, nx = self.shape
		if tuple(data.shape[-2:]) != (ny, nx): raise ValueError("the Aberrator was made for maps of %d x %d pixels" % (ny, nx))
		maps, cstride = _planes(data, ny, nx)
		if A.is_tensor(maps) and A.is_tensor(self.gamma) and maps.device != self.gamma.device: raise ValueError("the map and the Aberrator live on different devices")
		out = self.points(maps, cstride)
		del maps
		if data.ndim > 2:
			ncomp = int(data.shape[-3]); npix = ny*nx; esz = out.dtype.itemsize if not A.is_tensor(out) else out.element_size()
			nlead = int(out.shape[0])//ncomp
			for s, c1, c2 in enmap.spin_helper(spin, ncomp):
				if s == 0: continue
				_lib.check(_lib.load().pxm_rotate_pol(npix, nlead, A.ptr(out)+c1*npix*esz, A.ptr(out)+(c1+1)*npix*esz, ncomp*npix,
					A.DT[A.np_dtype(out)], A.ptr(self.gamma), int(s), A.device_index(), A.current_stream()))
		return _wrap_like(out.reshape(tuple(data.shape)), map, self.wcs)

class Modulator:
	def __init__(self, shape, wcs, dir=dir_equ, beta=beta, modulation="T2lin", T0=T_cmb, freq=150e9, dipole=False, map_unit=1e-6,
			spin=[0, 2], dtype=np.float64, nthread=None, _like=None):
		"""The modulation map A of a geometry, kept on the device (aberration.Modulator, aberration.py:164-195):

		  modulator = Modulator(shape, wcs)
		  for map in maps: omap = modulator(map)      # in place"""
		if modulation not in _MODES: raise ValueError("Urecognized modulation mode '%s'" % modulation)
		wcsutils.separable_geometry(shape, wcs)
		dtype = _real_dtype(dtype)
		alm_mod = calc_boost_field(-beta, dir, nthread=nthread, modulation=True, mod_exp=-1)[1]
		mod = _work_map(alm_mod.shape[:-1], shape, wcs, dtype)
		curvedsky.alm2map(A.put(np.ascontiguousarray(alm_mod, np.result_type(dtype, 0j))), mod, spin=0)
		# (the modulation goes back with the map: on the device for device maps, an ndmap for numpy maps)
		self.A = mod if _like is None or A.is_tensor(A.unwrap(_like)) or _lib.is_hostsim() else enmap.ndmap(A.host(mod), wcs)
		self._dev = A.unwrap(mod)
		self.nthread = nthread; self.modulation = modulation; self.T0 = T0; self.freq = freq; self.dipole = dipole
		self.dtype = dtype; self.spin = spin; self.map_unit = map_unit
	def __call__(self, map, spin=None):
		if spin is None: spin = self.spin
		if A.np_dtype(A.unwrap(map)) != self.dtype: warnings.warn("Modulator dtype does not match argument dtype")
		return apply_modulation(map, self._dev, spin=spin, T0=self.T0, freq=self.freq, map_unit=self.map_unit, mode=self.modulation, dipole=self.dipole)

# ---- the boost ---------------------------------------------------------------------------------------------------------------------
def calc_boost_1d(z, beta):
	"""z: the cosine of the angle from the direction of travel in the rest frame -> (z_obs, A): where that direction is seen, and the
	modulation there, T_obs(z_obs) = A T_rest(z).  -beta gives the reverse (aberration.calc_boost_1d, aberration.py:197-207)."""
	gamma = (1-beta**2)**-0.5
	z_obs = (z+beta)/(1+z*beta)
	np.clip(z_obs, -1, 1, out=z_obs)
	mod = 1/(gamma*(1-z_obs*beta))
	return z_obs, mod

def fully(shape, wcs, tol=0.1):
	"""the rows of the geometry cover (nearly) the whole sky"""
	minfo = curvedsky.analyse_geometry(shape, wcs)
	if minfo.ducc_geo is None: return False
	return abs(shape[-2]/minfo.ducc_geo.ny) > 1-tol

def beta2lmax(beta):
	"""band limit of the boost fields: the reference's empirical formula"""
	beta = np.abs(beta)
	gamma = (1-beta**2)**-0.5
	return int(np.ceil(1/(4e-3+1/gamma)**0.62*14+3.5))

def calc_boost_field(beta, dir, lmax=None, nthread=None, modulation=False, mod_exp=1):
	"""alm [2, nelem] of the deflection field of the boost (spin 1: along the meridians of the direction of travel dir = [ra, dec]), and
	with modulation also the alm of A**mod_exp (aberration.calc_boost_field, aberration.py:224-244).  The fields are analysed about the
	pole (curvedsky.prof2alm) and turned to dir (curvedsky.rotate_alm).  numpy arrays: they are tiny."""
	if lmax is None: lmax = beta2lmax(beta)
	n = lmax+2
	itheta = np.arange(0, n)*np.pi/(n-1)
	iz = np.cos(itheta)
	oz, mod = calc_boost_1d(iz, beta)
	otheta = np.arccos(oz)
	dpos = np.zeros([2, n])
	dpos[0] = otheta-itheta
	def to_dir(alm): return np.asarray(A.host(curvedsky.rotate_alm(alm, 0, np.pi/2-float(dir[1]), float(dir[0]))))
	alm = to_dir(curvedsky.prof2alm(dpos, spin=1))
	if not modulation: return alm
	mod **= mod_exp
	return alm, to_dir(curvedsky.prof2alm(mod, spin=0))

# ---- modulation ------------------------------------------------------------------------------------------------------------------
def apply_modulation(map, A_, T0=T_cmb, freq=150e9, map_unit=1e-6, mode="T2lin", dipole=False, spin=[0, 2]):
	"""map [..., ny, nx] modulated in place by A_ [ny, nx] (aberration.apply_modulation, aberration.py:285-354), one kernel pass
	(pxm_modulate).  mode: None | "none"; "plain" | "T2T": map *= A, with dipole the first component gets (A-1) T0/map_unit added;
	"T2lin", "lin2T": true temperature <-> linearised units at freq; "lin2lin": both, A applied in between.  With dipole the scalar
	components (spin 0 of `spin`) keep the monopole's own boost.  "lin2T" takes off utils.T_cmb, not T0, as the reference does.
	The arithmetic is float64 whatever the map's dtype.  Returns map."""
	if mode not in _MODES: raise ValueError("Urecognized modulation mode '%s'" % mode)
	code = _MODES[mode]
	if code == 0: return map
	data = A.unwrap(map)
	ny, nx = (int(n) for n in data.shape[-2:])
	dt = _real_dtype(A.np_dtype(data))
	if tuple(A.unwrap(A_).shape[-2:]) != (ny, nx): raise ValueError("the modulation and the map disagree on the pixel shape")
	maps, cstride = _planes(data, ny, nx)
	mod = A.put(A_, dt, device=maps.device if A.is_tensor(maps) else None)
	ncomp = int(data.shape[-3]) if data.ndim > 2 else 1
	flags = np.zeros(ncomp, bool)
	if data.ndim > 2:
		for s, c1, c2 in enmap.spin_helper(spin, ncomp): flags[c1:c2] = s == 0
	else: flags[:] = True
	lib = _lib.load(); esz = dt.itemsize
	for lead in range(int(maps.shape[0])//ncomp):
		for c0 in range(0, ncomp, 64):
			nc = min(64, ncomp-c0)
			mask = sum(1 << i for i in range(nc) if flags[c0+i])
			# (T2T adds the dipole to the stack's first component alone)
			dip = int(bool(dipole)) if code != 1 or c0 == 0 else 0
			_lib.check(lib.pxm_modulate(ny*nx, nc, A.ptr(maps)+(lead*ncomp+c0)*cstride*esz, A.DT[dt], int(cstride), A.ptr(mod), mask, code, dip,
				float(T0), float(freq), float(map_unit), A.device_index(), A.current_stream()))
	if A.ptr(maps) != A.ptr(data):      # a staged or compacted copy: bring the result back into the caller's array
		data[...] = (maps if A.is_tensor(data) else A.host(maps)).reshape(data.shape)
	return map
