"""Matched filters and the simple source finder of the reference's pixell/analysis.py, on the device.

matched_filter_constcov / _white / _constcorr_lowcorr / _constcorr_smoothivar are the reference's compositions of UHT transforms
(analysis.py:124-304) over pixell_amd.uharm.UHT, flat or curved; NmatConstcov and NmatConstcorr are its flat-sky noise models (:395-471);
FinderSimple and MeasurerSimple (:508-583, :899-929) turn a map into a catalogue and read a catalogue off a map.  The steps scipy and numpy.linalg do for
the reference run as HIP kernels: labels.label and labels.stats (connected components, centres of mass and peak values, csrc/label.hip),
enmap.labeled_distance_transform (growing), solve_mapsys (pxm_solve_mapsys, the per-pixel solve of flux = kappa^-1 rho) and enmap.at.
Host maps in give host maps out; dmaps in give dmaps out on that device, and no full-size map goes to the host: what comes back is the
catalogue, a numpy recarray with the reference's fields.

Not here: matched_filter_constcorr_dual, NmatWavelet, the simulate methods, FinderMulti / FinderMultiSafe / FinderIterative, MeasurerMulti / MeasurerIterative and the Modellers.

Where this differs from the reference on purpose: a pixel whose kappa is singular gets NaN in its fluxes and errors
where the reference's np.linalg.solve raises LinAlgError for the whole map; labels are grown with exact distances where the reference's
default "cellgrid" distances are approximate."""
import numpy as np
from . import enmap, uharm, labels, _lib, _arrays as A

arcmin = np.pi/180/60

class Bunch(dict):
	"""a dictionary whose entries are attributes too (the reference's bunch.Bunch)"""
	__getattr__ = dict.__getitem__
	__setattr__ = dict.__setitem__

def _on(x, like):
	"""a host array or number next to the data `like`: a tensor on its device when that is a tensor"""
	if not A.is_tensor(like) or A.is_tensor(x) or np.ndim(x) == 0: return x
	return A.torch().as_tensor(np.ascontiguousarray(x), device=like.device)
def _complex(d): return d.to(A.tdtype(np.result_type(A.np_dtype(d), 0j))) if A.is_tensor(d) else d+0j
def _sum(d, axes): return d.sum(tuple(axes)) if A.is_tensor(d) else np.sum(d, tuple(axes))
def _maximum0(d): return d.clamp(min=0) if A.is_tensor(d) else np.maximum(d, 0)

def _like(res, like):
	"""res with the geometry of `like`, where it has one"""
	return enmap._wrap(res, like) if hasattr(like, "wcs") else res

def sanitize_kappa(kappa, tol=1e-4, inplace=False):
	"""Raise the diagonal of kappa [n, n, ny, nx] to at least tol times its own maximum (analysis.py:1046-1050)"""
	d = enmap._data(kappa)
	if not inplace: d = d.clone() if A.is_tensor(d) else np.array(d)
	for i in range(d.shape[0]):
		if A.is_tensor(d): d[i, i] = d[i, i].clamp(min=float(d[i, i].max())*tol)
		else: d[i, i] = np.maximum(d[i, i], np.max(d[i, i])*tol)
	return kappa if inplace else _like(d, kappa)

def solve_mapsys(kappa, rho):
	"""flux[:, y, x] = solve(kappa[:, :, y, x], rho[:, y, x]) and dflux[a] = sqrt(inv(kappa)[a, a]) for every pixel: (flux, dflux), each
	[n, ny, nx] (analysis.py:1052-1060).  A 2-D kappa is the scalar case, rho/kappa and kappa**-0.5.  float32 or float64 maps (others are
	converted to float64), FP64 arithmetic, n up to 8; a singular pixel gets NaN."""
	k, r = enmap._data(kappa), enmap._data(rho)
	if not A.is_tensor(k): k = np.asarray(k)
	if not A.is_tensor(r): r = np.asarray(r)
	if k.ndim == 2: return _like(r/k, rho), _like(k**-0.5, kappa)
	if k.ndim != 4 or r.ndim != 3 or k.shape[0] != k.shape[1] or tuple(k.shape[1:]) != tuple(r.shape):
		raise ValueError("solve_mapsys needs kappa [n,n,ny,nx] and rho [n,ny,nx]")
	n = int(k.shape[0])
	if n > 8: raise NotImplementedError("solve_mapsys: systems of more than 8 components are not implemented")
	if n == 1: return _like(r/k[0], rho), _like(k[0]**-0.5, rho)
	device = A.device_of(k, r)
	dt = A.np_dtype(k) if A.np_dtype(k) in (np.dtype(np.float32), np.dtype(np.float64)) else np.dtype(np.float64)
	dk, dr = A.put(k, dt, device), A.put(r, dt, device)
	flux, dflux = A.empty(tuple(r.shape), dt, device=device), A.empty(tuple(r.shape), dt, device=device)
	npix = int(r.shape[1])*int(r.shape[2])
	_lib.check(_lib.load().pxm_solve_mapsys(n, npix, A.ptr(dk), A.ptr(dr), A.ptr(flux), A.ptr(dflux), A.DT[dt], A.device_index(), A.current_stream()))
	if device is None: flux, dflux = A.host(flux), A.host(dflux)
	return _like(flux, rho), _like(dflux, rho)

def get_flat_sky_correction(pixratio):
	"""(the factor of rho, the factor of kappa) that make up for the change of the pixel size over a flat-sky patch (analysis.py:1062-1063)"""
	return (0.5*(1+pixratio**2))**-0.5, 1/pixratio

def rpow(fmap, exp=2):
	"""The fourier-space map of a real map taken to the power exp in real space (analysis.py:1077-1082)"""
	norm = enmap.area(fmap.shape, fmap.wcs)**0.5
	m = enmap._data(enmap.ifft(_like(_complex(enmap._data(fmap)/norm), fmap), normalize="phys")).real
	return _like(enmap._data(enmap.fft(_like(_complex(m**exp), fmap), normalize="phys")).real*norm, fmap)

def make_circle_labels(shape, wcs, pixs, inds=None, r=2*arcmin, device=None):
	"""An int32 label map [ny, nx] with inds[i] (default i+1) within r radians of pixel pixs[:, i] (analysis.py:1124-1130); on `device`
	when one is given"""
	pixs = np.asarray(pixs)
	if inds is None: inds = np.arange(1, len(pixs[0])+1)
	mask = np.zeros(tuple(shape[-2:]), np.int32)
	mask[pixs[0], pixs[1]] = inds
	mask = enmap.ndmap(mask, wcs) if device is None else enmap.dmap(A.put(mask, np.int32, device), wcs)
	dists, lab = enmap.labeled_distance_transform(mask, rmax=r)
	d = enmap._data(lab)
	d[enmap._data(dists) >= r] = 0
	return lab

# ---- matched filters over a UHT (analysis.py:124-304) -------------------------------------------------------------------------------
def matched_filter_constcov(map, B, iN, uht=None, spin=0):
	"""(rho, kappa) of a matched filter under a noise covariance that is constant over the map, diagonal in harmonic space: B the beam and
	iN the inverse noise power, both harmonic profiles of uht (analysis.py:124-152).  flux = rho/kappa, dflux = kappa**-0.5."""
	if uht is None: uht = uharm.UHT(map.shape, map.wcs)
	d = enmap._data(map)
	pixarea = _on(np.asarray(enmap.pixsizemap(map.shape, map.wcs, broadcastable=True)), d)
	rho = uht.map2harm_adjoint(uht.hmul(B*iN, uht.map2harm(map, spin=spin)), spin=spin)
	kappa = uht.sum_hprof(B**2*iN)/(4*np.pi)
	return _like(enmap._data(rho)/pixarea, map), kappa

def matched_filter_white(map, B, ivar, uht=None, B2=None, high_acc=False):
	"""(rho, kappa) under white noise of inverse variance ivar per pixel (analysis.py:154-191); B2: the harmonic profile of the real-space
	square of the beam (default: uht.hprof_rpow(B, 2))"""
	if uht is None: uht = uharm.UHT(map.shape, map.wcs)
	d, iv = enmap._data(map), enmap._data(ivar)
	P = _on(1/np.asarray(enmap.pixsizemap(map.shape, map.wcs, broadcastable=True)), d)
	if B2 is None: B2 = uht.hprof_rpow(B, 2)
	rho = uht.map2harm_adjoint(uht.hmul(B, uht.harm2map_adjoint(_like(iv*d, map))))
	kappa = uht.map2harm_adjoint(uht.hmul(B2, uht.harm2map_adjoint(_like(iv, map))))
	return _like(P*enmap._data(rho), map), _like(P*enmap._data(kappa), map)

def matched_filter_constcorr_lowcorr(map, B, ivar, iC, uht=None, B2=None, high_acc=False, S=None, iS=None):
	"""(rho, kappa) under the noise model inv(N) = ivar**0.5 iC ivar**0.5, iC the inverse harmonic power of the whitened noise, with kappa
	from a beam^2-weighted white stand-in for iC (analysis.py:193-263).  high_acc: rescale kappa by its exact value in the central pixel.
	S, iS: optional maps -> maps applied around the harmonic filter of rho."""
	if uht is None: uht = uharm.UHT(map.shape, map.wcs)
	d, iv = enmap._data(map), enmap._data(ivar)
	pixarea = _on(np.asarray(enmap.pixsizemap(map.shape, map.wcs, broadcastable=True)), d)
	V = iv**0.5
	W = _on(np.asarray(uht.quad_weights()), d)
	if B2 is None: B2 = uht.hprof_rpow(B, 2)
	if S is None: S = lambda x: x
	if iS is None: iS = lambda x: x
	iC_white = np.asarray(uht.sum_hprof(B**2*iC)/uht.sum_hprof(B**2))
	m = lambda x: _like(x, map)
	dat = enmap._data
	def filt(x): return dat(uht.harm2map(uht.hmul(B, uht.harm2map_adjoint(m(V*dat(iS(uht.map2harm_adjoint(uht.hmul(iC, uht.map2harm(S(m(V*x))))))))))))/pixarea
	rho = filt(d)
	kappa = dat(uht.map2harm_adjoint(uht.hmul(B2, uht.harm2map_adjoint(m(iv*W*_on(iC_white[..., None, None], d))))))/pixarea**2
	if high_acc:
		py, px = int(map.shape[-2])//2, int(map.shape[-1])//2
		u = d*0; u[..., py, px] = 1
		src = dat(uht.harm2map(uht.hmul(B, uht.map2harm(m(u/pixarea)))))
		kappa_ii = dat(uht.harm2map(uht.hmul(B, uht.harm2map_adjoint(m(V*dat(uht.map2harm_adjoint(uht.hmul(iC, uht.map2harm(m(V*src))))))))))/pixarea
		alpha = kappa[..., py, px]/kappa_ii[..., py, px]
		kappa = kappa/alpha[..., None, None]
	return m(rho), m(kappa)

def matched_filter_constcorr_smoothivar(map, B, ivar, iC, uht=None):
	"""(rho, kappa) under the same noise model with the beam commuted past ivar**0.5: good where the hit count changes slowly
	(analysis.py:265-304)"""
	if uht is None: uht = uharm.UHT(map.shape, map.wcs)
	d, iv = enmap._data(map), enmap._data(ivar)
	V = iv**0.5
	P = _on(1/np.asarray(enmap.pixsizemap(map.shape, map.wcs, broadcastable=True)), d)
	rho = P*V*enmap._data(uht.map2harm_adjoint(uht.hmul(B*iC, uht.harm2map_adjoint(_like(V*d, map)))))
	kappa = iv*_on(np.asarray(uht.sum_hprof(B**2*iC)/(4*np.pi))[..., None, None], d)*P
	return _like(rho, map), _like(kappa, map)

# ---- flat-sky noise models (analysis.py:395-471) ------------------------------------------------------------------------------------
class Nmat:
	def matched_filter(self, map, beam, cache=None): raise NotImplementedError

def _flat_setup(nm, iN):
	if iN.ndim != 4: raise ValueError("iN must be a map with 4 axes [n,n,ny,nx]")
	nm.pixsize = enmap.pixsize(iN.shape, iN.wcs)
	nm.pixratio = np.asarray(enmap.pixsizemap(iN.shape, iN.wcs, broadcastable=True))/nm.pixsize

def _check_map_beam(map, beam):
	if map.ndim != 3 or beam.ndim != 3 or tuple(map.shape) != tuple(beam.shape): raise ValueError("map and beam must be maps [n,ny,nx] of one shape")

def _m2h(x, like, **kw): return enmap._data(enmap.map2harm(_like(_complex(x), like), spin=0, normalize="phys", **kw))
def _h2m(x, like, **kw): return enmap._data(enmap.harm2map(_like(x, like), spin=0, normalize="phys", **kw))

class NmatConstcov(Nmat):
	def __init__(self, iN, apod):
		"""A noise model of constant covariance: iN [n,n,ny,nx] the inverse noise power in 2-D fourier space, apod the apodisation the map
		gets before its transform (analysis.py:395-406)"""
		self.iN, self.apod = iN, apod
		_flat_setup(self, iN)
		self.fsky = enmap.area(iN.shape, iN.wcs)/(4*np.pi)
	def matched_filter(self, map, beam, cache=None):
		"""rho [n,ny,nx], kappa [n,n,ny,nx] for map [n,ny,nx] and the beam transform beam [n,ny,nx] (analysis.py:407-426)"""
		_check_map_beam(map, beam)
		d = enmap._data(map); b, iN = _on(enmap._data(beam), d), _on(enmap._data(self.iN), d)
		fr, fk = (_on(f, d) for f in get_flat_sky_correction(self.pixratio))
		apod = _on(enmap._data(self.apod), d) if hasattr(self.apod, "shape") else self.apod
		pre = enmap._data(enmap.map_mul(_complex(iN), _m2h(d*apod, map)))/self.pixsize
		rho = enmap._data(enmap.map2harm_adjoint(_like(b*pre, map), spin=0, normalize="phys"))*fr
		kappa0 = _sum(b[:, None]*iN*b[None, :], (-2, -1))/(4*np.pi*self.fsky)
		kappa = kappa0[:, :, None, None]*fk+0*rho[None]
		return _like(rho, map), _like(kappa, map)

class NmatConstcorr(Nmat):
	def __init__(self, iN, ivar):
		"""A noise model of constant correlation: inv(N) = ivar**0.5 iN ivar**0.5, iN [n,n,ny,nx] in 2-D fourier space, ivar [n,ny,nx]
		(analysis.py:433-444)"""
		self.iN, self.ivar = iN, ivar
		if ivar.ndim != 3: raise ValueError("ivar must be a map with 3 axes")
		_flat_setup(self, iN)
	def matched_filter(self, map, beam, beam2=None, cache=None):
		"""rho [n,ny,nx], kappa [n,n,ny,nx] (analysis.py:445-471); beam2: the fourier map of the real-space square of the beam"""
		_check_map_beam(map, beam)
		d = enmap._data(map); b, iN, iv = _on(enmap._data(beam), d), _on(enmap._data(self.iN), d), _on(enmap._data(self.ivar), d)
		V = iv**0.5
		b2 = _on(enmap._data(beam2), d) if beam2 is not None else enmap._data(rpow(_like(b, map), 2))
		iN_white = _sum(b[:, None]*iN*b[None, :], (-2, -1))/_sum(b[:, None]*b[None, :], (-2, -1))
		fr, fk = (_on(f, d) for f in get_flat_sky_correction(self.pixratio))
		pre = _m2h(fr*V*_h2m(enmap._data(enmap.map_mul(_complex(iN), _m2h(V*d, map))), map), map)/self.pixsize
		rho = _h2m(b*pre, map)
		kappa = _h2m(b2*_m2h(iv, map), map)/self.pixsize*fk
		kappa = _maximum0(kappa)**0.5
		kappa = kappa[:, None]*iN_white[:, :, None, None]*kappa[None, :]
		return _like(rho, map), _like(kappa, map)

# ---- finder and measurer (analysis.py:508-583, 899-929) -----------------------------------------------------------------------------
def _cat_dtype(ncomp):
	return [("ra", "d"), ("dec", "d"), ("snr", "d"), ("flux_tot", "d"), ("dflux_tot", "d"), ("flux", "d", (ncomp,)), ("dflux", "d", (ncomp,))]

def _totals(rho, kappa, scaling):
	"""rho_tot, kappa_tot, snr_tot as data, for the data of rho [n,ny,nx] and kappa [n,n,ny,nx]"""
	s = _on(np.zeros(rho.shape[0], A.np_dtype(rho))+scaling, rho)
	rho_tot = _sum(rho*s[:, None, None], (0,))
	kappa_tot = _sum(s[:, None, None, None]*kappa*s[None, :, None, None], (0, 1))
	return rho_tot, kappa_tot, rho_tot/kappa_tot**0.5

def _read(m, pixs, order): return A.host(enmap.at(m, pixs, unit="pix", order=order))

class FinderSimple:
	def __init__(self, nmat, beam, scaling=1, save_snr=False):
		"""A finder of one class of objects in maps [nfreq,ny,nx]: beam [nfreq,ny,nx] is the fourier profile of the objects, scaling how
		their signal changes between the frequencies, nmat the noise model (analysis.py:508-533)"""
		self.beam, self.nmat, self.scaling = beam, nmat, scaling
		self.order = 3
		self.grow = 0.75*arcmin
		self.grow0 = 20*arcmin
		self.save_snr, self.snr = save_snr, None
	def __call__(self, map, snmin=5, snrel=None, penalty=None):
		"""Bunch(cat, snmin, snr, snlim): the catalogue (a numpy recarray: ra, dec, snr, flux_tot, dflux_tot, flux[n], dflux[n], by falling
		S/N) of the regions of map [n,ny,nx] whose S/N reaches snmin*penalty (with snrel: at least snrel times the highest S/N); snr is
		the S/N map, where the input lives"""
		if map.ndim != 3: raise ValueError("map must be a map with 3 axes")
		ncomp = int(map.shape[0])
		if penalty is None: penalty = 1
		rho, kappa = self.nmat.matched_filter(map, self.beam)
		kappa = sanitize_kappa(kappa)
		rho_tot, kappa_tot, snr_tot = _totals(enmap._data(rho), enmap._data(kappa), self.scaling)
		pen = _on(enmap._data(penalty), snr_tot) if hasattr(penalty, "shape") else penalty
		if snrel is not None: snmin = max(snmin, float((snr_tot/pen).max())*snrel)
		snlim = snmin*penalty if not hasattr(penalty, "shape") else _like(snmin*pen, map)
		lab, nlabel = labels.label(snr_tot >= (snmin*pen))
		cat = np.zeros(nlabel, _cat_dtype(ncomp)).view(np.recarray)
		snr_map = _like(snr_tot, map)
		if nlabel == 0: return Bunch(cat=cat, snmin=snmin, snr=snr_map, snlim=snlim)
		dists, dom = enmap.labeled_distance_transform(_like(lab, map), rmax=self.grow0)
		grown = enmap._data(dom)*(enmap._data(dists) <= self.grow)
		st = labels.stats(grown, values=snr_tot, weights=snr_tot**2, nlabel=nlabel)
		pixs = np.ascontiguousarray(A.host(st.center_of_mass()).T)
		cat.ra, cat.dec = enmap.pix2sky(map.shape, map.wcs, pixs)[::-1]
		cat.snr = A.host(st.vmax)
		del lab, dists, dom, grown
		flux_tot, dflux_tot = solve_mapsys(_like(kappa_tot, map), _like(rho_tot, map))
		cat.flux_tot = _read(flux_tot, pixs, self.order)
		cat.dflux_tot = _read(dflux_tot, pixs, 0)
		del flux_tot, dflux_tot, rho_tot, kappa_tot
		flux, dflux = solve_mapsys(kappa, rho)
		cat.flux = _read(flux, pixs, self.order).T
		cat.dflux = _read(dflux, pixs, 0).T
		if self.save_snr and self.snr is None: self.snr = snr_map
		cat = cat[np.argsort(cat.snr)[::-1]]
		return Bunch(cat=cat, snmin=snmin, snr=snr_map, snlim=snlim)

class MeasurerSimple:
	def __init__(self, nmat, beam, scaling=1):
		self.beam, self.nmat, self.scaling = beam, nmat, scaling
		self.order = 3
	def __call__(self, map, icat):
		"""Bunch(cat): icat with snr, flux_tot, dflux_tot, flux and dflux read off map [n,ny,nx] at its positions (analysis.py:899-929)"""
		if map.ndim != 3: raise ValueError("map must be a map with 3 axes")
		cat = icat.copy()
		pixs = enmap.sky2pix(map.shape, map.wcs, [icat.dec, icat.ra])
		rho, kappa = self.nmat.matched_filter(map, self.beam)
		kappa = sanitize_kappa(kappa)
		rho_tot, kappa_tot, snr_tot = _totals(enmap._data(rho), enmap._data(kappa), self.scaling)
		flux_tot, dflux_tot = solve_mapsys(_like(kappa_tot, map), _like(rho_tot, map))
		cat.snr = _read(_like(snr_tot, map), pixs, 0)
		cat.flux_tot = _read(flux_tot, pixs, self.order)
		cat.dflux_tot = _read(dflux_tot, pixs, 0)
		flux, dflux = solve_mapsys(kappa, rho)
		cat.flux = _read(flux, pixs, self.order).T
		cat.dflux = _read(dflux, pixs, 0).T
		return Bunch(cat=cat)
