"""Curved-sky CMB lensing on the device: the call signatures of pixell.lensing (lensing.py:78-133, 367-632).

lens_map_curved is gradient synthesis -> deflection -> point synthesis -> polarisation rotation, declination band by declination
band.  The two transforms are curvedsky.alm2map(deriv=True) and curvedsky.alm2map_pos; the elementwise step between them -- the
observed pixel positions, their geodesic offset by the gradient and the induced polarisation rotation -- is one kernel
(pxm_deflect, csrc/lensing.hip) that reads the band's gradient and writes positions in the form the point plan takes, followed by
one in-place rotation (pxm_rotate_pol).  No position map is made and nothing leaves the device.

Not here: the flat-sky lens_map, lens_map_flat, displace_map, delens_map and delens_grad interpolate maps with splines, which this
package does not have; method="lenspyx" needs the lenspyx package."""
import numpy as np
from . import enmap, curvedsky, _lib, _arrays as A, wcs as wcsutils

degree = np.pi/180

def phi_to_kappa(phi_alm, phi_ainfo=None):
	"""lensing potential alm -> convergence alm: phi_lm l (l+1) / 2"""
	return curvedsky.almxfl(alm=phi_alm, lfilter=lambda l: l*(l+1)/2, ainfo=phi_ainfo)

def kappa_to_phi(kappa_alm, kappa_ainfo=None):
	"""convergence alm -> lensing potential alm: kappa_lm / (l (l+1) / 2), the monopole set to zero"""
	def inverse(l):
		f = np.zeros(len(l))
		f[1:] = 2.0/(l[1:]*(l[1:]+1))
		return f
	return curvedsky.almxfl(alm=kappa_alm, lfilter=inverse, ainfo=kappa_ainfo)

def pole_wrap(pos):
	"""pos [{dec,ra},...] with points that went over a pole reflected back: dec -> +-pi - dec, ra -> ra + pi"""
	if A.is_tensor(pos):
		torch = A.torch()
		a = pos.clone()
		north, south = a[0] > np.pi/2, a[0] < -np.pi/2
		a[0] = torch.where(north, np.pi-a[0], torch.where(south, -np.pi-a[0], a[0]))
		a[1] = torch.where(north | south, a[1]+np.pi, a[1])
		return a
	a = np.array(pos)
	north, south = a[0] > np.pi/2, a[0] < -np.pi/2
	a[0] = np.where(north, np.pi-a[0], np.where(south, -np.pi-a[0], a[0]))
	a[1] = np.where(north | south, a[1]+np.pi, a[1])
	return a

# ---- deflection ------------------------------------------------------------------------------------------------------------
def _device_array(x, dtype=None):
	"""x where the library reads it: numpy arrays go to the GPU (they stay numpy in the simulator), tensors must be there already and
	keep their strides"""
	if A.is_tensor(x): return A.require_gpu(x) if dtype is None else A.require_gpu(x).to(A.tdtype(dtype))
	return A.put(x, dtype)

def _deflect(grad, geodesic, want_psi, pos=None, geometry=None):
	"""pxm_deflect: grad [2, ...] (device array, f32 | f64, pixels contiguous) at the positions pos [{dec,ra}(,psi0), ...] (device array, f64,
	contiguous) or at the pixel centres of geometry = (shape, wcs) -> loc [npts, 2] = (colatitude, ra in [0, 2 pi)), psi [npts] | None"""
	npts = int(np.prod(grad.shape[1:], dtype=np.int64))
	if A.np_dtype(grad) not in (np.dtype(np.float32), np.dtype(np.float64)): raise ValueError("the gradient must be float32 or float64")
	if A.is_tensor(grad):
		inner = grad[0]
		if not inner.is_contiguous(): grad = grad.contiguous()
		gstride = grad.stride(0) if grad.shape[0] > 1 else npts
	else:
		grad = np.ascontiguousarray(grad); gstride = npts
	if grad.shape[0] != 2: raise ValueError("the gradient must have shape [2, ...]")
	loc = A.empty((npts, 2), np.float64, like=grad)
	psi = A.empty((npts,), np.float64, like=grad) if want_psi else None
	if pos is not None:
		if tuple(pos.shape[1:]) != tuple(grad.shape[1:]) or pos.shape[0] not in (2, 3): raise ValueError("positions [{dec,ra}(,psi0), ...] and gradient [2, ...] disagree on their shapes")
		geo = (0, 0, 0.0, 0.0, 0.0, 0.0, A.ptr(pos), int(pos.shape[0]))
	else:
		shape, wcs = geometry
		geo = wcsutils.separable_geometry(shape, wcs)+(None, 0)
		if tuple(shape[-2:]) != tuple(grad.shape[1:]): raise ValueError("geometry and gradient disagree on the pixel shape")
	_lib.check(_lib.load().pxm_deflect(npts, *geo, A.ptr(grad), A.DT[A.np_dtype(grad)], int(gstride), int(bool(geodesic)),
		A.ptr(loc), A.ptr(psi), A.device_index(), A.current_stream()))
	return loc, psi

def offset_by_grad(ipos, grad, geodesic=True, pol=None, _loc=False, _geometry=None):
	"""The positions ipos [{dec,ra}(,psi0),...] moved by grad [{d/ddec, (d/dra)/cos dec},...] (what curvedsky.alm2map(deriv=True)
	returns): along the geodesic that leaves each point in the direction of the gradient, for its length; geodesic=False adds the
	gradient to the coordinates instead (faster in the reference, wrong near the poles; here both are one kernel pass).  Returns
	[{dec,ra},...], or [{dec,ra,psi},...] when pol is true or, with pol=None, ipos has a third component: psi is the rotation of the
	polarisation basis under the parallel transport (plus ipos[2] if given; 0 when not geodesic).  ra comes back in [0, 2 pi).
	Device arrays in, device arrays out; numpy in, numpy out.
	Internal: _loc=True returns (loc [npts, 2] = (colatitude, ra), psi [npts] | None) as the kernel wrote them, on the device;
	_geometry=(shape, wcs) takes the pixel centres of that geometry as ipos (ipos=None) without making them."""
	grad, ipos = A.unwrap(grad), A.unwrap(ipos)
	like = getattr(ipos, "wcs", None)
	on_host = not A.is_tensor(grad) and not (ipos is not None and A.is_tensor(ipos))
	nin = 2 if ipos is None else int(ipos.shape[0])
	ncomp = 2 if pol is False or (pol is None and nin <= 2) else 3
	dgrad = _device_array(grad)
	dpos = None
	if ipos is not None:
		dpos = A.put(ipos, np.float64)
		if A.is_tensor(dpos) and A.is_tensor(dgrad) and dpos.device != dgrad.device: dgrad = dgrad.to(dpos.device)
	loc, psi = _deflect(dgrad, geodesic, ncomp > 2, pos=dpos, geometry=_geometry)
	if _loc: return loc, psi
	pixshape = tuple(grad.shape[1:])
	out = A.empty((ncomp,)+pixshape, np.float64, like=loc)
	o2 = out.reshape(ncomp, -1)
	o2[0] = np.pi/2-loc[:, 0]; o2[1] = loc[:, 1]
	if ncomp > 2: o2[2] = psi
	if on_host: out = A.host(out)
	if not A.is_tensor(out) and like is not None: out = enmap.ndmap(out, like)
	return out

# ---- simulation ------------------------------------------------------------------------------------------------------------
def rand_alm(ps_lensinput, lmax=None, dtype=np.float64, seed=None, phi_seed=None, verbose=False, ncomp=None):
	"""(phi_alm, cmb_alm [ncomp, nelem], ainfo) drawn from the joint spectrum ps_lensinput [1+ncomp, 1+ncomp, nl] of (phi, T, E, B).
	phi_seed: phi and the CMB are drawn from separate seeds (uncorrelated white numbers, coloured together).  The numbers are those of
	the reference for the same seeds (numpy's legacy generator, curvedsky.rand_alm_white)."""
	ctype = np.result_type(dtype, 0j)
	ps_lensinput = np.asarray(ps_lensinput)
	if ncomp is not None: ps_lensinput = ps_lensinput[:1+ncomp, :1+ncomp]
	if phi_seed is None:
		alm, ainfo = curvedsky.rand_alm(ps_lensinput, lmax=lmax, seed=seed, dtype=ctype, return_ainfo=True)
	else:
		wps, ainfo = curvedsky.prepare_ps(ps_lensinput, lmax=lmax)
		alm = np.empty((wps.shape[0], ainfo.nelem), ctype)
		curvedsky.rand_alm_white(ainfo, alm=alm[:1], seed=phi_seed)
		curvedsky.rand_alm_white(ainfo, alm=alm[1:], seed=seed)
		colour = (curvedsky._multi_sqrt(wps)/np.sqrt(2.0)).astype(dtype)
		alm = np.asarray(ainfo.lmul(alm, colour, alm))
		# m = 0 is real with the full variance.  The reference stops this one short of l = lmax (its slice ends at lmax, not lmax + 1);
		# kept, so that a seed gives the reference's alm bit for bit
		m0 = alm[:, :ainfo.lmax]
		m0.imag = 0; m0.real *= 2**0.5
	return alm[0], alm[1:], ainfo

def rand_map(shape, wcs, ps_lensinput, lmax=None, dtype=np.float64, seed=None, phi_seed=None, spin=[0, 2], output="l", geodesic=True, verbose=False, delta_theta=None):
	"""lens_map_curved of a realisation of rand_alm with as many CMB components as the map has"""
	shape = tuple(shape)
	ncomp = 1 if len(shape) == 2 else shape[-3]
	phi_alm, cmb_alm, ainfo = rand_alm(ps_lensinput, lmax=lmax, dtype=dtype, seed=seed, phi_seed=phi_seed, verbose=verbose, ncomp=ncomp)
	return lens_map_curved(shape, wcs, phi_alm, cmb_alm, phi_ainfo=ainfo, dtype=dtype, spin=spin, output=output, geodesic=geodesic,
		verbose=verbose, delta_theta=delta_theta)

# ---- the lensing operation ---------------------------------------------------------------------------------------------------
def _band_size(ny, wcs, delta_theta):
	"""rows per declination band: delta_theta in rows, shrunk so that the last band is not a sliver (the reference's rule, lensing.py:450-455)"""
	if delta_theta is None: return ny
	rows = int(np.round(abs(delta_theta/degree/wcs.wcs.cdelt[1])))
	if rows < 1: raise ValueError("delta_theta is smaller than a pixel row")
	return max(int(ny/(ny//rows+0.5)), 1)

def _rotate_band(obs, psi):
	"""in place: the last two components of the band obs [ncomp, rows, nx] rotated by 2 psi.  The band may be rows of a larger device map:
	its components are then a whole map apart, each one's rows still contiguous"""
	npix = int(obs.shape[-2])*int(obs.shape[-1]); ncomp = int(obs.shape[0])
	cstride = obs.stride(0) if A.is_tensor(obs) else npix
	esz = A.np_dtype(obs).itemsize
	_lib.check(_lib.load().pxm_rotate_pol(npix, 1, A.ptr(obs)+(ncomp-2)*cstride*esz, A.ptr(obs)+(ncomp-1)*cstride*esz, 0,
		A.DT[A.np_dtype(obs)], A.ptr(psi), 2, A.device_index(), A.current_stream()))

def lens_map_curved(shape, wcs, phi_alm, cmb_alm, phi_ainfo=None, dtype=np.float64, spin=[0, 2], output="l", method="pixell",
		geodesic=True, delta_theta=None, epsilon=None, nthreads=0, verbose=False):
	"""Lensed CMB maps from the alm of the lensing potential and of the CMB (lensing.lens_map_curved, lensing.py:367-503).
	shape, wcs: the output geometry (separable cylindrical; of shape only the last three axes count); cmb_alm [ncomp, nelem] or
	[nelem], (T, E, B) for the default spin=[0, 2]; output: which maps to return, in this order -- "l" lensed CMB, "u" unlensed CMB,
	"p" lensing potential, "k" convergence, "a" deflection (the gradient of the potential, [2, ny, nx]).  geodesic: move the points along
	geodesics and rotate the polarisation accordingly (default); False adds the gradient to the coordinates.  delta_theta: height in
	radians of the declination bands the work is done in (default: the whole map at once); a band needs its gradient, positions and
	rotation angles (40 bytes per pixel) and its point plan on the device.  epsilon: accuracy of the point synthesis (None:
	alm2map_pos's default for the dtype).  With CUDA tensors for the alm nothing is copied to the host and dmaps come back; numpy in,
	ndmaps out.  Always returns a tuple."""
	if method == "lenspyx": raise NotImplementedError("method 'lenspyx' needs the lenspyx package, which this implementation does not use")
	if method != "pixell": raise ValueError("method must be one of 'pixell' or 'lenspyx'")
	if any(c not in "lupka" for c in output): raise ValueError("output may hold the letters l, u, p, k, a, not '%s'" % output)
	if not wcsutils.is_separable(wcs): raise NotImplementedError("lens_map_curved: only separable cylindrical geometries")
	oshape = tuple(shape[-3:])
	shape = ((1,)+oshape) if len(oshape) == 2 else oshape
	ncomp, ny, nx = shape
	on_device = A.is_tensor(phi_alm) or A.is_tensor(cmb_alm)
	ctype = np.result_type(dtype, 0j)
	def prep(alm):
		alm = _device_array(alm)
		return alm if A.np_dtype(alm) == ctype else _device_array(alm, ctype)
	phi_d, cmb_d = prep(phi_alm), prep(cmb_alm)
	if cmb_d.ndim == 1: cmb_d = cmb_d[None]
	if cmb_d.shape[0] != ncomp: raise ValueError("cmb_alm has %d components, the map %d" % (cmb_d.shape[0], ncomp))
	tens = A.is_tensor(phi_d)
	def new_map(pre, band=None):
		"""an output map (on the device when the alm came from there), or, with band = (lshape, lwcs), a work map of one band on the device"""
		shp, w = (tuple(pre)+(ny, nx), wcs) if band is None else (tuple(pre)+tuple(band[0][-2:]), band[1])
		if tens and (on_device or band is not None):
			return enmap.dmap(A.empty(shp, dtype, like=phi_d), w)
		return enmap.empty(shp, w, dtype=dtype)
	def rows(m, i1, i2): return m[..., i1:i2, :]
	host_alm = lambda a: a if on_device or not tens else A.host(a)       # (maps on the host take host alm through the package's own staging)
	bsize = _band_size(ny, wcs, delta_theta)
	maps = {}
	if "p" in output: maps["p"] = new_map(())
	if "k" in output:
		maps["k"] = new_map(())
		kappa = phi_to_kappa(host_alm(phi_d), phi_ainfo=phi_ainfo)
		for i1 in range(0, ny, bsize): curvedsky.alm2map(kappa, rows(maps["k"], i1, i1+bsize), spin=0, ainfo=phi_ainfo)
		del kappa
	if "a" in output: maps["a"] = new_map((2,))
	if "u" in output: maps["u"] = new_map((ncomp,))
	if "l" in output: maps["l"] = new_map((ncomp,))
	for i1 in range(0, ny, bsize):
		i2 = min(i1+bsize, ny)
		band = wcsutils.slice_geometry(shape, wcs, (slice(i1, i2), slice(None)))
		if "p" in output: curvedsky.alm2map(host_alm(phi_d), rows(maps["p"], i1, i2), spin=0, ainfo=phi_ainfo)
		if "a" in output and ("l" not in output or on_device or not tens):
			grad = rows(maps["a"], i1, i2)
			curvedsky.alm2map(host_alm(phi_d), grad, deriv=True, ainfo=phi_ainfo)
		elif "a" in output or "l" in output:
			grad = new_map((2,), band)
			curvedsky.alm2map(phi_d, grad, deriv=True, ainfo=phi_ainfo)
			if "a" in output: rows(maps["a"], i1, i2)[...] = A.host(grad)
		if "u" in output: curvedsky.alm2map(host_alm(cmb_d), rows(maps["u"], i1, i2), spin=spin)
		if "l" not in output: continue
		rotate = geodesic and ncomp > 1
		loc, psi = offset_by_grad(None, grad, geodesic=geodesic, pol=rotate, _loc=True, _geometry=band)
		del grad
		dest = rows(maps["l"], i1, i2)
		in_place = isinstance(dest, enmap.dmap)
		obs = dest.tensor if in_place else (new_map((ncomp,), band).tensor if tens else np.empty((ncomp, i2-i1, nx), dtype))
		got = curvedsky.alm2map_pos(cmb_d, loc=loc.reshape(i2-i1, nx, 2), map=obs, spin=spin, epsilon=epsilon)
		if A.ptr(got) != A.ptr(obs): obs[...] = got
		del loc, got
		if rotate: _rotate_band(obs, psi)
		del psi
		if not in_place: dest[...] = A.host(obs)
	res = []
	for c in output:
		m = maps[c]
		if c in "lu": m = m[0] if len(oshape) == 2 else m
		res.append(m)
	return tuple(res)
