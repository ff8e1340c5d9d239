"""Curved-sky wavelet (needlet) transforms on the device: the interface of pixell.wavelets.WaveletTransform over the HIP transforms.

A wavelet basis is a set of isotropic harmonic filters f_i(l), i = 0 .. n-1, with sum_i f_i(l)^2 = 1 on [lmin, lmax], each vanishing
(or negligible) above its own band limit lmaxs[i].  The coefficients of a map m are the maps

    w_i = Y_i (f_i / norm_i) A m                      (map2wave)

(A: analysis at the basis' lmax; Y_i: synthesis on the grid of scale i, only as fine as lmaxs[i] needs), and the transpose

    m = Y sum_i (f_i norm_i) A_i w_i                  (wave2map)

gives the map back because the f_i^2 add up to one.  norm_i^2 = sum_l f_i(l)^2 (2l+1)/4pi, so that the variance of w_i of a
homogeneous field is its power spectrum near lmids[i].  The coefficients live in a multimap (pixell_amd.multimap): ndmaps for numpy
maps (staged through the device), dmaps for enmap.dmap input, and then nothing leaves HBM.

How it runs: ONE analysis, ONE launch of the filter bank (almops.bank_split_groups: every scale's filtered, truncated alm, the input
read once), then one batched synthesis per DISTINCT geometry -- the scales that share a grid (all those with lmax <= 90 share the 2
degree grid) are a leading batch axis with a common band limit L = max lmaxs of the group; rows above a scale's own lmaxs[i] are zero and
add nothing.  wave2map is the mirror image: one batched analysis per distinct geometry at the group's L, one bank_merge (which drops
what lies above each lmaxs[i]), one synthesis.  The transform owns the plans it uses (sht.PlanPin): after the first call no plan is built again, whatever
the size of the process-wide plan cache.

Flat-sky mode, the variance transform and the Haar / digital / scale-discrete bases of the reference are not here."""
import numpy as np
from . import enmap, curvedsky, multimap, almops, sht, _arrays as A, wcs as wcsutils

degree = np.pi/180

# ---------------------------------------------------------------------------------------
# bases
# ---------------------------------------------------------------------------------------
def trim_kernel(a, tol):
	"""a lowpass profile a in [0, 1] stretched by tol at both ends and clipped, so that it reaches exactly 0 and 1"""
	return np.clip(a*(1+2*tol)-tol, 0, 1)

class _ButterBase:
	"""wavelets from differences of Butterworth lowpass profiles B_i(l) = 1/(1 + (l/l_i)^a), l_i = lmin step^(i+1/2), a = shape/ln(step):
	f_i^2 = B_i - B_(i-1), with B_(-1) = 0 and B_(n-1) = 1, n = floor(log_step(lmax/lmin))"""
	def __init__(self, step, shape, lmin, lmax):
		self.step, self.shape, self.lmin, self.lmax = step, shape, lmin, lmax
		if lmin is not None and lmax is not None:
			self.n = int((np.log(lmax)-np.log(lmin))/np.log(step))
			self.lmaxs = self._cut(self._reach()*self.step**(np.arange(self.n)+0.5)).astype(int)
			self.lmaxs[-1] = lmax
	def lowpass(self, i, l): return 1/(1+(l/(self.lmin*self.step**(i+0.5)))**(self.shape/np.log(self.step)))
	def __call__(self, i, l):
		l = np.asarray(l)
		prof = np.full(l.shape, 1.0) if i == self.n-1 else self.kernel(i, l)
		if i > 0: prof = prof-self.kernel(i-1, l)
		return prof**0.5
	def get_variance_basis(self):
		raise NotImplementedError("the variance transform (a radial Fourier transform of the squared profiles) is not implemented")

class Butterworth(_ButterBase):
	"""Butterworth wavelets: well localised in both spaces, but the filters have tails to all l; scale i is cut where its lowpass
	has fallen to tol"""
	def __init__(self, step=2, shape=7, tol=1e-3, lmin=None, lmax=None):
		self.tol = tol
		_ButterBase.__init__(self, step, shape, lmin, lmax)
	def with_bounds(self, lmin, lmax): return Butterworth(step=self.step, shape=self.shape, tol=self.tol, lmin=lmin, lmax=lmax)
	def kernel(self, i, l): return self.lowpass(i, l)
	# B_i(l) = tol  <=>  l = l_i (1/tol - 1)^(1/a)
	def _reach(self): return self.lmin*(1/self.tol-1)**(np.log(self.step)/self.shape)
	_cut = staticmethod(np.round)

class ButterTrim(_ButterBase):
	"""Butterworth wavelets whose lowpass profiles are trimmed (trim_kernel), which makes every filter exactly band limited: the
	default basis"""
	def __init__(self, step=2, shape=7, trim=1e-2, lmin=None, lmax=None):
		self.trim = trim
		_ButterBase.__init__(self, step, shape, lmin, lmax)
	def with_bounds(self, lmin, lmax): return ButterTrim(step=self.step, shape=self.shape, trim=self.trim, lmin=lmin, lmax=lmax)
	def kernel(self, i, l): return trim_kernel(self.lowpass(i, l), self.trim)
	# B_i(l) (1 + 2 trim) - trim = 0  <=>  l = l_i ((1 + 2 trim)/trim - 1)^(1/a)
	def _reach(self): return self.lmin*((1+2*self.trim)/self.trim-1)**(np.log(self.step)/self.shape)
	_cut = staticmethod(np.ceil)

class CosineNeedlet:
	"""cosine-shaped needlets (Coulton et al. 2023, arXiv:2307.01258): filter i rises as cos from the previous peak to its own peak
	lpeaks[i] and falls to the next one.  Intervals are half open, so the last filter is zero AT l = lpeaks[-1]."""
	def __init__(self, lpeaks):
		self.lpeaks = lpeaks
		self.lmaxs = np.append(self.lpeaks[1:], self.lpeaks[-1])
		self.lmins = np.append(self.lpeaks[0], self.lpeaks[:-1])
		self.lmin, self.lmax = self.lpeaks[0], self.lpeaks[-1]
	@property
	def n(self): return len(self.lpeaks)
	def with_bounds(self, lmin, lmax):
		"""the peaks fix the bounds: a copy"""
		return CosineNeedlet(self.lpeaks)
	def __call__(self, i, l):
		l = np.asarray(l); out = l*0.0
		here = self.lpeaks[i]
		if i > 0:
			prev = self.lpeaks[i-1]; up = (l >= prev) & (l < here)
			out[up] = np.cos(np.pi*(here-l[up])/(here-prev)/2.)
		if i < self.n-1:
			nxt = self.lpeaks[i+1]; down = (l >= here) & (l < nxt)
			out[down] = np.cos(np.pi*(l[down]-here)/(nxt-here)/2.)
		return out
	def get_variance_basis(self):
		raise NotImplementedError("the variance transform is not implemented")

# ---------------------------------------------------------------------------------------
# geometries
# ---------------------------------------------------------------------------------------
def make_wavelet_geometry_curved(ishape, iwcs, ores, minres=2*degree):
	"""the geometry of a wavelet scale that needs resolution ores (radians) on the patch (ishape, iwcs): the full-sky Fejer-1 grid whose
	resolution divides pi and is at least as fine as both ores and minres (SHTs need such a grid), cropped to the patch's bounding box --
	declinations clipped to the sphere, one row more at the upper end so that the last full-sky row is kept, at most one turn in RA --
	and rounded to whole pixels.  Assumes dec increasing with y and RA decreasing with x, as in the standard geometries."""
	res = min(np.pi/np.ceil(np.pi/ores), minres)
	box = enmap.corners(ishape, iwcs)
	box[:, 0] = np.clip(box[:, 0], -np.pi/2, np.pi/2)
	box[1, 1] = box[0, 1]+np.clip(box[1, 1]-box[0, 1], -2*np.pi, 2*np.pi)
	tshape, twcs = enmap.fullsky_geometry(res=res)
	pbox = enmap.skybox2pixbox(tshape, twcs, box)
	pbox[np.argmax(pbox[:, 0]), 0] += 1
	pbox[:, 1] += enmap._rewind(pbox[0, 1], 0, tshape[-1])-pbox[0, 1]
	pbox = np.round(pbox).astype(int)
	(y0, x0), (y1, x1) = pbox
	if y1 <= y0 or x1 <= x0: raise ValueError("make_wavelet_geometry_curved: the patch must have dec increasing with y and RA decreasing with x")
	owcs = twcs.deepcopy()
	owcs.wcs.crpix[0] -= x0; owcs.wcs.crpix[1] -= y0
	return (int(y1-y0), int(x1-x0)), owcs

# ---------------------------------------------------------------------------------------
# the transform
# ---------------------------------------------------------------------------------------
def _consecutive(idx): return all(b == a+1 for a, b in zip(idx[:-1], idx[1:]))

def _split_last(x, n, npix):
	"""x[..., n*npix] -> x[..., n, npix] without a copy"""
	if A.is_tensor(x): return x.unflatten(-1, (n, npix))
	v = x.view(); v.shape = x.shape[:-1]+(n, npix); return v


class WaveletTransform:
	"""map2wave / wave2map between a map on uht's geometry and its wavelet coefficients (a multimap).

	 from pixell_amd import enmap, uharm, wavelets, multimap
	 uht  = uharm.UHT(shape, wcs, mode="curved", lmax=lmax)
	 wt   = wavelets.WaveletTransform(uht)              # ButterTrim basis; wt.nlevel scales on wt.geometries
	 wmap = wt.map2wave(enmap.dmap(tensor, wcs))        # multimap.dmaps: wmap.maps[i] is scale i, wmap *= 2 etc. act on all of them
	 N    = multimap.var(wmap)                          # [nlevel]: the power near wt.lmids
	 omap = wt.wave2map(wmap)

	basis: a basis object (lmin / lmax are derived from the geometry and uht.lmax where the basis leaves them open); ores: resolution of
	the wavelet maps in radians, a number for all scales or one per scale (default: what each scale's band limit needs, at most the input's and
	at least 2 degrees); norms: replaces the normalisation; geometries: the scales' (shape, wcs) given explicitly."""
	def __init__(self, uht, basis=ButterTrim(), ores=None, norms=None, geometries=None):
		if uht.mode == "flat": raise NotImplementedError("WaveletTransform: flat-sky mode (uht.mode == 'flat') is not implemented; use a UHT with mode='curved'")
		self.uht, self.basis = uht, basis
		ires = np.max(enmap.pixshapebounds(uht.shape, uht.wcs))
		if self.basis.lmax is None or self.basis.lmin is None:
			lmin, lmax = self.basis.lmin, self.basis.lmax
			if lmax is None: lmax = min(int(np.ceil(np.pi/ires)), uht.lmax)
			if lmin is None: lmin = min(int(np.ceil(np.pi/np.max(enmap.extent(uht.shape, uht.wcs)))), lmax)
			self.basis = basis.with_bounds(lmin, lmax)
		if geometries is None:
			oress = np.maximum(np.pi/self.basis.lmaxs, ires) if ores is None else np.zeros(self.basis.n)+ores
			geometries = [make_wavelet_geometry_curved(uht.shape, uht.wcs, o) for o in oress]
		self.geometries = [(tuple(int(n) for n in shape[-2:]), wcs) for shape, wcs in geometries]
		if len(self.geometries) != self.basis.n: raise ValueError("WaveletTransform: %d geometries for a basis of %d scales" % (len(self.geometries), self.basis.n))
		ls = self.get_ls(0)
		self.filters = tuple(self.basis(i, ls) for i in range(self.nlevel))
		W = [F**2*(2*ls+1)/(4*np.pi) for F in self.filters]
		self.norms = np.array([np.sum(w)**0.5 for w in W])
		self.lmids = np.array([np.sum(w*ls)/np.sum(w) for w in W])
		if norms is not None: self.norms[:] = norms
		self.pin = sht.PlanPin()                       # the plans of the input geometry and of every scale group live as long as this object
		self.ainfo = curvedsky.alm_info(lmax=self.basis.lmax)
		self._ainfos = {}
	@property
	def shape(self): return self.uht.shape
	@property
	def wcs(self): return self.uht.wcs
	@property
	def geometry(self): return self.shape, self.wcs
	@property
	def nlevel(self): return len(self.geometries)
	def get_ls(self, i):
		"""the multipoles the filter of scale i is tabulated on"""
		return self.uht.l
	def get_variance_transform(self):
		return WaveletTransform(self.uht, basis=self.basis.get_variance_basis(), norms=self.norms**2, geometries=self.geometries)
	# ---- helpers
	def _groups(self, scales):
		"""[(L, [scale indices], (shape, wcs))]: the requested scales by distinct geometry, L the largest band limit of each group"""
		groups = {}
		for i in scales:
			key = enmap._geo_key(*self.geometries[i])
			groups.setdefault(key if key is not None else ("scale", i), []).append(i)
		return [(int(max(self.basis.lmaxs[i] for i in idx)), idx, self.geometries[idx[0]]) for idx in groups.values()]
	def _small(self, L):
		if L not in self._ainfos: self._ainfos[L] = curvedsky.alm_info(lmax=L)
		return self._ainfos[L]
	def _check_pre(self, pre):
		if len(pre) > 0: list(enmap.spin_helper([0, 2], pre[-1]))          # T or T,Q,U ...: a cut pair raises as in the transforms themselves
	def _wave_data(self, wave): return wave.tensor if isinstance(wave, multimap.dmaps) else np.asarray(wave)
	def _as_map(self, data, wcs): return enmap.dmap(data, wcs) if A.is_tensor(data) else enmap.ndmap(data, wcs)
	# ---- transforms
	def map2wave(self, map, owave=None, fl=None, scales=None, fill_value=None):
		"""wavelet coefficients of map[..., ny, nx] (leading dimensions: T, or T,Q,U with the transforms' default spin [0, 2]) as a multimap:
		dmaps for an enmap.dmap, ndmaps (staged through the device) for a numpy map.  owave: a multimap with this transform's geometries
		to write into.  fl: a filter (array from l = 0, or function of l) applied to the map in harmonic space on the way.  scales: the indices
		to compute; the others cost no transform and hold fill_value (default 0)."""
		pre = tuple(map.shape[:-2]); self._check_pre(pre)
		want = sorted(set(range(self.nlevel) if scales is None else [int(i) for i in scales]))
		dm, staged = enmap._to_device(map)
		mdata = curvedsky._mdata(dm); rdt = A.np_dtype(mdata)
		geos = [(pre+shape, wcs) for shape, wcs in self.geometries]
		offs = multimap._offsets(multimap.nopre(geos))
		fresh = owave is None or A.is_tensor(self._wave_data(owave)) != A.is_tensor(mdata) or owave.dtype != rdt
		if owave is not None and (tuple(owave.npixs) != tuple(offs[1:]-offs[:-1]) or tuple(owave.pre) != pre): raise ValueError("map2wave: owave does not have this transform's geometries and the map's leading dimensions")
		work = multimap.zeros(geos, rdt, device=mdata.device if A.is_tensor(mdata) else None) if fresh else owave
		wdata = self._wave_data(work)
		with self.pin:
			alm = curvedsky.map2alm(dm, ainfo=self.ainfo)
			if fl is not None:
				fl = np.asarray(fl(np.arange(self.ainfo.lmax+1.0)) if callable(fl) else fl)
				if fl.ndim > 1: alm = curvedsky.almxfl(alm, fl, ainfo=self.ainfo); fl = None          # (one filter per component: its own pass)
			filters = [self.filters[i]/self.norms[i] for i in range(self.nlevel)]
			if fl is not None:
				flp = np.zeros(self.ainfo.lmax+1); flp[:min(len(fl), len(flp))] = fl[:len(flp)]
				filters = [f*flp for f in filters]
			table = almops._filter_table(filters, self.basis.lmaxs, self.ainfo.lmax+1, A.np_dtype(alm))
			groups = self._groups(want)
			apre = pre if pre else (1,)
			salms = almops.bank_split_groups(self.ainfo, alm.reshape(apre+(alm.shape[-1],)), table, self.basis.lmaxs, [(L, idx) for L, idx, geo in groups])
			for (L, idx, (shape, wcs)), salm in zip(groups, salms):
				ng = len(idx); npix = shape[0]*shape[1]
				block = wdata[..., offs[idx[0]]:offs[idx[-1]+1]] if _consecutive(idx) else None
				tgt = curvedsky._as_view(block, (ng, 1)+shape) if block is not None and pre == () else None       # scalar maps, side by side: written in place
				direct = tgt is not None
				if not direct: tgt = A.empty((ng,)+apre+shape, rdt, like=mdata)
				curvedsky.alm2map(salm, self._as_map(tgt, wcs), ainfo=self._small(L))
				if direct: continue
				src = tgt.reshape((ng,)+pre+(npix,))
				if block is not None: _split_last(block, ng, npix)[...] = src.movedim(0, -2) if A.is_tensor(src) else np.moveaxis(src, 0, -2)
				else:
					for k, i in enumerate(idx): wdata[..., offs[i]:offs[i+1]] = src[k]
		for i in range(self.nlevel):
			if i not in want and not (fresh and fill_value is None): wdata[..., offs[i]:offs[i+1]] = 0 if fill_value is None else fill_value
		if owave is None: return work.to_host() if staged else work
		if work is not owave:
			host = work.to_host() if isinstance(work, multimap.dmaps) else work
			if isinstance(owave, multimap.dmaps): owave.tensor.copy_(A.torch().as_tensor(np.asarray(host), device=owave.tensor.device))
			else: owave[...] = host
		return owave
	def wave2map(self, wave, omap=None):
		"""the map of the wavelet coefficients `wave` (multimap.ndmaps or dmaps): the transpose of map2wave, and its inverse for coefficients
		that came from it.  omap: a map on this transform's geometry to write into.  Every scale is analysed at the common band limit of
		the scales that share its grid; what lies above its own lmaxs[i] is dropped when the scales are summed."""
		pre = tuple(wave.pre); self._check_pre(pre)
		if tuple(wave.npixs) != tuple(s[0]*s[1] for s, w in self.geometries): raise ValueError("wave2map: the multimap does not have this transform's geometries")
		wdata = self._wave_data(wave); staged = not A.is_tensor(wdata)
		if staged: wdata = A.put(wdata); staged = A.is_tensor(wdata)
		rdt = A.np_dtype(wdata); cdt = np.result_type(rdt, 0j)
		offs = multimap._offsets(wave.geometries)
		apre = pre if pre else (1,)
		table = almops._filter_table([self.filters[i]*self.norms[i] for i in range(self.nlevel)], self.basis.lmaxs, self.ainfo.lmax+1, cdt)
		groups = self._groups(range(self.nlevel))
		with self.pin:
			salms = []
			for L, idx, (shape, wcs) in groups:
				ng = len(idx); npix = shape[0]*shape[1]
				block = wdata[..., offs[idx[0]]:offs[idx[-1]+1]] if _consecutive(idx) else None
				src = curvedsky._as_view(block, (ng, 1)+shape) if block is not None and pre == () else None
				if src is None:
					src = A.empty((ng,)+apre+shape, rdt, like=wdata); flat = src.reshape((ng,)+pre+(npix,))
					if block is not None: flat[...] = _split_last(block, ng, npix).movedim(-2, 0) if A.is_tensor(block) else np.moveaxis(_split_last(block, ng, npix), -2, 0)
					else:
						for k, i in enumerate(idx): flat[k] = wdata[..., offs[i]:offs[i+1]]
				salms.append(curvedsky.map2alm(self._as_map(src, wcs), ainfo=self._small(L)))
			oalm = A.empty(apre+(self.ainfo.nelem,), cdt, like=wdata)
			almops.bank_merge_groups(self.ainfo, salms, table, self.basis.lmaxs, [(L, idx) for L, idx, geo in groups], oalm)
			kind_ok = omap is not None and isinstance(omap, enmap.dmap) == A.is_tensor(wdata) and omap.dtype == rdt and tuple(omap.shape) == pre+tuple(self.shape)
			if kind_ok: work = omap
			else:
				work = self._as_map(A.zeros(pre+tuple(self.shape), rdt, like=wdata), self.wcs)
			curvedsky.alm2map(oalm.reshape(pre+(self.ainfo.nelem,)), work, ainfo=self.ainfo)
		if omap is None: return enmap._to_host(work) if staged else work
		if work is not omap:
			host = enmap._to_host(work)
			if isinstance(omap, enmap.dmap): omap.tensor.copy_(A.torch().as_tensor(np.asarray(host), device=omap.tensor.device))
			else: omap[...] = host
		return omap
