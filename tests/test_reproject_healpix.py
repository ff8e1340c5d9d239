"""pixell_amd.healpix (pxm_healpix_index, pxm_healpix_interp) and reproject.map2healpix / healpix2map (pxm_map2healpix, pxm_healpix2map, and
the harmonic route through curvedsky): the pixel arithmetic against this file's own numpy statement of the RING scheme and against the
ring tables of curvedsky.get_ring_info_healpix; the reprojections against the reference's own map2healpix / healpix2map as
tests/golden/make_reproject.py drives them (fixture reproject.npz), against the unfused device path and against band-limited truth.
healpy is nowhere: parity with it is not pinned.

Tolerances (EPS = 2^-52; m a healpix map, f a CAR map, c the array the taps read):
  pix2ang            4e-15 of the ring tables' centres: the 2e-15 test_healpix.py pins those tables at, once more for the device's asin / acos
  ang2pix            exact, except where a floor argument of the numpy statement lies within 1e-9 of an integer (at most 0.1 % of random
                     directions, none on the shifted grid); on the unshifted grid, whose columns lie on face boundaries, either pixel
                     of a tie is accepted and at most 3.2 % of the pixels may need that
  weights            sum to 1 within 4 EPS, >= 0, indices in [0, npix); at pixel centres the value is the map's within 64 EPS max|m|
  ring-bilinear      64 EPS max|m| + 8 EPS (4 nside) max|dm|, dm the largest difference among a point's four taps (test_interpol.py's
                     second and third term with 4 nside for max(ny, nx)); float32 maps: + 2^-24 max|m|
  CAR -> healpix     test_thumbnails.py's: 4 E_ref max|f| + 64 EPS max|c| + max(8, 4 K_pos) EPS max(ny, nx) max|dc|, + s dang max|f| for a
                     spin-s pair, + 2^-24 max|f| for float32 results; order 0 without rotation is exact.  K_pos and dang: the fixture's
  healpix -> CAR     order 1: the ring-bilinear bound with max(8, 4 K_pos) in its second term, + s dang max|m|; order 0: equality under
                     the exclusion rule of ang2pix
  harm               1e-10 max|.|, the figure test_healpix.py pins the analysis routes with
Each body runs in the host simulator (*_sim) and on the GPU (*_gpu)."""
import os
import numpy as np
import pytest
from pixell_amd import curvedsky, enmap, healpix, interpol, reproject
from pixell_amd.wcs import CarWCS

EPS = 2.0**-52
degree = np.pi/180
NSIDES = (1, 2, 3, 4, 8)
ROTS = {"none": None, "galequ": "gal,equ", "equgal": "equ,gal", "euler": (0.3, 1.1, -0.7)}

@pytest.fixture(scope="module")
def fx(golden_dir):
	return dict(np.load(os.path.join(golden_dir, "reproject.npz")))

def host(x):
	if isinstance(x, enmap.dmap): x = x.tensor
	return x.detach().cpu().numpy() if hasattr(x, "data_ptr") else np.asarray(x)
def ident(a): return a
def cuda(a):
	import torch
	return torch.as_tensor(np.ascontiguousarray(a), device="cuda")
def as_map(dev, a, wcs): return enmap.ndmap(a, wcs) if dev is ident else enmap.dmap(dev(a), wcs)

def car(shift=0.37):
	"""the full-sky CAR grid (36, 72) at 5 degrees (enmap.fullsky_geometry: its columns lie on ra = 5 k degrees), the columns shifted by `shift` pixel"""
	shape, wcs = enmap.fullsky_geometry(res=5*degree)
	assert shape == (36, 72)
	wcs.wcs.crpix[0] += shift
	return shape, wcs
def geometry(numbers):
	n = np.asarray(numbers, float)
	return (int(n[0]), int(n[1])), CarWCS(cdelt=n[2:4], crval=n[4:6], crpix=n[6:8])

# ---- the RING scheme in numpy (this file's own statement of csrc/healpix.hip's docstring) ------------------------------------------------
def np_ring(nside, r):
	"""(theta, phi0, first pixel, pixels) of the rings r (1-based from the north; entries outside 1 .. 4 nside - 1 give rubbish that nobody reads)"""
	r = np.asarray(r, np.int64); nl4, npix = 4*nside, 12*nside**2
	south = r > 2*nside
	j = np.where(south, nl4-r, r)
	cap = j < nside
	jc = np.maximum(np.where(cap, j, 1), 1)
	theta = np.where(cap, 2*np.arcsin(jc/(np.sqrt(6.0)*nside)), np.arccos(np.clip((2*nside-j)*(2.0/(3*nside)), -1, 1)))
	theta = np.where(south, np.pi-theta, theta)
	phi0 = np.where(cap, np.pi/(4*jc), np.where((j-nside) % 2 == 0, np.pi/nl4, 0.0))
	start = np.where(cap, np.where(south, npix-2*j*(j+1), 2*j*(j-1)), 2*nside*(nside-1)+(r-nside)*nl4)
	return theta, phi0, start, np.where(cap, 4*jc, nl4)

def np_omz(theta, north): return 2*np.sin(0.5*np.where(north, theta, np.pi-theta))**2

def np_ang2pix(nside, theta, phi):
	"""(pix, margin): the pixel that holds each direction, and how far the nearest floor argument (or the cap / belt decision, in pixels)
	lies from an integer"""
	theta, phi = np.broadcast_arrays(np.asarray(theta, float), np.asarray(phi, float))
	nl4, npix = 4*nside, 12*nside**2
	z = np.cos(theta); za = np.abs(z)
	tt = np.fmod(phi, 2*np.pi); tt = np.where(tt < 0, tt+2*np.pi, tt)/(np.pi/2); tt = np.where(tt >= 4, tt-4, tt)
	def frac(a): return np.abs(a-np.round(a))
	t1, t2 = nside*(0.5+tt), nside*z*0.75
	jp, jm = np.floor(t1-t2).astype(np.int64), np.floor(t1+t2).astype(np.int64)
	ir = nside+1+jp-jm; ks = 1-(ir & 1)
	belt = 2*nside*(nside-1)+(ir-1)*nl4+((jp+jm-nside+ks+1) >> 1) % nl4
	mbelt = np.minimum(frac(t1-t2), frac(t1+t2))
	tp = tt-np.floor(tt); tmp = nside*np.sqrt(3*np_omz(theta, z > 0))
	cp, cm = np.floor(tp*tmp).astype(np.int64), np.floor((1-tp)*tmp).astype(np.int64)
	ic = cp+cm+1
	ip = np.floor(tt*ic).astype(np.int64) % (4*ic)
	capp = np.where(z > 0, 2*ic*(ic-1)+ip, npix-2*ic*(ic+1)+ip)
	mcap = np.minimum(np.minimum(frac(tp*tmp), frac((1-tp)*tmp)), np.minimum(frac(tt*ic), frac(tt)))
	isbelt = za <= 2.0/3
	return np.where(isbelt, belt, capp), np.minimum(np.where(isbelt, mbelt, mcap), np.abs(za-2.0/3)*nside)

def np_weights(nside, theta, phi):
	"""(pix [4, n], w [4, n]) of the ring-bilinear value"""
	theta, phi = np.broadcast_arrays(np.asarray(theta, float), np.asarray(phi, float))
	nl4, npix = 4*nside, 12*nside**2
	z = np.cos(theta); za = np.abs(z)
	i = np.floor(nside*np.sqrt(3*np_omz(theta, z > 0))).astype(np.int64)
	ir1 = np.where(za <= 2.0/3, np.floor(nside*(2-1.5*z)).astype(np.int64), np.where(z > 0, i, nl4-i-1))
	ir1 = np.clip(ir1, 0, nl4-1); ir2 = ir1+1
	def pair(r):
		th, phi0, start, n = np_ring(nside, r)
		t = (phi-phi0)/(2*np.pi/n); fl = np.floor(t)
		i1 = fl.astype(np.int64) % n
		return th, start+i1, start+(i1+1) % n, t-fl
	th1, a1, a2, wa = pair(ir1); th2, b1, b2, wb = pair(ir2)
	north, south = ir1 == 0, ir2 == nl4
	wt = np.where(north, theta/th2, np.where(south, (theta-th1)/(np.pi-th1), (theta-th1)/np.where(th2 != th1, th2-th1, 1)))
	wt = np.clip(wt, 0, 1)
	pix = np.array([a1, a2, b1, b2]); w = np.array([(1-wa)*(1-wt), wa*(1-wt), (1-wb)*wt, wb*wt])
	fn, fs = (1-wt)/4, wt/4
	w = np.where(north, np.array([fn, fn, (1-wb)*wt+fn, wb*wt+fn]), np.where(south, np.array([(1-wa)*(1-wt)+fs, wa*(1-wt)+fs, fs, fs]), w))
	pix = np.where(north, np.array([(b1+2) & 3, (b2+2) & 3, b1, b2]), np.where(south, np.array([a1, a2, npix-4+((a1-(npix-4)+2) & 3), npix-4+((a2-(npix-4)+2) & 3)]), pix))
	return pix, w

def table_centres(nside):
	"""(theta, phi) of every pixel from the ring tables of curvedsky.get_ring_info_healpix"""
	ri = curvedsky.get_ring_info_healpix(nside)
	theta = np.concatenate([np.full(int(n), t) for t, n in zip(ri.theta, ri.nphi)])
	phi = np.concatenate([p0+2*np.pi*np.arange(int(n))/float(n) for p0, n in zip(ri.phi0, ri.nphi)])
	return theta, phi

def directions(nside, n=20000):
	rng = np.random.default_rng(100+nside)
	return np.arccos(rng.uniform(-1, 1, n)), rng.uniform(0, 2*np.pi, n)

def grid_angles(shape, wcs):
	pos = np.asarray(enmap.posmap(shape, wcs))
	return np.pi/2-pos[0].reshape(-1), pos[1].reshape(-1)

# ---- 1. index arithmetic ---------------------------------------------------------------------------------------------------------------
def index_body(dev, on_device):
	for nside in NSIDES+(16,):
		npix = healpix.nside2npix(nside)
		assert npix == 12*nside**2 and healpix.npix2nside(npix) == nside
		p = np.arange(npix)
		theta, phi = healpix.pix2ang(nside, dev(p))
		assert hasattr(theta, "data_ptr") == on_device and host(theta).dtype == np.float64
		tt, tp = table_centres(nside)
		err = max(np.max(np.abs(host(theta)-tt)), np.max(np.abs(host(phi)-tp)))
		print("nside %d: pix2ang within %.3g of the ring tables" % (nside, err))
		assert err <= 4e-15
		back = healpix.ang2pix(nside, theta, phi)
		assert host(back).dtype == np.int64 and np.array_equal(host(back), p), nside
		# the numpy statement's own round trip (what pins the statement, not the device)
		assert np.array_equal(np_ang2pix(nside, tt, tp)[0], p)
	for nside in NSIDES:
		for name, (th, ph), cap in (("random", directions(nside), 1e-3), ("shifted grid", grid_angles(*car()), 0.0)):
			want, margin = np_ang2pix(nside, th, ph)
			keep = margin > 1e-9
			share = 1-np.mean(keep)
			got = host(healpix.ang2pix(nside, dev(th), dev(ph)))
			print("nside %d %s: excluded share %.3g, smallest margin %.3g" % (nside, name, share, margin.min()))
			assert share <= cap and np.array_equal(got[keep], want[keep]), (nside, name)
		# ties: the unshifted grid's columns at ra = k 90 degrees lie on face boundaries
		th, ph = grid_angles(*car(shift=0.0))
		want, margin = np_ang2pix(nside, th, ph)
		got = host(healpix.ang2pix(nside, dev(th), dev(ph)))
		d = 1e-7
		either = np.array([np_ang2pix(nside, th+a*d, ph+b*d)[0] for a in (-1, 0, 1) for b in (-1, 0, 1)])
		needed = got != want
		print("nside %d unshifted grid: %.2f %% of the pixels on a boundary, %.2f %% needed the allowance" % (nside, 100*np.mean(margin < 1e-9), 100*np.mean(needed)))
		assert np.all(np.any(either == got[None], 0)) and np.mean(needed) <= 0.032, nside
	with pytest.raises(ValueError): healpix.npix2nside(13)
	if not on_device:
		with pytest.raises(ValueError): healpix.pix2ang(2, np.array([48]))

def big_nside_body(dev, on_device):
	"""nside 8192: first, middle and last pixel of 300 rings over caps and belt, through the 64-bit path and the integer square root"""
	nside = 8192
	ri = curvedsky.get_ring_info_healpix(nside)
	rings = np.unique(np.concatenate([[0, 1, 2, nside-2, nside-1, nside, nside+1, 2*nside-1, 2*nside, 3*nside-1, 3*nside, 3*nside+1, 4*nside-3, 4*nside-2],
		np.linspace(0, 4*nside-2, 288).astype(np.int64)]))      # (the ends are listed twice)
	assert len(rings) == 300
	off, n = ri.offsets[rings].astype(np.int64), ri.nphi[rings].astype(np.int64)
	p = np.concatenate([off, off+n//2, off+n-1])
	assert p.max() == 12*nside**2-1 and p.max() > 2**29
	theta, phi = healpix.pix2ang(nside, dev(p))
	k = np.concatenate([0*n, n//2, n-1])
	tt = np.tile(ri.theta[rings], 3); tp = np.tile(ri.phi0[rings], 3)+2*np.pi*k/np.tile(n, 3)
	assert np.max(np.abs(host(theta)-tt)) <= 4e-15 and np.max(np.abs(host(phi)-tp)) <= 4e-15
	assert np.array_equal(host(healpix.ang2pix(nside, theta, phi)), p)

# ---- 2. ring-bilinear weights ------------------------------------------------------------------------------------------------------------
def bilinear_tol(nside, m, taps, f32, k=8.0):
	mm = float(np.max(np.abs(m)))
	dm = float(np.max(taps.max(0)-taps.min(0))) if taps.size else 0.0
	return 64*EPS*mm+k*EPS*(4*nside)*dm+(2.0**-24*mm if f32 else 0.0)

def weights_body(dev, on_device):
	worst = 0.0
	for nside in NSIDES:
		npix = 12*nside**2
		rng = np.random.default_rng(7+nside)
		m = rng.integers(-2**20, 2**20, (2, npix)).astype(np.float64)/2**20
		th, ph = directions(nside)
		th = np.concatenate([th, [1e-9, 1e-3, np.pi-1e-3, np.pi-1e-9]*3]); ph = np.concatenate([ph, rng.uniform(-7, 14, 12)])
		pix, w = healpix.get_interp_weights(nside, dev(th), dev(ph))
		assert hasattr(pix, "data_ptr") == on_device and pix.shape == (4, len(th)) and w.shape == (4, len(th))
		pix, w = host(pix), host(w)
		assert pix.dtype == np.int64 and pix.min() >= 0 and pix.max() < npix
		assert w.min() >= 0 and np.max(np.abs(w.sum(0)-1)) <= 4*EPS
		# at pixel centres
		ct, cp = healpix.pix2ang(nside, dev(np.arange(npix)))
		at = host(healpix.get_interp_val(dev(m), ct, cp))
		assert at.shape == (2, npix)
		err = np.max(np.abs(at-m))
		print("nside %d: centres within %.3g (tol %.3g)" % (nside, err, 64*EPS*np.max(np.abs(m))))
		assert err <= 64*EPS*np.max(np.abs(m))
		# against the numpy statement
		npx, nw = np_weights(nside, th, ph)
		for dt in (np.float64, np.float32):
			md = m.astype(dt)
			want = np.array([np.sum(nw*np.float64(md[c])[npx], 0) for c in range(2)])
			got = healpix.get_interp_val(dev(md), dev(th), dev(ph))
			assert host(got).dtype == dt and hasattr(got, "data_ptr") == on_device
			tol = bilinear_tol(nside, md, np.concatenate([np.float64(md[c])[npx] for c in range(2)], 1), dt == np.float32)
			err = np.max(np.abs(np.float64(host(got))-want))
			print("nside %d %s: ring-bilinear error %.3g (tol %.3g)" % (nside, np.dtype(dt).name, err, tol))
			worst = max(worst, err/tol)
			assert err <= tol
		# order 0 is the containing pixel; one map, shaped directions
		near = host(healpix.get_interp_val(dev(m[0]), dev(th[:6].reshape(2, 3)), dev(ph[:6].reshape(2, 3)), order=0))
		assert near.shape == (2, 3) and np.array_equal(near, m[0][host(healpix.ang2pix(nside, dev(th[:6]), dev(ph[:6])))].reshape(2, 3))
	print("ring-bilinear: worst error / tol = %.3f" % worst)
	with pytest.raises(ValueError): healpix.get_interp_val(dev(m), dev(th), dev(ph), order=3)

# ---- the spline coefficients' definition and the CAR tolerance (as in test_thumbnails.py; border "constant": mirror on both axes) ---------
def ext_index(i, n):
	if n == 1: return 0
	P = 2*(n-1); m = i % P
	return m if m < n else P-m
def collocation(n):
	B = np.zeros((n, n))
	for k in range(n):
		for d, w in ((-1, 1/6), (0, 4/6), (1, 1/6)): B[k, ext_index(k+d, n)] += w
	return B
_dense = {}
def dense_coefficients(f, key):
	if key in _dense: return _dense[key]
	f = np.asarray(f, np.float64)
	c = np.linalg.solve(collocation(f.shape[-2]), np.moveaxis(f, -2, 0).reshape(f.shape[-2], -1)).reshape((f.shape[-2],)+f.shape[:-2]+f.shape[-1:])
	c = np.moveaxis(c, 0, -2)
	c = np.linalg.solve(collocation(f.shape[-1]), np.moveaxis(c, -1, 0).reshape(f.shape[-1], -1)).reshape((f.shape[-1],)+f.shape[:-1])
	_dense[key] = np.ascontiguousarray(np.moveaxis(c, 0, -1))
	return _dense[key]

def tol_of(eref, kpos, f, c, f32_out=False):
	f, c = np.asarray(f, np.float64), np.asarray(c, np.float64)
	dc = max([float(np.max(np.abs(np.diff(c, axis=a)))) for a in (-2, -1) if c.shape[a] > 1]+[0.0])
	t = 4*eref*np.max(np.abs(f))+64*EPS*np.max(np.abs(c))+max(8.0, 4*kpos)*EPS*max(c.shape[-2:])*dc
	return t+(2.0**-24*np.max(np.abs(f)) if f32_out else 0.0)

class Worst:
	"""the largest error / tol of a body's cases; tol may be an array (a bound per output pixel)"""
	def __init__(self, name): self.name, self.ratio, self.where = name, 0.0, ""
	def check(self, tag, got, want, tol):
		got, want = np.float64(host(got)), np.float64(want)
		assert got.shape == want.shape, (tag, got.shape, want.shape)
		ratio = float(np.max(np.abs(got-want)/tol)) if got.size else 0.0
		print("%s: worst error %.3g, error / tol %.3g" % (tag, float(np.max(np.abs(got-want))) if got.size else 0.0, ratio))
		if ratio > self.ratio: self.ratio, self.where = ratio, tag
		assert ratio <= 1, tag
	def report(self): print("%s: worst error / tol = %.3f (%s)" % (self.name, self.ratio, self.where))

# ---- the closed form, in numpy -----------------------------------------------------------------------------------------------------------
def Rz(t): return np.array([[np.cos(t), -np.sin(t), 0], [np.sin(t), np.cos(t), 0], [0, 0, 1]])
def Ry(t): return np.array([[np.cos(t), 0, np.sin(t)], [0, 1, 0], [-np.sin(t), 0, np.cos(t)]])
def closed_form(rot, dec, ra):
	"""(dec', ra', psi): where the direction (dec, ra) of an output pixel is read, M n, and the angle of M e_ra(n) in the (east, north) frame
	there; M = Rz(a) Ry(b) Rz(c) for [a, b, c] = inv_euler(rot2euler(rot))[::-1]"""
	if rot is None: return dec, ra, 0*dec
	a, b, c = reproject.inv_euler(reproject.rot2euler(rot))[::-1]
	M = Rz(a) @ Ry(b) @ Rz(c)
	n = np.array([np.cos(dec)*np.cos(ra), np.cos(dec)*np.sin(ra), np.sin(dec)]); e = np.array([-np.sin(ra), np.cos(ra), 0*ra])
	V, E = np.einsum("ij,j...->i...", M, n), np.einsum("ij,j...->i...", M, e)
	ce = V[0]*E[1]-V[1]*E[0]; cn = (V[0]**2+V[1]**2)*E[2]-V[2]*(V[0]*E[0]+V[1]*E[1])
	return np.arctan2(V[2], np.hypot(V[0], V[1])), np.arctan2(V[1], V[0]), np.arctan2(cn, ce)

# ---- 3. method="spline" against the fixture ----------------------------------------------------------------------------------------------
M2H_CASES = [("S", 8, r, o) for r in ROTS for o in (0, 1, 3)]+[("S", 3, r, o) for r in ("none", "euler") for o in (0, 1, 3)]+[("B", 4, "euler", 1)]

def map2healpix_body(fx, dev, on_device):
	eref, kpos = float(fx["E_ref"]), float(fx["K_pos"]); W = Worst("CAR -> healpix")
	for g, nside, rname, order in M2H_CASES:
		shape, wcs = geometry(fx[g+"_geo"])
		want = fx["m2h_%s%d_%s_%d" % (g, nside, rname, order)]
		dang = np.float64(fx["dang_m2h_%s%d_%s" % (g, nside, rname)])
		for dt in (np.float64, np.float32):
			f = fx[g+"_map"].astype(dt)
			fmax = float(np.max(np.abs(f)))
			got = reproject.map2healpix(as_map(dev, f, wcs), nside=nside, rot=ROTS[rname], method="spline", order=order)
			assert hasattr(got, "data_ptr") == on_device and host(got).dtype == dt and got.shape == (3, 12*nside**2)
			got = host(got)
			name = "%s nside %d %s order %d %s" % (g, nside, rname, order, np.dtype(dt).name)
			f32 = 2.0**-24*fmax if dt == np.float32 else 0.0
			if order == 0:
				keep = ~fx["tie_m2h_%s%d" % (g, nside)] if rname == "none" else np.ones(want.shape[-1], bool)
				assert np.array_equal(got[0][keep], want[0][keep]), name      # exact: T always, Q and U without rotation
				if rname == "none": assert np.array_equal(got[:, keep], want[:, keep]), name
				else: W.check(name+" Q U", got[1:], want[1:], 2*dang*fmax+64*EPS*fmax+f32)
				continue
			base = tol_of(eref, kpos, f, dense_coefficients(f, g) if order == 3 else f, f32_out=dt == np.float32)
			W.check(name+" T", got[0], want[0], base)
			W.check(name+" Q U", got[1:], want[1:], base+2*dang*fmax)
	# spin=[0]: nothing is a pair; [ny, nx]: the T row; [2, 3, ny, nx]: each leading entry rotates its own pair
	shape, wcs = geometry(fx["B_geo"]); f = fx["B_map"]
	base = tol_of(eref, kpos, f, f)
	W.check("B spin [0]", reproject.map2healpix(as_map(dev, f, wcs), nside=4, rot=ROTS["euler"], method="spline", order=1, spin=[0]), fx["m2h_B4_euler_1_spin0"], base)
	shape, wcs = geometry(fx["S_geo"]); f = fx["S_map"]; fmax = float(np.max(np.abs(f)))
	base = tol_of(eref, kpos, f, f); dang = np.float64(fx["dang_m2h_S8_euler"])
	r3 = host(reproject.map2healpix(as_map(dev, f, wcs), nside=8, rot=ROTS["euler"], method="spline", order=1))
	r2 = reproject.map2healpix(as_map(dev, f[0], wcs), nside=8, rot=ROTS["euler"], method="spline", order=1)
	assert r2.shape == (768,) and np.array_equal(host(r2), r3[0])
	r23 = host(reproject.map2healpix(as_map(dev, np.array([f, 2*f]), wcs), nside=8, rot=ROTS["euler"], method="spline", order=1))
	assert r23.shape == (2, 3, 768) and np.array_equal(r23[0], r3)
	for k in (0, 1): W.check("S [2, 3] entry %d" % k, r23[k], fx["m2h_S8_23"][k], (k+1)*(base+2*dang*fmax))
	W.report()

def h2m_cases(fx):
	for key in sorted(fx):
		if key.startswith("h2m_") and "QU" not in key:
			p = key.split("_")
			yield key, ("B" if p[1][0] == "B" else "S"), int(p[1].lstrip("B")), p[2], int(p[3])

def healpix2map_body(fx, dev, on_device):
	kpos = float(fx["K_pos"]); W = Worst("healpix -> CAR")
	mapkind = enmap.dmap if on_device else enmap.ndmap
	for key, g, nside, rname, order in h2m_cases(fx):
		shape, wcs = geometry(fx[g+"_geo"])
		want = fx[key]
		pos = np.asarray(enmap.posmap(shape, wcs))
		dec, ra, psi = closed_form(ROTS[rname], pos[0], pos[1])
		dang = np.float64(fx["dang_h2m_%s_%s" % (g, rname)]) if rname != "none" else 0*dec
		for dt in (np.float64, np.float32):
			h = fx["heal%d" % nside].astype(dt)
			if want.ndim == 2: h = h[0]
			hmax = float(np.max(np.abs(h)))
			res = reproject.healpix2map(dev(h), shape, wcs, rot=ROTS[rname], method="spline", order=order)
			assert isinstance(res, mapkind) and res.dtype == dt and res.shape == h.shape[:-1]+shape and res.wcs is wcs
			got = host(res)
			name = "%s order %d %s" % (key, order, np.dtype(dt).name)
			f32 = 2.0**-24*hmax if dt == np.float32 else 0.0
			if order == 0:
				_, margin = np_ang2pix(nside, np.pi/2-dec, ra)
				keep = margin > 1e-9
				print("%s: excluded share %.3g" % (name, 1-np.mean(keep)))
				assert 1-np.mean(keep) <= (0.0 if rname == "none" else 1e-3) and np.array_equal(got[keep], want[keep]), name
				if key == "h2m_8_euler_0":
					full = host(reproject.healpix2map(dev(fx["heal8"].astype(dt)), shape, wcs, rot=ROTS[rname], method="spline", order=0))
					assert np.array_equal(full[0], got)
					W.check(name+" Q U", full[1:][:, keep], fx["h2m_8_euler_0_QU"][:, keep], (2*dang*hmax+64*EPS*hmax+f32)[keep])
				continue
			npx, _ = np_weights(nside, np.pi/2-dec, ra)
			taps = np.float64(h)[..., npx].reshape(-1, 4, dec.size).transpose(1, 0, 2).reshape(4, -1)
			base = bilinear_tol(nside, h, taps, dt == np.float32, k=max(8.0, 4*kpos))
			if want.ndim == 2: W.check(name, got, want, base)
			else:
				W.check(name+" T", got[0], want[0], base)
				W.check(name+" Q U", got[1:], want[1:], base+2*dang*hmax)
	W.report()

def extensive_body(fx, dev, on_device):
	eref, kpos = float(fx["E_ref"]), float(fx["K_pos"])
	shape, wcs = geometry(fx["S_geo"])
	one = np.ones(shape)
	ps = np.asarray(enmap.pixsizemap(shape, wcs))
	for order in (0, 1):
		ref = fx["ext_m2h_%d" % order]
		got = host(reproject.map2healpix(as_map(dev, one, wcs), nside=8, method="spline", order=order, spin=[0], extensive=True))
		tol = tol_of(eref, kpos, one, one)*(4*np.pi/768)/ps.min()
		print("extensive CAR -> healpix order %d: sums to %.9f (the reference's %.9f, of %d), worst difference %.3g (tol %.3g)" % (order, got.sum(), ref.sum(), one.size, np.max(np.abs(got-ref)), tol))
		assert np.max(np.abs(got-ref)) <= tol and abs(got.sum()-one.size) <= abs(ref.sum()-one.size)+768*tol
		ref = fx["ext_h2m_%d" % order]
		res = reproject.healpix2map(dev(np.ones(768)), shape, wcs, method="spline", order=order, spin=[0], extensive=True)
		got = host(res)
		tol = 64*EPS*ps.max()/(4*np.pi/768)
		print("extensive healpix -> CAR order %d: sums to %.9f (the reference's %.9f, of 768), worst difference %.3g (tol %.3g)" % (order, got.sum(), ref.sum()*shape[1], np.max(np.abs(got-ref[:, None])), tol))
		assert np.max(np.abs(got-ref[:, None])) <= tol and abs(got.sum()-768) <= abs(ref.sum()*shape[1]-768)+one.size*tol
		plain = host(reproject.healpix2map(dev(np.ones(768)), shape, wcs, method="spline", order=order, spin=[0]))
		assert np.max(np.abs(plain-1)) <= 4*EPS and not np.allclose(got, plain)

def fused_body(fx, dev, on_device):
	"""map2healpix(spline) against enmap.at at the closed form's positions followed by enmap.rotate_pol by minus its angle"""
	kpos = float(fx["K_pos"]); W = Worst("fused against unfused")
	shape, wcs = geometry(fx["S_geo"])
	nside = 8
	tt, tp = table_centres(nside)
	for rname in ("none", "euler", "equgal"):
		dec, ra, psi = closed_form(ROTS[rname], np.pi/2-tt, tp)
		for dt in (np.float64, np.float32):
			f = fx["S_map"].astype(dt)
			m = as_map(dev, f, wcs)
			for order in (1, 3):
				ip = interpol.interpolator(m, npre=1, order=order, border="constant", cval=0.0)
				tol = tol_of(0.0, kpos, f, host(ip.arr), f32_out=dt == np.float32)+(3*2.0**-24*np.max(np.abs(f)) if dt == np.float32 else 0.0)      # (the unfused path rounds to float32 twice)
				v = enmap.at(m, dev(np.array([dec, ra])), ip=ip)
				if rname != "none": v = enmap.rotate_pol(v, dev(-psi), axis=-2)
				got = reproject.map2healpix(m, nside=nside, rot=ROTS[rname], method="spline", order=order)
				assert host(got).dtype == dt
				W.check("%s %s order %d" % (rname, np.dtype(dt).name, order), got, host(v), tol)
	W.report()

# ---- 4. method="harm" ----------------------------------------------------------------------------------------------------------------------
def harm_body(fx, dev, on_device):
	from oracle import sht_oracle as so
	lmax, nside = 12, 8
	alm = fx["harm_alm"]
	shape, wcs = geometry(fx["F_geo"])
	mi = curvedsky.analyse_geometry((3,)+shape, wcs)
	ms = so._tri_mstart(lmax, lmax)
	car_truth = np.zeros((3,)+shape)
	so.synthesis_2d(alm=alm[:1], map=car_truth[:1], spin=0, lmax=lmax, mstart=ms, geometry="F1", phi0=mi.phi0)
	so.synthesis_2d(alm=alm[1:], map=car_truth[1:], spin=2, lmax=lmax, mstart=ms, geometry="F1", phi0=mi.phi0)
	car_truth = np.ascontiguousarray(car_truth[:, ::-1, ::-1])
	ri = curvedsky.get_ring_info_healpix(nside)
	kw = dict(theta=ri.theta, nphi=ri.nphi, phi0=ri.phi0, ringstart=ri.offsets, lmax=lmax)
	truth = np.concatenate([so.synthesis(alm=alm[:1], spin=0, **kw), so.synthesis(alm=alm[1:], spin=2, **kw)])
	m = as_map(dev, car_truth, wcs)
	got = reproject.map2healpix(m, nside=nside, lmax=lmax)      # (method="harm" is the default)
	assert hasattr(got, "data_ptr") == on_device and got.shape == (3, 768)
	err = np.max(np.abs(host(got)-truth))/np.max(np.abs(truth))
	print("harm CAR -> healpix: %.3g of max|.|" % err)
	assert err <= 1e-10
	# with a rotation: the T field at R^-1 n, through one-pixel rings of the oracle (as test_rotate_alm.py evaluates it)
	tt, tp = table_centres(nside)
	n = np.array([np.sin(tt)*np.cos(tp), np.sin(tt)*np.sin(tp), np.cos(tt)])
	for rname in ("galequ", "euler"):
		psi, theta, phi = reproject.rot2euler(ROTS[rname])
		src = (Rz(phi) @ Ry(theta) @ Rz(psi)).T @ n
		th, ph = np.arccos(np.clip(src[2], -1, 1)), np.arctan2(src[1], src[0])
		want = so.synthesis(alm=alm[:1], spin=0, theta=th, nphi=np.ones(768, np.int64), phi0=ph, ringstart=np.arange(768, dtype=np.int64), lmax=lmax)[0]
		got = host(reproject.map2healpix(m, nside=nside, lmax=lmax, rot=ROTS[rname], method="harm"))
		err = np.max(np.abs(got[0]-want))/np.max(np.abs(want))
		print("harm CAR -> healpix %s, T: %.3g of max|.|" % (rname, err))
		assert err <= 1e-10
	# healpix -> CAR against the fixture
	heal = fx["harm_heal4"]
	for rname in ("none", "galequ"):
		for niter in (0, 2):
			want = fx["harm_h2m_%s_%d" % (rname, niter)]
			res = reproject.healpix2map(dev(heal), shape, wcs, lmax=lmax, rot=ROTS[rname], method="harm", niter=niter)
			assert isinstance(res, enmap.dmap if on_device else enmap.ndmap) and res.shape == (3,)+shape
			err = np.max(np.abs(host(res)-want))/np.max(np.abs(want))
			print("harm healpix -> CAR %s niter %d: %.3g of max|.|" % (rname, niter, err))
			assert err <= 1e-10
	# the alm is made and rotated on the device, for host input too
	a = reproject._harm_map2alm(car_truth, wcs, lmax, [0, 2], 0)
	assert hasattr(a, "data_ptr") == on_device and reproject._harm(a, ROTS["euler"]) is a
	a = reproject._harm_heal2alm(heal, lmax, [0, 2], 0)
	assert hasattr(a, "data_ptr") == on_device
	if on_device: assert isinstance(reproject.map2healpix(enmap.ndmap(car_truth, wcs), nside=nside, lmax=lmax), np.ndarray)

# ---- 5. interface --------------------------------------------------------------------------------------------------------------------------
def interface_body(fx, dev, on_device):
	shape, wcs = geometry(fx["S_geo"]); f = fx["S_map"]
	m = as_map(dev, f, wcs)
	kw = dict(method="spline", order=0)
	assert reproject.map2healpix(m, **kw).shape == (3, 12*16**2)      # 5 degrees: nside 11.7 -> 16
	assert reproject.map2healpix(m, nside_mode="mul32", **kw).shape == (3, 12*32**2) and reproject.map2healpix(m, nside_mode="any", **kw).shape == (3, 12*12**2)
	assert [reproject.restrict_nside(13.2, mode) for mode in ("pow2", "mul32", "any")] == [16, 32, 14] and reproject.restrict_nside(5.0, "mul32") == 5
	assert reproject.restrict_nside(13.2, "pow2", round="floor") == 8 and reproject.restrict_nside(0.2, "any", round="floor") == 1
	with pytest.raises(ValueError): reproject.restrict_nside(4, "odd")
	assert np.max(np.abs(reproject.rot2euler("gal,equ")-curvedsky.euler_angs[("gal", "equ")])) <= 1e-12
	assert reproject.inv_euler([1, 2, 3]) == [-3, -2, -1] and np.array_equal(reproject.rot2euler((0.3, 1.1, -0.7)), [0.3, 1.1, -0.7])
	with pytest.raises(ValueError): reproject.rot2euler("gal")
	with pytest.raises(ValueError): reproject.rot2euler("gal,hor")
	# out= is filled in place and returned
	want = host(reproject.map2healpix(m, nside=8, rot="equ,gal", method="spline", order=1))
	out = dev(np.zeros((3, 768)))
	assert reproject.map2healpix(m, out=out, rot="equ,gal", method="spline", order=1) is out and np.array_equal(host(out), want)
	heal = fx["heal8"]
	wantm = host(reproject.healpix2map(dev(heal), shape, wcs, rot="equ,gal", method="spline", order=1))
	omap = as_map(dev, np.zeros((3,)+shape), wcs)
	assert reproject.healpix2map(dev(heal), out=omap, rot="equ,gal", method="spline", order=1) is omap and np.array_equal(host(omap), wantm)
	# a transposed view equals the contiguous array
	ft = dev(np.ascontiguousarray(f.swapaxes(-1, -2))).swapaxes(-1, -2)
	ht = dev(np.ascontiguousarray(heal.T)).swapaxes(0, 1)
	if on_device: assert not ft.is_contiguous() and not ht.is_contiguous()
	mt = enmap.dmap(ft, wcs) if on_device else enmap.ndmap(ft, wcs)
	assert np.array_equal(host(reproject.map2healpix(mt, nside=8, rot="equ,gal", method="spline", order=1)), want)
	assert np.array_equal(host(reproject.healpix2map(ht, shape, wcs, rot="equ,gal", method="spline", order=1)), wantm)
	# bsize and verbose have no effect
	assert np.array_equal(host(reproject.map2healpix(m, nside=8, rot="equ,gal", method="spline", order=1, bsize=7, verbose=True)), want)
	# what raises
	with pytest.raises(ValueError, match="Only order 0 and order 1"): reproject.healpix2map(dev(heal), shape, wcs, method="spline", order=3)
	with pytest.raises(ValueError, match="not recognized"): reproject.map2healpix(m, nside=8, method="cubic")
	with pytest.raises(ValueError, match="not recognized"): reproject.healpix2map(dev(heal), shape, wcs, method="cubic")
	tilted = CarWCS(cdelt=wcs.wcs.cdelt, crval=[wcs.wcs.crval[0], 10.0], crpix=wcs.wcs.crpix)
	with pytest.raises(NotImplementedError): reproject.map2healpix(as_map(dev, f, tilted), nside=8, method="spline")
	with pytest.raises(NotImplementedError): reproject.healpix2map(dev(heal), shape, tilted, method="spline")
	if on_device: elsewhere = np.zeros((3, 768))
	else:
		import torch
		elsewhere = torch.zeros((3, 768), dtype=torch.float64)
	with pytest.raises(ValueError, match="different devices"): reproject.map2healpix(m, out=elsewhere, method="spline")
	with pytest.raises(ValueError): reproject.map2healpix(m, out=dev(np.zeros((2, 768))), method="spline")
	with pytest.raises(ValueError): reproject.healpix2map(dev(heal), method="spline")


@pytest.mark.hostsim
def test_index_sim(): index_body(ident, False)
@pytest.mark.hostsim
def test_big_nside_sim(): big_nside_body(ident, False)
@pytest.mark.hostsim
def test_weights_sim(): weights_body(ident, False)
@pytest.mark.hostsim
def test_map2healpix_spline_sim(fx): map2healpix_body(fx, ident, False)
@pytest.mark.hostsim
def test_healpix2map_spline_sim(fx): healpix2map_body(fx, ident, False)
@pytest.mark.hostsim
def test_extensive_sim(fx): extensive_body(fx, ident, False)
@pytest.mark.hostsim
def test_fused_against_unfused_sim(fx): fused_body(fx, ident, False)
@pytest.mark.hostsim
def test_harm_sim(fx): harm_body(fx, ident, False)
@pytest.mark.hostsim
def test_interface_sim(fx): interface_body(fx, ident, False)

@pytest.mark.gpu
def test_index_gpu(): index_body(cuda, True)
@pytest.mark.gpu
def test_big_nside_gpu(): big_nside_body(cuda, True)
@pytest.mark.gpu
def test_weights_gpu(): weights_body(cuda, True)
@pytest.mark.gpu
def test_map2healpix_spline_gpu(fx): map2healpix_body(fx, cuda, True)
@pytest.mark.gpu
def test_healpix2map_spline_gpu(fx): healpix2map_body(fx, cuda, True)
@pytest.mark.gpu
def test_extensive_gpu(fx): extensive_body(fx, cuda, True)
@pytest.mark.gpu
def test_fused_against_unfused_gpu(fx): fused_body(fx, cuda, True)
@pytest.mark.gpu
def test_harm_gpu(fx): harm_body(fx, cuda, True)
@pytest.mark.gpu
def test_interface_gpu(fx): interface_body(fx, cuda, True)
