"""Generate tests/golden/reproject.npz: inputs and what the REFERENCE's own reproject.map2healpix / healpix2map give
(pixell/reproject.py:118-361), for tests/test_reproject_healpix.py.

Run:  python tests/golden/make_reproject.py      (needs the reference checkout _ref_harness.py points at, cython, gcc and scipy; never run on the GPU box)

The reference is imported through _ref_harness.py with the long-double oracle as ducc0.sht.experimental, ducc0.sht.rotate_alm from
make_aberration.py (oracle synthesis at the turned positions, oracle analysis) and two empty astropy.coordinates / astropy.units stubs.
Its spline route imports healpy, which is not installed: the module `healpy` below is a STAND-IN WRITTEN HERE, in plain numpy, from the
published RING pixelisation (Gorski et al. 2005) and the ring-bilinear rule of HEALPix's get_interpol as csrc/healpix.hip's docstring
states them: pix2ang from the reference's own get_ring_info_healpix tables, ang2pix and get_interp_val from the formulas.  It is this
maker's code, not the reference's and not healpy's; parity with healpy is not pinned.  Only arrays are saved.

Geometries: S the full-sky CAR grid (36, 72) at 5 degrees with its columns shifted by 0.37 pixel; F the same unshifted; B a band of 14 x 30
pixels that does not go round the sky.  Maps: float64 multiples of 2^-20 (so that float32 holds the same numbers), T in [-1, 1), Q and U in
[-1/2, 1/2) (make_thumbnails.py says why).  Rotations: none, "gal,equ", "equ,gal", (0.3, 1.1, -0.7).
Keys (rot one of none, galequ, equgal, euler):
  m2h_<geo><nside>_<rot>_<order>      map2healpix(method="spline") of the map of <geo>: [3, npix] (order 0 without rotation: float32, exact)
  m2h_B4_euler_1_spin0                the same with spin=[0]; m2h_S8_23: of the map [2, 3, ny, nx] = (f, 2 f), rot euler, order 1
  h2m_<nside>_<rot>_<order>           healpix2map(method="spline") onto S: [3, ny, nx] (nside 8, euler), otherwise [ny, nx] of the T map alone to keep
                                      the file small (order 0: float32, exact); h2m_8_euler_0_QU: the rotated Q, U of order 0; h2m_B4_euler_1 onto B
  dang_m2h_<geo><nside>_<rot>, dang_h2m_<geo>_<rot>    per output pixel, |the reference's finite-difference angle - the closed form| (float32, rounded up)
  K_pos          the largest distance of the reference's pixel coordinates (CAR -> healpix) or ring coordinates phi 4 nside / 2 pi, theta 4 nside / pi
                 (healpix -> CAR) from the closed form in numpy, in units of 2^-52 max(ny, nx) or 2^-52 4 nside
  E_ref          the reference's filtered map against the dense solve, relative to max|f| (as in thumbnails.npz)
  ext_*          extensive=True on all-ones hit maps: the sums the reference's results have, and the results
  harm_h2m_<rot>_<niter>              healpix2map(method="harm", lmax 12) of a band-limited nside-4 map onto F: [3, 36, 72]
  tie_m2h_<geo><nside>    without rotation the healpix rings at dec = 0 and (nside 8) at +-30 degrees lie halfway between two rows of the grid:
                 their pixels are rounding ties of order 0 (asserted: whole belt rings at those dec, and none with a rotation), which the test leaves out at order 0
Asserted here: no CAR pixel coordinate lies within 1e-6 of 0 or n - 1 on an axis read with "constant"; no floor argument of the stand-in's ang2pix lies within 1e-6 of an integer on S or B.

The reference's healpix2map(spin=[0]) of a [3, npix] map with a rotation raises IndexError (it asks for an angle it did not compute): no such case.

As run for the committed fixture:
  CAR -> healpix S nside 8 none: dang up to 0 rad, K_pos 0.444
  CAR -> healpix S nside 8 galequ: dang up to 4.76e-06 rad, K_pos 0.889
  CAR -> healpix S nside 8 equgal: dang up to 5.06e-06 rad, K_pos 0.889
  CAR -> healpix S nside 8 euler: dang up to 4.22e-06 rad, K_pos 0.889
  CAR -> healpix S nside 3 none: dang up to 0 rad, K_pos 0.444
  CAR -> healpix S nside 3 euler: dang up to 8.99e-07 rad, K_pos 0.444
  CAR -> healpix B nside 4 euler: dang up to 2.34e-06 rad, K_pos 1.07
  healpix -> CAR S galequ: dang up to 9.32e-06 rad, K_pos 0.318
  healpix -> CAR S equgal: dang up to 8.34e-06 rad, K_pos 0.318
  healpix -> CAR S euler: dang up to 3.89e-06 rad, K_pos 0.318
  healpix -> CAR B euler: dang up to 1.26e-05 rad, K_pos 0.318
  the stand-in's ang2pix: smallest margin of a floor argument over every order-0 call 7.96e-06
  K_pos = 1.07, E_ref = 2.67e-15
  extensive CAR -> healpix order 0: 2592 pixels in, the result sums to 2445.835015      (border "constant": what lies beyond the first and last row and column is lost)
  extensive healpix -> CAR order 0: 768 pixels in, the result sums to 768.000000
  extensive CAR -> healpix order 1: 2592 pixels in, the result sums to 2542.992819
  extensive healpix -> CAR order 1: 768 pixels in, the result sums to 768.000000
  reproject.npz: 855797 bytes
"""
import sys, os, types
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..")); sys.path.insert(0, HERE)
from oracle import sht_oracle as so
import _ref_harness as H
from make_interpol import dense_coefficients, geo_numbers
from make_aberration import rotate_alm

degree = np.pi/180
NSIDES = (1, 2, 3, 4, 8)
ROTS = {"none": None, "galequ": "gal,equ", "equgal": "equ,gal", "euler": (0.3, 1.1, -0.7)}

# ---- the healpy stand-in (this maker's own code) -------------------------------------------------------------------------------------
def np_ring(nside, r):
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

def healpy_standin(cs):
	hp = types.ModuleType("healpy")
	def pix2ang(nside, ipix):
		ri = cs.get_ring_info_healpix(nside)
		theta = np.concatenate([np.full(int(n), t) for t, n in zip(ri.theta, ri.nphi)])
		phi = np.concatenate([p0+2*np.pi*np.arange(int(n))/float(n) for p0, n in zip(ri.phi0, ri.nphi)])
		return np.array([theta[ipix], phi[ipix]])
	def ang2pix(nside, theta, phi):
		pix, margin = np_ang2pix(nside, theta, phi)
		hp.margins.append(float(margin.min()))
		return pix
	def get_interp_val(m, theta, phi):
		pix, w = np_weights(cs.npix2nside(len(m)), theta, phi)
		return np.sum(w*np.asarray(m, np.float64)[pix], 0)
	hp.pix2ang, hp.ang2pix, hp.get_interp_val, hp.margins = pix2ang, ang2pix, get_interp_val, []
	return hp

# ---- the closed form, in numpy -------------------------------------------------------------------------------------------------------
def Rz(t): return np.array([[np.cos(t), -np.sin(t), 0], [np.sin(t), np.cos(t), 0], [0, 0, 1]])
def Ry(t): return np.array([[np.cos(t), 0, np.sin(t)], [0, 1, 0], [-np.sin(t), 0, np.cos(t)]])
def closed_form(euler, dec, ra):
	"""(dec', ra', psi) of M n and of M e_ra(n) at M n, M = Rz(a) Ry(b) Rz(c) for euler = [a, b, c] (None: no rotation)"""
	if euler is None: return dec, ra, 0*dec
	M = Rz(euler[0]) @ Ry(euler[1]) @ Rz(euler[2])
	n = np.array([np.cos(dec)*np.cos(ra), np.cos(dec)*np.sin(ra), np.sin(dec)]); e = np.array([-np.sin(ra), np.cos(ra), 0*ra])
	V, E = np.einsum("ij,j...->i...", M, n), np.einsum("ij,j...->i...", M, e)
	ce = V[0]*E[1]-V[1]*E[0]; cn = (V[0]**2+V[1]**2)*E[2]-V[2]*(V[0]*E[0]+V[1]*E[1])
	return np.arctan2(V[2], np.hypot(V[0], V[1])), np.arctan2(V[1], V[0]), np.arctan2(cn, ce)

def up32(a):
	a = np.asarray(a, np.float64); f = a.astype(np.float32)
	return np.where(f.astype(np.float64) < a, np.nextafter(f, np.float32(np.inf)), f).astype(np.float32)

def main(write=True):
	sht = types.ModuleType("sht_exp")
	for name in ["synthesis_2d", "adjoint_synthesis_2d", "analysis_2d", "adjoint_analysis_2d", "synthesis", "adjoint_synthesis", "get_gridweights"]: setattr(sht, name, getattr(so, name))
	ns = H.load_reference(sht)
	for name in ("coordinates", "units"):
		m = types.ModuleType("astropy."+name); sys.modules["astropy."+name] = m; setattr(sys.modules["astropy"], name, m)
	import ducc0
	ducc0.sht.rotate_alm = rotate_alm
	hp = healpy_standin(ns.curvedsky); sys.modules["healpy"] = hp
	from pixell import coordinates, reproject
	enmap, utils, cs = ns.enmap, ns.utils, ns.curvedsky
	out, rep = {}, []
	def say(s): rep.append(s); print(s)
	rng = np.random.default_rng(20261021)

	shapeF, wcsF = enmap.fullsky_geometry(res=5*degree); shapeF = tuple(int(v) for v in shapeF[-2:])
	assert shapeF == (36, 72)
	wcsS = wcsF.deepcopy(); wcsS.wcs.crpix[0] += 0.37
	wcsB = wcsF.deepcopy(); wcsB.wcs.crpix = np.array([15.3, 4.5]); shapeB = (14, 30)
	geos = {"S": (shapeF, wcsS), "F": (shapeF, wcsF), "B": (shapeB, wcsB)}
	def iqu(shape):
		f = rng.integers(-2**20, 2**20, (3,)+shape).astype(np.float64)/2**20
		f[1:] = rng.integers(-2**19, 2**19, (2,)+shape).astype(np.float64)/2**20
		return f
	maps = {"S": iqu(shapeF), "B": iqu(shapeB)}
	heal = {nside: iqu((12*nside**2,)) for nside in NSIDES}
	for g, (shape, wcs) in geos.items(): out[g+"_geo"] = geo_numbers(shape, wcs)
	for g in maps: out[g+"_map"] = maps[g]
	for nside in NSIDES: out["heal%d" % nside] = heal[nside]
	def euler_of(rot): return None if rot is None else np.array(reproject.inv_euler(reproject.rot2euler(rot))[::-1])
	kpos = 0.0

	# ---- CAR -> healpix ----
	def m2h_meta(g, nside, rname):
		"""dang per healpix pixel and K_pos of the case, with the tie and edge assertions"""
		shape, wcs = geos[g]
		pos = hp.pix2ang(nside, np.arange(12*nside**2))[::-1].copy(); pos[1] = np.pi/2-pos[1]
		eul = euler_of(ROTS[rname])
		dec, ra, psi = closed_form(eul, pos[1], pos[0])
		if eul is not None:
			full = coordinates.transform_euler(eul, pos, pol=True)
			rpos, ang = full[1::-1], full[2]
		else: rpos, ang = pos[1::-1], 0*psi
		pix = np.asarray(enmap.sky2pix(shape, wcs, rpos))
		cpix = np.array([(dec/degree-wcs.wcs.crval[1])/wcs.wcs.cdelt[1]+wcs.wcs.crpix[1]-1, (ra/degree-wcs.wcs.crval[0])/wcs.wcs.cdelt[0]+wcs.wcs.crpix[0]-1])
		d = (pix-cpix+36) % 72-36      # (whole turns of the sky: the rewind is the kernel's)
		k = float(np.max(np.abs(d)))/(2.0**-52*max(shape))
		own = pix.copy()
		# rounding ties: without rotation, whole healpix rings that lie halfway between two rows of the grid; nothing else
		tie = np.any(np.abs(own+0.5-np.round(own+0.5)) < 1e-6, 0)
		assert rname == "none" or not np.any(tie), "%s nside %d %s: %d coordinates on a rounding tie" % (g, nside, rname, np.sum(tie))
		if rname == "none":
			assert np.all(np.isin(np.round(pos[1][tie]/degree, 6), (-30.0, 0.0, 30.0))) and np.sum(tie) % (4*nside) == 0
			out["tie_m2h_%s%d" % (g, nside)] = tie
		edge = min(np.abs(own[a]-v).min() for a in (0, 1) for v in (0, shape[a]-1))
		assert edge > 1e-6, "%s nside %d %s: a coordinate %.3g pixel from the edge of the constant border" % (g, nside, rname, edge)
		return np.abs((ang-psi+np.pi) % (2*np.pi)-np.pi), k
	for g, nside, rnames, orders in (("S", 8, tuple(ROTS), (0, 1, 3)), ("S", 3, ("none", "euler"), (0, 1, 3)), ("B", 4, ("euler",), (1,))):
		shape, wcs = geos[g]
		imap = enmap.ndmap(maps[g], wcs)
		for rname in rnames:
			dang, k = m2h_meta(g, nside, rname); kpos = max(kpos, k)
			out["dang_m2h_%s%d_%s" % (g, nside, rname)] = up32(dang)
			say("  CAR -> healpix %s nside %d %s: dang up to %.3g rad, K_pos %.3g" % (g, nside, rname, dang.max(), k))
			for order in orders:
				res = np.asarray(reproject.map2healpix(imap, nside=nside, rot=ROTS[rname], method="spline", order=order))
				assert res.shape == (3, 12*nside**2)
				if order == 0 and rname == "none":
					assert np.array_equal(res.astype(np.float32), res); res = res.astype(np.float32)
				out["m2h_%s%d_%s_%d" % (g, nside, rname, order)] = res
	out["m2h_B4_euler_1_spin0"] = np.asarray(reproject.map2healpix(enmap.ndmap(maps["B"], wcsB), nside=4, rot=ROTS["euler"], method="spline", order=1, spin=[0]))
	res = np.asarray(reproject.map2healpix(enmap.ndmap(np.array([maps["S"], 2*maps["S"]]), wcsS), nside=8, rot=ROTS["euler"], method="spline", order=1))
	assert res.shape == (2, 3, 768)
	out["m2h_S8_23"] = res
	c_ref = np.asarray(utils.interpolator(maps["S"], npre=1, order=3, border="constant").arr)
	eref = float(np.max(np.abs(c_ref-dense_coefficients(maps["S"], "constant")))/np.max(np.abs(maps["S"])))
	out["E_ref"] = eref

	# ---- healpix -> CAR ----
	def h2m_meta(g, rname):
		shape, wcs = geos[g]
		pos = np.asarray(enmap.posmap(shape, wcs)).reshape(2, -1)[::-1]
		eul = euler_of(ROTS[rname])
		dec, ra, psi = closed_form(eul, pos[1], pos[0])
		full = coordinates.transform_euler(eul, pos, pol=True)
		d = np.array([(full[1]-dec)/np.pi, ((full[0]-ra+np.pi) % (2*np.pi)-np.pi)/(2*np.pi)])
		return np.abs((full[2]-psi+np.pi) % (2*np.pi)-np.pi).reshape(shape), float(np.max(np.abs(d)))/2.0**-52
	for g in ("S", "B"):
		for rname in (("galequ", "equgal", "euler") if g == "S" else ("euler",)):
			dang, k = h2m_meta(g, rname); kpos = max(kpos, k)
			out["dang_h2m_%s_%s" % (g, rname)] = up32(dang)
			say("  healpix -> CAR %s %s: dang up to %.3g rad, K_pos %.3g" % (g, rname, dang.max(), k))
	def h2m(nside, rname, order, g="S", tonly=False, **kw):
		shape, wcs = geos[g]
		h = heal[nside][0] if tonly else heal[nside]
		return np.asarray(reproject.healpix2map(h, shape, wcs, rot=ROTS[rname], method="spline", order=order, **kw))
	for rname in ROTS:
		full = rname == "euler"
		out["h2m_8_%s_1" % rname] = h2m(8, rname, 1, tonly=not full)
	for nside in (1, 2, 3, 4):
		for rname in (("none", "euler") if nside == 3 else ("euler",)): out["h2m_%d_%s_1" % (nside, rname)] = h2m(nside, rname, 1, tonly=True)
	for nside in NSIDES:
		for rname in (("none", "euler") if nside in (3, 8) else ("euler",)):
			res = h2m(nside, rname, 0, tonly=True)
			assert np.array_equal(res.astype(np.float32), res)
			out["h2m_%d_%s_0" % (nside, rname)] = res.astype(np.float32)
	out["h2m_8_euler_0_QU"] = h2m(8, "euler", 0)[1:]
	out["h2m_B4_euler_1"] = h2m(4, "euler", 1, g="B")
	# (healpix2map(spin=[0]) of a [3, npix] map with a rotation raises IndexError in the reference: it asks for an angle it did not compute)
	say("  the stand-in's ang2pix: smallest margin of a floor argument over every order-0 call %.3g" % min(hp.margins))
	assert min(hp.margins) > 1e-6
	out["K_pos"] = kpos
	say("  K_pos = %.3g, E_ref = %.3g" % (kpos, eref))

	# ---- extensive ----
	ones = enmap.ndmap(np.ones(shapeF), wcsS)
	for order in (0, 1):
		res = np.asarray(reproject.map2healpix(ones, nside=8, method="spline", order=order, spin=[0], extensive=True))
		out["ext_m2h_%d" % order] = res
		say("  extensive CAR -> healpix order %d: %d pixels in, the result sums to %.6f" % (order, ones.size, res.sum()))
		res = np.asarray(reproject.healpix2map(np.ones(768), shapeF, wcsS, method="spline", order=order, spin=[0], extensive=True))
		out["ext_h2m_%d" % order] = res.mean(1)      # (a row's pixels are equal up to the rounding of the weights' sum)
		assert np.max(np.abs(res-res[:, :1])) < 1e-14
		say("  extensive healpix -> CAR order %d: 768 pixels in, the result sums to %.6f" % (order, res.sum()))

	# ---- harm ----
	lmax = 12
	alm = so.rand_alm_simple(lmax, 3, 5, spin=(0, 2))
	out["harm_alm"] = alm
	hmap = np.asarray(cs.alm2map_healpix(alm.copy(), nside=4, spin=[0, 2]))
	out["harm_heal4"] = hmap
	for rname in ("none", "galequ"):
		for niter in (0, 2):
			out["harm_h2m_%s_%d" % (rname, niter)] = np.asarray(reproject.healpix2map(hmap, shapeF, wcsF, lmax=lmax, rot=ROTS[rname], method="harm", niter=niter))
	if write:
		f = os.path.join(HERE, "reproject.npz")
		np.savez_compressed(f, **out)
		say("  reproject.npz: %d bytes" % os.path.getsize(f))
	return rep

if __name__ == "__main__":
	main()
