"""Generate tests/golden/thumbnails.npz: inputs and what the REFERENCE gives for the whole-map definition of reproject.thumbnails that
pixell_amd.reproject implements:
    ipos, ang = coordinates.transform("cel", ["cel", [[0, 0, ra, dec], False]], posmap(oshape, owcs)[::-1], pol=True)
    utils.interpol(map, map.sky2pix(ipos), order, border="constant", cval=0), then enmap.rotate_pol(., -ang)

Run:  python tests/golden/make_thumbnails.py      (needs the reference checkout _ref_harness.py points at, cython, gcc and scipy; never run on the GPU box)

The reference is imported through _ref_harness.py; pixell.coordinates also wants astropy.coordinates and astropy.units at import, for which
two empty stub modules are registered: the recentring path is pure numpy.  TAN thumbnails cannot be driven through the reference without
astropy: the tests pin them against the unfused device path instead.  Only arrays are saved.

Maps ([3] components; float64 values that are multiples of 2^-20, so that the float32 map is the same numbers; T uniform in [-1, 1), Q and U
uniform in [-1/2, 1/2).  The tests allow the rotated Q, U an extra 2 dang max|f| for the reference's angle error dang: an angle that is off
by d moves the pair by 2 d |P|, P = hypot(Q, U), so that term presumes |P| <= max|f| wherever the map is read.  Two components of the full
range would reach sqrt(2) max|f| before a cubic spline overshoots its samples (1.47 max|f| was seen); with half the range |P| stays below
sqrt(2)/2 times the overshoot, under max|f| = max|T|, as on a sky, where the polarisation is a fraction of the temperature):
  G   full sky 90 x 180 at 2 deg (enmap.fullsky_geometry).  Thumbnails: thumbnail_geometry(r=6 deg, res=1 deg, proj="car"), 13 x 13
  A   45 x 100 pixels of 30' at dec 50 deg, the patch of make_interpol.py: neither axis a multiple of 16, no wrap.  Thumbnails: a 9 x 13
      geometry of 15' pixels given as oshape / owcs
Objects {dec,ra} in degrees:
  G   (5.3, 30.4), (-35.7, -100.6) interior; (82.1, 60.3) near the pole; (20.2, 179.7), (-10.4, -179.1) across the RA seam (RA = -179.0 is a rounding tie of this grid: column 179.5)
  A   (50.1, 20.3), (45.3, 10.2) interior; (59.4, 43.1): its thumbnail hangs over the patch's edge, so that cval (0) appears
Expected values, orders 0, 1, 3 (keys <map>_<order> without and <map>_<order>_pol with the rotation, [nobj, 3, oy, ox]): the definition above
on the float64 map.  For the two seam objects of G the map is first extended by the reference's own wrapped
extract_pixbox([[0, -48], [ny, nx + 48]]) (asserted: the extension equals the map on the overlap), since the reference has no border that
is periodic along one axis only; every other object reads the plain map.
  *_ang       the reference's finite-difference angle, [nobj, oy, ox]
  dang_*      per object, the largest |reference angle - closed form| (the closed form: the module docstring of csrc/thumbs.hip, in numpy)
  K_pos       the largest |reference pixel coordinate - closed form| over both maps, in units of 2^-52 max(ny, nx)
  E_ref       the largest |c_ref - c_dense| / max|f| over G, extended G and A, c_ref the reference's filtered array (border "constant"), c_dense
              the float64 dense solution of B c = f along each axis under the mirror extension
  thumbs_block  for the record only (float32): what the reference's own thumbnails(method="spline", oversample=1, r=6 deg, res=1 deg) gives
              on G: every object on its own apodised, median-filled cut-out.  No test asserts anything about it
  tg_*        enmap.thumbnail_geometry(proj="car") for (r, res), (res, shape) and (r, shape): [oy, ox, cdelt_x, cdelt_y, crpix_x, crpix_y]
  psize_*     enmap.pixsizemap of A, G and the 13 x 13 thumbnail geometry, one value per row
Asserted here: no coordinate used at order 0 lies within 1e-6 pixel of a rounding tie, and none on an axis read with "constant" within 1e-6
pixel of 0 or n - 1: the tests have no case to leave out.

As run for the committed fixture:
  dang G = 2.39e-08 1.96e-07 7.47e-06 9.66e-08 4.73e-08 rad (the reference's finite-difference angle against the closed form, per object)
  dang A = 3.06e-07 2.58e-07 4.36e-07 rad (the reference's finite-difference angle against the closed form, per object)
  K_pos = 5.12 (the reference's pixel coordinates against the closed form in numpy float64, in units of 2^-52 max(ny, nx))
  E_ref = 4.44e-15 (the reference's filtered maps against the dense solve, relative to max|f|: G, extended G, A)
  G object 0 read from the extended map: within 0 of the plain map's values (order 3)
  the reference's own thumbnails (apodised cut-outs) against the whole-map values, per object of G: overall 1.1 0.93 1.1 0.8 0.85, central 5 x 5 0.02 0.017 0.061 0.035 0.025
  thumbnails.npz: 388773 bytes
"""
import sys, os, types
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_harness as H
from make_interpol import dense_coefficients, geo_numbers, make_wcs

degree = np.pi/180
ORDERS = (0, 1, 3)
OBJ = {"G": np.array([[5.3, 30.4], [-35.7, -100.6], [82.1, 60.3], [20.2, 179.7], [-10.4, -179.1]])*degree,
	"A": np.array([[50.1, 20.3], [45.3, 10.2], [59.4, 43.1]])*degree}
SEAM = {"G": (3, 4), "A": ()}
PAD = 48

def closed_form(oshape, owcs, obj):
	"""(dec, ra, psi) [oy, ox] of the pixels of a CAR thumbnail geometry centred on (0, 0) once its centre is put on obj = (dec, ra)"""
	j, i = np.mgrid[:oshape[-2], :oshape[-1]]
	x = (i+1-owcs.wcs.crpix[0])*owcs.wcs.cdelt[0]*degree; y = (j+1-owcs.wcs.crpix[1])*owcs.wcs.cdelt[1]*degree
	v = [np.cos(y)*np.cos(x), np.cos(y)*np.sin(x), np.sin(y)]; e = [-np.sin(x), np.cos(x), 0*x]
	sd, cd, sr, cr = np.sin(obj[0]), np.cos(obj[0]), np.sin(obj[1]), np.cos(obj[1])
	def rot(a):
		x1 = cd*a[0]-sd*a[2]
		return cr*x1-sr*a[1], sr*x1+cr*a[1], sd*a[0]+cd*a[2]
	V, E = rot(v), rot(e)
	ce = V[0]*E[1]-V[1]*E[0]; cn = (V[0]**2+V[1]**2)*E[2]-V[2]*(V[0]*E[0]+V[1]*E[1])
	return np.arctan2(V[2], np.hypot(V[0], V[1])), np.arctan2(V[1], V[0]), np.arctan2(cn, ce)

def main(write=True):
	ns = H.load_reference(types.ModuleType("sht_exp"))
	for name in ("coordinates", "units"):
		m = types.ModuleType("astropy."+name); sys.modules["astropy."+name] = m; setattr(sys.modules["astropy"], name, m)
	from pixell import coordinates, reproject
	enmap, utils = ns.enmap, ns.utils
	out, rep = {}, []
	def say(s): rep.append(s); print(s)

	rng = np.random.default_rng(20261021)
	shapeG, wcsG = enmap.fullsky_geometry(res=2*degree); shapeG = tuple(int(v) for v in shapeG[-2:])
	shapeA, wcsA = (45, 100), make_wcs([-0.5, 0.5], [20.0, 0.0], [50.3, -76.9])
	assert shapeG == (90, 180)
	geos = {"G": (shapeG, wcsG), "A": (shapeA, wcsA)}
	tshapeG, twcsG = enmap.thumbnail_geometry(r=6*degree, res=1*degree, proj="car")
	tshapeA, twcsA = enmap.thumbnail_geometry(res=0.25*degree, shape=(9, 13), proj="car")
	tgeos = {"G": (tuple(int(v) for v in tshapeG), twcsG), "A": (tuple(int(v) for v in tshapeA), twcsA)}
	assert tgeos["G"][0] == (13, 13) and tgeos["A"][0] == (9, 13)
	maps = {}
	for g, (shape, wcs) in geos.items():
		maps[g] = rng.integers(-2**20, 2**20, (3,)+shape).astype(np.float64)/2**20
		maps[g][1:] = rng.integers(-2**19, 2**19, (2,)+shape).astype(np.float64)/2**20      # Q, U: half of T's range (the docstring says why)
		assert np.array_equal(maps[g].astype(np.float32).astype(np.float64), maps[g])
		out[g+"_geo"], out[g+"_map"], out[g+"_obj"], out[g+"_tgeo"] = geo_numbers(shape, wcs), maps[g], OBJ[g], geo_numbers(*tgeos[g])

	# ---- the whole-map definition ----
	mG = enmap.ndmap(maps["G"], wcsG)
	ext = mG.extract_pixbox(np.array([[0, -PAD], [shapeG[0], shapeG[1]+PAD]]))
	assert ext.shape == (3, 90, 180+2*PAD) and np.array_equal(ext[..., PAD:-PAD], maps["G"]) and np.array_equal(ext[..., :PAD], maps["G"][..., -PAD:]) and np.array_equal(ext[..., -PAD:], maps["G"][..., :PAD])
	kpos, eref = 0.0, 0.0
	for g, (shape, wcs) in geos.items():
		oshape, owcs = tgeos[g]
		opos = enmap.posmap(oshape, owcs)
		plain = enmap.ndmap(maps[g], wcs)
		res = {(o, p): [] for o in ORDERS for p in (0, 1)}
		angs, dang = [], []
		for k, obj in enumerate(OBJ[g]):
			m = ext if k in SEAM[g] else plain
			full = coordinates.transform("cel", ["cel", [[0, 0, obj[1], obj[0]], False]], opos[::-1], pol=True)
			ipos, ang = full[1::-1], full[2]
			nopol = coordinates.transform("cel", ["cel", [[0, 0, obj[1], obj[0]], False]], opos[::-1], pol=False)
			assert nopol.shape[0] == 2 and np.array_equal(nopol, full[:2])
			pix = np.asarray(m.sky2pix(ipos))
			# the assertions, on the coordinates of the plain map
			own = pix-np.array([0, PAD])[:, None, None] if k in SEAM[g] else pix.copy()
			if g == "G": own[1] = own[1] % shape[1]
			tie = np.abs(own+0.5-np.round(own+0.5)).min()
			assert tie > 1e-6, "%s object %d: a coordinate %.3g pixel from a rounding tie" % (g, k, tie)
			for a in ((0,) if g == "G" else (0, 1)):
				edge = min(np.abs(own[a]-v).min() for v in (0, shape[a]-1))
				assert edge > 1e-6, "%s object %d: a coordinate %.3g pixel from the edge of the constant border" % (g, k, edge)
			# the closed form
			dec, ra, psi = closed_form(oshape, owcs, obj)
			cpix = np.array([(dec/degree-wcs.wcs.crval[1])/wcs.wcs.cdelt[1]+wcs.wcs.crpix[1]-1, (ra/degree-wcs.wcs.crval[0])/wcs.wcs.cdelt[0]+wcs.wcs.crpix[0]-1])
			d = own-cpix
			if g == "G": d[1] = (d[1]+90) % 180-90      # (whole turns of the sky: the rewind is the kernel's)
			else: d = (d+360) % 720-360
			kpos = max(kpos, float(np.max(np.abs(d)))/(2.0**-52*max(shape)))
			dang.append(float(np.max(np.abs((ang-psi+np.pi) % (2*np.pi)-np.pi))))
			angs.append(ang)
			for order in ORDERS:
				val = np.asarray(utils.interpol(m, pix, order=order, border="constant", cval=0.0))
				res[(order, 0)].append(val)
				res[(order, 1)].append(np.asarray(enmap.rotate_pol(enmap.ndmap(val, owcs), -ang)))
		for order in ORDERS:
			out["%s_%d" % (g, order)], out["%s_%d_pol" % (g, order)] = np.array(res[(order, 0)]), np.array(res[(order, 1)])
		out[g+"_ang"], out["dang_"+g] = np.array(angs), np.array(dang)
		say("  dang %s = %s rad (the reference's finite-difference angle against the closed form, per object)" % (g, " ".join("%.2e" % v for v in dang)))
		assert np.any(out[g+"_3"] == 0) == (g == "A")
		for arr in ((maps[g], np.asarray(ext)) if g == "G" else (maps[g],)):
			c_ref = np.asarray(utils.interpolator(arr, npre=1, order=3, border="constant").arr)
			eref = max(eref, float(np.max(np.abs(c_ref-dense_coefficients(arr, "constant")))/np.max(np.abs(arr))))
	out["K_pos"], out["E_ref"] = kpos, eref
	say("  K_pos = %.3g (the reference's pixel coordinates against the closed form in numpy float64, in units of 2^-52 max(ny, nx))" % kpos)
	say("  E_ref = %.3g (the reference's filtered maps against the dense solve, relative to max|f|: G, extended G, A)" % eref)
	# interior objects: the plain and the extended map agree
	k = 0; obj = OBJ["G"][k]
	full = coordinates.transform("cel", ["cel", [[0, 0, obj[1], obj[0]], False]], enmap.posmap(*tgeos["G"])[::-1], pol=False)
	say("  G object 0 read from the extended map: within %.3g of the plain map's values (order 3)" % np.max(np.abs(np.asarray(utils.interpol(ext, ext.sky2pix(full[1::-1]), order=3, border="constant"))-out["G_3"][0])))

	# ---- the reference's own thumbnails, for the record ----
	block = np.asarray(reproject.thumbnails(mG, OBJ["G"], r=6*degree, res=1*degree, proj="car", method="spline", oversample=1, order=3, pol=True))
	assert block.shape == out["G_3_pol"].shape
	out["thumbs_block"] = block.astype(np.float32)
	dist = np.abs(block-out["G_3_pol"])
	say("  the reference's own thumbnails (apodised cut-outs) against the whole-map values, per object of G: overall %s, central 5 x 5 %s" % (
		" ".join("%.2g" % v for v in dist.max((1, 2, 3))), " ".join("%.2g" % v for v in dist[..., 4:9, 4:9].max((1, 2, 3)))))

	# ---- thumbnail_geometry, pixsizemap ----
	def tg(**kw):
		shape, wcs = enmap.thumbnail_geometry(proj="car", **kw)
		return np.array([shape[-2], shape[-1], wcs.wcs.cdelt[0], wcs.wcs.cdelt[1], wcs.wcs.crpix[0], wcs.wcs.crpix[1]], float)
	out["tg_r_res"] = tg(r=6*degree, res=1*degree)
	out["tg_res_shape"] = tg(res=0.25*degree, shape=(8, 12))
	out["tg_r_shape"] = tg(r=np.array([2.0, 3.0])*degree, shape=(9, 14))
	out["tg_r_res2"] = tg(r=np.array([2.2, 3.4])*degree, res=np.array([0.5, -0.25])*degree)
	for g, (shape, wcs) in list(geos.items())+[("T", tgeos["G"])]:
		ps = np.asarray(enmap.pixsizemap(shape, wcs))
		assert ps.shape == tuple(shape[-2:]) and np.all(ps == ps[:, :1])
		out["psize_"+g] = ps[:, 0].copy()
	if write:
		f = os.path.join(HERE, "thumbnails.npz")
		np.savez_compressed(f, **out)
		say("  thumbnails.npz: %d bytes" % os.path.getsize(f))
	return rep

if __name__ == "__main__":
	main()
