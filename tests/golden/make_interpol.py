"""Generate tests/golden/interpol.npz: inputs and what the REFERENCE's utils.interpol, enmap.at and whole-map
utils.interpol(map, map.sky2pix(posmap(oshape, owcs))) give for them.

Run:  python tests/golden/make_interpol.py      (needs the reference checkout _ref_harness.py points at, cython, gcc and scipy; never run on the GPU box)

The reference is imported through _ref_harness.py (its utils and enmap on a linear-CAR stand-in for astropy's WCS).  Only arrays are saved.

Geometries and maps (a leading [2] axis; float64 values that are multiples of 2^-20, so that the float32 map is the same numbers and the file
compresses):
  A   45 x 100 pixels of 30' at dec 50 deg (rows 38.95 .. 60.95 deg), RA around 20 deg, neither axis a multiple of 16, no wrap.  The equator
      (where a separable geometry has its reference declination) is about 100 pixels from the patch, so the reference's own sky2pix, which
      forms (dec - crval)/cdelt before it adds crpix, rounds at the ulp of about a hundred pixels: the "few ulp of the coordinate's
      magnitude" that the third term of the tests' tolerance allows for.  (With 10' pixels that intermediate is 300 pixels, and the
      reference's own rounding noise, 4e-13 at order 1, exceeds that term.)
  B   full sky 90 x 180 (enmap.fullsky_geometry(res=2 deg): pixel x lies at RA = 180 - 2x deg, the seam on the centre of column 0)
Points:
  *_pix   [{y,x}, n] pixel coordinates for utils.interpol: a third inside the map, the rest up to 2.5 map sizes outside on either side
  *_pos   [{dec,ra}, n] sky coordinates for enmap.at.  A: inside and up to 20 pixels outside.  B: inside; RA = +-pi (1 - 1e-5), "on" the seam
          (1e-3 pixel from it: exactly on it the "constant" border flips with the last bit of the coordinate); between the last and the first
          column (x in (179, 180)); the same kinds of points up to three turns of the sky away; within a pixel of both poles
Outputs, for orders 0, 1, 3, the reference's borders "nearest", "wrap", "mirror", "constant" (cval 0.7) and float32 / float64 maps (keys
<what>_<geometry>_<f4|f8>_<order>_<border>):
  ip_*    utils.interpol(map, pix)          at_*    enmap.at(map, pos)
  Order 3 on a float32 map is not stored: the reference rounds scipy's float64 coefficients into the float32 copy of the map and returns
  float32, the device keeps float64 coefficients and returns float64.  The float32 and float64 maps hold the same
  numbers, so the float64 map's values are the expected ones; asserted here: the reference's float32 values are within 64 * 2^-24 of them
Projections (keys P?_<border>_<order>, float64 maps; P?_geo the output geometry), each the whole-map interpolation on the output's pixels:
  P1   B -> a 60 x 100 patch of 2.6 deg pixels (1.3 x), offset by a fraction of a pixel, across the seam: "constant" and "grid-wrap", order 3
  P2   A -> A shifted by (0.25, -0.4) pixel: "constant", orders 1 and 3
  P4   A -> the pixel-compatible sub-geometry rows 10:30, columns 20:50: "constant", order 3
  P1_block   for the record only: what the reference's own enmap.project gives for P1 "constant" (float32): output rows in blocks, each on an
             apodised band of the input
E_ref: the largest |c_ref - c_dense| / max|f| over both geometries and the five borders, c_ref the reference's filtered array
(utils.interpolator(...).arr: scipy.ndimage.spline_filter), c_dense the float64 dense solution of B c = f along each axis, B the
(1/6, 4/6, 1/6) collocation matrix under the border's extension (condition number <= 3: good to a few ulp).
Asserted here: no coordinate used at order 0 lies within 1e-6 pixel of a rounding tie, and none used with "constant" within 1e-6 pixel of 0
or n - 1: the tests have no case to leave out.

As run for the committed fixture:
  order 3 on the float32 maps: the reference's float32 values are within 9.81e-08 of those of the float64 maps (not stored)
  P4 (pixel-compatible): the interpolated values are within 8.88e-16 of the input's pixels
  the reference's blockwise project, P1 constant: off the whole-map values by 0.00139
  E_ref = 3.55e-15 (the reference's filtered maps against the dense solve, relative to max|f|, both geometries, five borders)
  scipy's "nearest" start on a 9-sample line: 4.19e-12 off the dense solve (its error falls as 0.268^(2n): nothing at 45 samples)
  interpol.npz: 569724 bytes
"""
import sys, os, types
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_harness as H

degree = np.pi/180
ORDERS, REF_BORDERS, CVAL = (0, 1, 3), ("nearest", "wrap", "mirror", "constant"), 0.7
EXTENSION = {"nearest": "reflect", "mirror": "mirror", "constant": "mirror", "wrap": "mirror", "grid-wrap": "periodic"}

def ext_index(i, n, rule):
	if n == 1: return 0
	if rule == "mirror": P = 2*(n-1); m = i % P; return m if m < n else P-m
	if rule == "reflect": P = 2*n; m = i % P; return m if m < n else P-1-m
	return i % n

def collocation(n, rule):
	B = np.zeros((n, n))
	for k in range(n):
		for d, w in ((-1, 1/6), (0, 4/6), (1, 1/6)): B[k, ext_index(k+d, n, rule)] += w
	return B

def dense_coefficients(f, border):
	"""the solution of B c = f along the last two axes of f"""
	rule = EXTENSION[border]
	c = np.linalg.solve(collocation(f.shape[-2], rule), np.moveaxis(np.asarray(f, float), -2, 0).reshape(f.shape[-2], -1)).reshape((f.shape[-2],)+f.shape[:-2]+f.shape[-1:])
	c = np.moveaxis(c, 0, -2)
	c = np.linalg.solve(collocation(f.shape[-1], rule), np.moveaxis(c, -1, 0).reshape(f.shape[-1], -1)).reshape((f.shape[-1],)+f.shape[:-1])
	return np.moveaxis(c, 0, -1)

def geo_numbers(shape, wcs):
	return np.concatenate([np.array([shape[-2], shape[-1]], float), np.array(wcs.wcs.cdelt, float), np.array(wcs.wcs.crval, float), np.array(wcs.wcs.crpix, float)])

def make_wcs(cdelt, crval, crpix):
	w = H.StubWCS(naxis=2)
	w.wcs.cdelt, w.wcs.crval, w.wcs.crpix = np.array(cdelt, float), np.array(crval, float), np.array(crpix, float)
	w.wcs.ctype = ["RA---CAR", "DEC--CAR"]
	return w

def main(write=True):
	ns = H.load_reference(types.ModuleType("sht_exp"))
	enmap, utils = ns.enmap, ns.utils
	out, rep = {}, []
	def say(s): rep.append(s); print(s)
	def check_coords(pix, shape, what, constant=True):
		"""the two assertions on a set of pixel coordinates [{y,x}, ...]"""
		pix = np.asarray(pix, float).reshape(2, -1)
		tie = np.abs(pix+0.5-np.round(pix+0.5)).min()
		assert tie > 1e-6, "%s: a coordinate %.3g pixel from a rounding tie" % (what, tie)
		if constant:
			edge = min(np.abs(pix[a]-v).min() for a in (0, 1) for v in (0, shape[-2+a]-1))
			assert edge > 1e-6, "%s: a coordinate %.3g pixel from the edge of the constant border" % (what, edge)

	rng = np.random.default_rng(20251020)
	shapeA, wcsA = (45, 100), make_wcs([-0.5, 0.5], [20.0, 0.0], [50.3, -76.9])
	shapeB, wcsB = enmap.fullsky_geometry(res=2*degree); shapeB = tuple(int(v) for v in shapeB[-2:])
	assert shapeB == (90, 180)
	geos = {"A": (shapeA, wcsA), "B": (shapeB, wcsB)}
	maps = {}
	for g, (shape, wcs) in geos.items():
		out[g+"_geo"] = geo_numbers(shape, wcs)
		maps[g] = rng.integers(-2**20, 2**20, (2,)+shape).astype(np.float64)/2**20
		assert np.array_equal(maps[g].astype(np.float32).astype(np.float64), maps[g])
		out[g+"_map"] = maps[g]
	assert abs(enmap.pix2sky(shapeA, wcsA, [22, 50], safe=False)[0]/degree-50) < 0.1
	out["cval"] = CVAL

	# ---- points ----
	def pix_points(shape, n):
		ny, nx = shape
		y = np.concatenate([rng.uniform(0, ny-1, n//3), rng.uniform(-2.5*ny, 3.5*ny, n-n//3)])
		x = np.concatenate([rng.uniform(0, nx-1, n//3), rng.uniform(-2.5*nx, 3.5*nx, n-n//3)])
		return np.array([y, x])
	out["A_pix"], out["B_pix"] = pix_points(shapeA, 36), pix_points(shapeB, 60)
	posA = enmap.pix2sky(shapeA, wcsA, np.array([np.concatenate([rng.uniform(0, 44, 20), rng.uniform(-20, 64, 12)]), np.concatenate([rng.uniform(0, 99, 20), rng.uniform(-20, 119, 12)])]), safe=False)
	pixB = 2*degree
	inside = enmap.pix2sky(shapeB, wcsB, np.array([rng.uniform(0, 89, 20), rng.uniform(0, 179, 20)]), safe=False)
	seam = np.array([rng.uniform(-1.3, 1.3, 4), np.array([1, -1, 1, -1])*np.pi*(1-1e-5)])
	gap = enmap.pix2sky(shapeB, wcsB, np.array([rng.uniform(0, 89, 6), rng.uniform(179.05, 179.95, 6)]), safe=False)
	poles = np.array([[np.pi/2-0.3*pixB, np.pi/2-0.8*pixB, -np.pi/2+0.45*pixB, -np.pi/2+0.9*pixB], rng.uniform(-np.pi, np.pi, 4)])
	near = np.concatenate([inside, seam, gap, poles], 1)
	far = near[:, rng.choice(near.shape[1], 24, replace=False)].copy()
	far[1] += 2*np.pi*rng.choice([-3, -2, -1, 1, 2, 3], 24)
	posB = np.concatenate([near, far], 1)
	out["A_pos"], out["B_pos"] = np.asarray(posA), posB
	pos = {"A": out["A_pos"], "B": out["B_pos"]}

	# ---- utils.interpol and enmap.at ----
	f32dev = [0.0]
	for g, (shape, wcs) in geos.items():
		check_coords(out[g+"_pix"], shape, g+"_pix")
		check_coords(enmap.sky2pix(shape, wcs, pos[g]), shape, g+"_pos")
		for dt, tag in ((np.float64, "f8"), (np.float32, "f4")):
			m = enmap.ndmap(maps[g].astype(dt), wcs)
			for order in ORDERS:
				for border in REF_BORDERS:
					key = "%s_%s_%d_%s" % (g, tag, order, border)
					vi = np.asarray(utils.interpol(m, out[g+"_pix"], order=order, border=border, cval=CVAL))
					va = np.asarray(enmap.at(m, pos[g], order=order, border=border, cval=CVAL))
					assert vi.dtype == dt and va.dtype == dt and vi.shape == (2, out[g+"_pix"].shape[1])
					if order == 3 and dt == np.float32:
						# the reference stores scipy's float64 coefficients back into the float32 copy of the map and so returns float32; the device keeps
						# float64 coefficients.  The two maps hold the same numbers, so the float64 map's values are what a float32 map is checked against
						k8 = "%s_f8_%d_%s" % (g, order, border)
						f32dev[0] = max(f32dev[0], float(np.max(np.abs(vi-out["ip_"+k8]))), float(np.max(np.abs(va-out["at_"+k8]))))
						continue
					out["ip_"+key], out["at_"+key] = vi, va

	say("  order 3 on the float32 maps: the reference's float32 values are within %.3g of those of the float64 maps (not stored)" % f32dev[0])
	assert f32dev[0] < 64*2.0**-24
	# ---- projections: the whole map in one go ----
	shape1, wcs1 = (60, 100), make_wcs([-2.6, 2.6], [160.37, 0.0], [50.2, 30.73])
	shape2, wcs2 = shapeA, wcsA.deepcopy(); wcs2.wcs.crpix = wcsA.wcs.crpix-np.array([-0.4, 0.25])      # output pixel o is input pixel o + (0.25, -0.4) in {y,x}
	shape4, wcs4 = enmap.slice_geometry(shapeA, wcsA, (slice(10, 30), slice(20, 50))); shape4 = tuple(int(v) for v in shape4[-2:])
	out["P1_geo"], out["P2_geo"], out["P4_geo"] = geo_numbers(shape1, wcs1), geo_numbers(shape2, wcs2), geo_numbers(shape4, wcs4)
	def whole(g, oshape, owcs, order, border):
		m = enmap.ndmap(maps[g], geos[g][1])
		pix = m.sky2pix(enmap.posmap(oshape, owcs))
		check_coords(pix, geos[g][0], "projection", constant=border == "constant")
		return np.asarray(utils.interpol(m, pix, order=order, border=border, cval=CVAL)), np.asarray(pix)
	out["P1_constant_3"], pix1 = whole("B", shape1, wcs1, 3, "constant")
	out["P1_grid-wrap_3"], _ = whole("B", shape1, wcs1, 3, "grid-wrap")
	assert np.any(out["P1_constant_3"] == CVAL) and np.any(out["P1_constant_3"] != CVAL)
	out["P2_constant_3"], pix2 = whole("A", shape2, wcs2, 3, "constant")
	out["P2_constant_1"], _ = whole("A", shape2, wcs2, 1, "constant")
	assert np.max(np.abs(pix2-(np.mgrid[:45, :100]+np.array([0.25, -0.4])[:, None, None]))) < 1e-9
	out["P4_constant_3"], pix4 = whole("A", shape4, wcs4, 3, "constant")
	assert np.max(np.abs(pix4-(np.mgrid[10:30, 20:50]))) < 1e-9
	say("  P4 (pixel-compatible): the interpolated values are within %.3g of the input's pixels" % np.max(np.abs(out["P4_constant_3"]-maps["A"][:, 10:30, 20:50])))
	block = np.asarray(enmap.project(enmap.ndmap(maps["B"], wcsB), shape1, wcs1, order=3, border="constant", cval=CVAL, force=True))      # (force: straight to the block loop)
	out["P1_block"] = block.astype(np.float32)
	say("  the reference's blockwise project, P1 constant: off the whole-map values by %.3g" % np.max(np.abs(block-out["P1_constant_3"])))

	# ---- E_ref ----
	eref = 0.0
	for g, (shape, wcs) in geos.items():
		for border in REF_BORDERS+("grid-wrap",):
			c_ref = np.asarray(utils.interpolator(maps[g], npre=1, order=3, border=border).arr)
			e = float(np.max(np.abs(c_ref-dense_coefficients(maps[g], border)))/np.max(np.abs(maps[g])))
			eref = max(eref, e)
	line = rng.standard_normal(9)
	import scipy.ndimage
	short = float(np.max(np.abs(scipy.ndimage.spline_filter1d(line, 3, mode="nearest")-np.linalg.solve(collocation(9, "reflect"), line)))/np.max(np.abs(line)))
	out["E_ref"] = eref
	say("  E_ref = %.3g (the reference's filtered maps against the dense solve, relative to max|f|, both geometries, five borders)" % eref)
	say("  scipy's \"nearest\" start on a 9-sample line: %.3g off the dense solve (its error falls as 0.268^(2n): nothing at 45 samples)" % short)
	if write:
		f = os.path.join(HERE, "interpol.npz")
		np.savez_compressed(f, **out)
		say("  interpol.npz: %d bytes" % os.path.getsize(f))
	return rep

if __name__ == "__main__":
	main()
