"""Generate tests/golden/distances.npz: inputs and what the REFERENCE's enmap.distance_from / distance_transform /
labeled_distance_transform / apod and distances.find_edges give for them.

Run:  python tests/golden/make_distances.py      (needs /root/reference, cython, gcc and scipy; never run on the GPU box)

The reference is imported through _ref_harness.py; its cython/distances.pyx + distances_core.c are compiled into a temporary directory
and registered as pixell.distances.  Only arrays are saved.

The expected distances are the reference's method="simple" results: its brute-force loop over every (pixel, point) pair in Vincenty's
atan2 form, the reference's own exact path.  Next to them lies an np.longdouble evaluation of the same formula from the same float64
coordinates (stored on every 7th pixel, to keep the file small), and E_ref, the reference's largest absolute error against it over all
pixels of all cases.  The tests bound the device's error by
tol = max(4 E_ref, 8 * 2^-52 * pi).  What the reference's default method="cellgrid" gives is stored as the yardstick: a port of it
fails that bound by many orders of magnitude.

Cases (keys <case>_*):
  A   45 x 100 patch of the 0.5' full-sky geometry (rows 16800:16845, columns 1200:1300: dec 50 deg; neither axis a multiple of 16, x does
      not wrap); 341 points: 37 anywhere inside, one 3 pixels and one 40 pixels beyond an edge, two coincident, 300 within 8 x 8 pixels
  B   full sky 90 x 180 (the seam wraps); 40 points, two on the RA seam, one within a pixel of each pole; B1: a single point (distances up
      to the antipode)
  C   distance_transform: CA [2, 45, 100] on A's geometry (plane 0: discs, a one-pixel hole, a hole cut by the corner; plane 1: all true
      but one disc), CB on B's geometry (a hole across the seam and a polar cap); the all-true and all-false masks need no fixture
  D   labeled_distance_transform on A's geometry: three labelled regions, two of them touching
  E   apod_mask / grow_mask / shrink_mask on A's geometry: the exact distance transforms of the mask, of the mask with its border
      cleared (edge=True) and of its complement; asserted here: no distance lies within 1e-9 rad of 4.3 pixels (grow / shrink), so that
      a `<` cannot flip (apod_mask, width 6 pixels, is continuous in the distance at its width).  apod: a [2, 20, 30] map, widths (3, 5),
      all four fills, cosine profile, and "lin" with fill "zero"
  *_edges: the reference's find_edges / find_edges_labeled output as a sorted array without repeats (the reference lists the border
      first and three of the four corners twice)

As run for the committed fixtures:
  cellgrid, A (arbitrary points): off by 0.000615 rad = 4.226 pixel; B: off by 0.0233 rad
  cellgrid, CA (pixel-centred points): off by 0 rad = 0.000 pixel
  cellgrid, E (pixel-centred points, border cleared): off by 4.94e-06 rad = 0.034 pixel
  E: the distance nearest to a threshold is 3.22e-06 rad from it
  E_ref = 6.92e-16 rad (the reference's simple method against the long double evaluation, all cases)
  distances.npz: 548005 bytes
so tol = max(4 E_ref, 8 * 2^-52 * pi) = 5.58e-15 rad.  The device's worst distance error over all cases of tests/test_distances.py, as
the tests print it: 1.33e-15 rad on an MI355X (case B1, the single point), 1.44e-15 rad in the host simulator (case CB).
"""
import sys, os, types, subprocess, tempfile, sysconfig
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_harness as H

arcmin = np.pi/180/60

def build_distances(tmp):
	src = os.path.join(H.REF, "cython")
	subprocess.check_call([sys.executable, "-m", "cython", "-3", "-I", src, os.path.join(src, "distances.pyx"), "-o", os.path.join(tmp, "distances.c")])
	inc = [sysconfig.get_paths()["include"], np.get_include(), src]
	out = os.path.join(tmp, "distances"+sysconfig.get_config_var("EXT_SUFFIX"))
	subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-fopenmp", "-w"]+["-I"+i for i in inc]+[os.path.join(tmp, "distances.c"), os.path.join(src, "distances_core.c"), "-o", out, "-lm"])
	sys.path.insert(0, tmp)
	import distances
	return distances

def vincenty(pdec, pra, qdec, qra, dtype=np.float64):
	"""[ny, nx, npoint] distances in the form of distances_core.c:87-132, evaluated in dtype"""
	pdec, pra = np.asarray(pdec, dtype)[:, None, None], np.asarray(pra, dtype)[None, :, None]
	qdec, qra = np.asarray(qdec, dtype)[None, None, :], np.asarray(qra, dtype)[None, None, :]
	dra = pra-qra
	y1 = np.cos(qdec)*np.sin(dra)
	y2 = np.cos(pdec)*np.sin(qdec)-np.sin(pdec)*np.cos(qdec)*np.cos(dra)
	return np.arctan2(np.sqrt(y1*y1+y2*y2), np.sin(pdec)*np.sin(qdec)+np.cos(pdec)*np.cos(qdec)*np.cos(dra))

def long_min(dec, ra, pts):
	"""the nearest-point distance in long double, a chunk of points at a time; returned as float64"""
	best = np.full((len(dec), len(ra)), np.inf, np.longdouble)
	for i0 in range(0, pts.shape[1], 64):
		best = np.minimum(best, vincenty(dec, ra, pts[0, i0:i0+64], pts[1, i0:i0+64], np.longdouble).min(-1))
	return best

def geo_numbers(shape, wcs):
	return np.concatenate([np.array([shape[-2], shape[-1]], float), np.array(wcs.wcs.cdelt, float), np.array(wcs.wcs.crval, float), np.array(wcs.wcs.crpix, float)])

def main(write=True):
	tmp = tempfile.mkdtemp(prefix="pixell_distances_")
	distances = build_distances(tmp)
	sys.modules["pixell.distances"] = distances
	ns = H.load_reference(types.ModuleType("sht_exp"))
	import pixell
	pixell.distances = distances
	enmap = ns.enmap
	out, rep, eref = {}, [], [0.0]
	def say(s): rep.append(s); print(s)
	def uniq(e): return np.unique(np.asarray(e, np.int64))

	fshape, fwcs = enmap.fullsky_geometry(res=0.5*arcmin)
	shapeA, wcsA = enmap.slice_geometry(fshape, fwcs, (slice(16800, 16845), slice(1200, 1300)))
	shapeA = tuple(int(v) for v in shapeA[-2:])
	shapeB, wcsB = enmap.fullsky_geometry(res=2*np.pi/180); shapeB = tuple(int(v) for v in shapeB[-2:])
	assert shapeA == (45, 100) and shapeB == (90, 180)
	out["A_geo"], out["B_geo"] = geo_numbers(shapeA, wcsA), geo_numbers(shapeB, wcsB)
	axA, axB = enmap.posaxes(shapeA, wcsA), enmap.posaxes(shapeB, wcsB)
	out["A_dec"], out["A_ra"], out["B_dec"], out["B_ra"] = axA[0], axA[1], axB[0], axB[1]
	pixA = abs(wcsA.wcs.cdelt[1])*np.pi/180
	out["A_pix"] = pixA

	def points_case(tag, shape, wcs, ax, pts):
		d, dom = enmap.distance_from(shape, wcs, pts, domains=True, method="simple")
		dl = long_min(ax[0], ax[1], pts)
		err = float(np.max(np.abs(np.asarray(d, np.longdouble)-dl)))
		eref[0] = max(eref[0], err)
		out[tag+"_points"], out[tag+"_simple"], out[tag+"_long_sub"] = pts, np.asarray(d), np.float64(dl).reshape(-1)[::7]
		cg = np.asarray(enmap.distance_from(shape, wcs, pts, method="cellgrid"))
		out[tag+"_cellgrid_err"] = float(np.max(np.abs(cg-np.asarray(d))))
		return np.asarray(d), out[tag+"_cellgrid_err"]

	# ---- A ----
	rng = np.random.default_rng(20250301)
	ys = np.concatenate([rng.uniform(0, 44, 37), [-3.0, 20.0], [30.3, 30.3], rng.uniform(10, 18, 300)])
	xs = np.concatenate([rng.uniform(0, 99, 37), [40.3, 139.0], [71.7, 71.7], rng.uniform(52, 60, 300)])
	ptsA = np.asarray(enmap.pix2sky(shapeA, wcsA, np.array([ys, xs]), safe=False))
	_, cgA = points_case("A", shapeA, wcsA, axA, ptsA)
	# ---- B ----
	rng = np.random.default_rng(7)
	pixB = 2*np.pi/180
	decB = np.concatenate([rng.uniform(-80, 80, 36)*np.pi/180, [0.3, -0.8], [np.pi/2-0.6*pixB, -np.pi/2+0.4*pixB]])
	raB = np.concatenate([rng.uniform(-np.pi, np.pi, 36), [np.pi-1e-3, -np.pi+0.01], [1.0, -2.0]])
	_, cgB = points_case("B", shapeB, wcsB, axB, np.array([decB, raB]))
	points_case("B1", shapeB, wcsB, axB, np.array([[0.4], [2.0]]))
	say("  cellgrid, A (arbitrary points): off by %.3g rad = %.3f pixel; B: off by %.3g rad" % (cgA, cgA/pixA, cgB))

	# ---- C ----
	def dt_case(tag, shape, wcs, ax, mask):
		m = enmap.ndmap(mask, wcs)
		d = np.asarray(enmap.distance_transform(m, method="simple"))
		worst = 0.0
		for i, mi in enumerate(mask.reshape((-1,)+mask.shape[-2:])):
			e = uniq(distances.find_edges(mi, flat=True))
			pts = np.array([ax[0][e//shape[1]], ax[1][e % shape[1]]])
			dl = long_min(ax[0], ax[1], pts)*mi
			worst = max(worst, float(np.max(np.abs(np.asarray(d.reshape((-1,)+mask.shape[-2:])[i], np.longdouble)-dl))))
			out["%s_edges%d" % (tag, i)] = e
		eref[0] = max(eref[0], worst)
		out[tag+"_mask"], out[tag+"_simple"] = mask, d
		return d
	yy, xx = np.mgrid[:45, :100]
	m0 = np.ones((45, 100), bool)
	for cy, cx, r in [(12.3, 20.1, 5.2), (30.0, 55.5, 8.4), (20.0, 80.0, 3.0)]: m0 &= (yy-cy)**2+(xx-cx)**2 > r*r
	m0[40, 10] = False; m0 &= (yy-44)**2+(xx-99)**2 > 6.5**2
	m1 = (yy-22.5)**2+(xx-31.2)**2 > 7.7**2
	maskCA = np.array([m0, m1])
	dCA = dt_case("CA", shapeA, wcsA, axA, maskCA)
	cg = np.asarray(enmap.distance_transform(enmap.ndmap(maskCA, wcsA), method="cellgrid"))
	out["CA_cellgrid_err"] = float(np.max(np.abs(cg-dCA)))
	say("  cellgrid, CA (pixel-centred points): off by %.3g rad = %.3f pixel" % (out["CA_cellgrid_err"], out["CA_cellgrid_err"]/pixA))
	yb, xb = np.mgrid[:90, :180]
	maskCB = (yb > 6) & ~((np.abs(yb-50) < 7) & ((xb < 5) | (xb > 171)))
	dt_case("CB", shapeB, wcsB, axB, maskCB)

	# ---- D ----
	labels = np.zeros((45, 100), np.int32)
	labels[5:15, 10:30] = 1; labels[15:22, 18:40] = 2; labels[30:40, 60:75] = 7
	dD, domD = enmap.labeled_distance_transform(enmap.ndmap(labels, wcsA), method="simple")
	out["D_labels"], out["D_simple"], out["D_domains"] = labels, np.asarray(dD), np.asarray(domD)
	out["D_edges"] = uniq(distances.find_edges_labeled(labels, flat=True))

	# ---- E ----
	rng = np.random.default_rng(11)
	mE = np.ones((45, 100), bool)
	for k in range(6):
		cy, cx, r = rng.uniform(5, 40), rng.uniform(5, 95), rng.uniform(2, 7)
		mE &= (yy-cy)**2+(xx-cx)**2 > r*r
	mEe = mE.copy(); mEe[0, :] = False; mEe[-1, :] = False; mEe[:, 0] = False; mEe[:, -1] = False
	out["E_mask"] = mE
	dts = {}
	for tag, m in (("E_dt", mE), ("E_dt_edge", mEe), ("E_dt_not", ~mE)):
		dts[tag] = out[tag] = np.asarray(enmap.distance_transform(enmap.ndmap(m, wcsA), method="simple"))
	r_gs, r_ap = 4.3*pixA, 6*pixA
	out["E_r"], out["E_width"] = r_gs, r_ap
	gap = min(np.min(np.abs(dts["E_dt"]-r_gs)), np.min(np.abs(dts["E_dt_not"]-r_gs)))      # (apod_mask is continuous in the distance at its width: no threshold there)
	cgE = np.asarray(enmap.distance_transform(enmap.ndmap(mEe, wcsA), method="cellgrid"))
	out["E_cellgrid_err"] = float(np.max(np.abs(cgE-dts["E_dt_edge"])))
	say("  cellgrid, E (pixel-centred points, border cleared): off by %.3g rad = %.3f pixel" % (out["E_cellgrid_err"], out["E_cellgrid_err"]/pixA))
	say("  E: the distance nearest to a threshold is %.3g rad from it" % gap)
	assert gap > 1e-9, "a distance sits on a threshold: change the mask"
	mapE = rng.standard_normal((2, 20, 30))
	out["E_map"] = mapE
	for fill in ("zero", "mean", "median", "crossfade"):
		out["E_apod_"+fill] = np.asarray(enmap.apod(enmap.ndmap(mapE.copy(), wcsA), (3, 5), profile="cos", fill=fill))
	out["E_apod_lin"] = np.asarray(enmap.apod(enmap.ndmap(mapE.copy(), wcsA), 4, profile="lin"))

	out["E_ref"] = eref[0]
	say("  E_ref = %.3g rad (the reference's simple method against the long double evaluation, all cases)" % eref[0])
	if write:
		f = os.path.join(HERE, "distances.npz")
		np.savez_compressed(f, **out)
		say("  distances.npz: %d bytes" % os.path.getsize(f))
	return rep

if __name__ == "__main__":
	main()
