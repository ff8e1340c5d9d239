"""pixell_amd.distances (find_edges, find_edges_labeled, distance_from_points) and enmap.distance_from / distance_transform /
labeled_distance_transform / grow_mask / shrink_mask / apod_mask / apod, against the reference's exact method="simple" results of
tests/golden/make_distances.py (fixture distances.npz).
  distances   |d - min(d_simple, rmax)| <= tol = max(4 E_ref, 8 * 2^-52 * pi) rad on every pixel; E_ref, from the fixture, is the
              reference's own error against a long double evaluation (a few 1e-16); the factor 4 is for a libm that differs from glibc by an
              ulp or two in sin, cos and atan2, the floor a few roundings at the largest distance.  The reference's default "cellgrid" is
              off by 1e-6 to 1e-2 rad on the same cases: a port of it fails.
  domains     not compared by index (pixel-centred points tie by symmetry): j is right when r(p, j) <= d_simple(p) + tol, r the float64
              Vincenty distance evaluated here; within tol of rmax -1 or a valid j passes; beyond rmax it must be -1
  edges       the reference's as sorted arrays, ascending
  pruning     4096 uniform points on the 90 x 180 full sky: the tiles look at less than a quarter of ntile * npoint points (brute force: 1)
Each case runs in the host simulator (*_sim, here) and on the GPU (*_gpu).
Measured worst distance errors (the prints below), tol being 5.58e-15 rad: 1.44e-15 rad in the host simulator (case CB), 1.33e-15 rad on an
MI355X (case B1); the pruning case looks at 0.143 of ntile * npoint."""
import os
import numpy as np
import pytest
from pixell_amd import enmap, distances
from pixell_amd.wcs import CarWCS

FLOOR = 8*2.0**-52*np.pi

@pytest.fixture(scope="module")
def fx(golden_dir):
	return dict(np.load(os.path.join(golden_dir, "distances.npz")))

def geometry(numbers, pre=()):
	n = np.asarray(numbers, float)
	return tuple(pre)+(int(n[0]), int(n[1])), CarWCS(cdelt=n[2:4], crval=n[4:6], crpix=n[6:8])

def host(x):
	if isinstance(x, enmap.dmap): x = x.tensor
	return x.detach().cpu().numpy() if hasattr(x, "data_ptr") else np.asarray(x)
def ident(a): return a
def cuda(a):
	import torch
	return torch.as_tensor(np.ascontiguousarray(a), device="cuda")
def as_map(dev, a, wcs): return enmap.ndmap(a, wcs) if dev is ident else enmap.dmap(dev(a), wcs)
def tol_of(fx): return max(4*float(fx["E_ref"]), FLOOR)

def vincenty(pdec, pra, qdec, qra):
	"""float64, elementwise, in the form of the reference's simple method"""
	dra = pra-qra
	y1 = np.cos(qdec)*np.sin(dra)
	y2 = np.cos(pdec)*np.sin(qdec)-np.sin(pdec)*np.cos(qdec)*np.cos(dra)
	return np.arctan2(np.sqrt(y1*y1+y2*y2), np.sin(pdec)*np.sin(qdec)+np.cos(pdec)*np.cos(qdec)*np.cos(dra))

def check(tag, fx, dec, ra, pts, got, want, rmax=None, dom=None, where=None):
	"""every pixel (of `where`): the distance against min(want, rmax), the domain by the distance of the point it names"""
	tol = tol_of(fx)
	got = np.float64(host(got)); sel = np.ones(want.shape, bool) if where is None else where
	exp = want if rmax is None else np.minimum(want, rmax)
	err = np.abs(got-exp)[sel].max() if sel.any() else 0.0
	print("%s: worst distance error %.3g rad (tol %.3g)" % (tag, err, tol))
	assert got.shape == want.shape and err <= tol, tag
	if dom is None: return err
	dom = host(dom)
	assert dom.shape == want.shape and dom.dtype == np.int32 and dom.max() < pts.shape[1] and dom.min() >= -1, tag
	named = dom >= 0
	pd, pr = np.broadcast_to(dec[:, None], want.shape), np.broadcast_to(ra[None, :], want.shape)
	r = np.full(want.shape, np.inf); r[named] = vincenty(pd[named], pr[named], pts[0][dom[named]], pts[1][dom[named]])
	ok = np.where(named, r <= want+tol, False)
	if rmax is not None:
		ok &= want <= rmax+tol                      # a named point is within rmax
		ok |= ~named & (want >= rmax-tol)           # no point named: none is within rmax
	assert np.all(ok[sel]), "%s: %d wrong domains" % (tag, np.sum(~ok[sel]))
	return err

# ---- bodies ---------------------------------------------------------------------------------------------------------------------
def points_body(fx, dev, on_device):
	worst = 0
	for g, tag, rmaxs in (("A", "A", (None, 6.0, 0.3)), ("B", "B", (None, 0.2)), ("B", "B1", (None,))):
		shape, wcs = geometry(fx[g+"_geo"])
		dec, ra, pts, want = fx[g+"_dec"], fx[g+"_ra"], fx[tag+"_points"], fx[tag+"_simple"]
		assert np.max(np.abs(want.reshape(-1)[::7]-fx[tag+"_long_sub"])) <= float(fx["E_ref"])
		for rm in rmaxs:
			rmax = None if rm is None else (rm*float(fx["A_pix"]) if g == "A" else rm)
			d, dom = enmap.distance_from(shape, wcs, dev(pts), domains=True, rmax=rmax)
			assert isinstance(d, enmap.dmap if on_device else enmap.ndmap) and isinstance(dom, enmap.dmap if on_device else enmap.ndmap) and d.dtype == np.float64
			worst = max(worst, check("%s rmax %s" % (tag, rm), fx, dec, ra, pts, d, want, rmax, dom))
			if rmax is not None: assert np.any(host(dom) < 0) and np.any(host(dom) >= 0)
		print("cellgrid yardstick %s: %.3g rad" % (tag, float(fx[tag+"_cellgrid_err"])))
		assert float(fx[tag+"_cellgrid_err"]) > 1e3*tol_of(fx) or tag == "B1"
	assert fx["B1_simple"].max() > 3.1      # (up to the antipode)
	# without domains, float32 output, every method name, the method form
	shape, wcs = geometry(fx["A_geo"])
	for method in ("cellgrid", "bubble", "simple"):
		d = enmap.distance_from(shape, wcs, dev(fx["A_points"]), method=method)
		check("A "+method, fx, fx["A_dec"], fx["A_ra"], fx["A_points"], d, fx["A_simple"])
	o32 = as_map(dev, np.zeros(shape, np.float32), wcs)
	assert enmap.distance_from(shape, wcs, dev(fx["A_points"]), omap=o32) is o32
	assert np.array_equal(host(o32), np.float32(host(d)))
	assert np.array_equal(host(o32.distance_from(dev(fx["A_points"]))), host(d))
	# no points
	z = np.zeros((2, 0))
	d, dom = enmap.distance_from(shape, wcs, dev(z), domains=True)
	assert np.all(np.isinf(host(d))) and np.all(host(dom) == -1) and host(d).shape == shape
	d = enmap.distance_from(shape, wcs, dev(z), rmax=0.25)
	assert np.all(host(d) == 0.25)
	print("worst distance error of the point cases: %.3g rad" % worst)

def edges_body(fx, dev, on_device):
	cases = [(fx["CA_mask"][0], fx["CA_edges0"], False), (fx["CA_mask"][1], fx["CA_edges1"], False), (fx["CB_mask"], fx["CB_edges0"], False), (fx["D_labels"], fx["D_edges"], True)]
	for arr, want, lab in cases:
		f = distances.find_edges_labeled if lab else distances.find_edges
		e = f(dev(arr), flat=True)
		assert hasattr(e, "data_ptr") == on_device and host(e).dtype == np.int64
		assert np.array_equal(host(e), want) and np.all(np.diff(host(e)) > 0)
		y, x = f(dev(arr))
		assert np.array_equal(host(y), want//arr.shape[1]) and np.array_equal(host(x), want % arr.shape[1])
	ny, nx = 45, 100
	border = np.unique(np.concatenate([np.arange(nx), (ny-1)*nx+np.arange(nx), np.arange(ny)*nx, np.arange(ny)*nx+nx-1]))
	assert np.array_equal(host(distances.find_edges(dev(np.zeros((ny, nx), bool)), flat=True)), border)
	assert host(distances.find_edges(dev(np.ones((ny, nx), bool)), flat=True)).shape == (0,)
	# more than one block of the edge finder, a count that is no multiple of anything: every pixel of a 37 x 61 checkerboard's zeros
	yy, xx = np.mgrid[:37, :61]
	cb = ((yy+xx) % 2).astype(np.uint8)
	assert np.array_equal(host(distances.find_edges(dev(cb), flat=True)), np.flatnonzero(cb == 0))

def transform_body(fx, dev, on_device):
	worst = 0
	for g, tag in (("A", "CA"), ("B", "CB")):
		mask, want = fx[tag+"_mask"], fx[tag+"_simple"]
		shape, wcs = geometry(fx[g+"_geo"], mask.shape[:-2])
		assert mask.ndim == (3 if tag == "CA" else 2)
		d = enmap.distance_transform(as_map(dev, mask, wcs))
		assert isinstance(d, enmap.dmap if on_device else enmap.ndmap) and d.dtype == np.float64 and d.shape == mask.shape
		for i, (mi, wi, di) in enumerate(zip(mask.reshape((-1,)+mask.shape[-2:]), want.reshape((-1,)+mask.shape[-2:]), np.float64(host(d)).reshape((-1,)+mask.shape[-2:]))):
			worst = max(worst, check("%s[%d]" % (tag, i), fx, None, None, None, di, wi))
			assert np.all(di[~mi] == 0) and np.all(di[mi] > 0)
		dm = as_map(dev, mask, wcs).distance_transform(rmax=0.01 if g == "A" else 0.3)
		check(tag+" rmax", fx, None, None, None, dm, want, 0.01 if g == "A" else 0.3)
	# float32 and float64 omap, filled in place
	mask, want = fx["CA_mask"], fx["CA_simple"]
	shape, wcs = geometry(fx["A_geo"], (2,))
	for dt in (np.float32, np.float64):
		o = as_map(dev, np.full(mask.shape, 7, dt), wcs)
		assert enmap.distance_transform(as_map(dev, mask, wcs), omap=o) is o and o.dtype == dt
		if dt == np.float64: check("CA omap f64", fx, None, None, None, o, want)
		else: assert np.max(np.abs(np.float64(host(o))-want)) <= 2.0**-24*want.max()
	# all true: no edge, infinity (rmax with one); all false: zero
	t = as_map(dev, np.ones(shape[-2:], bool), wcs)
	assert np.all(np.isinf(host(enmap.distance_transform(t)))) and np.all(host(enmap.distance_transform(t, rmax=0.5)) == 0.5)
	assert not np.any(host(enmap.distance_transform(as_map(dev, np.zeros(shape[-2:], bool), wcs))))
	with pytest.raises(ValueError): enmap.distance_transform(t, method="heap")
	print("worst distance error of the transforms: %.3g rad" % worst)

def labeled_body(fx, dev, on_device):
	labels, want, wdom = fx["D_labels"], fx["D_simple"], fx["D_domains"]
	shape, wcs = geometry(fx["A_geo"])
	d, dom = enmap.labeled_distance_transform(as_map(dev, labels, wcs))
	assert isinstance(d, enmap.dmap if on_device else enmap.ndmap) and dom.dtype == np.int32
	check("D", fx, None, None, None, d, want)
	dom = host(dom)
	assert np.all(np.float64(host(d))[labels != 0] == 0) and set(np.unique(dom)) == {1, 2, 7}
	# a label is right when the nearest pixel of that label is as near as the nearest labelled pixel (inside a region: the region's own)
	dec, ra = fx["A_dec"], fx["A_ra"]
	e = fx["D_edges"]; ey, ex = e//shape[1], e % shape[1]
	r = vincenty(dec[:, None, None], ra[None, :, None], dec[ey][None, None, :], ra[ex][None, None, :])
	el = labels.reshape(-1)[e]
	for l in (1, 2, 7):
		sel = dom == l
		assert np.all(r[..., el == l].min(-1)[sel] <= r.min(-1)[sel]+tol_of(fx))
	assert np.mean(dom == wdom) > 0.99      # (the reference names the same label except at ties)
	# rmax: beyond it odomains keeps what it held
	od = as_map(dev, np.full(shape, -5, np.int32), wcs)
	d2, dom2 = enmap.labeled_distance_transform(as_map(dev, labels, wcs), odomains=od, rmax=3*float(fx["A_pix"]))
	assert dom2 is od
	far = want > 3*float(fx["A_pix"])+tol_of(fx)
	assert np.all(host(od)[far] == -5) and np.all(host(od)[(want > 0) & (want < 3*float(fx["A_pix"])-tol_of(fx))] > 0)      # (inside a region the edge of it may be further than rmax)
	check("D rmax", fx, None, None, None, d2, want, 3*float(fx["A_pix"]))

def apod_body(fx, dev, on_device):
	mask, r, width = fx["E_mask"], float(fx["E_r"]), float(fx["E_width"])
	shape, wcs = geometry(fx["A_geo"])
	m = as_map(dev, mask, wcs)
	tol = tol_of(fx)/width
	cos = lambda x: 0.5*(1-np.cos(np.pi*x))
	for edge, key in ((True, "E_dt_edge"), (False, "E_dt")):
		x = np.minimum(fx[key], width)/width
		for prof, model in ((enmap.apod_profile_cos, cos), (enmap.apod_profile_lin, lambda x: x), (lambda x: x**2, lambda x: x**2)):
			a = enmap.apod_mask(m, width=width, edge=edge, profile=prof)
			assert isinstance(a, enmap.dmap if on_device else enmap.ndmap)
			err = np.max(np.abs(np.float64(host(a))-model(x)))
			assert err <= 4*tol+4*2.0**-52, (edge, err)      # (|profile'| <= 2 on [0, 1], and the roundings of the profile itself)
	assert np.array_equal(host(m.apod_mask(width=width)), host(enmap.apod_mask(m, width=width)))
	g, s = enmap.grow_mask(m, r), enmap.shrink_mask(m, r)
	assert isinstance(g, enmap.dmap if on_device else enmap.ndmap)
	assert np.array_equal(host(g) != 0, fx["E_dt_not"] < r) and np.array_equal(host(s) != 0, fx["E_dt"] >= r)
	assert np.array_equal(host(m.grow_mask(r)), host(g)) and (host(g) != 0).sum() > mask.sum() > (host(s) != 0).sum() > 0
	em = as_map(dev, fx["E_map"], wcs)
	for fill in ("zero", "mean", "median", "crossfade"):
		a = enmap.apod(em, (3, 5), fill=fill)
		np.testing.assert_allclose(host(a), fx["E_apod_"+fill], rtol=0, atol=1e-14, err_msg=fill)
	np.testing.assert_allclose(host(em.apod(4, profile="lin")), fx["E_apod_lin"], rtol=0, atol=1e-14)
	assert np.array_equal(host(em), fx["E_map"])
	c = em.copy()
	assert enmap.apod(c, (3, 5), inplace=True) is c and np.allclose(host(c), fx["E_apod_zero"], rtol=0, atol=1e-14)
	with pytest.raises(ValueError): enmap.apod(em, 3, fill="wrap")

def haversine_min(dec, ra, pts):
	"""the nearest point of every pixel by the separable form of h, float64 numpy, and its Vincenty distance"""
	sy = np.sin(0.5*(dec[:, None]-pts[0][None, :]))**2
	sx = np.cos(pts[0])[None, :]*np.sin(0.5*(ra[:, None]-pts[1][None, :]))**2
	best = np.empty((len(dec), len(ra)), int)
	for y in range(len(dec)): best[y] = np.argmin(sy[y][None, :]+np.cos(dec[y])*sx, -1)
	return vincenty(dec[:, None], ra[None, :], pts[0][best], pts[1][best])

def pruning_body(fx, dev):
	shape, wcs = geometry(fx["B_geo"])
	rng = np.random.default_rng(4096)
	pts = np.array([np.arcsin(rng.uniform(-1, 1, 4096)), rng.uniform(-np.pi, np.pi, 4096)])
	d, stats = distances.distance_from_points(shape, wcs, points=dev(pts), return_stats=True)
	stats = host(stats)
	assert stats.shape == (6, 12) and stats.dtype == np.int32 and stats.min() > 0
	frac = stats.sum()/(stats.size*4096.0)
	print("pruning: the tiles looked at %.4f of ntile * npoint (%.1f points per tile on average)" % (frac, stats.mean()))
	assert frac < 0.25
	want = haversine_min(fx["B_dec"], fx["B_ra"], pts)
	err = np.max(np.abs(np.float64(host(d))-want))
	print("pruning: worst distance error %.3g rad" % err)
	assert err <= tol_of(fx)
	# pixel indices in place of coordinates, a skip map, float32 stats off: the same distances where the search runs
	pix = rng.choice(shape[0]*shape[1], 50, replace=False)
	ppos = np.array([fx["B_dec"][pix//shape[1]], fx["B_ra"][pix % shape[1]]])
	skip = rng.random(shape) < 0.7; skip[:20, :40] = False
	d1, dom1 = distances.distance_from_points(shape, wcs, pix=dev(pix), domains=True, skip=dev(skip))
	assert np.all(host(d1)[~skip] == 0) and np.all(host(dom1)[~skip] == -1)
	check("pixel indices, skip map", fx, fx["B_dec"], fx["B_ra"], ppos, d1, haversine_min(fx["B_dec"], fx["B_ra"], ppos), dom=dom1, where=skip)
	assert np.all(host(d1).reshape(-1)[pix] <= tol_of(fx))

def gap_body(fx, dev):
	"""a 40 x 170 patch of 2 deg pixels that covers 340 deg of RA and does not wrap (RA increasing with x, declination decreasing with y), 200
	points all over the sphere: those in the 20 deg gap are near to both ends of the map.  Expected: the float64 model, evaluated here."""
	shape, wcs = (40, 170), CarWCS(cdelt=[2.0, -2.0], crval=[0.0, 0.0], crpix=[85.5, 20.5])
	dec, ra = enmap.posaxes(shape, wcs)
	assert abs(ra[-1]-ra[0]-338*np.pi/180) < 1e-12 and dec[0] > dec[-1]
	rng = np.random.default_rng(170)
	pts = np.array([np.arcsin(rng.uniform(-1, 1, 200)), rng.uniform(-2.6, 2.6, 200)])
	pts[0, :8] = np.linspace(-0.6, 0.6, 8); pts[1, :8] = np.pi+rng.uniform(-0.05, 0.05, 8)      # in the gap
	want = haversine_min(dec, ra, pts)
	for rmax in (None, 0.3):
		d, dom = enmap.distance_from(shape, wcs, dev(pts), domains=True, rmax=rmax)
		check("gap rmax %s" % rmax, fx, dec, ra, pts, d, want, rmax, dom)
	dom = host(enmap.distance_from(shape, wcs, dev(pts), domains=True)[1])
	assert dom.min() >= 0 and np.any(dom[:, :3] < 8) and np.any(dom[:, -3:] < 8)      # (points in the gap win at both ends)

def determinism_body(fx, dev):
	shape, wcs = geometry(fx["A_geo"])
	run = lambda: [host(v) for v in enmap.distance_from(shape, wcs, dev(fx["A_points"]), domains=True, rmax=6*float(fx["A_pix"]))]
	a, b = run(), run()
	assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.any(a[1] >= 0)
	# the two coincident points: the lower index is named
	assert not np.any(a[1] == 40) and np.any(a[1] == 39)

def errors_body(fx, dev):
	shape, wcs = geometry(fx["A_geo"])
	tilted = CarWCS(cdelt=wcs.wcs.cdelt, crval=[wcs.wcs.crval[0], 10.0], crpix=wcs.wcs.crpix)
	with pytest.raises(NotImplementedError): enmap.distance_from(shape, tilted, dev(fx["A_points"]))
	with pytest.raises(NotImplementedError): enmap.distance_transform(as_map(dev, fx["E_mask"], tilted))
	with pytest.raises(ValueError): enmap.distance_from(shape, wcs, dev(fx["A_points"]), method="heap")
	with pytest.raises(ValueError): distances.distance_from_points(shape, wcs)
	with pytest.raises(ValueError): distances.distance_from_points(shape, wcs, points=dev(fx["A_points"]), omap=as_map(dev, np.zeros(shape, np.int32), wcs))
	with pytest.raises(ValueError): distances.find_edges(dev(np.zeros((2, 3, 4), bool)))

# ---- host simulator -------------------------------------------------------------------------------------------------------------
@pytest.mark.hostsim
def test_distance_from_sim(fx): points_body(fx, ident, False)
@pytest.mark.hostsim
def test_find_edges_sim(fx): edges_body(fx, ident, False)
@pytest.mark.hostsim
def test_distance_transform_sim(fx): transform_body(fx, ident, False)
@pytest.mark.hostsim
def test_labeled_distance_transform_sim(fx): labeled_body(fx, ident, False)
@pytest.mark.hostsim
def test_apod_grow_shrink_sim(fx): apod_body(fx, ident, False)
@pytest.mark.hostsim
def test_pruning_sim(fx): pruning_body(fx, ident)
@pytest.mark.hostsim
def test_points_in_the_gap_of_a_wide_patch_sim(fx): gap_body(fx, ident)
@pytest.mark.hostsim
def test_determinism_sim(fx): determinism_body(fx, ident)
@pytest.mark.hostsim
def test_errors_sim(fx): errors_body(fx, ident)

# ---- GPU ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_distance_from_gpu(fx):
	points_body(fx, cuda, True)
	points_body(fx, ident, False)      # host arrays in, host maps out
@pytest.mark.gpu
def test_find_edges_gpu(fx): edges_body(fx, cuda, True); edges_body(fx, ident, False)
@pytest.mark.gpu
def test_distance_transform_gpu(fx): transform_body(fx, cuda, True); transform_body(fx, ident, False)
@pytest.mark.gpu
def test_labeled_distance_transform_gpu(fx): labeled_body(fx, cuda, True); labeled_body(fx, ident, False)
@pytest.mark.gpu
def test_apod_grow_shrink_gpu(fx): apod_body(fx, cuda, True); apod_body(fx, ident, False)
@pytest.mark.gpu
def test_pruning_gpu(fx): pruning_body(fx, cuda)
@pytest.mark.gpu
def test_points_in_the_gap_of_a_wide_patch_gpu(fx): gap_body(fx, cuda)
@pytest.mark.gpu
def test_determinism_gpu(fx): determinism_body(fx, cuda)
@pytest.mark.gpu
def test_errors_gpu(fx): errors_body(fx, cuda)

@pytest.mark.gpu
def test_side_stream_gpu(fx):
	"""a search and a transform on a stream of their own: bit for bit those of the default stream"""
	import torch
	shape, wcs = geometry(fx["A_geo"])
	pts, mask = cuda(fx["A_points"]), enmap.dmap(cuda(fx["CA_mask"]), wcs)
	d0, dom0 = enmap.distance_from(shape, wcs, pts, domains=True)
	t0 = enmap.distance_transform(mask)
	torch.cuda.synchronize()
	side = torch.cuda.Stream()
	with torch.cuda.stream(side):
		d1, dom1 = enmap.distance_from(shape, wcs, pts, domains=True)
		t1 = enmap.distance_transform(mask)
	side.synchronize()
	assert torch.equal(d0.tensor, d1.tensor) and torch.equal(dom0.tensor, dom1.tensor) and torch.equal(t0.tensor, t1.tensor)
	assert np.max(np.abs(host(d1)-fx["A_simple"])) <= tol_of(fx)
