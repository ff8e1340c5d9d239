"""pixell_amd.labels (label, stats and the scipy-shaped readers) and analysis.solve_mapsys.
  labels   exactly those of a raster-order flood fill written here (scipy.ndimage.label's numbering: components in ascending order of
           their lowest flat pixel index), and the same n, at both connectivities, with and without wrap; the large checkerboards have
           their labels in closed form.  Cases sit on the seams of the kernel's TILE x TILE tiles.
  stats    count, box, vmax, vmin, argmax, argmin exactly numpy's (the lowest index among equals); each of the four sums within
           count * 2^-52 * sum(|terms|) of a float64 np.bincount, the worst case of a sum in any order
  solve    |x - np.linalg.solve| <= 8 n 2^-52 cond * max|x| per pixel, cond from np.linalg.cond (matrices drawn with cond <= 1e4); the
           same for sqrt(diag(inv)); float32 maps: the same plus 2^-23 for the rounding of the output
Each case runs in the host simulator (*_sim) and on the GPU (*_gpu).
Measured (the prints below), host simulator and MI355X alike: the worst sum error is 0.44 of its bound, the worst solve error 0.12 of its tolerance."""
import numpy as np
import pytest
from pixell_amd import enmap, labels, analysis, _lib
from pixell_amd.wcs import CarWCS

T = labels.TILE

def host(x):
	if isinstance(x, enmap.dmap): x = x.tensor
	return x.detach().cpu().numpy() if hasattr(x, "data_ptr") else np.asarray(x)
def ident(a): return a
def cuda(a):
	import torch
	return torch.as_tensor(np.ascontiguousarray(a), device="cuda")

def flood(mask, connectivity=1, wrap=False):
	"""raster-order flood fill: (labels int32, n)"""
	ny, nx = mask.shape
	lab, n = np.zeros((ny, nx), np.int32), 0
	nb = [(-1, 0), (1, 0), (0, -1), (0, 1)]+([(-1, -1), (-1, 1), (1, -1), (1, 1)] if connectivity == 2 else [])
	for p in np.flatnonzero(mask):
		if lab.flat[p]: continue
		n += 1; lab.flat[p] = n; stack = [divmod(p, nx)]
		while stack:
			cy, cx = stack.pop()
			for dy, dx in nb:
				y, x = cy+dy, cx+dx
				if wrap: x %= nx
				if 0 <= y < ny and 0 <= x < nx and mask[y, x] and not lab[y, x]: lab[y, x] = n; stack.append((y, x))
	return lab, n

_want = {}
def want(name, mask, conn, wrap):
	key = (name, conn, wrap)
	if key not in _want: _want[key] = flood(mask != 0, conn, wrap)
	return _want[key]

def random_mask(fill, shape=(37, 53)):
	return (np.random.default_rng(int(fill*100)).random(shape) < fill).astype(np.uint8)

def serpentine():
	m = np.zeros((4*T+3, 8*T+3), np.uint8)
	m[::2] = 1
	m[1::4, -1] = 1; m[3::4, 0] = 1
	return m

def checkerboard(ny, nx):
	yy, xx = np.mgrid[:ny, :nx]
	return ((yy+xx) % 2 == 0).astype(np.uint8)

def cases():
	c = {}
	for fill in (0.1, 0.4, 0.6, 0.9): c["random %.1f" % fill] = random_mask(fill)
	c["random wide"] = random_mask(0.6, (3*T+5, 4*T+7))      # (near the percolation threshold: components that wander through many tiles)
	c["empty"] = np.zeros((37, 53), np.uint8)
	c["full"] = np.ones((37, 53), np.uint8)
	m = np.zeros((37, 53), np.uint8); m[0, 0] = m[0, -1] = m[-1, 0] = m[-1, -1] = 1; c["corners"] = m
	c["1 x 70"] = random_mask(0.5, (1, 70)); c["70 x 1"] = random_mask(0.5, (70, 1))
	m = np.zeros((1, 71), np.uint8); m[0, ::2] = 1; c["alternating row"] = m
	c["serpentine"] = serpentine()
	m = serpentine(); m[2*T+1, -1] = 0; c["cut serpentine"] = m
	m = np.zeros((3*T+5, 3*T+2), np.uint8); m[:, 3] = 1; m[:, 3+2*T] = 1; m[-1, 3:3+2*T+1] = 1; c["U"] = m
	# arms that start in different tile rows and columns and meet only at the bottom: the arm that starts last in tile order holds the lowest pixel
	m = np.zeros((3*T+5, 6*T+3), np.uint8)
	m[2*T+1:, 2] = 1; m[T+3:, 2*T+5] = 1; m[1:, 5*T+1] = 1; m[-1, 2:5*T+2] = 1; m[5, 5*T+1:] = 1
	c["late root"] = m
	m = np.zeros((2*T, 2*T), np.uint8); m[T-1, T-1] = m[T, T] = 1; c["diagonal"] = m
	m = np.zeros((2*T, 2*T), np.uint8); m[T-1, T] = m[T, T-1] = 1; c["anti-diagonal"] = m
	c["checkerboard"] = checkerboard(2*T, 2*T)
	m = np.zeros((20, 40), np.uint8); m[5:9, :3] = 1; m[5:9, -2:] = 1; m[12, 0] = 1; m[13, -1] = 1; c["wrap blob"] = m
	return c

CASES = cases()

# ---- bodies ---------------------------------------------------------------------------------------------------------------------
def label_body(dev, on_device):
	for name, mask in CASES.items():
		for conn in (1, 2):
			for wrap in (False, True):
				exp, n = want(name, mask, conn, wrap)
				got, gn = labels.label(dev(mask), connectivity=conn, wrap=wrap)
				assert hasattr(got, "data_ptr") == on_device and gn == n, (name, conn, wrap, gn, n)
				got = host(got)
				assert got.dtype == np.int32 and np.array_equal(got, exp), (name, conn, wrap)
	assert want("serpentine", CASES["serpentine"], 1, False)[1] == 1 and want("cut serpentine", CASES["cut serpentine"], 1, False)[1] == 2
	assert want("U", CASES["U"], 1, False)[1] == 1 and want("late root", CASES["late root"], 1, False)[1] == 1
	for name in ("diagonal", "anti-diagonal"): assert want(name, CASES[name], 1, False)[1] == 2 and want(name, CASES[name], 2, False)[1] == 1
	assert want("checkerboard", CASES["checkerboard"], 1, False)[1] == 2*T*T and want("checkerboard", CASES["checkerboard"], 2, False)[1] == 1
	# the blob that straddles column 0 is one label with wrap and two without; the two single pixels touch diagonally across the seam
	assert want("wrap blob", CASES["wrap blob"], 1, True)[1] == 3 and want("wrap blob", CASES["wrap blob"], 1, False)[1] == 4
	assert want("wrap blob", CASES["wrap blob"], 2, True)[1] == 2 and want("wrap blob", CASES["wrap blob"], 2, False)[1] == 4
	# maps: the geometry comes along, and the method is the function
	wcs = CarWCS(cdelt=[0.5, 0.5], crval=[0.0, 0.0], crpix=[27.0, 19.0])
	m = enmap.dmap(dev(CASES["random 0.4"]), wcs) if on_device else enmap.ndmap(CASES["random 0.4"], wcs)
	lab, n = m.label(connectivity=2)
	assert isinstance(lab, enmap.dmap if on_device else enmap.ndmap) and lab.wcs is wcs
	assert np.array_equal(host(lab), want("random 0.4", CASES["random 0.4"], 2, False)[0])

def big_checkerboard_body(dev):
	"""1024 x 2048: 2048 counting blocks and a million labels, both more than one workgroup of the scan takes"""
	ny, nx = 1024, 2048
	cb = checkerboard(ny, nx)
	lab, n = labels.label(dev(cb), connectivity=1)
	exp = np.zeros((ny, nx), np.int32); exp[cb != 0] = np.arange(1, ny*nx//2+1)
	assert n == ny*nx//2 and np.array_equal(host(lab), exp)
	lab2, n2 = labels.label(dev(cb), connectivity=2, wrap=True)
	assert n2 == 1 and np.array_equal(host(lab2), cb.astype(np.int32))
	return cb, exp

def views_body(dev):
	rng = np.random.default_rng(5)
	base = (rng.random((60, 90)) < 0.45)
	full = dev(base.astype(np.uint8))
	for view, ref in ((full.T, base.T), (full[::2, 1::3], base[::2, 1::3]), (dev(base), base), (dev(np.where(base, -0.5, 0.0)), base)):
		got, n = labels.label(view, connectivity=2)
		exp, en = labels.label(dev(np.ascontiguousarray(ref).astype(np.uint8)), connectivity=2)
		assert n == en and np.array_equal(host(got), host(exp)) and np.array_equal(host(exp), flood(ref, 2)[0])

def determinism_body(dev):
	m = dev(CASES["random wide"])
	a, b = labels.label(m, wrap=True), labels.label(m, wrap=True)
	assert a[1] == b[1] and np.array_equal(host(a[0]), host(b[0]))

def errors_body(dev):
	fake = np.lib.stride_tricks.as_strided(np.zeros(1, np.uint8), shape=(65536, 32768), strides=(0, 0))      # 2^31 pixels, one byte
	with pytest.raises(_lib.PxsError): labels.label(fake)
	with pytest.raises(ValueError): labels.label(dev(np.zeros((3, 4), np.uint8)), connectivity=3)
	with pytest.raises(ValueError): labels.label(dev(np.zeros((2, 3, 4), np.uint8)))
	with pytest.raises(_lib.PxsError): labels.stats(dev(np.array([[0, 1, 3]], np.int32)), nlabel=2)
	with pytest.raises(_lib.PxsError): labels.stats(dev(np.array([[0, -1, 1]], np.int32)), nlabel=2)

def expected_stats(lab, n, v, w):
	"""numpy's table of labels 1 .. n: v, w float64 arrays or None"""
	ny, nx = lab.shape
	flat = lab.reshape(-1).astype(np.int64); fg = np.flatnonzero((flat > 0) & (flat <= n)); s = flat[fg]-1
	yy, xx = fg//nx, fg % nx
	e = {"count": np.bincount(s, minlength=n).astype(np.int64)}
	for key, init, arr, op in (("ymin", ny, yy, np.minimum), ("ymax", -1, yy, np.maximum), ("xmin", nx, xx, np.minimum), ("xmax", -1, xx, np.maximum)):
		e[key] = np.full(n, init, np.int32); op.at(e[key], s, arr.astype(np.int32))
	wf = np.ones(fg.size) if w is None else w.reshape(-1)[fg]
	vf = np.zeros(fg.size) if v is None else v.reshape(-1)[fg]
	for key, terms in (("sum_w", wf), ("sum_wy", wf*yy), ("sum_wx", wf*xx), ("sum_v", vf)):
		e[key] = np.bincount(s, weights=terms, minlength=n); e[key+"_abs"] = np.bincount(s, weights=np.abs(terms), minlength=n)
	for key, arg, init, op in (("vmax", "argmax", -np.inf, np.maximum), ("vmin", "argmin", np.inf, np.minimum)):
		ext = np.full(n, init); op.at(ext, s, vf)
		pos = np.full(n, ny*nx, np.int64); hit = vf == ext[s]; np.minimum.at(pos, s[hit], fg[hit])
		none = (e["count"] == 0) | (v is None)
		e[key] = np.where(none, np.nan, ext); e[arg] = np.where(none, -1, pos)
	return e

def check_stats(tag, st, e, on_device):
	worst = 0.0
	for key in ("count", "ymin", "ymax", "xmin", "xmax", "vmax", "vmin", "argmax", "argmin"):
		got = getattr(st, key)
		assert hasattr(got, "data_ptr") == on_device and host(got).dtype == e[key].dtype, (tag, key)
		assert np.array_equal(host(got), e[key], equal_nan=True), (tag, key)
	for key in ("sum_w", "sum_wy", "sum_wx", "sum_v"):
		err, bound = np.abs(host(getattr(st, key))-e[key]), e["count"]*2.0**-52*e[key+"_abs"]
		assert np.all(err <= bound), (tag, key, float(np.max(err-bound)))
		worst = max(worst, float(np.max(err/np.maximum(bound, 1e-300))))
	return worst

def stats_body(dev, on_device, extra=()):
	rng = np.random.default_rng(77)
	worst = 0.0
	maps = [("random 0.4", want("random 0.4", CASES["random 0.4"], 1, False)), ("random 0.1", want("random 0.1", CASES["random 0.1"], 2, False)),
		("random 0.9", want("random 0.9", CASES["random 0.9"], 1, True)), ("checkerboard", want("checkerboard", CASES["checkerboard"], 1, False))]+list(extra)
	for name, (lab, n) in maps:
		for dt in (np.float64, np.float32):
			v, w = rng.standard_normal(lab.shape).astype(dt), rng.random(lab.shape).astype(dt)
			st = labels.stats(dev(lab), values=dev(v), weights=dev(w), nlabel=n+3)      # (three labels that do not occur)
			assert st.nlabel == n+3
			e = expected_stats(lab, n+3, np.float64(v), np.float64(w))
			assert np.all(e["count"][n:] == 0) and np.all(np.isnan(e["vmax"][n:])) and np.all(e["argmin"][n:] == -1) and np.all(e["ymin"][n:] == lab.shape[0])
			worst = max(worst, check_stats(name, st, e, on_device))
		const = np.full(lab.shape, 2.5)      # every pixel of a label ties for its maximum and its minimum
		st = labels.stats(dev(lab), values=dev(const))
		e = expected_stats(lab, n, const, None)
		check_stats(name+" constant", st, e, on_device)
		if n > 0: assert np.array_equal(e["argmax"], e["argmin"]) and np.all(lab.reshape(-1)[e["argmax"]] == np.arange(1, n+1))
		check_stats(name+" bare", labels.stats(dev(lab)), expected_stats(lab, n, None, None), on_device)
	print("worst sum error / bound: %.3g" % worst)
	# grown labels are labels too
	wcs = CarWCS(cdelt=[0.5/60, 0.5/60], crval=[0.0, 0.0], crpix=[27.0, 19.0])
	lab, n = want("random 0.1", CASES["random 0.1"], 2, False)
	lm = enmap.dmap(dev(lab), wcs) if on_device else enmap.ndmap(lab, wcs)
	dist, dom = enmap.labeled_distance_transform(lm, rmax=1.2*0.5/60*np.pi/180)
	grown = host(dom)*(host(dist) <= 1.2*0.5/60*np.pi/180)
	assert grown.dtype == np.int32 and (grown != 0).sum() > (lab != 0).sum()
	v = rng.standard_normal(lab.shape)
	check_stats("grown", labels.stats(dev(grown), values=dev(v), weights=dev(v**2), nlabel=n), expected_stats(grown, n, v, v**2), on_device)

def readers_body(dev, on_device):
	rng = np.random.default_rng(78)
	lab, n = want("random 0.4", CASES["random 0.4"], 1, False)
	v = rng.standard_normal(lab.shape)
	w = v**2
	e, ew = expected_stats(lab, n, v, None), expected_stats(lab, n, None, w)
	index = np.arange(1, n+1)
	nx = lab.shape[1]
	close = lambda a, b: np.allclose(host(a), b, rtol=1e-12, atol=0)
	com = labels.center_of_mass(dev(w), dev(lab), index)
	assert hasattr(com, "data_ptr") == on_device and host(com).shape == (n, 2)
	assert close(com[:, 0], ew["sum_wy"]/ew["sum_w"]) and close(com[:, 1], ew["sum_wx"]/ew["sum_w"])
	assert np.array_equal(host(labels.maximum(dev(v), dev(lab), index)), e["vmax"]) and np.array_equal(host(labels.minimum(dev(v), dev(lab), index)), e["vmin"])
	assert np.array_equal(host(labels.maximum_position(dev(v), dev(lab), index)), np.stack([e["argmax"]//nx, e["argmax"] % nx], -1))
	assert np.array_equal(host(labels.minimum_position(dev(v), dev(lab), index)), np.stack([e["argmin"]//nx, e["argmin"] % nx], -1))
	assert close(labels.sum_labels(dev(v), dev(lab), index), e["sum_v"])
	# a scalar index, an index that is no label, no index, no labels
	assert host(labels.maximum(dev(v), dev(lab), 3)).shape == () and float(host(labels.maximum(dev(v), dev(lab), 3))) == e["vmax"][2]
	assert np.array_equal(host(labels.maximum(dev(v), dev(lab), [2, n+5, 0])), [e["vmax"][1], np.nan, np.nan], equal_nan=True)
	assert np.array_equal(host(labels.sum_labels(dev(v), dev(lab), [n+5, 1]))[:1], [0.0])
	assert float(host(labels.maximum(dev(v), dev(lab)))) == v[lab != 0].max() and float(host(labels.minimum(dev(v)))) == v.min()
	assert np.isclose(float(host(labels.sum_labels(dev(v)))), v.sum(), rtol=1e-12)
	assert tuple(host(labels.maximum_position(dev(v)))) == np.unravel_index(np.argmax(v), v.shape)
	objs = labels.find_objects(dev(lab))
	assert len(objs) == n and all(o == (slice(e["ymin"][i], e["ymax"][i]+1, None), slice(e["xmin"][i], e["xmax"][i]+1, None)) for i, o in enumerate(objs))
	assert labels.find_objects(dev(lab), n+2)[n:] == [None, None]

def spd(rng, n, shape):
	"""random symmetric positive-definite matrices [n, n, ny, nx] with condition numbers up to 1e4 * 0.9"""
	k = np.empty((n, n)+shape)
	for y in range(shape[0]):
		for x in range(shape[1]):
			q, _ = np.linalg.qr(rng.standard_normal((n, n)))
			lam = 10.0**rng.uniform(0, np.log10(9e3), n) if n > 1 else np.array([rng.uniform(1, 5)])
			a = (q*lam) @ q.T
			k[:, :, y, x] = 0.5*(a+a.T)
	return k

def solve_body(dev, on_device):
	rng = np.random.default_rng(79)
	shape = (9, 11)
	wcs = CarWCS(cdelt=[0.5, 0.5], crval=[0.0, 0.0], crpix=[6.0, 5.0])
	worst = 0.0
	for n in (1, 2, 3, 8):
		kappa, rho = spd(rng, n, shape), rng.standard_normal((n,)+shape)
		for dt, floor in ((np.float64, 0.0), (np.float32, 2.0**-23)):
			k, r = kappa.astype(dt), rho.astype(dt)
			km = np.moveaxis(np.float64(k), (0, 1), (-2, -1)); rm = np.moveaxis(np.float64(r), 0, -1)
			cond = np.linalg.cond(km)
			assert cond.max() <= 1e4
			ex = np.linalg.solve(km, rm[..., None])[..., 0]; ed = np.sqrt(np.einsum("...aa->...a", np.linalg.inv(km)))
			sing = (4, 7)
			if n > 1:
				k[:, :, sing[0], sing[1]] = 0      # a singular pixel: NaN there, the neighbours untouched
				k[1, :, 2, 3] = 0; k[:, 1, 2, 3] = 0      # and one with an empty row and column
			flux, dflux = analysis.solve_mapsys(enmap.dmap(dev(k), wcs) if on_device else enmap.ndmap(k, wcs), enmap.dmap(dev(r), wcs) if on_device else enmap.ndmap(r, wcs))
			assert isinstance(flux, enmap.dmap if on_device else enmap.ndmap) and isinstance(dflux, enmap.dmap if on_device else enmap.ndmap)
			assert flux.dtype == dt and dflux.dtype == dt and flux.shape == (n,)+shape and dflux.shape == (n,)+shape
			f, d = np.moveaxis(np.float64(host(flux)), 0, -1), np.moveaxis(np.float64(host(dflux)), 0, -1)
			good = np.ones(shape, bool)
			if n > 1:
				good[sing] = False; good[2, 3] = False
				assert np.all(np.isnan(f[~good])) and np.all(np.isnan(d[~good]))
			tol = 8*n*2.0**-52*cond+floor
			ef = np.abs(f-ex).max(-1)/np.abs(ex).max(-1); edd = np.abs(d-ed).max(-1)/np.abs(ed).max(-1)
			assert np.all(ef[good] <= tol[good]) and np.all(edd[good] <= tol[good]), (n, dt, float((ef/tol)[good].max()), float((edd/tol)[good].max()))
			if dt == np.float64: worst = max(worst, float((ef/tol)[good].max()), float((edd/tol)[good].max()))
	print("solve_mapsys: worst error / tolerance %.3g" % worst)
	with pytest.raises(NotImplementedError):
		analysis.solve_mapsys(dev(np.zeros((9, 9, 2, 2))), dev(np.zeros((9, 2, 2))))
	# the 2-D kappa of the reference's first branch
	k2, r2 = rng.uniform(1, 2, shape), rng.standard_normal(shape)
	f2, d2 = analysis.solve_mapsys(dev(k2), dev(r2))
	assert np.allclose(host(f2), r2/k2, rtol=1e-15) and np.allclose(host(d2), k2**-0.5, rtol=1e-15)

# ---- host simulator -------------------------------------------------------------------------------------------------------------
@pytest.mark.hostsim
def test_label_sim(): label_body(ident, False)
@pytest.mark.hostsim
def test_label_views_sim(): views_body(ident)
@pytest.mark.hostsim
def test_label_determinism_sim(): determinism_body(ident)
@pytest.mark.hostsim
def test_label_errors_sim(): errors_body(ident)
@pytest.mark.hostsim
def test_stats_sim(): stats_body(ident, False)
@pytest.mark.hostsim
def test_readers_sim(): readers_body(ident, False)
@pytest.mark.hostsim
def test_solve_mapsys_sim(): solve_body(ident, False)

# ---- GPU ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_label_gpu(): label_body(cuda, True); label_body(ident, False)
@pytest.mark.gpu
def test_label_big_checkerboard_gpu():
	cb, exp = big_checkerboard_body(cuda)
	stats_body(cuda, True, extra=[("big checkerboard", (exp, cb.size//2))])
@pytest.mark.gpu
def test_label_views_gpu(): views_body(cuda)
@pytest.mark.gpu
def test_label_determinism_gpu(): determinism_body(cuda)
@pytest.mark.gpu
def test_label_errors_gpu(): errors_body(cuda)
@pytest.mark.gpu
def test_stats_gpu(): stats_body(cuda, True); stats_body(ident, False)
@pytest.mark.gpu
def test_readers_gpu(): readers_body(cuda, True); readers_body(ident, False)
@pytest.mark.gpu
def test_solve_mapsys_gpu(): solve_body(cuda, True); solve_body(ident, False)
