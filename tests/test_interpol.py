"""pixell_amd.interpol (spline_filter, interpol, interpolator) and enmap.at / enmap.project, against the reference's utils.interpol, enmap.at and
whole-map utils.interpol(map, map.sky2pix(posmap(oshape, owcs))) of tests/golden/make_interpol.py (fixture interpol.npz), against scipy
itself, and against the dense solve that defines the coefficients.

Tolerance, per case (f the map, c the array the taps read: the dense coefficients at order 3, f at order 1; ny, nx the map's shape):
    tol = 4 E_ref max|f| + 64 2^-52 max|c| + 8 2^-52 max(ny, nx) max|dc|
  E_ref     the reference's own error: the deviation of scipy's filtered array from the float64 dense solution of B c = f, relative to max|f|.
            Against the fixture: the fixture's E_ref (3.55e-15).  Against scipy live: that, or the same deviation measured on the case at hand
            where it is larger: scipy's start value under "nearest" is off by about 0.268^(2n) on a line of n samples (4e-4 at n = 2, 4e-12
            at n = 9, see make_interpol.py), which is the reference's error and not the device's; the comparison with the dense solve of the
            same case carries the fixture's E_ref and is the sharp one
  2nd term  a 16-term sum whose weights each carry a few roundings
  3rd term  a pixel coordinate that differs by a few ulp of its magnitude, times the largest difference dc of neighbouring coefficients
  float32 results (orders 0, 1 on float32 maps) may in addition round the other way: + 2^-24 max|f|.  Order 0 is exact.
Order 3 on a float32 map: the reference rounds the coefficients to float32 and returns float32; the device keeps float64.
The fixture's two maps hold the same numbers, so the float64 map's values are the expected ones.

Each body runs in the host simulator (*_sim, here) and on the GPU (*_gpu).  Worst error / tol over the cases of each body, as the tests print them:
                      host simulator      MI355X
  small shapes        0.250             0.250   ((2, 2) "nearest" order 3 against scipy)
  fixture A, B        0.220             0.220   (at, A, float64, order 1, "mirror")
  chunked case        0.049             0.056   (the coefficients)
  project             0.282             0.282   (P2, order 1)
"""
import os
import numpy as np
import pytest
import scipy.ndimage as ndi
from pixell_amd import enmap, interpol
from pixell_amd.wcs import CarWCS

EPS = 2.0**-52
BORDERS = ("nearest", "mirror", "constant", "wrap", "grid-wrap")
REF_BORDERS = ("nearest", "wrap", "mirror", "constant")
ORDERS = (0, 1, 3)
EXTENSION = {"nearest": "reflect", "mirror": "mirror", "constant": "mirror", "wrap": "mirror", "grid-wrap": "periodic"}

@pytest.fixture(scope="module")
def fx(golden_dir):
	return dict(np.load(os.path.join(golden_dir, "interpol.npz")))

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

# ---- the definition of the coefficients, and the tolerance --------------------------------------------------------------------------
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

_dense = {}
def dense_coefficients(f, border, key=None):
	"""the float64 solution of B c = f along the last two axes of f (kept per key: the fixture's maps are solved once)"""
	rule = EXTENSION[border]
	if key is not None and (key, rule) in _dense: return _dense[(key, rule)]
	f = np.asarray(f, np.float64)
	c = np.linalg.solve(collocation(f.shape[-2], rule), np.moveaxis(f, -2, 0).reshape(f.shape[-2], -1)).reshape((f.shape[-2],)+f.shape[:-2]+f.shape[-1:])
	c = np.moveaxis(c, 0, -2)
	c = np.linalg.solve(collocation(f.shape[-1], rule), np.moveaxis(c, -1, 0).reshape(f.shape[-1], -1)).reshape((f.shape[-1],)+f.shape[:-1])
	c = np.ascontiguousarray(np.moveaxis(c, 0, -1))
	if key is not None: _dense[(key, rule)] = c
	return c

def tol_of(eref, f, c, f32_out=False):
	f, c = np.asarray(f, np.float64), np.asarray(c, np.float64)
	dc = max([float(np.max(np.abs(np.diff(c, axis=a)))) for a in (-2, -1) if c.shape[a] > 1]+[0.0])
	t = 4*eref*np.max(np.abs(f))+64*EPS*np.max(np.abs(c))+8*EPS*max(c.shape[-2:])*dc
	return t+(2.0**-24*np.max(np.abs(f)) if f32_out else 0.0)

def scipy_interpol(arr, pts, order, border, cval):
	"""what the reference's SplineInterpolator does with scipy (utils.py:696-720), in float64"""
	arr = np.asarray(arr)
	flat = arr.reshape((-1,)+arr.shape[-2:])
	if order > 1: flat = np.array([ndi.spline_filter(np.float64(a), order=order, mode=border) for a in flat])
	res = np.array([ndi.map_coordinates(a, pts.reshape(2, -1), order=order, mode=border, cval=cval, prefilter=False) for a in flat])
	return res.reshape(arr.shape[:-2]+pts.shape[1:])

def safe_points(rng, shape, n):
	"""n points [{y,x}, n]: a third inside, the rest up to 2.5 map sizes outside, none within 1e-6 pixel of a rounding tie or of 0 or n - 1"""
	ny, nx = shape
	pts = np.array([np.concatenate([rng.uniform(0, max(ny-1, 0.5), n//3), rng.uniform(-2.5*ny, 3.5*ny, n-n//3)]),
		np.concatenate([rng.uniform(0, max(nx-1, 0.5), n//3), rng.uniform(-2.5*nx, 3.5*nx, n-n//3)])])
	assert np.abs(pts+0.5-np.round(pts+0.5)).min() > 1e-6
	assert min(np.abs(pts[a]-v).min() for a in (0, 1) for v in (0, shape[a]-1)) > 1e-6
	return pts

class Worst:
	"""the largest error / tol of a body's cases"""
	def __init__(self, name): self.name, self.ratio, self.where = name, 0.0, ""
	def check(self, tag, got, want, tol):
		got, want = np.float64(host(got)), np.float64(want)
		assert got.shape == want.shape, (tag, got.shape, want.shape)
		err = float(np.max(np.abs(got-want))) if got.size else 0.0
		print("%s: worst error %.3g (tol %.3g)" % (tag, err, tol))
		if tol > 0 and err/tol > self.ratio: self.ratio, self.where = err/tol, tag
		assert err <= tol, tag
	def report(self): print("%s: worst error / tol = %.3f (%s)" % (self.name, self.ratio, self.where))

# ---- bodies ---------------------------------------------------------------------------------------------------------------------
def small_body(fx, dev, on_device):
	"""lines shorter than the halo: every border and order against scipy live and against the dense solve"""
	eref = float(fx["E_ref"]); W = Worst("small shapes")
	rng = np.random.default_rng(33)
	one = interpol.spline_filter(dev(np.array([[1.2345678901234567]])), border="mirror")
	assert host(one).shape == (1, 1) and host(one)[0, 0] == 1.2345678901234567      # n = 1: the coefficient is the value
	for shape in ((1, 7), (7, 1), (2, 2), (3, 5), (31, 33)):
		f = rng.standard_normal((2,)+shape)
		pts = safe_points(rng, shape, 60)
		for border in BORDERS:
			dense = dense_coefficients(f, border)
			live = np.array([ndi.spline_filter(a, order=3, mode=border) for a in f])
			ecase = max(eref, float(np.max(np.abs(live-dense))/np.max(np.abs(f))))
			c = interpol.spline_filter(dev(f), border=border)
			assert hasattr(c, "data_ptr") == on_device and host(c).dtype == np.float64
			W.check("%s %s coefficients, dense" % (shape, border), c, dense, 4*eref*np.max(np.abs(f))+64*EPS*np.max(np.abs(dense)))
			for order in ORDERS:
				tag = "%s %s order %d" % (shape, border, order)
				got = interpol.interpol(dev(f), dev(pts), order=order, border=border, cval=0.7)
				assert host(got).shape == (2, 60) and host(got).dtype == np.float64
				if order == 0: assert np.array_equal(host(got), scipy_interpol(f, pts, 0, border, 0.7)), tag
				elif order == 1: W.check(tag+", scipy", got, scipy_interpol(f, pts, 1, border, 0.7), tol_of(eref, f, f))
				else:
					W.check(tag+", scipy", got, scipy_interpol(f, pts, 3, border, 0.7), tol_of(ecase, f, dense))
					want = np.array([ndi.map_coordinates(a, pts, order=3, mode=border, cval=0.7, prefilter=False) for a in dense])
					W.check(tag+", dense", got, want, tol_of(eref, f, dense))
	W.report()

def fixture_body(fx, dev, on_device):
	"""utils.interpol and enmap.at of the reference on the geometries A and B"""
	eref, cval = float(fx["E_ref"]), float(fx["cval"]); W = Worst("fixture A, B")
	for g in ("A", "B"):
		shape, wcs = geometry(fx[g+"_geo"], (2,))
		pix, pos = fx[g+"_pix"], fx[g+"_pos"]
		for dt, tag in ((np.float64, "f8"), (np.float32, "f4")):
			f = fx[g+"_map"].astype(dt)
			m = as_map(dev, f, wcs)
			for order in ORDERS:
				for border in REF_BORDERS:
					key = "%s_%s_%d_%s" % (g, "f8" if order == 3 else tag, order, border)
					odt = np.float64 if order == 3 else dt
					c = dense_coefficients(f, border, key=g) if order == 3 else f
					tol = 0.0 if order == 0 else tol_of(eref, f, c, f32_out=odt == np.float32)
					vi = interpol.interpol(dev(f), dev(pix), order=order, border=border, cval=cval)
					va = enmap.at(m, dev(pos), order=order, border=border, cval=cval)
					for v in (vi, va): assert hasattr(v, "data_ptr") == on_device and host(v).dtype == odt
					W.check("ip %s %s order %d %s" % (g, tag, order, border), vi, fx["ip_"+key], tol)
					W.check("at %s %s order %d %s" % (g, tag, order, border), va, fx["at_"+key], tol)
	W.report()

def chunk_body(fx, dev, on_device):
	"""(2 cy + 37) x (2 cx + 53) with [3] leading maps: full chunks, a chunk boundary and a remainder on both axes; expected values from scipy live"""
	eref = float(fx["E_ref"]); W = Worst("chunked case")
	cy, cx = interpol.CHUNK
	shape = (2*cy+37, 2*cx+53)
	rng = np.random.default_rng(77)
	f64 = rng.integers(-2**20, 2**20, (3,)+shape).astype(np.float64)/2**20      # (the float32 map holds the same numbers)
	pts = safe_points(rng, shape, 3000)
	pts[:, :600] = np.array([rng.choice([cy, 2*cy], 600)+rng.uniform(-3, 3, 600), rng.choice([cx, 2*cx], 600)+rng.uniform(-3, 3, 600)])      # around the chunk boundaries
	assert np.abs(pts+0.5-np.round(pts+0.5)).min() > 1e-6
	for border in ("mirror", "nearest", "grid-wrap"):
		live = np.array([ndi.spline_filter(a, order=3, mode=border) for a in f64])
		dense = dense_coefficients(f64, border)
		ecase = max(eref, float(np.max(np.abs(live-dense))/np.max(np.abs(f64))))
		want = np.array([ndi.map_coordinates(a, pts, order=3, mode=border, prefilter=False) for a in live])
		for dt in (np.float32, np.float64):
			f = f64.astype(dt)
			c = interpol.spline_filter(dev(f), border=border)
			assert host(c).dtype == np.float64 and host(c).shape == f.shape
			W.check("%s %s coefficients" % (border, np.dtype(dt).name), c, live, 4*ecase*np.max(np.abs(f))+64*EPS*np.max(np.abs(live)))
			W.check("%s %s values" % (border, np.dtype(dt).name), interpol.interpol(dev(f), dev(pts), border=border), want, tol_of(ecase, f, live))
	W.report()

def api_body(fx, dev, on_device, monkeypatch):
	eref, cval = float(fx["E_ref"]), float(fx["cval"])
	shape, wcs = geometry(fx["B_geo"], (2,))
	f, pos = fx["B_map"], fx["B_pos"]
	m = as_map(dev, f, wcs)
	tol = tol_of(eref, f, dense_coefficients(f, "constant", key="B"))
	want = fx["at_B_f8_3_constant"]
	kind = (lambda v: hasattr(v, "data_ptr")) if on_device else (lambda v: isinstance(v, np.ndarray))
	# unit "pix": the same values from the pixel coordinates of the positions; the method form; a single position
	pix = enmap.sky2pix(shape, wcs, pos)
	for a, n in enumerate(shape[-2:]): pix[a] = n/2.0+(pix[a]-n/2.0+90.0) % 180.0-90.0      # (the rewind of sky2pix(safe=True): |360/cdelt| = 180 pixels on both axes)
	vp = enmap.at(m, dev(pix), border="constant", cval=cval, unit="pix")
	assert kind(vp) and np.max(np.abs(host(vp)-want)) <= tol
	assert np.array_equal(host(m.at(dev(pos), border="constant", cval=cval)), host(enmap.at(m, dev(pos), cval=cval)))
	v1 = enmap.at(m, dev(pos[:, 3]), cval=cval)
	assert host(v1).shape == (2,) and np.max(np.abs(host(v1)-want[:, 3])) <= tol
	v2 = enmap.at(m, dev(pos.reshape(2, 2, -1)), cval=cval)
	assert host(v2).shape == (2, 2, pos.shape[1]//2) and np.array_equal(host(v2).reshape(2, -1), host(enmap.at(m, dev(pos), cval=cval)))
	with pytest.raises(ValueError): enmap.at(m, dev(pos), unit="deg")
	# safe: positions a turn of the sky off land where they belong; without it they are outside the map
	off = pos+np.array([[0.0], [2*np.pi]])
	assert np.max(np.abs(host(enmap.at(m, dev(off), cval=cval))-want)) <= tol
	unsafe = host(enmap.at(m, dev(off), cval=cval, safe=False))
	xoff = enmap.sky2pix(shape, wcs, off)[1]
	assert np.all(unsafe[:, (xoff < -1e-6) | (xoff > 179+1e-6)] == cval) and np.any(unsafe != cval)
	# ip= reuse: no filter launch after the interpolator is made, and the same values bit for bit
	calls = []
	real = interpol._filter
	monkeypatch.setattr(interpol, "_filter", lambda d, border: (calls.append(border), real(d, border))[1])
	ip = interpol.interpolator(m, npre=1, order=3, border="constant", cval=cval)
	assert calls == ["constant"] and ip.prefiltered and ip.order == 3 and ip.npre == 1
	a1 = enmap.at(m, dev(pos), ip=ip); a2 = enmap.at(m, dev(pos), ip=ip); a3 = interpol.interpol(m, dev(pix), ip=ip)
	assert calls == ["constant"] and np.array_equal(host(a1), host(a2)) and np.max(np.abs(host(a1)-want)) <= tol and np.max(np.abs(host(a3)-want)) <= tol
	assert np.array_equal(host(a1), host(enmap.at(m, dev(pos), cval=cval))) and len(calls) == 2
	# out=
	o = dev(np.full(want.shape, 7.0))
	assert interpol.interpol(dev(f), dev(pix), out=o, border="constant", cval=cval) is o and np.array_equal(host(o), host(a3))
	with pytest.raises(ValueError): interpol.interpol(dev(f), dev(pix), out=dev(np.zeros(want.shape, np.float32)))
	with pytest.raises(ValueError): interpol.interpol(dev(f), dev(pix), out=dev(np.zeros((2, 3))))
	# kinds: numpy in, numpy out; tensors or a dmap in, tensors out
	assert kind(interpol.interpol(dev(f), dev(pix))) and kind(interpol.spline_filter(dev(f)))
	assert isinstance(interpol.spline_filter(m), enmap.dmap if on_device else enmap.ndmap)
	if on_device:
		assert isinstance(interpol.interpol(f, pix), np.ndarray) and isinstance(enmap.at(enmap.ndmap(f, wcs), pos), np.ndarray)
		assert hasattr(interpol.interpol(f, dev(pix)), "data_ptr") and hasattr(interpol.interpol(dev(f), pix), "data_ptr")
		assert np.array_equal(interpol.interpol(f, pix, border="constant", cval=cval), host(a3))
	# the mode aliases, orders 0 and 1 of spline_filter
	for mode, order in (("nn", 0), ("nearest", 0), ("lin", 1), ("linear", 1), ("cub", 3), ("cubic", 3)):
		assert np.array_equal(host(interpol.interpol(dev(f), dev(pix), mode=mode, order=5)), host(interpol.interpol(dev(f), dev(pix), order=order)))
	assert np.array_equal(host(interpol.spline_filter(dev(f.astype(np.float32)), order=1)), f) and host(interpol.spline_filter(dev(f), order=0)).dtype == np.float64
	# integer maps at order 0: their own dtype, exactly; at order 1 they are float64
	rng = np.random.default_rng(5)
	for dt, hi in ((np.uint8, 256), (np.int32, 2**31-1)):
		im = rng.integers(0, hi, (2, 90, 180)).astype(dt)
		for border in BORDERS:
			got = interpol.interpol(dev(im), dev(fx["B_pix"]), order=0, border=border, cval=3)
			assert host(got).dtype == dt and np.array_equal(host(got), scipy_interpol(im, fx["B_pix"], 0, border, 3)), (dt, border)
		assert host(enmap.at(as_map(dev, im, wcs), dev(pos), mode="nn")).dtype == dt
		assert host(interpol.interpol(dev(im), dev(fx["B_pix"]), order=1)).dtype == np.float64
	# what is refused
	with pytest.raises(ValueError): interpol.interpol(dev(f), dev(pix), border="reflect")
	with pytest.raises(ValueError): interpol.interpol(dev(f), dev(pix), mode="quintic")
	with pytest.raises(ValueError): interpol.spline_filter(dev(f), border="zero")
	for order in (2, 4, 5):
		with pytest.raises(NotImplementedError): interpol.interpol(dev(f), dev(pix), order=order)
		with pytest.raises(NotImplementedError): interpol.spline_filter(dev(f), order=order)
	with pytest.raises(NotImplementedError): interpol.interpol(dev(f), dev(pix), mode="fourier")
	with pytest.raises(NotImplementedError): enmap.at(m, dev(pos), mode="fft")
	with pytest.raises(NotImplementedError): interpol.interpol(dev(f), dev(np.zeros((3, 5))))      # three interpolated axes
	tilted = CarWCS(cdelt=wcs.wcs.cdelt, crval=[wcs.wcs.crval[0], 10.0], crpix=wcs.wcs.crpix)
	with pytest.raises(NotImplementedError): enmap.at(as_map(dev, f, tilted), dev(pos))
	with pytest.raises(NotImplementedError): enmap.project(as_map(dev, f, tilted), shape, wcs)
	with pytest.raises(NotImplementedError): enmap.project(m, shape, tilted)

def project_body(fx, dev, on_device):
	eref, cval = float(fx["E_ref"]), float(fx["cval"]); W = Worst("project")
	mapkind = enmap.dmap if on_device else enmap.ndmap
	cases = (("B", "P1", "constant", 3), ("B", "P1", "grid-wrap", 3), ("A", "P2", "constant", 3), ("A", "P2", "constant", 1), ("A", "P4", "constant", 3))
	for g, p, border, order in cases:
		shape, wcs = geometry(fx[g+"_geo"], (2,))
		oshape, owcs = geometry(fx[p+"_geo"])
		f = fx[g+"_map"]
		m = as_map(dev, f, wcs)
		want = fx["%s_%s_%d" % (p, border, order)]
		c = dense_coefficients(f, border, key=g) if order == 3 else f
		res = enmap.project(m, oshape, owcs, order=order, border=border, cval=cval)
		assert isinstance(res, mapkind) and res.shape == (2,)+oshape and res.dtype == np.float64 and res.wcs is owcs
		W.check("%s %s order %d" % (p, border, order), res, want, tol_of(eref, f, c))
		if p == "P1" and border == "constant":
			assert np.any(host(res) == cval) and np.any(host(res) != cval)
			assert np.array_equal(host(m.project(oshape, owcs, cval=cval)), host(res))
	print("the reference's blockwise project (for the record): off its own whole-map values by %.3g" % np.max(np.abs(np.float64(fx["P1_block"])-fx["P1_constant_3"])))
	# a pixel-compatible geometry: the map's own pixels
	W.check("P4 against the map's pixels", enmap.project(as_map(dev, fx["A_map"], geometry(fx["A_geo"])[1]), *geometry(fx["P4_geo"])), fx["A_map"][:, 10:30, 20:50],
		tol_of(eref, fx["A_map"], dense_coefficients(fx["A_map"], "constant", key="A")))
	# an equal geometry: an exact copy, of the map's own dtype
	shape, wcs = geometry(fx["A_geo"], (2,))
	for dt in (np.float32, np.float64):
		m = as_map(dev, fx["A_map"].astype(dt), wcs)
		same = enmap.project(m, shape, CarWCS(cdelt=wcs.wcs.cdelt, crval=wcs.wcs.crval, crpix=wcs.wcs.crpix))
		assert isinstance(same, mapkind) and same is not m and same.dtype == dt and np.array_equal(host(same), fx["A_map"])
	W.report()

# ---- host simulator -------------------------------------------------------------------------------------------------------------
@pytest.mark.hostsim
def test_small_shapes_sim(fx): small_body(fx, ident, False)
@pytest.mark.hostsim
def test_fixture_interpol_and_at_sim(fx): fixture_body(fx, ident, False)
@pytest.mark.hostsim
def test_chunked_filter_sim(fx): chunk_body(fx, ident, False)
@pytest.mark.hostsim
def test_api_sim(fx, monkeypatch): api_body(fx, ident, False, monkeypatch)
@pytest.mark.hostsim
def test_project_sim(fx): project_body(fx, ident, False)

# ---- GPU ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_small_shapes_gpu(fx): small_body(fx, cuda, True)
@pytest.mark.gpu
def test_fixture_interpol_and_at_gpu(fx): fixture_body(fx, cuda, True)
@pytest.mark.gpu
def test_chunked_filter_gpu(fx): chunk_body(fx, cuda, True)
@pytest.mark.gpu
def test_api_gpu(fx, monkeypatch): api_body(fx, cuda, True, monkeypatch)
@pytest.mark.gpu
def test_project_gpu(fx): project_body(fx, cuda, True)
