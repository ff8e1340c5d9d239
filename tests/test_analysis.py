"""pixell_amd.analysis (NmatConstcov, NmatConstcorr, FinderSimple, MeasurerSimple) against the reference's results on the two-frequency
patches of tests/golden/make_analysis.py (fixtures analysis.npz, analysis_uht.npz): E at dec 0, S at dec -50 deg.
  labels     labels.label(snr >= snlim) of the recorded S/N map equals the recorded scipy.ndimage.label output exactly; the labels our
             finder grows equal the reference's grown labels exactly (the generator asserts that no pixel sits within 1e-6 of the
             threshold and no distance within 4 x the reference's own cellgrid error of finder.grow)
  rho, kappa relative to max|.| of each map: TOL1 = 1e-12, what tests/test_flatsky.py allows one 2-D transform against this reference,
             times the transforms in the chain: 2 for NmatConstcov's rho, 4 for NmatConstcorr's rho (two round trips) and kappa (rpow's
             round trip, then one more); NmatConstcov's kappa has no transform: TOL1
  catalogue  same length and order; ra, dec (relative to one pixel), snr, flux_tot, dflux_tot, flux, dflux (relative to the column's
             maximum) within 10 x 4 TOL1: every column is a linear or ratio-of-linear read-out of those maps with O(1) conditioning
  UHT filters  matched_filter_constcov, _white, _constcorr_lowcorr (with and without high_acc), _constcorr_smoothivar on the flat and the
             curved geometry of the uharm fixtures (analysis_uht.npz), relative to max|.|: 1e-12 (flat, tests/test_flatsky.py) or 1e-11
             (curved, tests/test_uharm.py) per transform, times the transforms of the chain (CHAIN below)
Each case runs in the host simulator (*_sim) and on the GPU (*_gpu).
Measured worst values (the prints below) as fractions of their tolerances, host simulator / MI355X:
  rho, kappa of the noise models 0.00033 / 0.00036 (largest error 1.3e-15, NmatConstcorr's kappa)
  catalogues 0.076 / 0.076 (7.1e-14, the measurer's flux_tot at dec -50)
  UHT filters 0.00096 / 0.00089 (3.8e-14, the curved lowcorr kappa)"""
import os, sys
import numpy as np
import pytest
from pixell_amd import enmap, labels, analysis
from pixell_amd.wcs import CarWCS
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

TOL1 = 1e-12
SCALING = np.array([1.0, 0.8])
GROW = 0.89*np.pi/180/60      # finder.grow of the generator
COLS = ("ra", "dec", "snr", "flux_tot", "dflux_tot", "flux", "dflux")

def analysis_inputs(*a): return _from_generator("analysis_inputs", *a)
def _from_generator(name, *a):
	"""the generator's own input builders (numpy only; the reference is imported by its main() alone)"""
	import importlib.util
	spec = importlib.util.spec_from_file_location("_make_analysis_inputs", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_analysis.py"))
	src = open(spec.origin).read()
	ns = {"np": np, "arcmin": np.pi/180/60}
	start = src.index("def analysis_inputs"); end = src.index("def geo_numbers")
	exec(compile(src[start:end], spec.origin, "exec"), ns)
	return ns[name](*a)

@pytest.fixture(scope="module")
def fx(golden_dir):
	return dict(np.load(os.path.join(golden_dir, "analysis.npz")))

_cases = {}
def case(fx, tag):
	"""geometry and inputs of case E or S (the noise comes from the fixture's map)"""
	if tag not in _cases:
		n = fx[tag+"_geo"]
		shape, wcs = (int(n[0]), int(n[1])), CarWCS(cdelt=n[2:4], crval=n[4:6], crpix=n[6:8])
		l, pos = np.asarray(enmap.modlmap(shape, wcs)), np.asarray(enmap.posmap(shape, wcs))
		inp = analysis_inputs(shape, enmap.pixsize(shape, wcs), l, pos, 2024)
		assert np.max(np.abs(inp["map"]-fx[tag+"_map"])) <= 1e-9*np.max(np.abs(fx[tag+"_map"]))      # (a guard: the same sky as the generator's; the map used is the fixture's)
		inp["map"] = fx[tag+"_map"]
		_cases[tag] = (shape, wcs, inp)
	return _cases[tag]

def host(x):
	if isinstance(x, enmap.dmap): x = x.tensor
	return x.detach().cpu().numpy() if hasattr(x, "data_ptr") else np.asarray(x)
def ident(a): return a
def cuda(a):
	import torch
	return torch.as_tensor(np.ascontiguousarray(a), device="cuda")
def as_map(dev, a, wcs): return enmap.ndmap(np.array(a), wcs) if dev is ident else enmap.dmap(dev(a), wcs)

def rel(got, want): return float(np.max(np.abs(host(got)-want))/np.max(np.abs(want)))

def filters_body(fx, dev, on_device):
	shape, wcs, inp = case(fx, "E")
	m = lambda a: as_map(dev, a, wcs)
	kind = enmap.dmap if on_device else enmap.ndmap
	worst = 0.0
	rho, kappa = analysis.NmatConstcov(m(inp["iN"]), m(np.ones(shape))).matched_filter(m(inp["map"]), m(inp["beam"]))
	assert isinstance(rho, kind) and isinstance(kappa, kind) and rho.shape == (2,)+shape and kappa.shape == (2, 2)+shape
	for name, err, tol in (("constcov rho", rel(rho, fx["E_cov_rho"]), 2*TOL1), ("constcov kappa", rel(kappa, np.broadcast_to(fx["E_cov_kappa"], (2, 2)+shape)), TOL1)):
		print("%s: %.3g (tol %.3g)" % (name, err, tol)); worst = max(worst, err/tol)
		assert err <= tol, name
	rho, kappa = analysis.NmatConstcorr(m(inp["iN"]), m(inp["ivar"])).matched_filter(m(inp["map"]), m(inp["beam"]))
	assert isinstance(rho, kind) and isinstance(kappa, kind)
	k = host(kappa)
	for name, err, tol in (("constcorr rho", rel(rho, fx["E_corr_rho"]), 4*TOL1), ("constcorr kappa", rel(k[[0, 0, 1, 1], [0, 1, 0, 1]], fx["E_corr_kappa"][[0, 1, 1, 2]]), 4*TOL1)):
		print("%s: %.3g (tol %.3g)" % (name, err, tol)); worst = max(worst, err/tol)
		assert err <= tol, name
	print("worst rho / kappa error over its tolerance: %.3g" % worst)

def uht_inputs(*a): return _from_generator("uht_inputs", *a)
TOL_UHT = {"F": 1e-12, "C": 1e-11}      # one transform against this reference: tests/test_flatsky.py (flat), tests/test_uharm.py (curved)
# transforms in the chain of (rho, kappa); hprof_rpow is two, sum_hprof none (counted as one); high_acc divides by a chain of six more
CHAIN = {"constcov": (2, 1), "white": (2, 4), "lowcorr": (4, 4), "lowcorr_acc": (4, 10), "smoothivar": (2, 1)}

def uht_body(golden_dir, dev, on_device):
	from pixell_amd import uharm
	fu = dict(np.load(os.path.join(golden_dir, "analysis_uht.npz")))
	worst = 0.0
	for tag, mode, lmax in (("F", "flat", None), ("C", "curved", 24)):
		n = fu[tag+"_geo"]
		shape, wcs = (int(n[0]), int(n[1])), CarWCS(cdelt=n[2:4], crval=n[4:6], crpix=n[6:8])
		u = uharm.UHT(shape, wcs, mode=mode, lmax=lmax)
		B, iC = u.lprof2hprof(fu[tag+"_lbeam"]), u.lprof2hprof(fu[tag+"_linv"])
		m, ivar = as_map(dev, fu[tag+"_map"], wcs), as_map(dev, fu[tag+"_ivar"], wcs)
		res = {"constcov": analysis.matched_filter_constcov(m, B, iC, u), "white": analysis.matched_filter_white(m, B, ivar, u),
			"lowcorr": analysis.matched_filter_constcorr_lowcorr(m, B, ivar, iC, u), "lowcorr_acc": analysis.matched_filter_constcorr_lowcorr(m, B, ivar, iC, u, high_acc=True),
			"smoothivar": analysis.matched_filter_constcorr_smoothivar(m, B, ivar, iC, u)}
		for name, (rho, kappa) in res.items():
			assert isinstance(rho, enmap.dmap if on_device else enmap.ndmap)
			for what, got, ntr in (("rho", rho, CHAIN[name][0]), ("kappa", kappa, CHAIN[name][1])):
				want = fu["%s_%s_%s" % (tag, name, what)]
				assert np.shape(host(got)) == want.shape, (tag, name, what)
				err, tol = rel(got, want), ntr*TOL_UHT[tag]
				print("%s %s %s: %.3g (tol %.3g)" % (tag, name, what, err, tol)); worst = max(worst, err/tol)
				assert err <= tol, (tag, name, what, err)
	print("worst UHT filter error over its tolerance: %.3g" % worst)

def labels_body(fx, dev, on_device):
	for tag in ("E", "S"):
		snr, snlim = fx[tag+"_snr"], float(fx[tag+"_snlim"])
		lab, n = labels.label(dev(snr >= snlim))
		assert n == len(fx[tag+"_cat_snr"]) and np.array_equal(host(lab), fx[tag+"_labels"])
		shape, wcs, inp = case(fx, tag)
		dists, dom = enmap.labeled_distance_transform(as_map(dev, fx[tag+"_labels"], wcs), rmax=20*analysis.arcmin)
		grown = host(dom)*(host(dists) <= GROW)
		assert np.array_equal(grown, fx[tag+"_grown"]) and (grown != 0).sum() > (fx[tag+"_labels"] != 0).sum()

def check_cat(tag, cat, fx, prefix, wcs):
	tol = 10*4*TOL1
	pix = abs(wcs.wcs.cdelt[1])*np.pi/180
	worst = 0.0
	assert len(cat) == len(fx[prefix+"snr"]), tag
	for key in COLS:
		got, want = np.asarray(cat[key]), fx[prefix+key]
		assert got.shape == want.shape and got.dtype == np.float64, (tag, key)
		err = float(np.max(np.abs(got-want))/(pix if key in ("ra", "dec") else np.max(np.abs(want))))
		print("%s %s: %.3g (tol %.3g)" % (tag, key, err, tol)); worst = max(worst, err/tol)
		assert err <= tol, (tag, key, err)
	return worst

def finder_body(fx, dev, on_device):
	worst = 0.0
	for tag in ("E", "S"):
		shape, wcs, inp = case(fx, tag)
		m = lambda a: as_map(dev, a, wcs)
		nmat = analysis.NmatConstcorr(m(inp["iN"]), m(inp["ivar"]))
		finder = analysis.FinderSimple(nmat, m(inp["beam"]), scaling=SCALING); finder.grow = GROW
		res = finder(m(inp["map"]), snmin=5.0)
		assert isinstance(res.snr, enmap.dmap if on_device else enmap.ndmap) and isinstance(res.cat, np.recarray)
		assert res.snlim == float(fx[tag+"_snlim"]) and rel(res.snr, fx[tag+"_snr"]) <= 4*TOL1
		assert np.all(np.diff(res.cat.snr) <= 0)
		worst = max(worst, check_cat(tag+" finder", res.cat, fx, tag+"_cat_", wcs))
		icat = res.cat.copy(); icat.ra = fx[tag+"_mcat_ra"]; icat.dec = fx[tag+"_mcat_dec"]
		mres = analysis.MeasurerSimple(nmat, m(inp["beam"]), scaling=SCALING)(m(inp["map"]), icat)
		worst = max(worst, check_cat(tag+" measurer", mres.cat, fx, tag+"_mcat_", wcs))
		# nothing above the threshold: an empty catalogue of the same dtype
		none = analysis.FinderSimple(nmat, m(inp["beam"]), scaling=SCALING)(m(inp["map"]), snmin=1e3)
		assert len(none.cat) == 0 and none.cat.dtype == res.cat.dtype and isinstance(none.cat, np.recarray) and none.snlim == 1e3
		assert [(n, none.cat.dtype[n].shape) for n in none.cat.dtype.names] == [(k, ()) for k in COLS[:5]]+[("flux", (2,)), ("dflux", (2,))]
	print("worst catalogue error over its tolerance: %.3g" % worst)

def agree_body(fx):
	"""host maps in, host maps out; dmaps in, dmaps out; the two agree"""
	shape, wcs, inp = case(fx, "E")
	res = {}
	for dev in (ident, cuda):
		m = lambda a: as_map(dev, a, wcs)
		res[dev] = analysis.FinderSimple(analysis.NmatConstcorr(m(inp["iN"]), m(inp["ivar"])), m(inp["beam"]), scaling=SCALING)(m(inp["map"]))
	assert isinstance(res[ident].snr, enmap.ndmap) and isinstance(res[cuda].snr, enmap.dmap)
	assert rel(res[cuda].snr, host(res[ident].snr)) <= 4*TOL1 and len(res[cuda].cat) == len(res[ident].cat)
	for key in COLS: assert np.allclose(res[cuda].cat[key], res[ident].cat[key], rtol=0, atol=40*TOL1*np.max(np.abs(res[ident].cat[key])))

def helpers_body(dev):
	wcs = CarWCS(cdelt=[-0.5/60, 0.5/60], crval=[0.0, 0.0], crpix=[20.0, 10.0])
	rng = np.random.default_rng(3)
	k = rng.uniform(0.5, 2, (2, 2, 8, 9)); k[0, 0, 3, 3] = 1e-9
	s = host(analysis.sanitize_kappa(as_map(dev, k, wcs)))
	want = k.copy()
	for i in range(2): want[i, i] = np.maximum(k[i, i], k[i, i].max()*1e-4)
	assert np.array_equal(s, want)
	mat, vec = rng.standard_normal((3, 2, 8, 9)), rng.standard_normal((2, 8, 9))
	assert np.allclose(host(enmap.map_mul(as_map(dev, np.broadcast_to(mat[None], (1,)+mat.shape), wcs), as_map(dev, vec, wcs))), np.einsum("abyx,byx->ayx", mat, vec)[None], rtol=1e-14)
	assert np.array_equal(host(enmap.map_mul(as_map(dev, vec, wcs), as_map(dev, vec, wcs))), vec*vec)
	fr, fk = analysis.get_flat_sky_correction(np.array([0.9, 1.0]))
	assert np.allclose(fr, (0.5*(1+np.array([0.81, 1.0])))**-0.5) and np.allclose(fk, [1/0.9, 1.0])
	lab = host(analysis.make_circle_labels((30, 40), wcs, np.array([[5, 20], [7, 30]]), r=2*analysis.arcmin))
	assert lab.dtype == np.int32 and lab[5, 7] == 1 and lab[20, 30] == 2 and set(np.unique(lab)) == {0, 1, 2} and 30 < (lab == 1).sum() < 60

@pytest.mark.hostsim
def test_filters_sim(fx): filters_body(fx, ident, False)
@pytest.mark.hostsim
def test_labels_of_the_finder_sim(fx): labels_body(fx, ident, False)
@pytest.mark.hostsim
def test_finder_and_measurer_sim(fx): finder_body(fx, ident, False)
@pytest.mark.hostsim
def test_helpers_sim(): helpers_body(ident)
@pytest.mark.hostsim
def test_uht_filters_sim(golden_dir): uht_body(golden_dir, ident, False)

@pytest.mark.gpu
def test_filters_gpu(fx): filters_body(fx, cuda, True); filters_body(fx, ident, False)
@pytest.mark.gpu
def test_labels_of_the_finder_gpu(fx): labels_body(fx, cuda, True); labels_body(fx, ident, False)
@pytest.mark.gpu
def test_finder_and_measurer_gpu(fx): finder_body(fx, cuda, True); finder_body(fx, ident, False)
@pytest.mark.gpu
def test_host_and_device_agree_gpu(fx): agree_body(fx)
@pytest.mark.gpu
def test_uht_filters_gpu(golden_dir): uht_body(golden_dir, cuda, True); uht_body(golden_dir, ident, False)
@pytest.mark.gpu
def test_helpers_gpu(): helpers_body(cuda); helpers_body(ident)
