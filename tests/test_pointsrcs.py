"""pixell_amd.pointsrcs (sim_objects, its transpose, radial_sum / radial_bin, sim_srcs) and enmap.apply_window, against the float64
model of tests/golden/make_pointsrcs.py (fixtures pointsrcs.npz, pointsrcs_window.npz).  The bounds are in units of ulp = 2^-23 and
come from the float32 formats, not from what the kernels give:
  distance        |map * 1 deg - r64| <= 16 ulp max(r64, pixel size)     (a float32 numpy evaluation of the same formula: 3 ulp; the
                  reference's Vincenty form in float32: hundreds of ulp at these separations, so a port of it fails here)
  forward         max |out - expected| <= 64 ulp max |expected|          (float32 numpy: 0.7 ulp on A, 12 ulp on B)
  transpose       per object <= 64 ulp sum_p |P m|; adjointness to the worst-case float32 summation bound 4 n 2^-24 sum |a P m|
  radial sums     <= 4 n_k 2^-24 sum |m| over the bin's pixels, on the (object, bin) pairs outside the generator's guard band
Each case runs in the host simulator (*_sim, here) and on the GPU (*_gpu)."""
import os
import numpy as np
import pytest
from pixell_amd import enmap, pointsrcs
from pixell_amd.wcs import CarWCS, separable_geometry

ULP = 2.0**-23
arcmin = np.pi/180/60

@pytest.fixture(scope="module")
def fx(golden_dir):
	d = dict(np.load(os.path.join(golden_dir, "pointsrcs.npz")))
	d.update(np.load(os.path.join(golden_dir, "pointsrcs_window.npz")))
	return d

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

# ---- the model, as in the generator -----------------------------------------------------------------------------------------------
def dist64(pdec, pra, odec, ora):
	pdec, pra, odec, ora = np.float64(pdec)[:, None], np.float64(pra)[None, :], np.float64(odec), np.float64(ora)
	h = np.sin((pdec-odec)/2)**2+np.cos(pdec)*np.cos(odec)*np.sin((pra-ora)/2)**2
	return 2*np.arcsin(np.sqrt(np.minimum(h, 1)))
def prof64(prof, r):
	rs, vs = np.float64(prof[0]), np.float64(prof[1])
	return np.where(r >= rs[-1], 0.0, np.interp(r, rs, vs, left=vs[0], right=0.0))
def rcut32(prof, acol, vmin, rmax):
	vrel = np.float32(vmin)/np.max(np.abs(acol)).astype(np.float32)
	ks = np.where(np.abs(prof[1]) >= vrel)[0]
	rc = prof[0][min((ks[-1] if len(ks) else 0)+1, prof.shape[1]-1)]
	return np.float32(min(rc, np.float32(rmax)) if rmax > 0 else rc)

def ulps(got, want):
	return np.max(np.abs(np.float64(host(got))-want))/np.max(np.abs(want))/ULP

def test_pixel_coordinates_are_the_float32_axes(fx):
	"""what the kernels compute from (dec0, ddec, ra0, dra) and round to float32 is enmap.posaxes(dtype=float32) of the reference, bit for bit"""
	for g in "AB":
		shape, wcs = geometry(fx[g+"_geo"])
		ny, nx, dec0, ddec, ra0, dra = separable_geometry(shape, wcs, "auto")
		assert np.array_equal(np.float32(dec0+np.arange(ny)*ddec), fx[g+"_dec"])
		ra = np.float32(ra0+np.arange(nx)*dra)
		assert np.array_equal(ra, fx[g+"_ra"]) or np.allclose(np.exp(1j*np.float64(ra)), np.exp(1j*np.float64(fx[g+"_ra"])), rtol=0, atol=3e-7)
		dec, ra64 = enmap.posaxes(shape, wcs)
		assert np.allclose(dec, dec0+np.arange(ny)*ddec, rtol=0, atol=1e-14) and np.allclose(ra64, ra0+np.arange(nx)*dra, rtol=0, atol=1e-14)

# ---- bodies ---------------------------------------------------------------------------------------------------------------------
def distance_body(fx, dev):
	shape, wcs = geometry(fx["A_geo"])
	ramp = np.array([[0, np.pi/180], [0, 1]], np.float32)
	deg = np.float64(ramp[0, 1]); pix = abs(wcs.wcs.cdelt[1])*np.pi/180
	poss = fx["D_poss"]; worst = 0
	for i in range(poss.shape[1]):
		r64 = dist64(fx["A_dec"], fx["A_ra"], poss[0, i], poss[1, i])
		assert np.allclose(r64.reshape(-1)[::7], fx["R_r64_sub"][i], rtol=1e-13, atol=0)
		m = pointsrcs.sim_objects(shape, wcs, dev(poss[:, i:i+1]), dev(np.ones((1, 1), np.float32)), ramp, vmin=1e-12)
		ok = r64 < deg*(1-1e-6)
		err = np.abs(np.float64(host(m))[0]*deg-r64)/np.maximum(r64, pix)/ULP
		worst = max(worst, err[ok].max())
	print("distance: %.1f ulp of max(r, pixel) at most; the reference: %.0f ulp of a pixel" % (worst, fx["R_ref_err"]/pix/ULP))
	assert worst <= 16

def paint_cases(fx):
	gA, gB = geometry(fx["A_geo"]), geometry(fx["B_geo"])
	z26 = None
	yield "A0", gA, fx["A_poss"], fx["A_amps"], fx["A_prof"], z26, fx["A0_par"], fx["A0_expected"], (fx["A0_ref"], fx["A0_ref_err"])
	for t in ("A1", "A2", "A3"): yield t, gA, fx["A_poss"], fx["A_amps"], fx["A_prof"], z26, fx[t+"_par"], fx[t+"_expected"], None
	yield "B", gB, fx["B_poss"], fx["B_amps"], fx["B_prof"], None, (1e-12, 0), fx["B_expected"], (fx["B_ref"], fx["B_ref_err"])
	yield "C", gA, fx["C_poss"], fx["C_amps"], [fx["A_prof"], fx["C_prof2"]], fx["C_ids"], (1e-6, 0), fx["C_expected"], None

def forward_body(fx, dev, on_device):
	for tag, (shape, wcs), poss, amps, prof, ids, (vmin, rmax), want, ref in paint_cases(fx):
		got = pointsrcs.sim_objects(shape, wcs, dev(poss), dev(amps), prof, prof_ids=None if ids is None else dev(ids), vmin=float(vmin), rmax=float(rmax))
		assert isinstance(got, enmap.dmap if on_device else enmap.ndmap) and got.shape == want.shape and got.dtype == np.float32
		e = ulps(got, want)
		print("forward %s: %.2f ulp of the peak" % (tag, e))
		assert e <= 64, tag
		if ref is not None:      # the reference's conventions: its own output is as close to ours as it is to the model
			assert np.max(np.abs(np.float64(ref[0])-np.float64(host(got)))) <= ref[1]+64*ULP*np.max(np.abs(want)), tag
	# into maps that are there already and not zero: float32 and float64, updated in place
	(shape, wcs), want = geometry(fx["A_geo"]), fx["A1_expected"]
	yy, xx = np.mgrid[:shape[0], :shape[1]]
	base = np.array([np.sin(0.3*yy+c)*np.cos(0.2*xx-c)+0.1*c for c in range(3)])
	for dt in (np.float32, np.float64):
		b = base.astype(dt)
		omap = enmap.dmap(dev(b), wcs) if on_device else enmap.ndmap(b.copy(), wcs)
		res = pointsrcs.sim_objects(shape, wcs, dev(fx["A_poss"]), dev(fx["A_amps"]), fx["A_prof"], omap=omap, vmin=1e-3)
		assert res is omap and omap.dtype == dt
		e = ulps(omap, np.float64(b)+want)
		print("forward A1 into a %s map: %.2f ulp of the peak" % (np.dtype(dt).name, e))
		assert e <= 64

def maxmin_body(fx, dev, on_device):
	shape, wcs = geometry(fx["A_geo"])
	for op, c0 in (("max", 0.25), ("min", -0.25)):
		b = np.full((3,)+shape, c0, np.float32)
		omap = enmap.dmap(dev(b), wcs) if on_device else enmap.ndmap(b, wcs)
		pointsrcs.sim_objects(shape, wcs, dev(fx["A_poss"]), dev(fx["A_amps"]), fx["A_prof"], omap=omap, vmin=1e-3, op=op)
		e = ulps(omap, fx["A_"+op+"_expected"])
		print("%s: %.2f ulp of the peak" % (op, e))
		assert e <= 64, op
		assert not np.array_equal(fx["A_"+op+"_expected"], fx["A1_expected"]+c0)

def other_paths_body(fx, dev):
	"""the two paths the fixtures do not reach: profile tables too long for LDS (read from global memory), and more components than one pass
	over a tile's list carries in registers (4).  Expected: the model, evaluated here."""
	shape, wcs = geometry(fx["A_geo"])
	poss = fx["A_poss"][:, [0, 5, 24, 25]]
	amps = np.float32(np.random.default_rng(2).uniform(0.5, 3, (5, 4))*np.array([1, -1, 1, -1]))
	sigma = float(fx["beam_sigma"])
	rs = np.linspace(0, 8*sigma, 5000)
	prof = np.float32([rs, np.exp(-0.5*(rs/sigma)**2)])
	want = np.zeros((5,)+shape)
	for i in range(4):
		r = dist64(fx["A_dec"], fx["A_ra"], poss[0, i], poss[1, i])
		rc = np.float64(rcut32(prof, amps[:, i], 1e-3, 0))
		assert np.min(np.abs(r-rc)) > 2e-6*rc      # (no pixel sits on the cut radius, where float32 may decide either way: as the generator checks for its cases)
		want += np.float64(amps[:, i])[:, None, None]*np.where(r <= rc, prof64(prof, r), 0.0)
	got = pointsrcs.sim_objects(shape, wcs, dev(poss), dev(amps), prof, vmin=1e-3)
	e = ulps(got, want)
	print("5 components, 5000 profile samples: %.2f ulp of the peak" % e)
	assert got.shape == (5,)+shape and e <= 64

def determinism_body(fx, dev):
	shape, wcs = geometry(fx["A_geo"])
	run = lambda: host(pointsrcs.sim_objects(shape, wcs, dev(fx["C_poss"]), dev(fx["C_amps"]), [fx["A_prof"], fx["C_prof2"]], prof_ids=dev(fx["C_ids"]), vmin=1e-6))
	a, b = run(), run()
	assert np.array_equal(a, b) and np.any(a != 0)

def transpose_body(fx, dev, on_device):
	shape, wcs = geometry(fx["A_geo"])
	poss, amps, prof, vmin = fx["A_poss"], fx["A_amps"], fx["A_prof"], 1e-3
	m = (np.random.default_rng(1).random((3,)+shape)*2-1).astype(np.float32)
	want = np.zeros(amps.shape); asum = np.zeros(amps.shape); fwd_abs = 0.0; nmax = 0
	for i in range(amps.shape[1]):
		r = dist64(fx["A_dec"], fx["A_ra"], poss[0, i], poss[1, i])
		w = np.where(r <= np.float64(rcut32(prof, amps[:, i], vmin, 0)), prof64(prof, r), 0.0)
		want[:, i] = (np.float64(m)*w).sum((-2, -1)); asum[:, i] = np.abs(np.float64(m)*w).sum((-2, -1))
		fwd_abs += np.sum(np.abs(np.float64(amps[:, i]))*asum[:, i]); nmax = max(nmax, int((w != 0).sum()))
	acc = dev(amps.copy())
	mm = enmap.dmap(dev(m), wcs) if on_device else enmap.ndmap(m, wcs)
	res = pointsrcs.sim_objects(shape, wcs, dev(poss), acc, prof, omap=mm, vmin=vmin, transpose=True)
	assert res is mm and np.array_equal(host(mm), m)
	got = np.float64(host(acc))-np.float64(amps)
	rel = np.max(np.abs(got-want)/asum)/ULP
	print("transpose: %.2f ulp of sum |P m| per object" % rel)
	assert rel <= 64
	fwd = np.float64(host(pointsrcs.sim_objects(shape, wcs, dev(poss), dev(amps), prof, vmin=vmin)))
	lhs, rhs = np.sum(fwd*np.float64(m)), np.sum(np.float64(amps)*got)
	print("adjointness: |<Pa,m> - <a,P^T m>| = %.3g, bound %.3g" % (abs(lhs-rhs), 4*nmax*2.0**-24*fwd_abs))
	assert abs(lhs-rhs) <= 4*nmax*2.0**-24*fwd_abs

def seeded_map(seed, draws, shape):
	rng = np.random.default_rng(seed)
	for lo, hi, n in draws: rng.uniform(lo, hi, n)
	return rng.random(shape).astype(np.float32)*2-1

def radial_body(fx, dev, on_device):
	mapD = seeded_map(5, [(8, 72, 12), (8, 104, 12)], (2, 80, 112)); assert np.array_equal(mapD[:, 0, :8], fx["D_map_head"])
	mapE = seeded_map(9, [(-1.2, 1.2, 4), (-3, 3, 4)], (1, 90, 180)); assert np.array_equal(mapE[:, 0, :8], fx["E_map_head"])
	for tag, geo, poss, m in (("D1", "A_geo", fx["D_poss"], mapD), ("D2", "A_geo", fx["D_poss"], mapD), ("E", "B_geo", fx["E_poss"], mapE)):
		shape, wcs = geometry(fx[geo])
		mask, cnt, want, asum = fx[tag+"_mask"], fx[tag+"_cnt"], fx[tag+"_expected"], fx[tag+"_asum"]
		assert mask.mean() <= 0.30
		mm = enmap.dmap(dev(m), wcs) if on_device else enmap.ndmap(m, wcs)
		got = pointsrcs.radial_sum(mm, dev(poss), fx[tag+"_bins"])
		assert tuple(got.shape) == want.shape and (hasattr(got, "data_ptr") == on_device)
		good = np.broadcast_to(~mask[:, None, :], want.shape)
		tol = 4*cnt[:, None, :]*2.0**-24*asum
		err = np.abs(np.float64(host(got))-want)
		print("radial_sum %s: worst error / bound on the unmarked pairs %.3f (%d of %d pairs marked)" % (tag, np.max(np.where(good, err/np.maximum(tol, 1e-300), 0)), mask.sum(), mask.size))
		assert np.all(err[good] <= tol[good]), tag
		# the accumulating form adds to what is there
		acc = dev(np.ones(want.shape, np.float32))
		assert pointsrcs.radial_sum(mm, dev(poss), fx[tag+"_bins"], oprofs=acc) is acc
		assert np.all(np.abs(np.float64(host(acc))-1-want)[good] <= tol[good]+2*ULP*(1+np.abs(want[good])))
		# radial_bin: the ratio of two such sums; the count of pixels is exact in float32
		mean = np.float64(host(pointsrcs.radial_bin(mm, dev(poss), fx[tag+"_bins"])))
		full = good & np.broadcast_to(cnt[:, None, :] > 0, want.shape)
		n = np.broadcast_to(cnt[:, None, :], want.shape)
		assert np.all(np.abs(mean[full]-want[full]/n[full]) <= tol[full]/n[full]+ULP*np.abs(want[full]/n[full])), tag

def srcs_beam_body(fx, dev):
	shape, wcs = geometry(fx["A_geo"], (3,))
	sigma = float(fx["beam_sigma"])
	beam = pointsrcs.expand_beam(sigma, nsigma=5)
	np.testing.assert_allclose(beam, fx["beam_gauss"], rtol=1e-12, atol=0)
	np.testing.assert_allclose(pointsrcs.expand_beam(sigma, nsigma=4, rmax=7*arcmin), fx["beam_rmax"], rtol=1e-12, atol=0)
	assert pointsrcs.expand_beam(beam) is not None and np.array_equal(pointsrcs.expand_beam(beam), beam)
	np.testing.assert_allclose([pointsrcs.nsigma2rmax(np.float64(fx["A_prof"]), n) for n in (3, 5)], fx["nsig_rmax"], rtol=1e-12)
	srcs = fx["S_srcs"]
	a = pointsrcs.sim_srcs(shape, wcs, srcs, sigma)
	b = pointsrcs.sim_objects(shape, wcs, srcs.T[:2], np.float32(srcs.T[2:5]), beam, vmin=np.exp(-0.5*5**2))
	assert a.shape == shape and np.array_equal(host(a), host(b)) and np.any(host(a) != 0)
	c = pointsrcs.sim_srcs(shape, wcs, srcs, sigma, op=np.max)
	assert np.array_equal(host(c), host(pointsrcs.sim_objects(shape, wcs, srcs.T[:2], np.float32(srcs.T[2:5]), beam, vmin=np.exp(-0.5*5**2), op="max")))
	with pytest.raises(NotImplementedError): pointsrcs.sim_srcs(shape, wcs, srcs, sigma, method="python")
	assert pointsrcs.is_equi(beam[0]) and not pointsrcs.is_equi(fx["C_prof2"][0])

def window_body(fx, dev, on_device):
	_, wcs = geometry(fx["A_geo"])
	m = fx["F_map"]
	wy, wx = enmap.calc_window((40, 56), order=1, scale=2)
	np.testing.assert_allclose(wy, fx["F_wy"], rtol=1e-13, atol=1e-15); np.testing.assert_allclose(wx, fx["F_wx"], rtol=1e-13, atol=1e-15)
	for order in (0, 1):
		for p in (1, -1):
			src = enmap.dmap(dev(m), wcs) if on_device else enmap.ndmap(m.copy(), wcs)
			got = enmap.apply_window(src, pow=p, order=order)
			assert isinstance(got, type(src)) and np.array_equal(host(src), m)
			np.testing.assert_allclose(host(got), fx["F_o%d_p%+d" % (order, p)], rtol=1e-12, atol=1e-12)
	back = enmap.unapply_window(enmap.apply_window(src, order=1), order=1)
	np.testing.assert_allclose(host(back), m, rtol=1e-12, atol=1e-12)
	# pixwin=True in sim_objects is apply_window of the painted map
	shape, wcsA = geometry(fx["A_geo"])
	args = (shape, wcsA, dev(fx["A_poss"]), dev(fx["A_amps"]), fx["A_prof"])
	plain = pointsrcs.sim_objects(*args, vmin=1e-3)
	assert np.array_equal(host(pointsrcs.sim_objects(*args, vmin=1e-3, pixwin=True, pixwin_order=1)), host(enmap.apply_window(plain, order=1)))

def edges_body(fx, dev, on_device):
	shape, wcs = geometry(fx["A_geo"])
	empty = pointsrcs.sim_objects(shape, wcs, dev(np.zeros((2, 0), np.float32)), dev(np.zeros((3, 0), np.float32)), fx["A_prof"])
	assert empty.shape == (3,)+shape and not np.any(host(empty))
	far = pointsrcs.sim_objects(shape, wcs, dev(np.float32([[-0.3], [1.0]])), dev(np.float32([[2.0]])), fx["A_prof"])
	assert far.shape == (1,)+shape and not np.any(host(far))
	one = pointsrcs.sim_objects(shape, wcs, dev(fx["A_poss"]), dev(fx["A_amps"][0]), fx["A_prof"], vmin=1e-12)
	assert one.shape == shape and ulps(one, fx["A0_expected"][0]) <= 64
	assert pointsrcs.radial_sum(enmap.dmap(dev(np.ones(shape, np.float32)), wcs) if on_device else enmap.ones(shape, wcs, np.float32),
		dev(np.zeros((2, 0), np.float32)), np.arange(4)*arcmin).shape == (0, 3)
	# a default vmin: min |amps| * 1e-3
	d = pointsrcs.sim_objects(shape, wcs, dev(fx["A_poss"]), dev(fx["A_amps"]), fx["A_prof"])
	e = pointsrcs.sim_objects(shape, wcs, dev(fx["A_poss"]), dev(fx["A_amps"]), fx["A_prof"], vmin=float(np.abs(fx["A_amps"]).min())*1e-3)
	assert np.array_equal(host(d), host(e))

def errors_body(fx, dev):
	shape, wcs = geometry(fx["A_geo"])
	poss, amps, prof = dev(fx["A_poss"]), dev(fx["A_amps"]), fx["A_prof"]
	tilted = CarWCS(cdelt=wcs.wcs.cdelt, crval=[wcs.wcs.crval[0], 10.0], crpix=wcs.wcs.crpix)
	with pytest.raises(NotImplementedError): pointsrcs.sim_objects(shape, tilted, poss, amps, prof)
	with pytest.raises(NotImplementedError): pointsrcs.sim_objects(shape, wcs, poss, amps, prof, separable=False)
	with pytest.raises(NotImplementedError): pointsrcs.radial_sum(enmap.ndmap(np.zeros(shape, np.float32), tilted), fx["A_poss"], np.arange(3)*arcmin)
	with pytest.raises(ValueError): pointsrcs.sim_objects(shape, wcs, poss, amps, prof, op="mul")
	omap = enmap.zeros((3,)+shape, wcs, np.float32)
	with pytest.raises(ValueError): pointsrcs.sim_objects(shape, wcs, fx["A_poss"], np.float64(fx["A_amps"]), prof, omap=omap, vmin=1e-3, transpose=True)
	with pytest.raises(ValueError): pointsrcs.sim_objects(shape, wcs, fx["A_poss"], fx["A_amps"].copy(), prof, omap=omap, transpose=True)      # (no vmin)
	with pytest.raises(ValueError): pointsrcs.sim_objects(shape, wcs, fx["A_poss"], fx["A_amps"], prof, prof_ids=np.ones(26, np.int32))

# ---- host simulator -------------------------------------------------------------------------------------------------------------
@pytest.mark.hostsim
def test_distance_sim(fx): distance_body(fx, ident)
@pytest.mark.hostsim
def test_forward_sim(fx): forward_body(fx, ident, False)
@pytest.mark.hostsim
def test_max_min_sim(fx): maxmin_body(fx, ident, False)
@pytest.mark.hostsim
def test_long_profile_many_components_sim(fx): other_paths_body(fx, ident)
@pytest.mark.hostsim
def test_determinism_sim(fx): determinism_body(fx, ident)
@pytest.mark.hostsim
def test_transpose_sim(fx): transpose_body(fx, ident, False)
@pytest.mark.hostsim
def test_radial_sum_sim(fx): radial_body(fx, ident, False)
@pytest.mark.hostsim
def test_sim_srcs_and_beams_sim(fx): srcs_beam_body(fx, ident)
@pytest.mark.hostsim
def test_apply_window_sim(fx): window_body(fx, ident, False)
@pytest.mark.hostsim
def test_edge_cases_sim(fx): edges_body(fx, ident, False)
@pytest.mark.hostsim
def test_errors_sim(fx): errors_body(fx, ident)

# ---- GPU ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_distance_gpu(fx): distance_body(fx, cuda)
@pytest.mark.gpu
def test_forward_gpu(fx):
	forward_body(fx, cuda, True)
	forward_body(fx, ident, False)      # host arrays in, host maps out
@pytest.mark.gpu
def test_max_min_gpu(fx): maxmin_body(fx, cuda, True); maxmin_body(fx, ident, False)
@pytest.mark.gpu
def test_long_profile_many_components_gpu(fx): other_paths_body(fx, cuda)
@pytest.mark.gpu
def test_determinism_gpu(fx): determinism_body(fx, cuda)
@pytest.mark.gpu
def test_transpose_gpu(fx): transpose_body(fx, cuda, True); transpose_body(fx, ident, False)
@pytest.mark.gpu
def test_radial_sum_gpu(fx): radial_body(fx, cuda, True); radial_body(fx, ident, False)
@pytest.mark.gpu
def test_sim_srcs_and_beams_gpu(fx): srcs_beam_body(fx, ident)
@pytest.mark.gpu
def test_apply_window_gpu(fx): window_body(fx, cuda, True); window_body(fx, ident, False)
@pytest.mark.gpu
def test_edge_cases_gpu(fx): edges_body(fx, cuda, True); edges_body(fx, ident, False)
@pytest.mark.gpu
def test_errors_gpu(fx): errors_body(fx, cuda)

@pytest.mark.gpu
def test_side_stream_gpu(fx):
	"""one paint, one transpose and one radial sum on a stream of their own: the paint bit for bit that of the default stream"""
	import torch
	shape, wcs = geometry(fx["A_geo"])
	args = (shape, wcs, cuda(fx["C_poss"]), cuda(fx["C_amps"]), [fx["A_prof"], fx["C_prof2"]])
	ids = cuda(fx["C_ids"])
	m0 = pointsrcs.sim_objects(*args, prof_ids=ids, vmin=1e-6)
	p0 = pointsrcs.radial_sum(m0, args[2], np.arange(5)*arcmin)
	torch.cuda.synchronize()
	side = torch.cuda.Stream()
	with torch.cuda.stream(side):
		m1 = pointsrcs.sim_objects(*args, prof_ids=ids, vmin=1e-6)
		p1 = pointsrcs.radial_sum(m1, args[2], np.arange(5)*arcmin)
	side.synchronize()
	assert torch.equal(m0.tensor, m1.tensor) and ulps(m1, fx["C_expected"]) <= 64
	assert np.allclose(host(p0), host(p1), rtol=1e-4, atol=1e-4*float(p0.abs().max()))
