"""pixell_amd.lensing (offset_by_grad, pole_wrap, phi_to_kappa, kappa_to_phi, rand_alm, lens_map_curved) and enmap.posmap / rotate_pol
against the reference's pixell.lensing / enmap outputs in tests/golden/lensing.npz (tests/golden/make_lensing.py).  Small cases run in
the test-only host simulator, the reference test's own shapes on the GPU.

Pixel selection of the comparisons with the reference's offset_by_grad: its closed form loses the quadrant of ra (and some digits of
dec and psi) for points on a pole, so pixels whose distance from either pole does not exceed |grad| -- the pole rows of a CC grid --
are compared with a long-double evaluation of the vector form (vec_deflect below) instead, and their share is capped."""
import os
import numpy as np
import pytest
from pixell_amd import enmap, lensing, curvedsky, sht
from pixell_amd.wcs import CarWCS

TOL = 1e-12      # dec, ra cos(dec), psi against the reference: ~25x the 4e-14 between the two formulations in numpy, margin for the device's sincos / atan2
EPS = 1e-10      # accuracy asked of the point synthesis

@pytest.fixture(scope="module")
def fx(golden_dir):
	return dict(np.load(os.path.join(golden_dir, "lensing.npz")))

def geometry(numbers, pre=()):
	n = np.asarray(numbers)
	return tuple(pre)+(int(n[0]), int(n[1])), CarWCS(cdelt=n[2:4], crval=n[4:6], crpix=n[6:8])

def wrap(x): return np.abs(np.remainder(np.asarray(x, np.float64)+np.pi, 2*np.pi)-np.pi)

def vec_deflect(dec, ra, g0, g1, psi0=None):
	"""the geodesic offset in vector form, in long double: n' = cos d n + sin d t, t' = -sin d n + cos d t, psi = psi0 - 2 (a' - a)"""
	ft = np.longdouble
	dec, ra, g0, g1 = [np.asarray(x, ft) for x in (dec, ra, g0, g1)]
	sd, cd, sr, cr = np.sin(dec), np.cos(dec), np.sin(ra), np.cos(ra)
	d = np.hypot(g0, g1); zero = d == 0
	ds = np.where(zero, 1, d)
	ut, up = np.where(zero, 1, -g0/ds), np.where(zero, 0, g1/ds)
	n = np.array([cd*cr, cd*sr, sd]); et = np.array([sd*cr, sd*sr, -cd]); ep = np.array([-sr, cr, 0*sr])
	t = ut*et+up*ep
	n2 = np.cos(d)*n+np.sin(d)*t; t2 = -np.sin(d)*n+np.cos(d)*t
	r = np.hypot(n2[0], n2[1]); rs = np.where(r > 0, r, 1)
	cp, sp = np.where(r > 0, n2[0]/rs, 1), np.where(r > 0, n2[1]/rs, 0)
	x2 = (t2[0]*cp+t2[1]*sp)*n2[2]-t2[2]*r; y2 = t2[1]*cp-t2[0]*sp
	psi = -2*np.arctan2(y2*ut-x2*up, x2*ut+y2*up)
	if psi0 is not None: psi = psi+np.asarray(psi0, ft)
	return np.array([ft(np.pi)/2-np.arctan2(r, n2[2]), np.arctan2(n2[1], n2[0]), psi])

def covered(pos, grad):
	"""pixels further from both poles than their gradient is long"""
	return np.pi/2-np.abs(np.asarray(pos[0], np.float64)) > np.hypot(*np.asarray(grad, np.float64))

def host(x):
	if isinstance(x, enmap.dmap): x = x.tensor
	return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)

def check_deflect(got, pos, grad, ref, cap, psi0=None, rows=slice(None), what=""):
	"""got [2|3, ny, nx] against the reference on the covered pixels (rows: those the fixture kept) and the long-double vector form on the rest"""
	got = host(got); ok = covered(pos, grad)
	share = 1-ok.mean()
	print("%s: excluded share %.5f (cap %.5f)" % (what, share, cap))
	assert share <= cap+1e-12
	ld = vec_deflect(pos[0], pos[1], grad[0], grad[1], psi0)
	for name, want, sel in (("reference", np.asarray(ref), ok[rows]), ("long double", ld[:, rows], ~ok[rows])):
		g = got[:, rows]
		errs = [np.abs(g[0]-want[0]), wrap(g[1]-want[1])*np.cos(np.asarray(want[0], np.float64))]
		if got.shape[0] > 2: errs.append(wrap(g[2]-want[2]))
		worst = [float(e[sel].max()) if sel.any() else 0.0 for e in errs]
		print("%s vs %s: dec %.2e  ra cos(dec) %.2e  psi %.2e  (%d pixels)" % (what, name, worst[0], worst[1], worst[-1] if len(worst) > 2 else 0, int(sel.sum())))
		assert max(worst) <= TOL, (what, name, worst)

def from_loc(loc, psi, pixshape):
	loc = host(loc)
	res = [np.pi/2-loc[:, 0], loc[:, 1]]+([host(psi)] if psi is not None else [])
	return np.array(res).reshape((len(res),)+tuple(pixshape))

def deflect_body(fx, dev):
	"""dev: numpy array -> what the library is fed (numpy itself, a torch tensor on the CPU in the simulator or on the GPU)"""
	for key in ("cc", "f1", "ccy", "ccx"):
		pos, grad, ref = fx["d_%s_pos" % key], fx["d_%s_grad" % key], fx["d_%s_out" % key]
		cap = 2/19 if key != "f1" else 0.0
		got = lensing.offset_by_grad(dev(pos), dev(grad), pol=True)
		assert got.shape == ref.shape
		check_deflect(got, pos, grad, ref, cap, what=key+" positions")
		# the same from the geometry's numbers alone, in the form the point plan reads
		shape, wcs = geometry(fx["d_%s_geo" % key])
		assert np.allclose(np.asarray(enmap.posmap(shape, wcs)), pos, rtol=0, atol=1e-14)
		loc, psi = lensing.offset_by_grad(None, dev(grad), pol=True, _loc=True, _geometry=(shape, wcs))
		l = host(loc)
		assert l.shape == (pos[0].size, 2) and l[:, 0].min() >= 0 and l[:, 0].max() <= np.pi and l[:, 1].min() >= 0 and l[:, 1].max() <= 2*np.pi
		check_deflect(from_loc(loc, psi, pos.shape[1:]), pos, grad, ref, cap, what=key+" geometry")
	pos, grad = fx["d_cc_pos"], fx["d_cc_grad"]
	# the planted pixels are where they were put: a zero gradient is the identity (no 0/0), one along dec moves dec alone and does not rotate
	got = host(lensing.offset_by_grad(dev(pos), dev(grad), pol=True))
	assert np.all(np.isfinite(got))
	assert got[0, 3, 3] == pytest.approx(pos[0, 3, 3], abs=1e-15) and wrap(got[1, 3, 3]-pos[1, 3, 3]) < 1e-15 and got[2, 3, 3] == 0
	assert wrap(got[1, 0, 2]-pos[1, 0, 2]) < 1e-15 and got[2, 0, 2] == 0
	assert got[0, 4, 5] == pytest.approx(pos[0, 4, 5]+7e-4, abs=1e-15) and wrap(got[1, 4, 5]-pos[1, 4, 5]) < 1e-13 and abs(got[2, 4, 5]) < 1e-15
	# pol=False / pol=None: two components, the same numbers
	got2 = lensing.offset_by_grad(dev(pos), dev(grad), pol=False)
	assert got2.shape == fx["d_cc_out_nopol"].shape == (2,)+pos.shape[1:] and np.array_equal(host(got2), got[:2])
	assert lensing.offset_by_grad(dev(pos), dev(grad)).shape[0] == 2
	# a psi0 component is added to the rotation (and switches pol on)
	pos3 = np.concatenate([pos, fx["d_cc_psi0"][None]])
	got3 = lensing.offset_by_grad(dev(pos3), dev(grad))
	assert got3.shape[0] == 3
	check_deflect(got3, pos, grad, fx["d_cc_out_psi0"], 2/19, psi0=fx["d_cc_psi0"], what="cc psi0")
	# a float32 gradient: the arithmetic is float64 all the same
	g32 = fx["d_cc_grad32"]; assert g32.dtype == np.float32
	check_deflect(lensing.offset_by_grad(dev(pos), dev(g32), pol=True), pos, g32.astype(np.float64), fx["d_cc_out32"], 2/19, what="cc float32")
	# not geodesic: the gradient added to the coordinates, points that pass a pole reflected, no rotation
	gn, ref = fx["d_cc_grad_ng"], fx["d_cc_out_ng"]
	got = host(lensing.offset_by_grad(dev(pos), dev(gn), geodesic=False, pol=True))
	ok = np.abs(pos[0]) < np.pi/2-1e-6          # (on a pole itself g1 / cos(dec) has no meaning: 1e13 radians in the reference)
	assert 1-ok.mean() <= 2/19+1e-12 and np.all(np.isfinite(got))
	for y, x in ((1, 3), (17, 6), (2, 9)): assert abs(pos[0, y, x]+gn[0, y, x]) > np.pi/2      # the planted pixels do cross a pole
	errs = [np.abs(got[0]-ref[0])[ok].max(), (wrap(got[1]-ref[1])*np.cos(ref[0]))[ok].max(), np.abs(got[2]).max()]
	print("not geodesic: dec %.2e ra cos(dec) %.2e psi %.2e" % tuple(errs))
	assert max(errs) <= TOL and np.abs(got[0]).max() <= np.pi/2
	assert np.allclose(host(lensing.pole_wrap(dev(fx["pw_in"]))), fx["pw_out"], rtol=0, atol=1e-15)

def rotate_body(fx, dev):
	m, ang = fx["r_map"], fx["r_ang"]
	for dt, tag in ((np.float64, "r_out_s%d"), (np.float32, "r_out32_s%d")):
		md = m.astype(dt)
		for spin in (0, 1, 2):
			ref = fx[tag % spin]
			got = enmap.rotate_pol(dev(md), dev(ang), spin=spin)
			assert host(got).dtype == dt and got.shape == ref.shape
			tol = 4*np.finfo(dt).eps*np.hypot(md[:, 1], md[:, 2])       # 4 ulp of the pair's magnitude
			err = np.abs(host(got).astype(np.float64)-ref)
			assert np.all(err[:, 1] <= tol) and np.all(err[:, 2] <= tol) and np.array_equal(host(got)[:, 0], md[:, 0]), (dt, spin, float(err.max()))
		# the input is left alone; a component view with gaps gives the same numbers
		big = np.zeros((2, 6, 19, 36), dt); big[:, ::2] = md
		bd = dev(big); view = bd[:, ::2]
		got = enmap.rotate_pol(view, dev(ang))
		assert np.array_equal(host(got), host(enmap.rotate_pol(dev(md), dev(ang)))) and np.array_equal(host(bd), big)
		# other components, another axis, a scalar angle, an angle per leading entry
		got = host(enmap.rotate_pol(dev(md), 0.3, comps=[0, 2]))
		assert np.allclose(got[:, 0], np.cos(0.6)*md[:, 0]-np.sin(0.6)*md[:, 2], rtol=0, atol=tol.max()) and np.array_equal(got[:, 1], md[:, 1])
		a2 = np.stack([ang, -0.5*ang])
		got = host(enmap.rotate_pol(dev(md), dev(a2[:, :, :]), axis=1))
		for b in range(2): assert np.allclose(got[b, 2], np.sin(2*a2[b])*md[b, 1]+np.cos(2*a2[b])*md[b, 2], rtol=0, atol=tol.max())
	# dmap in, dmap out with the same wcs
	shape, wcs = geometry(fx["d_cc_geo"])
	if not isinstance(dev(m), np.ndarray):
		d = enmap.rotate_pol(enmap.dmap(dev(m), wcs), dev(ang))
		assert isinstance(d, enmap.dmap) and d.wcs is wcs and np.array_equal(host(d), host(enmap.rotate_pol(dev(m), dev(ang))))
	else:
		d = enmap.rotate_pol(enmap.ndmap(m, wcs), ang)
		assert isinstance(d, enmap.ndmap) and d.wcs is wcs

def rel_groups(got, want, sel):
	"""relative L2 error per spin group of a T/Q/U map over the selected pixels: T alone, Q and U jointly"""
	got, want = host(got).astype(np.float64), np.asarray(want, np.float64)
	return [float(np.sqrt(np.sum((got[c]-want[c])[..., sel]**2)/np.sum(want[c][..., sel]**2))) for c in (slice(0, 1), slice(1, 3))]

def exact_points(alm, dec, ra, lmax, oracle):
	"""T/Q/U at the points (dec, ra): rings of one pixel -- the long-double oracle in the simulator, the ring synthesis on the GPU"""
	from test_alm2map_pos import exact
	loc = np.stack([np.pi/2-np.asarray(dec, np.float64).reshape(-1), np.asarray(ra, np.float64).reshape(-1)], 1)
	return np.concatenate([exact(alm[:1], loc, lmax, 0, oracle=oracle), exact(alm[1:], loc, lmax, 2, oracle=oracle)])

def check_excluded(lensed, grad, shape, wcs, cmb, lmax, cap, oracle):
	"""the pixels left out of the comparison with the reference-made map: against the long-double vector form + exact synthesis there"""
	pos = np.asarray(enmap.posmap(shape, wcs)); grad = host(grad).astype(np.float64)
	out = ~covered(pos, grad)
	assert out.mean() <= cap+1e-12
	if not out.any(): return
	d = vec_deflect(pos[0][out], pos[1][out], grad[0][out], grad[1][out])
	ex = exact_points(cmb, d[0], d[1], lmax, oracle)
	c, s = np.cos(2*d[2].astype(np.float64)), np.sin(2*d[2].astype(np.float64))
	want = np.array([ex[0], c*ex[1]-s*ex[2], s*ex[1]+c*ex[2]])
	got = host(lensed)[:, out]
	errs = [float(np.sqrt(np.sum((got[g]-want[g])**2)/np.sum(want[g]**2))) for g in (slice(0, 1), slice(1, 3))]
	print("excluded pixels (%d): T %.2e  QU %.2e" % (int(out.sum()), errs[0], errs[1]))
	assert max(errs) <= 2*EPS, errs

def bands_body(shape, wcs, phi, cmb, delta_theta, band_rows, monkeypatch):
	one, = lensing.lens_map_curved(shape, wcs, phi, cmb, epsilon=EPS)
	seen = []
	real = sht.points_plan
	def spy(loc, *a, **k):
		seen.append(int(loc.shape[0])); return real(loc, *a, **k)
	monkeypatch.setattr(sht, "points_plan", spy)
	three, = lensing.lens_map_curved(shape, wcs, phi, cmb, epsilon=EPS, delta_theta=delta_theta)
	monkeypatch.setattr(sht, "points_plan", real)
	assert len(seen) == 3 and sum(seen) == shape[-2]*shape[-1] and max(seen) <= band_rows*shape[-1], seen
	errs = rel_groups(three, host(one), slice(None))
	print("3 bands vs 1: T %.2e QU %.2e" % tuple(errs))
	assert max(errs) <= 2*EPS

# ---- simulator ------------------------------------------------------------------------------------------------------------------
@pytest.mark.hostsim
def test_deflect_sim(fx):
	deflect_body(fx, lambda a: a)

@pytest.mark.hostsim
def test_deflect_torch_sim(fx):
	torch = pytest.importorskip("torch")
	deflect_body(fx, torch.as_tensor)

@pytest.mark.hostsim
def test_rotate_pol_sim(fx):
	rotate_body(fx, lambda a: a)
	torch = pytest.importorskip("torch")
	rotate_body(fx, torch.as_tensor)

@pytest.mark.hostsim
def test_lens_map_curved_sim(fx):
	"""lmax 16 on the 10-degree CC grid against the fixture's expected map (reference offset_by_grad on the oracle's gradient, exact synthesis
	there, reference rotate_pol): relative L2 <= 2 epsilon per spin group (the NUFFT's epsilon + lmax x 1e-12 of position agreement)"""
	shape, wcs = geometry(fx["d_cc_geo"], (3,))
	cmb, phi, lmax = fx["e_cmb"], fx["e_phi"], 16
	pos = np.asarray(enmap.posmap(shape, wcs))
	l, a = lensing.lens_map_curved(shape, wcs, phi, cmb, output="la", epsilon=EPS)
	assert isinstance(l, enmap.ndmap) and l.shape == shape and a.shape == (2,)+shape[-2:]
	assert np.abs(np.asarray(a)-fx["e_grad"]).max() <= 1e-12*np.abs(fx["e_grad"]).max()
	ok = covered(pos, fx["e_grad"])
	assert 1-ok.mean() <= 2/19+1e-12
	errs = rel_groups(l, fx["e_lensed"], ok)
	print("lensed vs expected: T %.2e  QU %.2e" % tuple(errs))
	assert max(errs) <= 2*EPS
	check_excluded(l, a, shape, wcs, cmb, lmax, 2/19, oracle=True)
	# a single map comes back without its component axis (and is not rotated)
	t, = lensing.lens_map_curved(shape[-2:], wcs, phi, cmb[0], epsilon=EPS)
	assert t.shape == shape[-2:] and rel_groups(np.asarray(t)[None].repeat(3, 0), fx["e_lensed"], ok)[0] <= 2*EPS
	# outputs: count, order, shapes; u, p, k, a are plain alm2map calls
	assert len(lensing.lens_map_curved(shape, wcs, phi, cmb, output="l")) == 1
	lu = lensing.lens_map_curved(shape, wcs, phi, cmb, output="lu", epsilon=EPS)
	assert len(lu) == 2 and lu[0].shape == lu[1].shape == shape and np.array_equal(np.asarray(lu[0]), np.asarray(l))
	p, k, a2 = lensing.lens_map_curved(shape, wcs, phi, cmb, output="pka")
	assert p.shape == k.shape == shape[-2:] and a2.shape == (2,)+shape[-2:]
	assert np.array_equal(np.asarray(lu[1]), np.asarray(curvedsky.alm2map(cmb, enmap.zeros(shape, wcs))))
	assert np.array_equal(np.asarray(p), np.asarray(curvedsky.alm2map(phi, enmap.zeros(shape[-2:], wcs))))
	assert np.array_equal(np.asarray(k), np.asarray(curvedsky.alm2map(lensing.phi_to_kappa(phi), enmap.zeros(shape[-2:], wcs))))
	assert np.array_equal(np.asarray(a2), np.asarray(curvedsky.alm2map(phi, enmap.zeros((2,)+shape[-2:], wcs), deriv=True))) and np.array_equal(np.asarray(a2), np.asarray(a))
	with pytest.raises(NotImplementedError): lensing.lens_map_curved(shape, wcs, phi, cmb, method="lenspyx")
	with pytest.raises(ValueError): lensing.lens_map_curved(shape, wcs, phi, cmb, output="x")
	# tensors in, dmaps out
	torch = pytest.importorskip("torch")
	lt, = lensing.lens_map_curved(shape, wcs, torch.as_tensor(phi), torch.as_tensor(cmb), epsilon=EPS)
	assert isinstance(lt, enmap.dmap) and max(rel_groups(lt, fx["e_lensed"], ok)) <= 2*EPS

@pytest.mark.hostsim
def test_bands_sim(fx, monkeypatch):
	shape, wcs = geometry(fx["d_cc_geo"], (3,))
	bands_body(shape, wcs, fx["e_phi"], fx["e_cmb"], np.deg2rad(70), 7, monkeypatch)      # 19 rows in bands of 7, 7, 5

def kappa_body(dev):
	lmax = 100; l = np.arange(lmax+1.0)
	ps = np.zeros(lmax+1); ps[2:] = 1/l[2:]
	phi = curvedsky.rand_alm(ps, lmax=lmax, seed=12)
	kappa = lensing.phi_to_kappa(dev(phi))
	ai = curvedsky.alm_info(lmax)
	assert np.allclose(host(kappa)[ai.lm2ind(7, 3)], phi[ai.lm2ind(7, 3)]*28, rtol=1e-15)
	back = host(lensing.kappa_to_phi(kappa))
	assert np.all(np.isfinite(back)) and np.allclose(back, phi, rtol=1e-14, atol=0)

RAND_CASES = [(dict(seed=3, ncomp=3), "a_phi", "a_cmb"), (dict(seed=3, phi_seed=4, ncomp=3), "a_phi_ps", "a_cmb_ps"), (dict(seed=5, ncomp=1, dtype=np.float32), "a_phi_sp", "a_cmb_sp")]

def rand_alm_body(fx, same):
	for kw, kp, kc in RAND_CASES:
		p, c, ai = lensing.rand_alm(fx["a_ps"], **kw)
		assert ai.lmax == fx["a_ps"].shape[-1]-1 and p.dtype == fx[kp].dtype and c.shape == fx[kc].shape == (kw["ncomp"], ai.nelem)
		print(kw, "max |diff| phi %.2e cmb %.2e, elements that differ %d of %d" % (np.abs(p-fx[kp]).max(), np.abs(c-fx[kc]).max(), int((p != fx[kp]).sum()+(c != fx[kc]).sum()), p.size+c.size))
		assert same(p, fx[kp]) and same(c, fx[kc]), kw

@pytest.mark.hostsim
def test_phi_kappa_roundtrip_sim():
	kappa_body(lambda a: a)

@pytest.mark.hostsim
def test_rand_alm_bit_exact_sim(fx):
	"""lensing.rand_alm, with and without phi_seed and in single precision, bit for bit the reference's alm"""
	rand_alm_body(fx, np.array_equal)

@pytest.mark.hostsim
def test_rand_map_sim(fx):
	shape, wcs = geometry(fx["d_cc_geo"], (3,))
	ps = fx["a_ps"]*1e-6
	l, u = lensing.rand_map(shape, wcs, ps, lmax=16, seed=3, output="lu")
	p, c, ai = lensing.rand_alm(ps, lmax=16, seed=3, ncomp=3)
	want = lensing.lens_map_curved(shape, wcs, p, c, phi_ainfo=ai, output="lu")
	assert l.shape == shape and np.array_equal(np.asarray(l), np.asarray(want[0])) and np.array_equal(np.asarray(u), np.asarray(want[1]))

# ---- GPU ------------------------------------------------------------------------------------------------------------------------
def cuda(a):
	import torch
	return torch.as_tensor(a, device="cuda")

@pytest.fixture(scope="module")
def mm(fx, golden_dir):
	"""the reference's test_lensing inputs: 1-degree CC, lmax 400, lensing.rand_alm(seed=1) drawn here and pinned to the fixtures"""
	phi, cmb, ai = lensing.rand_alm(fx["m_ps"], lmax=400, seed=1, ncomp=3)
	ref_cmb = np.load(os.path.join(golden_dir, "lens_unlensed.npz"))["alm"]      # (to the bound of tests/test_almops.py on rand_alm, scaled to the alm)
	assert np.allclose(phi[::64], fx["m_phi_sub"], rtol=1e-11, atol=1e-13*np.abs(fx["m_phi_sub"]).max())
	assert np.allclose(cmb, ref_cmb, rtol=1e-11, atol=1e-13*np.abs(ref_cmb).max())
	shape, wcs = geometry(fx["g_geo"], (3,))
	return dict(phi=phi, cmb=cmb, shape=shape, wcs=wcs)

@pytest.mark.gpu
def test_deflect_gpu(fx):
	deflect_body(fx, cuda)
	deflect_body(fx, lambda a: a)      # host arrays in, host arrays out
	# the reference test's own shape: 1-degree CC (181 x 360), gradient 1e-3 * random
	shape, wcs = geometry(fx["g_geo"])
	grad = 1e-3*np.random.default_rng(11).random((2,)+shape)
	assert np.array_equal(grad[:, 0, :8], fx["g_grad_head"])
	pos = np.asarray(enmap.posmap(shape, wcs))
	rows = slice(None, None, 12)
	check_deflect(lensing.offset_by_grad(cuda(pos), cuda(grad), pol=True), pos, grad, fx["g_out12"], 2/181, rows=rows, what="1 degree positions")
	loc, psi = lensing.offset_by_grad(None, cuda(grad), pol=True, _loc=True, _geometry=(shape, wcs))
	assert loc.is_cuda and psi.is_cuda
	check_deflect(from_loc(loc, psi, shape), pos, grad, fx["g_out12"], 2/181, rows=rows, what="1 degree geometry")
	d = enmap.posmap(shape, wcs, device="cuda")
	assert isinstance(d, enmap.dmap) and np.array_equal(host(d), pos)

@pytest.mark.gpu
def test_rotate_pol_gpu(fx):
	rotate_body(fx, cuda)
	rotate_body(fx, lambda a: a)

@pytest.mark.gpu
def test_lens_map_curved_gpu(fx, mm):
	"""the reference's test_lensing shape with device tensors in: against the expected map of the fixture (every 4th row)"""
	import torch
	shape, wcs = mm["shape"], mm["wcs"]
	l, a = lensing.lens_map_curved(shape, wcs, cuda(mm["phi"]), cuda(mm["cmb"]), output="la", epsilon=EPS)
	assert isinstance(l, enmap.dmap) and l.tensor.is_cuda and l.shape == shape and isinstance(a, enmap.dmap) and a.shape == (2,)+shape[-2:]
	pos = np.asarray(enmap.posmap(shape, wcs))
	ok = covered(pos, host(a))
	assert 1-ok.mean() <= 2/181+1e-12
	errs = rel_groups(host(l)[:, ::4], fx["m_lensed4"], ok[::4])
	print("lensed vs expected: T %.2e  QU %.2e" % tuple(errs))
	assert max(errs) <= 2*EPS
	check_excluded(l, a, shape, wcs, mm["cmb"], 400, 2/181, oracle=False)
	# the reference's recorded result of its own test_lensing (tests/data/MM_lensed_071123.fits, every 4th row), with its own np.isclose;
	# the two pole rows left out
	rec = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lensing_recorded.npz"))["lensed4"]
	assert np.all(np.isclose(host(l)[:, ::4][:, 1:-1], rec[:, 1:-1]))
	# host arrays in, host maps out: the same numbers
	lh, = lensing.lens_map_curved(shape, wcs, mm["phi"], mm["cmb"], epsilon=EPS)
	assert isinstance(lh, enmap.ndmap) and max(rel_groups(lh, host(l), slice(None))) <= 2*EPS

@pytest.mark.gpu
def test_bands_gpu(mm, monkeypatch):
	bands_body(mm["shape"], mm["wcs"], cuda(mm["phi"]), cuda(mm["cmb"]), np.deg2rad(70), 72, monkeypatch)      # 181 rows in bands of 72, 72, 37

@pytest.mark.gpu
def test_side_stream_gpu(mm):
	"""one lens_map_curved on a stream of its own: positions and angles bit for bit those of the default stream, the map to epsilon"""
	import torch
	shape, wcs = mm["shape"], mm["wcs"]
	phi, cmb = cuda(mm["phi"]), cuda(mm["cmb"])
	l0, a0 = lensing.lens_map_curved(shape, wcs, phi, cmb, output="la", epsilon=EPS)
	loc0, psi0 = lensing.offset_by_grad(None, a0, pol=True, _loc=True, _geometry=(shape, wcs))
	torch.cuda.synchronize()
	side = torch.cuda.Stream()
	with torch.cuda.stream(side):
		l1, a1 = lensing.lens_map_curved(shape, wcs, phi, cmb, output="la", epsilon=EPS)
		loc1, psi1 = lensing.offset_by_grad(None, a0, pol=True, _loc=True, _geometry=(shape, wcs))
	side.synchronize()
	assert torch.equal(loc0, loc1) and torch.equal(psi0, psi1)
	errs = rel_groups(l1, host(l0), slice(None))
	assert max(errs) <= EPS, errs

@pytest.mark.gpu
def test_phi_kappa_roundtrip_gpu():
	kappa_body(lambda a: a); kappa_body(cuda)

@pytest.mark.gpu
def test_rand_alm_bit_exact_gpu(fx):
	rand_alm_body(fx, np.array_equal)
