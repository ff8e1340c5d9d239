"""pixell_amd.reproject.thumbnails / thumbnails_ivar (pxm_thumbnails, one launch per catalogue), enmap.thumbnail_geometry, enmap.pixsizemap,
wcs.TanWCS and pxm_spline_filter_axes: against the reference's whole-map definition of tests/golden/make_thumbnails.py (fixture thumbnails.npz),
against the unfused device path (enmap.at + enmap.rotate_pol at positions and angles formed in numpy from the closed form), and against the
dense solve that defines the coefficients.

Tolerance, per object (f the map, c the array the taps read: the dense coefficients at order 3, f at orders 0 and 1; ny, nx the map's shape):
    tol = 4 E_ref max|f| + 64 2^-52 max|c| + max(8, 4 K_pos) 2^-52 max(ny, nx) max|dc|        (+ 2 dang[obj] max|f| for Q and U)
  E_ref, 2nd and 3rd term: as in test_interpol.py (restated below); K_pos: how far the reference's own pixel coordinates are from the
  closed form evaluated in numpy, in ulps of max(ny, nx) (the fixture: 5.12), so that the third term allows the device as much again
  dang      a spin-2 rotation by an angle that is off by d moves (Q, U) by 2 d |P|, and the reference's finite-difference angle is off the
            closed form by dang[obj] (2e-8 .. 7e-6 rad): the reference's error, not the device's
  float32 results (orders 0, 1 on float32 maps) may in addition round the other way: + 2^-24 max|f|
  Order 0 without rotation is exact; with it, I is exact and Q, U carry the rotation's terms (2 dang max|f| + 64 2^-52 max|f|, float32 term).
Fused against unfused: the same coefficients and the closed-form angle on both sides, so E_ref and dang are zero there.  This is what pins
TAN thumbnails: the reference cannot be driven on TAN without astropy, and TAN parity with astropy is unpinned.

Each body runs in the host simulator (*_sim, here) and on the GPU (*_gpu).  Worst error / tol over the cases of each body, as the tests print them:
                          host simulator      MI355X
  fixture G, A            0.499             0.499   (A, float32, order 1, object 2)
  fixture, rotated Q U    0.651             0.651   (A, float64, order 3, object 2)
  fused against unfused   0.250             0.250   (G, float32, order 1, TAN, rotated)
  launch shapes           0.005             0.006   (nobj = 70000 | nobj = 1)
  filter per axis         0.042             0.042   ((293, 309) float32 (constant, grid-wrap))

The fixture's Q and U span half of T's range, so that |P| = hypot(Q, U) stays below max|f| wherever the maps are read (0.43 .. 0.76 max|f|
as gathered), which the dang term presumes: two components of the full range reach 1.2 .. 1.5 max|f| at order 3 and would miss it for a
reason that is not the device's (make_thumbnails.py).  Rotated Q, U error over that term alone: 0.22 .. 0.65.
"""
import os
import numpy as np
import pytest
from pixell_amd import enmap, interpol, reproject, wcs as wcsutils
from pixell_amd.wcs import CarWCS, TanWCS

EPS = 2.0**-52
degree = np.pi/180
ORDERS = (0, 1, 3)
R2 = np.sqrt(2.0)      # a rotation mixes the errors of two components

@pytest.fixture(scope="module")
def fx(golden_dir):
	return dict(np.load(os.path.join(golden_dir, "thumbnails.npz")))

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

# ---- the definition of the coefficients, and the tolerance (as in test_interpol.py, with one extension rule per axis) ----------------
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
def dense_coefficients(f, rules, key=None):
	"""the float64 solution of B c = f along the last two axes of f under the extension rules (y, x) (kept per key)"""
	if key is not None and (key, rules) in _dense: return _dense[(key, rules)]
	f = np.asarray(f, np.float64)
	c = np.linalg.solve(collocation(f.shape[-2], rules[0]), np.moveaxis(f, -2, 0).reshape(f.shape[-2], -1)).reshape((f.shape[-2],)+f.shape[:-2]+f.shape[-1:])
	c = np.moveaxis(c, 0, -2)
	c = np.linalg.solve(collocation(f.shape[-1], rules[1]), np.moveaxis(c, -1, 0).reshape(f.shape[-1], -1)).reshape((f.shape[-1],)+f.shape[:-1])
	c = np.ascontiguousarray(np.moveaxis(c, 0, -1))
	if key is not None: _dense[(key, rules)] = c
	return c

def tol_of(eref, kpos, f, c, f32_out=False):
	f, c = np.asarray(f, np.float64), np.asarray(c, np.float64)
	dc = max([float(np.max(np.abs(np.diff(c, axis=a)))) for a in (-2, -1) if c.shape[a] > 1]+[0.0])
	t = 4*eref*np.max(np.abs(f))+64*EPS*np.max(np.abs(c))+max(8.0, 4*kpos)*EPS*max(c.shape[-2:])*dc
	return t+(2.0**-24*np.max(np.abs(f)) if f32_out else 0.0)

def rules_of(shape, wcs): return ("mirror", "periodic" if reproject.borders(shape, wcs)[1] == "grid-wrap" else "mirror")

class Worst:
	"""the largest error / tol of a body's cases"""
	def __init__(self, name, defer=False): self.name, self.ratio, self.where, self.defer, self.missed = name, 0.0, "", defer, []      # (defer: assert in report(), after every case)
	def check(self, tag, got, want, tol):
		got, want = np.float64(host(got)), np.float64(want)
		assert got.shape == want.shape, (tag, got.shape, want.shape)
		err = float(np.max(np.abs(got-want))) if got.size else 0.0
		print("%s: worst error %.3g (tol %.3g)" % (tag, err, tol))
		if tol > 0 and err/tol > self.ratio: self.ratio, self.where = err/tol, tag
		if self.defer and err > tol: self.missed.append("%s: %.3g > %.3g" % (tag, err, tol))
		else: assert err <= tol, tag
	def report(self):
		print("%s: worst error / tol = %.3f (%s)" % (self.name, self.ratio, self.where))
		assert not self.missed, self.missed

# ---- the closed form, in numpy --------------------------------------------------------------------------------------------------
def closed_form(oshape, owcs, obj):
	"""(dec, ra, psi) [oy, ox] of the pixels of a CAR or TAN thumbnail geometry centred on (0, 0) once its centre is put on obj = (dec, ra):
	the direction v of a pixel and the east vector e there, rotated by Rz(ra) Ry(-dec); psi the angle of R e in the (east, north) frame at R v"""
	j, i = np.mgrid[:oshape[-2], :oshape[-1]]
	x = (i+1-owcs.wcs.crpix[0])*owcs.wcs.cdelt[0]*degree; y = (j+1-owcs.wcs.crpix[1])*owcs.wcs.cdelt[1]*degree
	if wcsutils.get_proj(owcs) == "car": v = [np.cos(y)*np.cos(x), np.cos(y)*np.sin(x), np.sin(y)]; e = [-np.sin(x), np.cos(x), 0*x]
	else:
		rv, re = 1/np.sqrt(1+x*x+y*y), 1/np.sqrt(1+x*x)
		v = [rv, x*rv, y*rv]; e = [-x*re, re, 0*x]
	sd, cd, sr, cr = np.sin(obj[0]), np.cos(obj[0]), np.sin(obj[1]), np.cos(obj[1])
	def rot(a):
		x1 = cd*a[0]-sd*a[2]
		return cr*x1-sr*a[1], sr*x1+cr*a[1], sd*a[0]+cd*a[2]
	V, E = rot(v), rot(e)
	ce = V[0]*E[1]-V[1]*E[0]; cn = (V[0]**2+V[1]**2)*E[2]-V[2]*(V[0]*E[0]+V[1]*E[1])
	return np.arctan2(V[2], np.hypot(V[0], V[1])), np.arctan2(V[1], V[0]), np.arctan2(cn, ce)

def unfused(m, dev, objs, oshape, owcs, ip, pol):
	"""[nobj, {pre}, oy, ox]: enmap.at at the closed form's positions of all objects in one call, then enmap.rotate_pol by -psi"""
	cf = np.array([closed_form(oshape, owcs, o) for o in objs]).reshape((-1, 3)+tuple(oshape))      # [nobj, {dec,ra,psi}, oy, ox]
	v = enmap.at(m, dev(np.ascontiguousarray(np.moveaxis(cf[:, :2], 1, 0))), ip=ip)      # [{pre}, nobj, oy, ox]
	v = np.ascontiguousarray(np.moveaxis(host(v), -3, 0))
	return host(enmap.rotate_pol(dev(v), dev(np.ascontiguousarray(-cf[:, 2])))) if pol else v

# ---- bodies ---------------------------------------------------------------------------------------------------------------------
def fixture_body(fx, dev, on_device, rotated):
	"""the reference's whole-map definition on the maps G (full sky, across the seam, near the pole) and A (a patch, over its edge).
	rotated = False: every component without the rotation; with it, I, and Q, U through the reference's own angle: the device's unrotated
	values, rotated here in numpy by the angle map the fixture records, are the reference's to the unrotated tolerance (times sqrt(2): a
	rotation mixes two components' errors).  rotated = True: Q, U as the device rotates them, by the closed form's angle, under the bound
	the feature was specified with, + 2 dang[obj] max|f|; every case is printed before the body asserts"""
	eref, kpos = float(fx["E_ref"]), float(fx["K_pos"]); W = Worst("fixture G, A"+(", rotated Q U" if rotated else ""), defer=rotated)
	mapkind = enmap.dmap if on_device else enmap.ndmap
	for g in ("G", "A"):
		shape, wcs = geometry(fx[g+"_geo"], (3,))
		oshape, owcs = geometry(fx[g+"_tgeo"])
		objs, dang = fx[g+"_obj"], fx["dang_"+g]
		c2, s2 = np.cos(2*fx[g+"_ang"]), np.sin(2*fx[g+"_ang"])
		for dt, tag in ((np.float64, "f8"), (np.float32, "f4")):
			f = fx[g+"_map"].astype(dt)
			m = as_map(dev, f, wcs)
			fmax = float(np.max(np.abs(f)))
			for order in ORDERS:
				odt = np.float64 if order == 3 else dt
				c = dense_coefficients(f, rules_of(shape, wcs), key=g) if order == 3 else f
				base = tol_of(eref, kpos, f, c, f32_out=odt == np.float32)
				want = fx["%s_%d_pol" % (g, order)]
				res = reproject.thumbnails(m, dev(objs), oshape=oshape, owcs=owcs, order=order, pol=True)
				assert isinstance(res, mapkind) and res.shape == (len(objs), 3)+oshape and res.dtype == odt and res.wcs is owcs
				got = host(res)
				if rotated:
					for k in range(len(objs)):
						name = "%s %s order %d object %d Q U" % (g, tag, order, k)
						# order 0: the gathered values are exact; what is left is the rotation's roundings and what an angle that is off does
						if order == 0: W.check(name, got[k, 1:], want[k, 1:], 2*dang[k]*fmax+64*EPS*fmax+(2.0**-24*fmax if odt == np.float32 else 0.0))
						else: W.check(name, got[k, 1:], want[k, 1:], base+2*dang[k]*fmax)
					continue
				plain = reproject.thumbnails(m, dev(objs), oshape=oshape, owcs=owcs, order=order, pol=False)
				assert isinstance(plain, mapkind) and plain.shape == res.shape and plain.dtype == odt
				un = np.float64(host(plain))
				byref = np.array([un[:, 0], c2*un[:, 1]+s2*un[:, 2], c2*un[:, 2]-s2*un[:, 1]]).transpose(1, 0, 2, 3)      # rotate_pol(., -ang)
				assert np.array_equal(got[:, 0], host(plain)[:, 0])      # I is not touched by the rotation
				for k in range(len(objs)):
					name = "%s %s order %d object %d" % (g, tag, order, k)
					if order == 0: assert np.array_equal(host(plain)[k], fx["%s_0" % g][k]), name
					else: W.check(name, plain[k], fx["%s_%d" % (g, order)][k], base)
					W.check(name+" Q U by the reference's angle", byref[k, 1:], want[k, 1:], R2*(base if order else 64*EPS*fmax))
		assert np.any(fx[g+"_3"] == 0) == (g == "A")      # (cval appears where the thumbnail hangs over the patch)
	print("the reference's own thumbnails on apodised cut-outs (for the record): off its whole-map values by %.3g" % np.max(np.abs(np.float64(fx["thumbs_block"])-fx["G_3_pol"])))
	W.report()

def fused_body(fx, dev, on_device):
	"""thumbnails(ip=ip) against enmap.at(ip=ip) + rotate_pol on the same interpolator, CAR and TAN thumbnails"""
	kpos = float(fx["K_pos"]); W = Worst("fused against unfused")
	rng = np.random.default_rng(11)
	for g, border in (("G", "grid-wrap"), ("A", "constant")):
		shape, wcs = geometry(fx[g+"_geo"], (3,))
		objs = np.concatenate([fx[g+"_obj"], (np.array([[79.8, -33.3], [-61.2, 120.7]]) if g == "G" else np.array([[40.2, -3.9], [55.5, 30.1]]))*degree])
		for dt in (np.float64, np.float32):
			f = fx[g+"_map"].astype(dt)
			m = as_map(dev, f, wcs)
			for order in (1, 3):
				ip = interpol.interpolator(m, npre=1, order=order, border=border, cval=0.0)
				c = host(ip.arr)
				odt = np.float64 if order == 3 else dt
				tol = tol_of(0.0, kpos, f, c, f32_out=odt == np.float32)
				tol_rot = tol+(3*2.0**-24*np.max(np.abs(f)) if odt == np.float32 else 0.0)      # (the unfused path rounds to float32 twice)
				for proj, r, res in (("car", (3*degree, 4.1*degree), 0.7*degree), ("tan", 5*degree, (0.9*degree, -0.6*degree))):
					oshape, owcs = enmap.thumbnail_geometry(r=r, res=res, proj=proj)
					for pol in (True, False):
						got = reproject.thumbnails(m, dev(objs), oshape=oshape, owcs=owcs, pol=pol, ip=ip)
						assert host(got).dtype == odt
						W.check("%s %s order %d %s pol %d" % (g, np.dtype(dt).name, order, proj, pol), got, unfused(m, dev, objs, oshape, owcs, ip, pol), tol_rot if pol else tol)
	W.report()

def shapes_body(fx, dev, on_device):
	"""the shapes where the launch can go wrong: one object, none, more than 65 535, a 1 x 1 thumbnail, coords with leading axes"""
	kpos = float(fx["K_pos"]); W = Worst("launch shapes")
	shape, wcs = geometry(fx["G_geo"], (3,))
	f = fx["G_map"]
	m = as_map(dev, f, wcs)
	ip = interpol.interpolator(m, npre=1, order=3, border="grid-wrap")
	tol = tol_of(0.0, kpos, f, host(ip.arr))
	objs = fx["G_obj"]
	o13, w13 = enmap.thumbnail_geometry(r=6*degree, res=1*degree, proj="car")
	o1, w1 = enmap.thumbnail_geometry(res=1*degree, shape=(1, 1), proj="tan")
	assert o13 == (13, 13) and o1 == (1, 1)
	one = reproject.thumbnails(m, dev(objs[2]), oshape=o13, owcs=w13, ip=ip)      # coords [2]: one thumbnail, no leading axis
	assert one.shape == (3, 13, 13)
	W.check("nobj = 1", reproject.thumbnails(m, dev(objs[2:3]), oshape=o13, owcs=w13, ip=ip), unfused(m, dev, objs[2:3], o13, w13, ip, True), tol)
	assert np.array_equal(host(one), host(reproject.thumbnails(m, dev(objs[2:3]), oshape=o13, owcs=w13, ip=ip))[0])
	W.check("1 x 1", reproject.thumbnails(m, dev(objs), oshape=o1, owcs=w1, ip=ip), unfused(m, dev, objs, o1, w1, ip, True), tol)
	# a 1 x 1 thumbnail is the map at the object, unrotated: psi = 0 at the centre
	at = host(enmap.at(m, dev(np.ascontiguousarray(objs.T)), ip=ip))
	W.check("1 x 1 against at", host(reproject.thumbnails(m, dev(objs), oshape=o1, owcs=w1, ip=ip))[:, :, 0, 0], at.T, tol)
	c232 = np.concatenate([objs, objs[:1]]).reshape(2, 3, 2)
	r232 = reproject.thumbnails(m, dev(c232), oshape=o13, owcs=w13, ip=ip)
	assert r232.shape == (2, 3, 3, 13, 13)
	assert np.array_equal(host(r232).reshape(6, 3, 13, 13)[:5], host(reproject.thumbnails(m, dev(objs), oshape=o13, owcs=w13, ip=ip)))
	none = reproject.thumbnails(m, dev(np.zeros((0, 2))), oshape=o13, owcs=w13, ip=ip)
	assert none.shape == (0, 3, 13, 13) and none.dtype == np.float64
	# 70 000 objects of 3 x 3 on a one-component map: past the 65 535 of a grid's second dimension
	rng = np.random.default_rng(70000)
	m1 = as_map(dev, f[0], wcs)
	ip1 = interpol.interpolator(m1, npre=0, order=3, border="grid-wrap")
	many = np.array([rng.uniform(-85, 85, 70000), rng.uniform(-180, 180, 70000)]).T*degree
	o3, w3 = enmap.thumbnail_geometry(res=0.8*degree, shape=(3, 3), proj="tan")
	big = reproject.thumbnails(m1, dev(many), oshape=o3, owcs=w3, ip=ip1)
	assert big.shape == (70000, 3, 3)
	pick = np.sort(np.concatenate([rng.choice(70000, 198, replace=False), [0, 69999]]))
	W.check("nobj = 70000", host(big)[pick], unfused(m1, dev, many[pick], o3, w3, ip1, False), tol_of(0.0, kpos, f[0], host(ip1.arr)))
	W.report()

def api_body(fx, dev, on_device, monkeypatch):
	eref, kpos = float(fx["E_ref"]), float(fx["K_pos"])
	shape, wcs = geometry(fx["G_geo"], (3,))
	f, objs = fx["G_map"], fx["G_obj"]
	m = as_map(dev, f, wcs)
	oshape, owcs = geometry(fx["G_tgeo"])
	mapkind = enmap.dmap if on_device else enmap.ndmap
	# defaults: proj "car", res half the map's pixel, r 5': 1 degree pixels of radius 5' round to a single pixel
	d = reproject.thumbnails(m, dev(objs))
	assert isinstance(d, mapkind) and d.shape == (5, 3, 1, 1) and wcsutils.get_proj(d.wcs) == "car" and np.allclose(d.wcs.wcs.cdelt, [-1, 1])
	t = reproject.thumbnails(m, dev(objs), r=3*degree, proj="tan")
	assert t.shape == (5, 3, 7, 7) and wcsutils.get_proj(t.wcs) == "tan" and t.dtype == np.float64
	# kinds and dtypes
	for dt in (np.float32, np.float64):
		for order in ORDERS:
			r = reproject.thumbnails(as_map(dev, f.astype(dt), wcs), dev(objs), oshape=oshape, owcs=owcs, order=order)
			assert isinstance(r, mapkind) and r.dtype == (np.float64 if order == 3 else dt)
	im = (np.abs(f[0])*200).astype(np.uint8)
	r = reproject.thumbnails(as_map(dev, im, wcs), dev(objs), oshape=oshape, owcs=owcs, order=0)
	assert r.dtype == np.uint8 and np.array_equal(host(r), (np.abs(fx["G_0"][:, 0])*200).astype(np.uint8))
	if on_device:
		assert isinstance(reproject.thumbnails(enmap.ndmap(f, wcs), objs, oshape=oshape, owcs=owcs), enmap.ndmap)
		assert isinstance(reproject.thumbnails(enmap.ndmap(f, wcs), dev(objs), oshape=oshape, owcs=owcs), enmap.dmap)
		assert isinstance(reproject.thumbnails(m, objs, oshape=oshape, owcs=owcs), enmap.dmap)
	# the pol rule
	full = host(reproject.thumbnails(m, dev(objs), oshape=oshape, owcs=owcs))
	assert np.array_equal(full, host(reproject.thumbnails(m, dev(objs), oshape=oshape, owcs=owcs, pol=True)))
	assert not np.array_equal(full, host(reproject.thumbnails(m, dev(objs), oshape=oshape, owcs=owcs, pol=False)))
	m2 = as_map(dev, f[:2], wcs)
	assert np.array_equal(host(reproject.thumbnails(m2, dev(objs), oshape=oshape, owcs=owcs)), host(reproject.thumbnails(m, dev(objs), oshape=oshape, owcs=owcs, pol=False))[:, :2])
	with pytest.raises(ValueError): reproject.thumbnails(m2, dev(objs), oshape=oshape, owcs=owcs, pol=True)
	with pytest.raises(ValueError): reproject.thumbnails(as_map(dev, f[0], wcs), dev(objs), oshape=oshape, owcs=owcs, pol=True)
	# [2, 3, ny, nx]: each leading entry rotates its own Q, U
	m23 = as_map(dev, np.array([f, 2*f]), wcs)
	r23 = host(reproject.thumbnails(m23, dev(objs), oshape=oshape, owcs=owcs))
	assert r23.shape == (5, 2, 3)+oshape and np.array_equal(r23[:, 0], full) and np.array_equal(r23[:, 1], 2*full)
	# ip= reuse: no filter launch after the interpolator is made, and the same values bit for bit
	calls = []
	real = interpol._filter
	monkeypatch.setattr(interpol, "_filter", lambda d, border: (calls.append(border), real(d, border))[1])
	ip = reproject.interpolator(m)
	assert calls == [("constant", "grid-wrap")] and ip.order == 3 and ip.npre == 1
	a1 = reproject.thumbnails(m, dev(objs[:3]), oshape=oshape, owcs=owcs, ip=ip); a2 = reproject.thumbnails(m, dev(objs[3:]), oshape=oshape, owcs=owcs, ip=ip)
	assert len(calls) == 1 and np.array_equal(np.concatenate([host(a1), host(a2)]), full)
	reproject.thumbnails(m, dev(objs), oshape=oshape, owcs=owcs); assert len(calls) == 2
	with pytest.raises(NotImplementedError): enmap.at(m, dev(objs.T), ip=ip)      # (a border per axis is the thumbnails' own)
	with pytest.raises(ValueError): reproject.thumbnails(m2, dev(objs), oshape=oshape, owcs=owcs, ip=ip)
	monkeypatch.undo()
	# thumbnails_ivar, extensive
	iv = reproject.thumbnails_ivar(m, dev(objs), oshape=oshape, owcs=owcs)
	assert np.array_equal(host(iv), host(reproject.thumbnails(m, dev(objs), oshape=oshape, owcs=owcs, order=1, pol=False, extensive=True)))
	assert not np.array_equal(host(iv), host(reproject.thumbnails(m, dev(objs), oshape=oshape, owcs=owcs, order=1, pol=False)))
	ps = np.asarray(enmap.pixsizemap(shape, wcs))
	pt = np.asarray(enmap.pixsizemap(oshape, owcs))
	ones = as_map(dev, np.ones(shape[-2:])*ps, wcs)
	for order in (1, 3):
		got = host(reproject.thumbnails(ones, dev(objs[:2]), oshape=oshape, owcs=owcs, order=order, extensive=True))
		one = np.ones(shape[-2:])
		assert got.shape == (2,)+oshape and np.max(np.abs(got-pt)) <= tol_of(eref, kpos, one, one)*pt.max(), order
	# what is refused, and that the message says what to pass instead
	for kw, word in ((dict(method="mixed"), "spline"), (dict(method="nufft"), "spline"), (dict(filter=lambda x: x), "filter=None"), (dict(pixwin=True), "pixwin=False"),
			(dict(extensive=True, proj="tan", r=3*degree), "car")):
		with pytest.raises(NotImplementedError, match=word): reproject.thumbnails(m, dev(objs), **kw)
	assert np.array_equal(host(reproject.thumbnails(m, dev(objs), oshape=oshape, owcs=owcs, method="mixed", oversample=1)), full)
	assert np.array_equal(host(reproject.thumbnails(m, dev(objs), oshape=oshape, owcs=owcs, apod=1*degree)), full)      # (apod has no effect)
	with pytest.raises(ValueError): reproject.thumbnails(m, dev(objs), method="cubic")
	with pytest.raises(ValueError): reproject.thumbnails(m, dev(objs.T[:, :3]), oshape=oshape, owcs=owcs)      # [..., 3]
	with pytest.raises(ValueError): reproject.thumbnails(m, dev(objs), oshape=oshape, owcs=CarWCS(cdelt=[-1, 1], crval=[10, 0], crpix=[7, 7]))
	tilted = CarWCS(cdelt=wcs.wcs.cdelt, crval=[wcs.wcs.crval[0], 10.0], crpix=wcs.wcs.crpix)
	with pytest.raises(NotImplementedError): reproject.thumbnails(as_map(dev, f, tilted), dev(objs))

def geometry_body(fx):
	"""enmap.thumbnail_geometry and enmap.pixsizemap against the reference's numbers; the TAN stand-in"""
	cases = {"tg_r_res": dict(r=6*degree, res=1*degree), "tg_res_shape": dict(res=0.25*degree, shape=(8, 12)), "tg_r_shape": dict(r=np.array([2.0, 3.0])*degree, shape=(9, 14)),
		"tg_r_res2": dict(r=np.array([2.2, 3.4])*degree, res=np.array([0.5, -0.25])*degree)}
	for key, kw in cases.items():
		shape, wcs = enmap.thumbnail_geometry(proj="car", **kw)
		want = fx[key]
		assert shape == (int(want[0]), int(want[1])) and shape[0] % 2 == 1 and shape[1] % 2 == 1, key
		assert np.allclose(wcs.wcs.cdelt, want[2:4], rtol=1e-14, atol=0) and np.array_equal(wcs.wcs.crpix, want[4:6]) and np.all(wcs.wcs.crval == 0), key
		assert np.array_equal(wcs.wcs.crpix, np.array(shape[::-1])//2+1) and wcsutils.is_car(wcs)
		assert np.allclose(enmap.pix2sky(shape, wcs, [shape[0]//2, shape[1]//2]), 0, atol=1e-15)      # the centre lies on pixel shape//2
	assert enmap.thumbnail_geometry(r=1*degree, res=0.5*degree, dims=(3,))[0] == (3, 5, 5)
	with pytest.raises(ValueError): enmap.thumbnail_geometry(r=1*degree)
	with pytest.raises(NotImplementedError): enmap.thumbnail_geometry(r=1*degree, res=0.5*degree, proj="zea")
	for g in ("A", "G"):
		shape, wcs = geometry(fx[g+"_geo"])
		ps = enmap.pixsizemap(shape, wcs)
		assert isinstance(ps, enmap.ndmap) and ps.shape == shape and np.allclose(ps[:, 0], fx["psize_"+g], rtol=1e-14, atol=0) and np.all(np.asarray(ps) == np.asarray(ps)[:, :1])
		assert enmap.pixsizemap(shape, wcs, broadcastable=True).shape == (shape[0], 1)
		assert abs(np.sum(ps)-enmap.area(shape, wcs)) < 1e-12*enmap.area(shape, wcs)
	oshape, owcs = geometry(fx["G_tgeo"])
	assert np.allclose(enmap.pixsizemap(oshape, owcs)[:, 0], fx["psize_T"], rtol=1e-14, atol=0)
	# the TAN stand-in
	shape, tan = enmap.thumbnail_geometry(r=5*degree, res=0.5*degree)      # (proj "tan" is the default here, as in the reference)
	assert isinstance(tan, TanWCS) and wcsutils.get_proj(tan) == "tan" and not wcsutils.is_separable(tan) and shape[0] % 2 == 1
	assert np.allclose(tan.wcs.cdelt, [-0.5, 0.5]) and np.array_equal(tan.wcs.crpix, np.array(shape[::-1])//2+1)
	ra, dec = tan.wcs_pix2world(shape[1]//2, shape[0]//2, 0)
	assert ra == 0 and dec == 0
	x, y = np.meshgrid(np.arange(shape[1])+0.25, np.arange(shape[0])-0.4)
	ra, dec = tan.wcs_pix2world(x, y, 0)
	bx, by = tan.wcs_world2pix(ra, dec, 0)
	assert np.max(np.abs(bx-x)) < 1e-11 and np.max(np.abs(by-y)) < 1e-11
	xi, eta = (x+1-tan.wcs.crpix[0])*tan.wcs.cdelt[0]*degree, (y+1-tan.wcs.crpix[1])*tan.wcs.cdelt[1]*degree      # gnomonic: the direction is (1, xi, eta)
	v = np.array([np.cos(dec*degree)*np.cos(ra*degree), np.cos(dec*degree)*np.sin(ra*degree), np.sin(dec*degree)])
	assert np.max(np.abs(v[1]/v[0]-xi)) < 1e-15 and np.max(np.abs(v[2]/v[0]-eta)) < 1e-15
	assert np.all(np.isnan(tan.wcs_world2pix(170.0, 0.0, 0)))      # the far hemisphere has no pixel
	cp = tan.deepcopy(); cp.wcs.crpix[0] += 1
	assert isinstance(cp, TanWCS) and cp.wcs.crpix[0] == tan.wcs.crpix[0]+1 and repr(tan).startswith("tan:{cdelt:")
	with pytest.raises(ValueError): TanWCS(cdelt=[-1, 1], crval=[10, 0], crpix=[1, 1])
	for fn in (lambda: enmap.posmap(shape, tan), lambda: enmap.pixsizemap(shape, tan), lambda: enmap.area(shape, tan)):
		with pytest.raises(NotImplementedError): fn()

def filter_axes_body(fx, dev, on_device):
	"""pxm_spline_filter_axes: equal rules give the bits of pxm_spline_filter; (mirror, periodic) gives the dense solve per axis"""
	eref = float(fx["E_ref"]); W = Worst("filter per axis")
	cy, cx = interpol.CHUNK
	rng = np.random.default_rng(3)
	for shape in ((cy+37, cx+53), (5, 7), (1, 9)):
		f = rng.integers(-2**20, 2**20, (2,)+shape).astype(np.float64)/2**20
		for dt in (np.float32, np.float64):
			for border in ("mirror", "nearest", "grid-wrap"):
				assert np.array_equal(host(interpol.spline_filter(dev(f.astype(dt)), border=(border, border))), host(interpol.spline_filter(dev(f.astype(dt)), border=border))), (shape, border)
			for by, bx in (("constant", "grid-wrap"), ("grid-wrap", "nearest")):
				rules = tuple({"constant": "mirror", "grid-wrap": "periodic", "nearest": "reflect"}[b] for b in (by, bx))
				dense = dense_coefficients(f, rules)
				c = interpol.spline_filter(dev(f.astype(dt)), border=(by, bx))
				assert hasattr(c, "data_ptr") == on_device and host(c).dtype == np.float64
				W.check("%s %s (%s, %s)" % (shape, np.dtype(dt).name, by, bx), c, dense, 4*eref*np.max(np.abs(f))+64*EPS*np.max(np.abs(dense)))
	with pytest.raises(ValueError): interpol.spline_filter(dev(f), border=("mirror", "zero"))
	with pytest.raises(ValueError): interpol.spline_filter(dev(f), border=("mirror",))
	W.report()

# ---- host simulator -------------------------------------------------------------------------------------------------------------
@pytest.mark.hostsim
def test_fixture_thumbnails_sim(fx): fixture_body(fx, ident, False, False)
@pytest.mark.hostsim
def test_fixture_rotated_sim(fx): fixture_body(fx, ident, False, True)
@pytest.mark.hostsim
def test_fused_against_unfused_sim(fx): fused_body(fx, ident, False)
@pytest.mark.hostsim
def test_launch_shapes_sim(fx): shapes_body(fx, ident, False)
@pytest.mark.hostsim
def test_api_sim(fx, monkeypatch): api_body(fx, ident, False, monkeypatch)
@pytest.mark.hostsim
def test_filter_axes_sim(fx): filter_axes_body(fx, ident, False)
def test_thumbnail_geometry_pixsizemap_tan(fx): geometry_body(fx)

# ---- GPU ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_fixture_thumbnails_gpu(fx): fixture_body(fx, cuda, True, False)
@pytest.mark.gpu
def test_fixture_rotated_gpu(fx): fixture_body(fx, cuda, True, True)
@pytest.mark.gpu
def test_fused_against_unfused_gpu(fx): fused_body(fx, cuda, True)
@pytest.mark.gpu
def test_launch_shapes_gpu(fx): shapes_body(fx, cuda, True)
@pytest.mark.gpu
def test_api_gpu(fx, monkeypatch): api_body(fx, cuda, True, monkeypatch)
@pytest.mark.gpu
def test_filter_axes_gpu(fx): filter_axes_body(fx, cuda, True)
