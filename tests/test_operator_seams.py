"""The operator kernels past their internal scan, list and grid seams: shapes at which a loop over a capacity constant takes its second
trip, a multi-workgroup scan carries from one workgroup to the next, or a grid-stride loop wraps.  The module tests (test_pointsrcs,
test_distances, test_lensing, test_alm2map_pos, test_alm_bank) pin the same kernels to the same models on small fixtures, where every one
of these loops runs once; the models, tolerances and helpers here are theirs.

Two rules hold for every case.  (1) It proves from the model side that it crosses its seam: tile, cell, block and chunk counts follow
from the shape, list lengths from the model's own discs, and each is asserted against its constant.  (2) The constants are read from the
kernel sources (K below), and shapes that are ours to choose are sized from them, so a retuned constant moves the case or fails its
crossing assertion; it cannot silently un-cross the seam.

  seam (code)                                              constant                     smallest crossing shape            case
  scan_dev.hpp scan_counts: carry between scan workgroups  256 SCAN_PER = 1024 counts   > 1024 tiles / cells / edge blocks  S2, D1, D2
  scan_dev.hpp scan_top_kernel: second trip                256 x 1024 = 262 144 counts  > 262 144 tiles / cells / blocks    S3, D1 large, D2 large
  srcsim.hip paint_kernel: second j0 step                  NCH = 64                     a tile with > 64 objects            S1
  srcsim.hip tile_sort_kernel: second e0 / c0 chunk        256 (the workgroup)          a tile with > 256 objects           S1
  srcsim.hip tile_sort / paint: grid-stride, prefetch      SRC_MAXBLK = 2048            > 2048 listed tiles                 S2
  distance.hip pxm_find_edges                              256 EDGE_PER = 1024 pixels   > 1 048 576 pixels                  D2
  distance.hip pxm_distance_from                           TILE = 16 (cells)            > 1024 cells                        D1
  points.hip scan_sums: carry across trips                 256 chunks of 1024 entries   > 1 048 576 points (RS_IPB = 1024)  P1
  lensing.hip deflect / rotate_pol(_vec): grid-stride      DEFLECT_MAXBLK = 2048 x 256  > 524 288 points (pairs of points)  L1
  bank.hip pxa_bank_split / merge: second group of scales  BANK_MAX = 32                > 32 scales                         B1
A kernel that gains a capacity constant gets a row here, its constant in K and a case below.

Bounds.  S1 / S2 forward, per pixel: (64 ULP + n_p 2^-24) S_p, S_p = sum_i |a_i P_i(r)| over the n_p objects that reach the pixel: the
module's 64 ulp for the float32 evaluation of one term plus the worst-case float32 summation term of transpose_body.  That is the bound
on a map that was zero.  On a map that held b_p the prior content is one more term of the float32 sum (as test_alm_bank counts it for
accumulate), rounded against once: 64 ULP S_p + n_p 2^-24 S_p + 2^-24 (|b_p| + S_p), the float32 sum of the objects' terms and one float32
addition of it to b_p (no float32 result can do better than 2^-24 |b_p|; a sum that started from b_p would need n_p times that).
max / min: 64 ULP of the largest |a_i P_i| at the pixel (max and min are 1-Lipschitz in every term).  A float32 numpy evaluation of the
same formulas, summed in ascending object order, is shown to stay inside the bound (S1), so it is not taken from the kernel.  The guard
band of the radial sums (S2) is 32 ULP max(r_last, pixel): twice the module's own bound on the float32 distance (16 ulp).

Measured time per test: the table at the end.  GPU only: S3, the large sizes of D1 and D2, and P1; every other case has its simulator twin.

  case (seconds, fixtures included)   MI355X    simulator
  S1 long lists                       0.3       0.6
  S2 many tiles                       0.8       3.0
  S3 second scan trip                 0.02      -
  D1 cells                            0.4       2.6
  D1 second scan trip                 0.05      -
  D2 edges                            0.5       1.9
  D2 second scan trip                 < 0.01    -
  P1 point sort                       2.1       -
  L1 deflect / rotate_pol             0.2 / 1.0 0.9 / 0.9
  B1 bank groups                      0.7       3.4
"""
import os, re
import numpy as np
import pytest
from pixell_amd import enmap, pointsrcs, distances, lensing, sht
from pixell_amd import _arrays as A
from pixell_amd.wcs import CarWCS, separable_geometry
from test_pointsrcs import dist64, prof64, rcut32, geometry, host, ident, cuda, ULP
from test_distances import vincenty
from test_lensing import vec_deflect, covered, wrap, TOL
import test_alm_bank as tb
import test_alm2map_pos as tp

# ---- the constants, from the kernel sources -------------------------------------------------------------------------------------
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pixell_amd", "csrc")
def source(fname):
	with open(os.path.join(CSRC, fname)) as f: return f.read()
def kconst(fname, name):
	"""`static const(expr) int ..., NAME = value` in a kernel source"""
	m = re.search(r"\bconst(?:expr)?\s+int\s+(?:\w+\s*=\s*\d+\s*,\s*)*%s\s*=\s*(\d+)\s*[;,]" % name, source(fname))
	assert m, "%s: no constant %s" % (fname, name)
	return int(m.group(1))
def kliteral(fname, pattern):
	"""a literal that has no name: every match of the pattern's group, which must all agree"""
	found = set(int(v) for v in re.findall(pattern, source(fname)))
	assert len(found) == 1, "%s: %r matches %s" % (fname, pattern, sorted(found))
	return found.pop()

WG = 256      # lanes of a workgroup: __launch_bounds__(256) of every kernel here
K = dict(
	SCAN_PER=kconst("scan_dev.hpp", "SCAN_PER"), TILE=kconst("srcsim.hip", "TILE"), NCH=kconst("srcsim.hip", "NCH"), SRC_MAXBLK=kconst("srcsim.hip", "SRC_MAXBLK"),
	SORT_CHUNK=kliteral("srcsim.hip", r"\b[ec]0 \+= (\d+)\)"), DTILE=kconst("distance.hip", "TILE"), EDGE_PER=kconst("distance.hip", "EDGE_PER"),
	DEFLECT_MAXBLK=kconst("lensing.hip", "DEFLECT_MAXBLK"), BANK_MAX=kconst("bank.hip", "BANK_MAX"), RS_IPB=kconst("points.hip", "RS_IPB"), PT_T=kconst("points.hip", "PT_T"),
	SCAN_CHUNK=kliteral("points.hip", r"(?:nch = \(L \+ \d+\)/|blockIdx\.x\*(?=\d+ \+ 4\*t)|sums\[i/)(\d+)"))      # the 1024 of scan_chunks, scan_add and their host code
SCAN_WG = WG*K["SCAN_PER"]            # counts per workgroup of scan_counts
SCAN_TRIP = WG*SCAN_WG                # counts per trip of scan_top_kernel
EDGE_BLK = WG*K["EDGE_PER"]           # pixels per edge block
STREAM_TRIP = WG*K["DEFLECT_MAXBLK"]  # points (or pairs of points) per trip of the lensing kernels' grid-stride loops

def test_constants_are_read():
	"""every constant is found in its source, and the scan of the point sort has the chunk its host code assumes"""
	assert all(v > 0 for v in K.values()), K
	assert kliteral("points.hip", r"nch = \(L \+ (\d+)\)/\d+")+1 == K["SCAN_CHUNK"]
	print(K)

def on(dev, a, wcs): return enmap.ndmap(a, wcs) if dev is ident else enmap.dmap(dev(a), wcs)

# ---- the model of sim_objects, object by object over each object's own window ---------------------------------------------------
def f32_axes(shape, wcs):
	"""the float32 pixel axes the kernels use (test_pixel_coordinates_are_the_float32_axes), and the geometry's numbers"""
	ny, nx, dec0, ddec, ra0, dra = separable_geometry(shape, wcs, "auto")
	return np.float32(dec0+np.arange(ny)*ddec), np.float32(ra0+np.arange(nx)*dra), (ny, nx, dec0, ddec, ra0, dra)

def window_of(dec, ra, odec, ora, rc, ddec, dra):
	"""rows and columns outside of which no pixel is within rc of the object: |ddec| <= rc, and |dra| <= asin(sin rc / cos dec), the
	half width of a small circle (every column when the disc holds a pole); a pixel and 1e-3 rc to spare"""
	ys = np.flatnonzero(np.abs(np.float64(dec)-odec) <= rc*1.001+abs(ddec))
	if abs(odec)+rc*1.001+abs(ddec) >= np.pi/2: return ys, np.arange(len(ra)), True
	w = np.arcsin(min(1.0, np.sin(rc*1.001)/np.cos(odec)))+abs(dra)
	dr = np.abs(np.remainder(np.float64(ra)-ora+np.pi, 2*np.pi)-np.pi)
	return ys, np.flatnonzero(dr <= w), False

def draw_clear_of_the_cut(rng, draw, dec, ra, rc_of, n):
	"""n positions from draw(rng, k) -> [2, k] such that no pixel lies within 2e-6 rc of an object's cut radius, where float32 may decide
	either way (as other_paths_body asserts for its objects)"""
	pos = np.float32(draw(rng, n))
	for _ in range(50):
		bad = []
		for i in range(n):
			rc = rc_of(i); ys, xs, _ = window_of(dec, ra, pos[0, i], pos[1, i], rc, dec[1]-dec[0], ra[1]-ra[0])
			if len(ys) and len(xs) and np.min(np.abs(dist64(dec[ys], ra[xs], pos[0, i], pos[1, i])-rc)) <= 2e-6*rc: bad.append(i)
		if not bad: return pos
		pos[:, bad] = np.float32(draw(rng, len(bad)))
	raise AssertionError("no clear draw")

class Painted:
	"""the float64 model of one sim_objects call: sum[c, p], S[c, p] = sum_i |a_i P_i|, n[p], the extremes per pixel, and per object the
	window (ys, xs), the profile P on it (0 beyond the cut radius) and the tiles its disc reaches"""
	def __init__(self, shape, wcs, poss, amps, prof, rcs, keep=True):
		dec, ra, (ny, nx, dec0, ddec, ra0, dra) = f32_axes(shape, wcs)
		T = K["TILE"]; self.nty, self.ntx = -(-ny//T), -(-nx//T)
		nc, nobj = amps.shape
		self.sum = np.zeros((nc, ny, nx)); self.S = np.zeros((nc, ny, nx)); self.n = np.zeros((ny, nx), int)
		self.hi = np.full((nc, ny, nx), -np.inf); self.lo = np.full((nc, ny, nx), np.inf); self.big = np.zeros((nc, ny, nx))
		self.per_tile = np.zeros(self.nty*self.ntx, int); self.obj = []; self.wraps = 0; self.polar = 0
		for i in range(nobj):
			rc = np.float64(rcs[i])
			ys, xs, polar = window_of(dec, ra, np.float64(poss[0, i]), np.float64(poss[1, i]), rc, ddec, dra)
			r = dist64(dec[ys], ra[xs], poss[0, i], poss[1, i])
			assert r.size == 0 or np.min(np.abs(r-rc)) > 2e-6*rc, "object %d: a pixel on the cut radius" % i
			reach = r <= rc
			P = np.where(reach, prof64(prof, r), 0.0)
			t = np.float64(amps[:, i])[:, None, None]*P
			w = np.ix_(np.arange(nc), ys, xs)
			self.sum[w] += t; self.S[w] += np.abs(t); self.n[np.ix_(ys, xs)] += reach
			self.hi[w] = np.maximum(self.hi[w], np.where(reach, t, -np.inf)); self.lo[w] = np.minimum(self.lo[w], np.where(reach, t, np.inf))
			self.big[w] = np.maximum(self.big[w], np.abs(t))
			yy, xx = np.nonzero(reach)
			tiles = np.unique((ys[yy]//T)*self.ntx+xs[xx]//T)
			self.per_tile[tiles] += 1
			self.polar += polar and reach.any(); self.wraps += bool(reach.any() and len(xs) < nx and xs.min() == 0 and xs.max() == nx-1)
			if keep: self.obj.append((ys, xs, P))
	def add_bound(self, base=None):
		"""per pixel, on a float32 map: the evaluation of the terms and the float32 sum; `base`: what the map held (one more term)"""
		if base is None: return (64*ULP+self.n*2.0**-24)*self.S
		return 64*ULP*self.S+self.n*2.0**-24*self.S+2.0**-24*(np.abs(base)+self.S)

def paint32(shape, wcs, poss, amps, prof, rcs):
	"""float32 numpy all the way, the objects added in ascending order: not the kernel's arithmetic (which takes the separable terms of h in
	float64), but the plainest float32 evaluation of the same formulas"""
	dec, ra, _ = f32_axes(shape, wcs)
	f = np.float32; rs, vs = f(prof[0]), f(prof[1]); n = len(rs)
	acc = np.zeros((amps.shape[0],)+tuple(shape[-2:]), f)
	cp = np.cos(dec)[:, None]
	for i in range(amps.shape[1]):
		sd = np.sin(f(0.5)*(dec[:, None]-f(poss[0, i]))); sr = np.sin(f(0.5)*(ra[None, :]-f(poss[1, i])))
		h = sd*sd+(cp*np.cos(f(poss[0, i])))*(sr*sr)
		r = f(2)*np.arcsin(np.sqrt(np.minimum(h, f(1))))
		k = np.clip(np.searchsorted(rs, r, side="right")-1, 0, n-2)
		P = vs[k]+(vs[k+1]-vs[k])*((r-rs[k])/(rs[k+1]-rs[k]))
		P = np.where(r < rs[0], vs[0], np.where(r >= rs[-1], f(0), P))
		P = np.where(r <= f(rcs[i]), P, f(0))
		assert P.dtype == f and r.dtype == f
		acc += f(amps[:, i])[:, None, None]*P
	return acc

# ---- S1: long tile lists -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pfx(golden_dir): return dict(np.load(os.path.join(golden_dir, "pointsrcs.npz")))

S1_VMIN = 1e-5
@pytest.fixture(scope="module")
def s1(pfx):
	"""600 objects inside a 24 x 24 pixel window centred on tile (3, 3) of geometry A, amplitudes of 1 to 3 with either sign: with
	vmin = 1e-5 every disc is cut at 4.8 sigma or more, 5.7 pixels, and reaches the central tile from anywhere in the window"""
	shape, wcs = geometry(pfx["A_geo"]); prof = pfx["A_prof"]; T = K["TILE"]
	dec, ra, (ny, nx, dec0, ddec, ra0, dra) = f32_axes(shape, wcs)
	nobj = 600; w0 = 3*T-(24-T)//2
	rng = np.random.default_rng(601)
	amps = np.float32(rng.uniform(1, 3, (3, nobj))*rng.choice([-1, 1], (3, nobj)))
	rcs = np.array([rcut32(prof, amps[:, i], S1_VMIN, 0) for i in range(nobj)])
	draw = lambda rng, k: np.array([dec0+(w0+rng.uniform(0, 24, k))*ddec, ra0+(w0+rng.uniform(0, 24, k))*dra])
	poss = draw_clear_of_the_cut(rng, draw, dec, ra, lambda i: np.float64(rcs[i]), nobj)
	model = Painted(shape, wcs, poss, amps, prof, rcs, keep=False)
	return dict(shape=shape, wcs=wcs, prof=prof, poss=poss, amps=amps, rcs=rcs, model=model)

def s1_crossing(model, nch=None, chunk=None):
	"""the model's own discs: one tile lists more objects than tile_sort_kernel ranks at a time, several more than paint_kernel stages"""
	nch = K["NCH"] if nch is None else nch; chunk = K["SORT_CHUNK"] if chunk is None else chunk
	longest = model.per_tile.max()
	print("S1: the longest tile list holds at least %d objects; %d tiles list more than NCH = %d" % (longest, np.sum(model.per_tile > nch), nch))
	assert longest > chunk and longest > nch, "does not reach the second chunk of the list sort"
	assert np.sum(model.per_tile > nch) >= 3, "does not reach the second step of the paint over several tiles"

def test_s1_model(s1):
	"""the case crosses its seams, and a float32 numpy evaluation stays inside the bound the kernels are held to"""
	s1_crossing(s1["model"])
	m = s1["model"]
	e32 = np.abs(np.float64(paint32(s1["shape"], s1["wcs"], s1["poss"], s1["amps"], s1["prof"], s1["rcs"]))-m.sum)
	print("S1: float32 numpy: worst error / bound %.3f" % np.max(e32/np.maximum(m.add_bound(), 1e-300)))
	assert np.all(e32 <= m.add_bound())

def s1_body(s1, dev, on_device):
	shape, wcs, prof, poss, amps, m = s1["shape"], s1["wcs"], s1["prof"], s1["poss"], s1["amps"], s1["model"]
	s1_crossing(m)
	run = lambda p, a, **kw: pointsrcs.sim_objects(shape, wcs, dev(np.ascontiguousarray(p)), dev(np.ascontiguousarray(a)), prof, vmin=S1_VMIN, **kw)
	rev = lambda **kw: run(poss[:, ::-1], amps[:, ::-1], **kw)
	# add, into a new map: the bound as it stands
	got = run(poss, amps)
	assert isinstance(got, enmap.dmap if on_device else enmap.ndmap) and got.dtype == np.float32
	g = np.float64(host(got)); err = np.abs(g-m.sum); bound = m.add_bound()
	print("S1 add: worst error / bound %.3f, %.2f ulp of the peak" % (np.max(err/np.maximum(bound, 1e-300)), err.max()/np.abs(m.sum).max()/ULP))
	assert np.all(err <= bound) and np.all(g[:, m.n == 0] == 0)
	assert np.array_equal(host(run(poss, amps)), host(got))
	gr = np.float64(host(rev()))
	assert np.all(np.abs(gr-m.sum) <= bound)
	assert np.all(np.abs(gr-g) <= 2*m.n*2.0**-24*m.S)      # (the same float32 terms in the opposite order: a list is ordered by object index)
	# into maps that are not zero, float32 and float64, every op
	yy, xx = np.mgrid[:shape[0], :shape[1]]
	base = np.array([np.sin(0.3*yy+c)*np.cos(0.2*xx-c)+0.1*c for c in range(3)])
	for dt in (np.float32, np.float64):
		b = base.astype(dt); b64 = np.float64(b)
		bound = m.add_bound(b64) if dt == np.float32 else 64*ULP*m.S+m.n*2.0**-53*m.S+2.0**-53*(np.abs(b64)+m.S)
		for op, want, tol in (("add", b64+m.sum, bound), ("max", np.maximum(b64, m.hi), 64*ULP*m.big), ("min", np.minimum(b64, m.lo), 64*ULP*m.big)):
			outs = []
			for f in (lambda **kw: run(poss, amps, **kw), lambda **kw: run(poss, amps, **kw), rev):
				omap = on(dev, b.copy(), wcs)
				assert f(omap=omap, op=op) is omap and omap.dtype == dt
				outs.append(host(omap))
			err = np.abs(np.float64(outs[0])-want)
			print("S1 %s into %s: worst error / bound %.3f" % (op, np.dtype(dt).name, np.max(err/np.maximum(tol, 1e-300))))
			assert np.all(err <= tol), (op, dt)
			assert np.array_equal(outs[0][:, m.n == 0], b[:, m.n == 0])
			assert np.array_equal(outs[0], outs[1])
			if op == "add": assert np.all(np.abs(np.float64(outs[2])-want) <= tol)
			else: assert np.array_equal(outs[0], outs[2]), op

@pytest.mark.hostsim
def test_s1_long_lists_sim(s1): s1_body(s1, ident, False)
@pytest.mark.gpu
def test_s1_long_lists_gpu(s1): s1_body(s1, cuda, True)

# ---- S2: many tiles --------------------------------------------------------------------------------------------------------------
S2_SHAPE = (800, 808)
def s2_geometry():
	"""the whole sky, 800 rows (half a pixel short of the poles) by 808 columns: 50 x 51 tiles, the last column of tiles half outside the map"""
	ny, nx = S2_SHAPE
	return S2_SHAPE, CarWCS(cdelt=[-360.0/nx, 180.0/ny], crval=[0.0, 0.0], crpix=[nx/2+0.5, ny/2+0.5])

def make_s2():
	shape, wcs = s2_geometry(); ny, nx = shape
	dec, ra, (_, _, dec0, ddec, ra0, dra) = f32_axes(shape, wcs)
	nobj = 3000; sigma = 1.25*abs(ddec)
	rs = np.linspace(0, 4*sigma, 200); prof = np.float32([rs, np.exp(-0.5*(rs/sigma)**2)])
	rng = np.random.default_rng(3000)
	amps = np.float32(rng.uniform(1, 3, (2, nobj))*rng.choice([-1, 1], (2, nobj)))
	vmin = 1e-4
	rcs = np.array([rcut32(prof, amps[:, i], vmin, 0) for i in range(nobj)])
	assert np.all(rcs == prof[0, -1])
	draw = lambda rng, k: np.array([dec0+rng.uniform(0, ny-1, k)*ddec, ra0+rng.uniform(-0.5, nx-0.5, k)*dra])
	def planted(rng, k):
		p = draw(rng, k)
		if k == nobj:
			p[:, 0] = [dec0+(ny-1.6)*ddec, 1.0]                                       # its disc holds the north pole
			p[:, 1] = [0.3, ra0-0.2*dra]; p[:, 2] = [-0.8, ra0+(nx-0.7)*dra]          # either side of the RA seam
		return p
	poss = draw_clear_of_the_cut(rng, planted, dec, ra, lambda i: np.float64(rcs[i]), nobj)
	m = (np.random.default_rng(3001).random((2,)+shape)*2-1).astype(np.float32)
	return dict(shape=shape, wcs=wcs, prof=prof, poss=poss, amps=amps, rcs=rcs, vmin=vmin, map=m, model=Painted(shape, wcs, poss, amps, prof, rcs))

@pytest.fixture(scope="module")
def s2(): return make_s2()

def s2_crossing(s2, shape=None, maxblk=None, scan_wg=None):
	"""50 x 51 tiles follow from the shape: more than one scan workgroup; the tiles that hold a pixel inside some disc are a lower bound
	on the listed tiles: more than the workgroups of the list kernels, so they stride and prefetch"""
	ny, nx = S2_SHAPE if shape is None else shape; T = K["TILE"]
	maxblk = K["SRC_MAXBLK"] if maxblk is None else maxblk; scan_wg = SCAN_WG if scan_wg is None else scan_wg
	ntiles = (-(-ny//T))*(-(-nx//T)); m = s2["model"]
	listed = int(np.sum(m.per_tile[:ntiles] > 0)) if ntiles <= len(m.per_tile) else 0
	print("S2: %d tiles, at least %d listed; %d discs hold a pole, %d windows wrap" % (ntiles, listed, m.polar, m.wraps))
	assert nx % T and ntiles > scan_wg and ntiles > maxblk
	assert listed > maxblk, "does not reach the grid-stride loop over the listed tiles"
	assert np.any(m.per_tile[scan_wg:] > 0) and np.any(m.per_tile[:scan_wg] > 0), "no list on either side of the scan's carry"
	assert m.polar >= 1 and m.wraps >= 2

def test_s2_model(s2): s2_crossing(s2)

def s2_body(s2, dev, on_device):
	shape, wcs, prof, poss, amps, vmin, mp, m = (s2[k] for k in ("shape", "wcs", "prof", "poss", "amps", "vmin", "map", "model"))
	s2_crossing(s2)
	dec, ra, (ny, nx, dec0, ddec, ra0, dra) = f32_axes(shape, wcs)
	nobj = poss.shape[1]
	# forward
	fwd = pointsrcs.sim_objects(shape, wcs, dev(poss), dev(amps), prof, vmin=vmin)
	g = np.float64(host(fwd)); err = np.abs(g-m.sum); bound = m.add_bound()
	print("S2 forward: worst error / bound %.3f" % np.max(err/np.maximum(bound, 1e-300)))
	assert g.shape == (2,)+shape and np.all(err <= bound) and np.all(g[:, m.n == 0] == 0)
	# transpose, and the radial sums around the same objects out to the cut radius
	bins = np.float32(np.linspace(0, 1, 5)*np.float64(s2["rcs"][0])); nbin = 4
	delta = 32*ULP*max(np.float64(bins[-1]), abs(ddec))
	want = np.zeros(amps.shape); asum = np.zeros(amps.shape); fwd_abs = 0.0; nmax = 0
	rsum = np.zeros((nobj, 2, nbin)); rabs = np.zeros((nobj, 2, nbin)); cnt = np.zeros((nobj, nbin), int); mask = np.zeros((nobj, nbin), bool)
	m64 = np.float64(mp)
	for i, (ys, xs, P) in enumerate(m.obj):
		mw = m64[np.ix_(np.arange(2), ys, xs)]
		want[:, i] = (mw*P).sum((-2, -1)); asum[:, i] = np.abs(mw*P).sum((-2, -1))
		fwd_abs += np.sum(np.abs(np.float64(amps[:, i]))*asum[:, i]); nmax = max(nmax, int((P != 0).sum()))
		r = dist64(dec[ys], ra[xs], poss[0, i], poss[1, i])
		near = [np.any(np.abs(r-np.float64(e)) < delta) for e in bins]
		for k in range(nbin):
			sel = (r >= np.float64(bins[k])) & (r < np.float64(bins[k+1]))
			rsum[i, :, k] = mw[:, sel].sum(-1); rabs[i, :, k] = np.abs(mw[:, sel]).sum(-1); cnt[i, k] = sel.sum(); mask[i, k] = near[k] or near[k+1]
	acc = dev(amps.copy()); mm = on(dev, mp, wcs)
	assert pointsrcs.sim_objects(shape, wcs, dev(poss), acc, prof, omap=mm, vmin=vmin, transpose=True) is mm and np.array_equal(host(mm), mp)
	got = np.float64(host(acc))-np.float64(amps)
	rel = np.max(np.abs(got-want)/asum)/ULP
	print("S2 transpose: %.2f ulp of sum |P m| per object" % rel)
	assert rel <= 64
	lhs, rhs = np.sum(g*m64), np.sum(np.float64(amps)*got)
	print("S2 adjointness: |<Pa,m> - <a,P^T m>| = %.3g, bound %.3g" % (abs(lhs-rhs), 4*nmax*2.0**-24*fwd_abs))
	assert abs(lhs-rhs) <= 4*nmax*2.0**-24*fwd_abs
	print("S2 radial: %d of %d (object, bin) pairs in the guard band" % (mask.sum(), mask.size))
	assert mask.mean() <= 0.30
	rs_ = pointsrcs.radial_sum(mm, dev(poss), bins)
	assert tuple(rs_.shape) == rsum.shape
	good = np.broadcast_to(~mask[:, None, :], rsum.shape)
	tol = 4*cnt[:, None, :]*2.0**-24*rabs
	err = np.abs(np.float64(host(rs_))-rsum)
	print("S2 radial_sum: worst error / bound %.3f" % np.max(np.where(good, err/np.maximum(tol, 1e-300), 0)))
	assert np.all(err[good] <= tol[good])
	mean = np.float64(host(pointsrcs.radial_bin(mm, dev(poss), bins)))
	full = good & np.broadcast_to(cnt[:, None, :] > 0, rsum.shape); n = np.broadcast_to(cnt[:, None, :], rsum.shape)
	assert np.all(np.abs(mean[full]-rsum[full]/n[full]) <= tol[full]/n[full]+ULP*np.abs(rsum[full]/n[full]))

@pytest.mark.hostsim
def test_s2_many_tiles_sim(s2): s2_body(s2, ident, False)
@pytest.mark.gpu
def test_s2_many_tiles_gpu(s2): s2_body(s2, cuda, True)

# ---- B1: more scales than one launch of the filter bank takes ----------------------------------------------------------------------
def b1_scales(lmax, nscale):
	"""the scales of scales_of(lmax), repeated (the filters are drawn per scale, so every repeat has its own)"""
	lmaxs, Ls = tb.scales_of(lmax)
	rep = -(-nscale//len(lmaxs))
	return (lmaxs*rep)[:nscale], (Ls*rep)[:nscale]

def b1_body():
	for groups in (1, 2):
		nscale = groups*K["BANK_MAX"]+1
		for lmax in (37, 300):
			scales = b1_scales(lmax, nscale)
			assert len(scales[0]) == nscale > groups*K["BANK_MAX"], "does not reach launch %d of the bank" % (groups+1)
			assert scales[0][-1] == 0 and scales[0][groups*K["BANK_MAX"]-1] == lmax//2      # (the group boundary falls between two different scales)
			for dtype in tb.DTYPES:
				tb.check_split(lmax, "tri", 1, dtype, seed=nscale, scales=scales)      # bit for bit the composition
				tb.check_merge(lmax, "tri", 1, dtype, seed=nscale+1, scales=scales)    # accumulate off and on, within nscale eps sum |f a|

@pytest.mark.hostsim
def test_b1_bank_groups_sim(): b1_body()
@pytest.mark.gpu
def test_b1_bank_groups_gpu(): b1_body()

# ---- L1: the grid-stride loops of the lensing kernels ------------------------------------------------------------------------------
def l1_shape():
	"""600 x 901, or as many rows of 901 as it takes to pass one trip of the loop by 3 per cent"""
	nx = 901; ny = max(600, -(-int(1.03*STREAM_TRIP)//nx))
	return ny, nx

def l1_deflect_body(dev):
	ny, nx = l1_shape(); npts = ny*nx
	assert npts > STREAM_TRIP and npts % WG, "does not reach the second trip of deflect_kernel"
	shape, wcs = (ny, nx), CarWCS(cdelt=[-360.0/nx, 180.0/(ny-1)], crval=[0.0, 0.0], crpix=[nx/2+0.5, (ny+1)/2])
	pos = np.asarray(enmap.posmap(shape, wcs))
	assert abs(pos[0, 0, 0]+np.pi/2) < 1e-12 and abs(pos[0, -1, 0]-np.pi/2) < 1e-12      # (the pole rows are there)
	rng = np.random.default_rng(901)
	grad = 1e-3*rng.random((2,)+shape)
	psi0 = rng.uniform(-1, 1, shape)
	idx = np.unique(np.concatenate([rng.choice(npts-1000, 19000, replace=False), np.arange(npts-1000, npts)]))
	assert idx[-1] == npts-1 and np.sum(idx >= STREAM_TRIP) >= 1000 and np.sum(idx < STREAM_TRIP) >= 1000
	p, g, s0 = pos.reshape(2, -1)[:, idx], grad.reshape(2, -1)[:, idx], psi0.reshape(-1)[idx]
	def compare(what, got, want, sel):
		got = host(got).reshape(got.shape[0], -1)[:, idx]
		errs = [np.abs(got[0]-want[0]), wrap(got[1]-want[1])*np.cos(np.asarray(want[0], np.float64))]
		if got.shape[0] > 2: errs.append(wrap(got[2]-want[2]))
		worst = [float(e[sel].max()) for e in errs]
		print("L1 %s: dec %.2e  ra cos(dec) %.2e  psi %.2e  (%d pixels)" % (what, worst[0], worst[1], worst[-1] if len(worst) > 2 else 0, int(sel.sum())))
		assert max(worst) <= TOL and np.all(np.isfinite(got)), (what, worst)
	every = np.ones(len(idx), bool)
	ld = vec_deflect(p[0], p[1], g[0], g[1])
	compare("geodesic", lensing.offset_by_grad(dev(pos), dev(grad), pol=False), ld[:2], every)
	compare("geodesic, psi", lensing.offset_by_grad(dev(pos), dev(grad), pol=True), ld, every)
	compare("geodesic, psi0", lensing.offset_by_grad(dev(np.concatenate([pos, psi0[None]])), dev(grad)), vec_deflect(p[0], p[1], g[0], g[1], s0), every)
	loc, psi = lensing.offset_by_grad(None, dev(grad), pol=True, _loc=True, _geometry=(shape, wcs))
	l = host(loc)
	# from the geometry's numbers the kernel forms dec0 + y ddec itself, an ulp from posmap's; within |grad| of a pole psi turns by 2 / |grad|
	# per unit of position, so there (the pole rows: the module's own selection rule) only the given positions above are compared
	far = covered(p, g)
	assert 1-covered(pos, grad).mean() <= 2/ny+1e-12 and not far.all()
	compare("geodesic, from the geometry", np.array([np.pi/2-l[:, 0], l[:, 1]]), ld[:2], every)
	compare("geodesic, from the geometry, psi", np.array([np.pi/2-l[:, 0], l[:, 1], host(psi)]), ld, far)
	# not geodesic: the gradient added to the coordinates, reflected at a pole, no rotation; on a pole itself g1 / cos(dec) has no meaning
	ok = np.abs(p[0]) < np.pi/2-1e-6
	assert 1-(np.abs(pos[0]) < np.pi/2-1e-6).mean() <= 2/ny+1e-12 and ok.any()
	ft = np.longdouble
	flat = lensing.pole_wrap(np.array([ft(p[0])+ft(g[0]), ft(p[1])+ft(g[1])/np.cos(ft(p[0]))]))
	compare("not geodesic", lensing.offset_by_grad(dev(pos), dev(grad), geodesic=False, pol=False), flat, ok)
	got = lensing.offset_by_grad(dev(pos), dev(grad), geodesic=False, pol=True)
	compare("not geodesic, psi", got, np.array([flat[0], flat[1], 0*flat[0]]), ok)
	assert not np.any(host(got)[2])

def l1_rotate_body(dev):
	nx = 901
	ny_vec = -(-2*int(1.0001*STREAM_TRIP+2)//nx); ny_vec += (ny_vec*nx) % 2      # an even number of pixels: no scalar tail
	ny_sc = l1_shape()[0]; ny_sc += 1-(ny_sc*nx) % 2                             # an odd number: pairs with an odd stride
	rng = np.random.default_rng(902)
	for dt in (np.float32, np.float64):
		for kernel, shape in (("vector", (3, ny_vec, nx)), ("scalar", (2, 3, ny_sc, nx))):
			npix = shape[-2]*shape[-1]; npre = int(np.prod(shape[:-3], dtype=int))
			m = rng.standard_normal(shape).astype(dt)
			ang = rng.uniform(-np.pi, np.pi, shape[-2:])
			# which kernel runs is decided by launch_rotate from what the wrapper hands to pxm_rotate_pol: the rule is evaluated here on those very
			# arguments (pointers included), recorded on their way in, so a wrapper that copied or re-strided its input could not switch kernels unseen
			calls = []; real = enmap._rotate_pairs_by
			def spy(data, psi, c0, c1, spin):
				n = int(np.prod(data.shape[2:], dtype=np.int64)); item = A.np_dtype(data).itemsize
				calls.append((n, int(data.shape[0]), A.ptr(data)+c0*n*item, A.ptr(data)+c1*n*item, int(data.shape[1])*n, item, A.ptr(psi)))
				return real(data, psi, c0, c1, spin)
			enmap._rotate_pairs_by = spy
			try: got = host(enmap.rotate_pol(dev(m), dev(ang)))
			finally: enmap._rotate_pairs_by = real
			assert len(calls) == 1
			npts, npair, pa, pb, pstride, item, ppsi = calls[0]
			vec = pa % (2*item) == 0 and pb % (2*item) == 0 and ppsi % 16 == 0 and (npair == 1 or pstride % 2 == 0)
			nvec = npts//2 if vec else 0
			assert npts == npix and npair == npre
			if kernel == "vector": assert nvec > STREAM_TRIP and nvec % WG and 2*nvec == npts, "does not reach the second trip of rotate_pol_vec_kernel"
			else: assert nvec == 0 and npts > STREAM_TRIP and npts % WG, "does not reach the second trip of rotate_pol_kernel"
			assert got.dtype == dt and got.shape == shape
			c, s = np.cos(2*ang), np.sin(2*ang); a, b = np.float64(m[..., 1, :, :]), np.float64(m[..., 2, :, :])
			tol = 4*np.finfo(dt).eps*np.hypot(a, b)      # the module's: 4 ulp of the pair's magnitude
			ea, eb = np.abs(np.float64(got[..., 1, :, :])-(c*a-s*b)), np.abs(np.float64(got[..., 2, :, :])-(s*a+c*b))
			print("L1 rotate_pol %s, %s kernel: worst error / bound %.3f" % (np.dtype(dt).name, kernel, max(np.max(ea/tol), np.max(eb/tol))))
			assert np.all(ea <= tol) and np.all(eb <= tol) and np.array_equal(got[..., 0, :, :], m[..., 0, :, :])

@pytest.mark.hostsim
def test_l1_deflect_sim(): l1_deflect_body(ident)
@pytest.mark.hostsim
def test_l1_rotate_pol_sim(): l1_rotate_body(ident)
@pytest.mark.gpu
def test_l1_deflect_gpu(): l1_deflect_body(cuda)
@pytest.mark.gpu
def test_l1_rotate_pol_gpu(): l1_rotate_body(cuda)

# ---- D1: distance_from over more cells than one scan workgroup counts ----------------------------------------------------------------
@pytest.fixture(scope="module")
def dtol(golden_dir):
	"""the tolerance of tests/test_distances.py: max(4 E_ref, 8 * 2^-52 * pi)"""
	from test_distances import tol_of
	return tol_of(dict(np.load(os.path.join(golden_dir, "distances.npz"))))

def cells_of(shape, wcs, pts):
	"""the cell a point is binned into, restated from distance.hip cell_of: that of the nearest pixel, clamped to the map"""
	ny, nx, dec0, ddec, ra0, dra = separable_geometry(shape, wcs, "auto"); T = K["DTILE"]
	period = 2*np.pi/abs(dra)
	y, x = (pts[0]-dec0)/ddec, (pts[1]-ra0)/dra
	x = x-period*np.floor((x-0.5*nx)/period+0.5)
	iy, ix = np.clip(np.rint(y), 0, ny-1).astype(int), np.clip(np.rint(x), 0, nx-1).astype(int)
	return (iy//T)*(-(-nx//T))+ix//T

def check_sampled(tag, tol, pdec, pra, pts, got, dom, rmax):
	"""tests/test_distances.py check(), on sampled pixels: the distance against min(brute force, rmax); a domain is right when the point it names
	is as near as the nearest (within tol of rmax, -1 or a point within rmax pass)"""
	want = vincenty(pdec[:, None], pra[:, None], pts[0][None, :], pts[1][None, :]).min(1)
	exp = want if rmax is None else np.minimum(want, rmax)
	err = np.abs(got-exp).max()
	print("%s: worst distance error %.3g rad (tol %.3g) on %d pixels" % (tag, err, tol, len(got)))
	assert err <= tol, tag
	assert dom.dtype == np.int32 and dom.max() < pts.shape[1] and dom.min() >= -1, tag
	named = dom >= 0
	r = np.full(want.shape, np.inf); r[named] = vincenty(pdec[named], pra[named], pts[0][dom[named]], pts[1][dom[named]])
	ok = np.where(named, r <= want+tol, False)
	if rmax is not None:
		ok &= want <= rmax+tol
		ok |= ~named & (want >= rmax-tol)
	assert np.all(ok), "%s: %d wrong domains" % (tag, np.sum(~ok))
	return want

def d1_body(dev, tol):
	T = K["DTILE"]; ncy = int(np.sqrt(SCAN_WG))+1; ncx = ncy+1
	ny, nx = ncy*T, ncx*T                      # 528 x 544: 33 x 34 cells
	ncell = (-(-ny//T))*(-(-nx//T))
	assert ncell > SCAN_WG, "does not reach the carry between the scan's workgroups"
	shape, wcs = (ny, nx), CarWCS(cdelt=[-1/30.0, 1/30.0], crval=[10.0, 0.0], crpix=[nx/2+0.5, ny/2+0.5-900])      # 2 arcmin pixels around dec 30 deg
	dec, ra = enmap.posaxes(shape, wcs)
	rng = np.random.default_rng(528)
	npt = 300; noff = 40
	pts = np.array([rng.uniform(dec.min(), dec.max(), npt), rng.uniform(ra.min(), ra.max(), npt)])
	side = rng.integers(0, 4, noff); far = np.deg2rad(rng.uniform(0.1, 2, noff))      # off the map by up to 2 degrees, on every side
	pts[0, :noff] = np.where(side == 0, dec.min()-far, np.where(side == 1, dec.max()+far, pts[0, :noff]))
	pts[1, :noff] = np.where(side == 2, ra.min()-far, np.where(side == 3, ra.max()+far, pts[1, :noff]))
	pts[:, 151] = pts[:, 150]                  # two points in one place: the lower index is named
	cells = cells_of(shape, wcs, pts)
	assert np.any(cells >= SCAN_WG) and np.any(cells < SCAN_WG) and cells.max() < ncell, "no occupied cell on either side of the carry"
	idx = np.unique(np.concatenate([rng.choice(ny*nx, 20000, replace=False), (np.arange(T)[:, None]*nx+np.arange(T)[None, :]).reshape(-1),
		((ny-T+np.arange(T))[:, None]*nx+(nx-T+np.arange(T))[None, :]).reshape(-1)]))
	pdec, pra = dec[idx//nx], ra[idx % nx]
	for rmax in (None, np.deg2rad(0.4)):
		d, dom = enmap.distance_from(shape, wcs, dev(pts), domains=True, rmax=rmax)
		d, dom = host(d), host(dom)
		assert d.shape == shape and d.dtype == np.float64
		want = check_sampled("D1 rmax %s" % rmax, tol, pdec, pra, pts, d.reshape(-1)[idx], dom.reshape(-1)[idx], rmax)
		assert not np.any(dom == 151) and np.any(dom == 150)
		if rmax is not None: assert np.any(dom < 0) and np.any(dom >= 0) and np.any(want > rmax) and np.any(want < rmax)
		plain = host(enmap.distance_from(shape, wcs, dev(pts), rmax=rmax))      # without domains: the same numbers
		assert np.array_equal(plain, d)

@pytest.mark.hostsim
def test_d1_cells_sim(dtol): d1_body(ident, dtol)
@pytest.mark.gpu
def test_d1_cells_gpu(dtol): d1_body(cuda, dtol)

def big_tile_grid(T):
	"""the smallest near-square grid of tiles with more tiles than one trip of scan_top_kernel takes: 512 x 513 tiles, 8192 x 8208 pixels, with the
	constants as they are"""
	nty = int(np.sqrt(SCAN_TRIP)); ntx = SCAN_TRIP//nty+1
	return nty, ntx, nty*T, ntx*T
def seam_tiles(nty, ntx):
	"""the first tile and the last, either side of the second trip of scan_top_kernel and of the first carry of scan_counts, two more"""
	return [0, nty*ntx-1, SCAN_TRIP-1, SCAN_TRIP, SCAN_WG-1, SCAN_WG, (nty//3)*ntx+ntx//2, (2*nty//3)*ntx+ntx//5]

@pytest.mark.gpu
def test_d1_second_scan_trip_gpu(dtol):
	"""eight points on a map of more than 262 144 cells: everything stays on the device but the windows around the points and a sample"""
	import torch
	T = K["DTILE"]; ncy, ncx, ny, nx = big_tile_grid(T)
	assert ncy*ncx > SCAN_TRIP, "does not reach the second trip of scan_top_kernel"
	shape, wcs = (ny, nx), CarWCS(cdelt=[-1/120.0, 1/120.0], crval=[0.0, 0.0], crpix=[nx/2+0.5, ny/2+0.5])
	dec, ra = enmap.posaxes(shape, wcs)
	tiles = np.array(seam_tiles(ncy, ncx)); ty, tx = tiles//ncx, tiles % ncx
	rng = np.random.default_rng(8192)
	py, px = ty*T+rng.uniform(2, T-3, 8), np.minimum(tx*T+rng.uniform(2, T-3, 8), nx-2)
	_, _, dec0, ddec, ra0, dra = separable_geometry(shape, wcs, "auto")
	pts = np.array([dec0+py*ddec, ra0+px*dra])
	assert np.array_equal(np.sort(cells_of(shape, wcs, pts)), np.sort(tiles))      # the occupied cells are the chosen ones: on both sides of each seam
	idx = [rng.choice(ny*nx, 5000, replace=False)]
	for y, x in zip(ty*T, tx*T): idx.append(((y+np.arange(T))[:, None]*nx+np.minimum(x+np.arange(T), nx-1)[None, :]).reshape(-1))
	idx = np.unique(np.concatenate(idx))
	pdec, pra = dec[idx//nx], ra[idx % nx]
	tidx = torch.as_tensor(idx, device="cuda")
	for rmax in (None, np.deg2rad(20.0)):
		d, dom = enmap.distance_from(shape, wcs, cuda(pts), domains=True, rmax=rmax)
		assert isinstance(d, enmap.dmap) and d.tensor.is_cuda and tuple(d.shape) == shape
		check_sampled("D1 large rmax %s" % rmax, dtol, pdec, pra, pts, d.tensor.reshape(-1)[tidx].cpu().numpy(), dom.tensor.reshape(-1)[tidx].cpu().numpy(), rmax)
		assert sorted(torch.unique(dom.tensor).cpu().tolist()) == list(range(8) if rmax is None else range(-1, 8))
		del d, dom

# ---- D2: the edge finder over more blocks than one scan workgroup counts ----------------------------------------------------------
def np_edges(m, labeled=False):
	"""distances.find_edges / find_edges_labeled in numpy: a zero pixel on the border or with a non-zero 4-neighbour; labelled: a non-zero
	pixel on the border or with a 4-neighbour of another value.  Ascending flat indices"""
	m = np.asarray(m); own = (m != 0) if labeled else (m == 0)
	other = np.zeros(m.shape, bool)
	for a, b in ((np.s_[1:, :], np.s_[:-1, :]), (np.s_[:-1, :], np.s_[1:, :]), (np.s_[:, 1:], np.s_[:, :-1]), (np.s_[:, :-1], np.s_[:, 1:])):
		other[a] |= (m[a] != m[b]) if labeled else (m[b] != 0)
	other[0, :] = other[-1, :] = other[:, 0] = other[:, -1] = True
	return np.flatnonzero(own & other)

@pytest.fixture(scope="module")
def d2():
	nx = 1040; ny = -(-SCAN_WG*EDGE_BLK//nx)+23      # 1032 x 1040: 1049 edge blocks
	mask = np.ones((ny, nx), np.uint8); labels = np.zeros((ny, nx), np.int32)
	rng = np.random.default_rng(1032)
	seam = SCAN_WG*EDGE_BLK                           # the first pixel of the second scan workgroup's first block
	holes = [divmod(seam-7, nx), divmod(seam+301, nx)]
	gy, gx = np.meshgrid(np.arange(6), np.arange(7), indexing="ij")
	for y, x in zip(gy.reshape(-1), gx.reshape(-1)): holes.append((20+y*(ny-60)//5+int(rng.integers(0, 9)), 20+x*(nx-60)//6+int(rng.integers(0, 9))))
	for k, (y, x) in enumerate(holes):
		assert 0 < y < ny-1 and 0 < x < nx-1
		mask[y, x] = 0; labels[y, x] = 1+k % 5
	for k, (y, x, h, w) in enumerate(((100, 300, 10, 15), (500, 820, 7, 30), (seam//nx-3, 600, 12, 9))):      # the last one straddles the seam's rows
		mask[y:y+h, x:x+w] = 0; labels[y:y+h, x:x+w] = 6+k
	return dict(mask=mask, labels=labels, wcs=CarWCS(cdelt=[-1/60.0, 1/60.0], crval=[5.0, 0.0], crpix=[nx/2+0.5, ny/2+0.5+1200]))

def d2_crossing(shape, edges, scan_wg=None):
	scan_wg = SCAN_WG if scan_wg is None else scan_wg
	nblk = -(-shape[0]*shape[1]//EDGE_BLK); blk = edges//EDGE_BLK
	print("D2: %d edge blocks, %d edge pixels, %d in the last block of scan workgroup 0, %d in the first of workgroup 1" % (nblk, len(edges), np.sum(blk == scan_wg-1), np.sum(blk == scan_wg)))
	assert nblk > scan_wg, "does not reach the carry between the scan's workgroups"
	assert np.any(blk == scan_wg-1) and np.any(blk == scan_wg) and np.any(blk > scan_wg), "no edge pixel next to the carry"

def d2_body(d2, dev, tol):
	mask, labels, wcs = d2["mask"], d2["labels"], d2["wcs"]; shape = mask.shape; ny, nx = shape
	want = np_edges(mask); lwant = np_edges(labels, True)
	d2_crossing(shape, want); d2_crossing(shape, lwant)
	e = host(distances.find_edges(dev(mask), flat=True))
	assert e.dtype == np.int64 and np.array_equal(e, want)
	assert np.array_equal(host(distances.find_edges_labeled(dev(labels), flat=True)), lwant)
	dec, ra = enmap.posaxes(shape, wcs)
	rng = np.random.default_rng(1040)
	idx = np.unique(np.concatenate([rng.choice(ny*nx, 20000, replace=False), want[::7]]))
	pdec, pra = dec[idx//nx], ra[idx % nx]
	# the transform: zero inside the zero regions, the distance of the nearest edge pixel elsewhere
	r = vincenty(pdec[:, None], pra[:, None], dec[want//nx][None, :], ra[want % nx][None, :])
	d = host(enmap.distance_transform(on(dev, mask, wcs)))
	exp = np.where(mask.reshape(-1)[idx] != 0, r.min(1), 0.0)
	err = np.abs(d.reshape(-1)[idx]-exp).max()
	print("D2 distance_transform: worst error %.3g rad (tol %.3g)" % (err, tol))
	assert d.shape == shape and d.dtype == np.float64 and err <= tol and np.all(d[mask == 0] == 0) and np.all(d[mask != 0] > 0)
	# the labelled form, int32 labels: the label named is that of a labelled pixel as near as the nearest
	r = vincenty(pdec[:, None], pra[:, None], dec[lwant//nx][None, :], ra[lwant % nx][None, :])
	dl, dom = enmap.labeled_distance_transform(on(dev, labels, wcs))
	dl, dom = host(dl), host(dom)
	exp = np.where(labels.reshape(-1)[idx] == 0, r.min(1), 0.0)
	err = np.abs(dl.reshape(-1)[idx]-exp).max()
	print("D2 labeled_distance_transform: worst error %.3g rad" % err)
	assert dom.dtype == np.int32 and err <= tol and np.all(dl[labels != 0] == 0)
	assert np.array_equal(dom[labels != 0], labels[labels != 0]) and set(np.unique(dom)) == set(np.unique(labels[labels != 0]))
	el = labels.reshape(-1)[lwant]; ds = dom.reshape(-1)[idx]
	assert np.all(np.where(el[None, :] == ds[:, None], r, np.inf).min(1) <= r.min(1)+tol)

@pytest.mark.hostsim
def test_d2_edges_sim(d2, dtol): d2_body(d2, ident, dtol)
@pytest.mark.gpu
def test_d2_edges_gpu(d2, dtol): d2_body(d2, cuda, dtol)

@pytest.mark.gpu
def test_d2_second_scan_trip_gpu():
	"""a mask of ones made on the device with more than 262 144 edge blocks and single zero pixels at chosen flat indices: each of them, and no
	other pixel, is an edge"""
	import torch
	nx = 16400; ny = -(-SCAN_TRIP*EDGE_BLK//nx)+15      # 16 384 x 16 400 with the constants as they are: 262 400 edge blocks
	npix = ny*nx; nblk = -(-npix//EDGE_BLK)
	assert nblk > SCAN_TRIP, "does not reach the second trip of scan_top_kernel"
	zeros = [nx+1, npix-nx-2]                            # the first and the last interior pixel
	for k in (1, SCAN_WG-1, SCAN_WG, SCAN_WG+1, SCAN_TRIP-1, SCAN_TRIP): zeros += [EDGE_BLK*k-1, EDGE_BLK*k]
	for k in (1, 2, WG-1, WG): zeros += [EDGE_BLK*SCAN_WG*k-1, EDGE_BLK*SCAN_WG*k]
	zeros = np.unique(zeros)
	assert zeros[-1] < npix and np.any(zeros//EDGE_BLK >= SCAN_TRIP) and np.any(zeros//EDGE_BLK == SCAN_TRIP-1)
	mask = torch.ones((ny, nx), dtype=torch.uint8, device="cuda")
	mask.view(-1)[torch.as_tensor(zeros, device="cuda")] = 0
	e = distances.find_edges(mask, flat=True)      # (a zero pixel with a non-zero neighbour or on the border: so is every one of a pair)
	assert e.is_cuda and e.dtype == torch.int64 and np.array_equal(e.cpu().numpy(), zeros)

# ---- S3: sim_objects over more tiles than one trip of scan_top_kernel takes ------------------------------------------------------------
@pytest.mark.gpu
def test_s3_second_scan_trip_gpu(pfx):
	"""eight objects on a float32 map of more than 262 144 tiles, made on the device: the windows around the objects against the model, and nothing
	outside of them"""
	import torch
	T = K["TILE"]; nty, ntx, ny, nx = big_tile_grid(T)
	assert nty*ntx > SCAN_TRIP, "does not reach the second trip of scan_top_kernel"
	shape, wcs = (ny, nx), CarWCS(cdelt=[-1/120.0, 1/120.0], crval=[0.0, 0.0], crpix=[nx/2+0.5, ny/2+0.5])
	dec, ra, (_, _, dec0, ddec, ra0, dra) = f32_axes(shape, wcs)
	prof = pfx["A_prof"]; vmin = 1e-3
	tiles = np.array(seam_tiles(nty, ntx)); ty, tx = tiles//ntx, tiles % ntx
	rng = np.random.default_rng(8208)
	amps = np.float32(rng.uniform(1, 3, (1, 8))*np.array([1, -1, 1, -1, 1, -1, 1, -1]))
	rcs = np.array([rcut32(prof, amps[:, i], vmin, 0) for i in range(8)])
	poss = np.zeros((2, 8), np.float32)
	for i in range(8):
		draw = lambda rng, k: np.array([dec0+(ty[i]*T+rng.uniform(3, T-4, k))*ddec, ra0+np.minimum(tx[i]*T+rng.uniform(3, T-4, k), nx-2)*dra])
		poss[:, i] = draw_clear_of_the_cut(rng, draw, dec, ra, lambda _: np.float64(rcs[i]), 1)[:, 0]
	omap = enmap.dmap(torch.zeros((1,)+shape, dtype=torch.float32, device="cuda"), wcs)
	assert pointsrcs.sim_objects(shape, wcs, cuda(poss), cuda(amps), prof, omap=omap, vmin=vmin) is omap
	listed = set(); wins = []; worst = 0; nz = 0; asum = 0.0
	for i in range(8):
		ys, xs, _ = window_of(dec, ra, np.float64(poss[0, i]), np.float64(poss[1, i]), np.float64(rcs[i]), ddec, dra)
		r = dist64(dec[ys], ra[xs], poss[0, i], poss[1, i]); reach = r <= np.float64(rcs[i])
		want = np.float64(amps[0, i])*np.where(reach, prof64(prof, r), 0.0)
		yy, xx = np.nonzero(reach); listed |= set(((ys[yy]//T)*ntx+xs[xx]//T).tolist())
		win = (slice(int(ys[0]), int(ys[-1])+1), slice(int(xs[0]), int(xs[-1])+1))
		assert np.array_equal(ys, np.arange(ys[0], ys[-1]+1)) and np.array_equal(xs, np.arange(xs[0], xs[-1]+1))
		assert all(win[0].stop <= w[0].start or w[0].stop <= win[0].start or win[1].stop <= w[1].start or w[1].stop <= win[1].start for w in wins)      # (disjoint)
		wins.append(win)
		got = omap.tensor[0][win]
		worst = max(worst, np.max(np.abs(np.float64(got.cpu().numpy())-want))/np.max(np.abs(want))/ULP)
		assert np.array_equal(got.cpu().numpy() != 0, want != 0) or np.all(np.abs(want[(got.cpu().numpy() != 0) != (want != 0)]) < 1e-37)
		nz += int(torch.count_nonzero(got)); asum += float(got.abs().sum(dtype=torch.float64))
	listed = np.array(sorted(listed))
	print("S3: %d tiles hold a pixel of a disc; worst error %.2f ulp of an object's peak" % (len(listed), worst))
	assert set(tiles.tolist()) <= set(listed.tolist()) and listed.min() == 0 and listed.max() == nty*ntx-1
	for seam in (SCAN_WG, SCAN_TRIP): assert np.any(listed == seam-1) and np.any(listed == seam)
	assert worst <= 64
	# nothing outside the windows: as many non-zero pixels, and as large a sum of |map|, as the windows hold
	total = float(omap.tensor.abs().sum(dtype=torch.float64))
	assert int(torch.count_nonzero(omap.tensor)) == nz and abs(total-asum) <= 1e-12*asum

# ---- P1: the point sort behind alm2map_pos past the carry of its scan ---------------------------------------------------------------
@pytest.mark.gpu
def test_p1_point_sort_gpu():
	"""1 049 601 points: the histogram of the sort has more chunks than one trip of scan_sums takes.  The sort decides where every point's
	value lands, so a wrong carry shows in the values at the points (against the oracle at 300 of them), in the comparison with the same
	call made in chunks whose sorts stay below the seam, and in the adjoint's dot-product identity"""
	from pixell_amd import _lib
	npts = (WG*K["SCAN_CHUNK"]//256+1)*K["RS_IPB"]+1      # 256: the 8-bit digits of the sort
	nblk = -(-npts//K["RS_IPB"]); L = 256*nblk; nc = -(-L//K["SCAN_CHUNK"])
	assert nc > WG, "does not reach the second trip of scan_sums"
	lmax = 255; eps = 1e-10
	good = _lib.load().pxf_fft_good_size
	nt, nph = sht.points_grid_shape(lmax, lmax)
	fine = lambda n: K["PT_T"]*int(good(max(2, -(-2*n//K["PT_T"]))))      # points.hip fine_size
	n1, n2 = fine(2*nt-2), fine(nph); nt2 = n2//K["PT_T"]
	loc = tp.special_loc(npts, 1049)
	rough = (np.floor(loc[:, 0]/(2*np.pi)*n1).astype(int)//K["PT_T"])*nt2+np.floor(np.remainder(loc[:, 1], 2*np.pi)/(2*np.pi)*n2).astype(int)//K["PT_T"]
	print("P1: %d points, %d sort blocks, %d chunks; fine grid %d x %d: %d tiles" % (npts, nblk, nc, n1, n2, (n1//K["PT_T"])*nt2))
	assert (n1//K["PT_T"])*nt2 > 256 and np.sum(rough >= 256) > npts//4 and np.sum(rough < 256) > npts//4, "the second digit of the sort key does not vary"
	rng = np.random.default_rng(1050)
	seam = K["SCAN_CHUNK"]*256      # the points whose blocks' histogram entries start a chunk of the scan
	must = np.unique([0, npts-1]+[k*seam+d for k in range(1, npts//seam+1) for d in (-1, 0) if k*seam+d < npts])
	idx = np.unique(np.concatenate([must, rng.choice(npts, 300-len(must), replace=False)]))
	assert all(k*seam+d in idx for k in range(1, npts//seam+1) for d in (-1, 0)) and npts//seam >= 4 and idx[0] == 0 and idx[-1] == npts-1 and 290 <= len(idx) <= 300
	step = 100000
	assert -(-step//K["RS_IPB"])*256 <= WG*K["SCAN_CHUNK"]      # (a chunk's own sort stays below the seam)
	for spin in (0, 2):
		nca = 1 if spin == 0 else 2
		a = tp.rand_alm(nca, lmax, seed=40+spin)
		m = sht.synthesis_general(alm=a, loc=loc, spin=spin, lmax=lmax, epsilon=eps)
		ref = tp.exact(a, loc[idx], lmax, spin, oracle=True)
		err = tp.rel(m[:, idx], ref)
		print("P1 spin %d: relative error at %d points %.2e" % (spin, len(idx), err))
		assert m.shape == (nca, npts) and err <= eps
		parts = np.concatenate([sht.synthesis_general(alm=a, loc=loc[o:o+step], spin=spin, lmax=lmax, epsilon=eps) for o in range(0, npts, step)], 1)
		assert np.array_equal(m, parts)
		y = np.random.default_rng(4).standard_normal(m.shape)
		at = sht.adjoint_synthesis_general(map=y, loc=loc, spin=spin, lmax=lmax, epsilon=eps)
		lhs = float(np.sum(m*y)); rhs = tp.alm_dot(a, at, lmax)
		assert abs(lhs-rhs) <= 1e-12*np.linalg.norm(m)*np.linalg.norm(y), (spin, abs(lhs-rhs)/(np.linalg.norm(m)*np.linalg.norm(y)))
