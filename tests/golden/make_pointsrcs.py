"""Generate tests/golden/pointsrcs.npz and pointsrcs_window.npz: inputs, a float64 model of pixell_amd.pointsrcs' semantics, and what the
REFERENCE's pixell.pointsrcs / enmap.apply_window give for the same inputs.

Run:  python tests/golden/make_pointsrcs.py      (needs /root/reference, cython and gcc; never run on the GPU box)

The reference is imported through _ref_harness.py; its cython/srcsim.pyx + srcsim_core.c are compiled into a temporary directory and
registered as pixell.srcsim.  Only arrays are saved.

The expected values are NOT the reference's.  The reference evaluates Vincenty's formula in float32 (it cancels for close points),
paints whole 8 x 8 cells, leaves the last radial bin incomplete and ignores `op`; pixell_amd defines (csrc/srcsim.hip)
  r = 2 asin sqrt(min(h, 1)), h = sin^2(ddec/2) + cos dec cos dec' sin^2(dra/2), coordinates rounded to float32
  P(r): linear interpolation of the profile, vs[0] below rs[0], 0 from the last sample on
  rcut_i = rs[min(k+1, n-1)], k the last sample with |vs[k]| >= vmin/max_c|amps[c,i]|, capped by rmax > 0; painted where r <= rcut_i
and `expected` is this script's own float64 numpy evaluation of that.  The reference's output is stored next to it with its error
against the model: a cross-check of the conventions, and the yardstick of how far off the reference is.

Cases (keys <case>_*):
  A   80 x 112 patch of the 0.5' full-sky geometry (rows 16800:16880, columns 1200:1312: dec 50 deg, RA 170 deg), 24 objects inside, one 3
      pixels outside an edge, one on a corner pixel; amps [3, 26]; Gaussian FWHM 1.4', 500 samples to 10 sigma; (vmin, rmax) = (1e-12, 0)
      [A0], (1e-3, 0) [A1], (1e-3, 3') [A2], (1e-12, 3') [A3]; max and min with (1e-3, 0) onto constant maps of +-0.25
  B   full sky 90 x 180, 40 objects (two on the RA seam, one within a pixel of each pole), sigma 1.2 pixels, vmin 1e-12
  C   A's geometry, 300 objects within 8 x 8 pixels, two profiles alternating (the second not equispaced, changing sign), vmin 1e-6
  D   radial_sum on A's geometry: 12 objects, a 2-component float32 map, bins of 8 x 1' and [0, .7, 1.1, 2, 3.3, 4, 6.5]'
  E   radial_sum on B's geometry with objects on the seam
  R   ramp profile [[0, 1 deg], [0, 1]], amplitude 1, D's objects one at a time: the map is r / 1 deg.  The model distance is stored on every
      7th pixel (the test evaluates the same float64 formula on all of them and is pinned to these).
  F   (pointsrcs_window.npz) enmap.apply_window on a 3 x 40 x 56 map, orders 0 and 1, pow +-1, reference with its numpy FFT engine
  beam_*, nsig_*: expand_beam / nsigma2rmax

Guard band of D and E: a pixel whose distance is within delta of a bin edge may fall on either side in float32.  delta = 2 x the
reference's measured distance error on R; every (object, bin) pair with such a pixel is marked in <case>_mask.  Asserted here: at most
30 % of the pairs are marked, and the reference agrees with the model on the unmarked pairs, its (incomplete) last bin excepted.
Also asserted: no pixel of a painted case lies within 2e-6 (relative) of an object's cut radius where the profile is still above 1e-9 there
(float32 may decide differently for such a pixel).

As run for the committed fixtures:
  A0: peak 2.873, reference off by 0.00035 = 1022 ulp of the peak
  B: peak 2.834, reference off by 3.76e-06 = 11 ulp of the peak
  smallest relative distance of a pixel from a cut radius: 2.03e-06
  R: the reference's distance error 9.75e-08 rad = 5624 ulp of the pixel size at most; guard band delta = 1.95e-07 rad
  D1: 29 % of the (object, bin) pairs marked; reference on the unmarked ones, last bin left out: 0.01 of the bound; its last bin is off by 8.94 on sums of scale 17
  D2: 14 % of the (object, bin) pairs marked; reference on the unmarked ones, last bin left out: 0.04 of the bound; its last bin is off by 29.6 on sums of scale 29.6
  E: 0 % of the (object, bin) pairs marked; reference on the unmarked ones, last bin left out: 0.00 of the bound; its last bin is off by 9.62 on sums of scale 26.2
  pointsrcs.npz: 823890 bytes, pointsrcs_window.npz: 260590 bytes
"""
import sys, os, types, subprocess, tempfile, sysconfig
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_harness as H

arcmin = np.pi/180/60
ULP = 2.0**-23

def build_srcsim(tmp):
	src = os.path.join(H.REF, "cython")
	subprocess.check_call([sys.executable, "-m", "cython", "-3", "-I", src, os.path.join(src, "srcsim.pyx"), "-o", os.path.join(tmp, "srcsim.c")])
	inc = [sysconfig.get_paths()["include"], np.get_include(), src]
	out = os.path.join(tmp, "srcsim"+sysconfig.get_config_var("EXT_SUFFIX"))
	subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-fopenmp", "-w"]+["-I"+i for i in inc]+[os.path.join(tmp, "srcsim.c"), os.path.join(src, "srcsim_core.c"), "-o", out, "-lm"])
	sys.path.insert(0, tmp)
	import srcsim
	return srcsim

# ---- the float64 model ------------------------------------------------------------------------------------------------------------
def dist64(pdec, pra, odec, ora):
	"""[ny, nx] distances of the pixels (float32 axes) from the object (float32 position), in float64"""
	pdec, pra, odec, ora = np.float64(pdec)[:, None], np.float64(pra)[None, :], np.float64(odec), np.float64(ora)
	h = np.sin((pdec-odec)/2)**2+np.cos(pdec)*np.cos(odec)*np.sin((pra-ora)/2)**2
	return 2*np.arcsin(np.sqrt(np.minimum(h, 1)))

def prof64(prof, r):
	rs, vs = np.float64(prof[0]), np.float64(prof[1])
	v = np.interp(r, rs, vs, left=vs[0], right=0.0)
	return np.where(r >= rs[-1], 0.0, v)

def rcut32(prof, acol, vmin, rmax):
	amax = np.max(np.abs(acol)).astype(np.float32)
	with np.errstate(divide="ignore"): vrel = np.float32(vmin)/amax
	ks = np.where(np.abs(prof[1]) >= vrel)[0]
	k = ks[-1] if len(ks) else 0
	rc = prof[0][min(k+1, prof.shape[1]-1)]
	if rmax > 0: rc = min(rc, np.float32(rmax))
	return np.float32(rc)

def model_paint(pdec, pra, poss, amps, profs, ids, vmin, rmax, op="add", base=None, near=None):
	ncomp, nobj = amps.shape
	out = np.zeros((ncomp, len(pdec), len(pra))) if base is None else np.float64(base).copy()
	for i in range(nobj):
		prof = profs[ids[i]]
		rc = np.float64(rcut32(prof, amps[:, i], vmin, rmax))
		r = dist64(pdec, pra, poss[0, i], poss[1, i])
		# (only where leaving a pixel out or taking it in would show: the profile has not dropped to nothing at the cut)
		if near is not None and np.max(np.abs(amps[:, i]))*abs(prof64(prof, np.array([rc*(1-1e-9)]))[0]) > 1e-9: near.append(np.min(np.abs(r-rc))/rc)
		P = prof64(prof, r); inside = r <= rc
		for c in range(ncomp):
			v = np.float64(amps[c, i])*P
			if op == "add": out[c] += np.where(inside, v, 0)
			elif op == "max": out[c] = np.where(inside, np.maximum(out[c], v), out[c])
			else: out[c] = np.where(inside, np.minimum(out[c], v), out[c])
	return out

def model_radial(pdec, pra, poss, m, bins, delta):
	"""(sums [nobj, ncomp, nbin], abs sums, pixel counts [nobj, nbin], mask [nobj, nbin] of the pairs with a pixel within delta of an edge of the bin)"""
	nobj = poss.shape[1]; nbin = len(bins)-1; b = np.float64(bins); m = np.float64(m)
	sums = np.zeros((nobj, m.shape[0], nbin)); asum = np.zeros_like(sums); cnt = np.zeros((nobj, nbin), int); mask = np.zeros((nobj, nbin), bool)
	for i in range(nobj):
		r = dist64(pdec, pra, poss[0, i], poss[1, i])
		edge_near = [np.any(np.abs(r-e) < delta) for e in b]
		for k in range(nbin):
			sel = (r >= b[k]) & (r < b[k+1])
			sums[i, :, k] = m[:, sel].sum(-1); asum[i, :, k] = np.abs(m[:, sel]).sum(-1); cnt[i, k] = sel.sum()
			mask[i, k] = edge_near[k] or edge_near[k+1]
	return sums, asum, cnt, mask

def geo_numbers(shape, wcs):
	return np.array([shape[-2], shape[-1]], float), np.array(wcs.wcs.cdelt, float), np.array(wcs.wcs.crval, float), np.array(wcs.wcs.crpix, float)

def pix2sky(enmap, shape, wcs, y, x):
	return enmap.pix2sky(shape, wcs, np.array([np.atleast_1d(y), np.atleast_1d(x)], float))

def main(write=True):
	tmp = tempfile.mkdtemp(prefix="pixell_srcsim_")
	srcsim = build_srcsim(tmp)
	sys.modules["pixell.srcsim"] = srcsim
	ns = H.load_reference(types.ModuleType("sht_exp"))
	import pixell
	pixell.srcsim = srcsim
	from pixell import pointsrcs
	enmap, utils = ns.enmap, ns.utils
	ns.fft.set_engine("numpy")
	out, rep = {}, []
	def say(s): rep.append(s); print(s)

	# ---- geometries ----
	fshape, fwcs = enmap.fullsky_geometry(res=0.5*arcmin)
	shapeA, wcsA = enmap.slice_geometry(fshape, fwcs, (slice(16800, 16880), slice(1200, 1312)))
	shapeA = tuple(int(v) for v in shapeA[-2:])
	shapeB, wcsB = enmap.fullsky_geometry(res=2*np.pi/180); shapeB = tuple(int(v) for v in shapeB[-2:])
	assert shapeA == (80, 112) and shapeB == (90, 180)
	out["A_geo"] = np.concatenate(geo_numbers(shapeA, wcsA)); out["B_geo"] = np.concatenate(geo_numbers(shapeB, wcsB))
	axA = enmap.posaxes(shapeA, wcsA, dtype=np.float32); axB = enmap.posaxes(shapeB, wcsB, dtype=np.float32)
	out["A_dec"], out["A_ra"], out["B_dec"], out["B_ra"] = axA[0], axA[1], axB[0], axB[1]
	pixA = abs(wcsA.wcs.cdelt[1])*np.pi/180

	sigma = 1.4*arcmin/(8*np.log(2))**0.5
	rs = np.linspace(0, 10*sigma, 500)
	gauss = np.array([rs, np.exp(-0.5*(rs/sigma)**2)]).astype(np.float32)
	out["A_prof"] = gauss

	def ref_paint(shape, wcs, poss, amps, prof, ids=None, vmin=None, rmax=None):
		return np.asarray(pointsrcs.sim_objects(shape, wcs, np.float64(poss), amps, prof, prof_ids=ids, vmin=vmin, rmax=rmax))

	# ---- A ----
	rng = np.random.default_rng(20240611)
	ys = np.concatenate([rng.uniform(2, 77, 24), [-3.0], [0.0]]); xs = np.concatenate([rng.uniform(2, 109, 24), [40.3], [111.0]])
	possA = np.float32(pix2sky(enmap, shapeA, wcsA, ys, xs))
	ampsA = (rng.uniform(0.5, 3, (3, 26))*rng.choice([-1, 1], (3, 26))).astype(np.float32)
	out["A_poss"], out["A_amps"] = possA, ampsA
	near = []
	for tag, vmin, rmax in [("A0", 1e-12, 0), ("A1", 1e-3, 0), ("A2", 1e-3, 3*arcmin), ("A3", 1e-12, 3*arcmin)]:
		exp = model_paint(axA[0], axA[1], possA, ampsA, [gauss], np.zeros(26, int), vmin, rmax, near=near)
		out[tag+"_par"] = np.array([vmin, rmax]); out[tag+"_expected"] = exp
		if tag == "A0":
			ref = ref_paint(shapeA, wcsA, possA, ampsA, gauss, vmin=vmin, rmax=rmax)
			err = np.max(np.abs(ref-exp)); out[tag+"_ref"] = ref; out[tag+"_ref_err"] = err
			say("  %s: peak %.3f, reference off by %.3g = %.0f ulp of the peak" % (tag, np.max(np.abs(exp)), err, err/np.max(np.abs(exp))/ULP))
	for op, c0 in (("max", 0.25), ("min", -0.25)):
		out["A_"+op+"_expected"] = model_paint(axA[0], axA[1], possA, ampsA, [gauss], np.zeros(26, int), 1e-3, 0, op=op, base=np.full((3,)+shapeA, c0), near=near)

	# ---- B ----
	rng = np.random.default_rng(7)
	pixB = 2*np.pi/180
	decB = np.concatenate([rng.uniform(-80, 80, 36)*np.pi/180, [0.3, -0.8], [np.pi/2-0.6*pixB, -np.pi/2+0.4*pixB]])
	raB = np.concatenate([rng.uniform(-np.pi, np.pi, 36), [np.pi-1e-3, -np.pi+0.01], [1.0, -2.0]])
	possB = np.float32([decB, raB])
	ampsB = (rng.uniform(0.5, 3, (1, 40))*rng.choice([-1, 1], (1, 40))).astype(np.float32)
	sB = 1.2*pixB; rB = np.linspace(0, 10*sB, 500)
	profB = np.array([rB, np.exp(-0.5*(rB/sB)**2)]).astype(np.float32)
	out["B_poss"], out["B_amps"], out["B_prof"] = possB, ampsB, profB
	exp = model_paint(axB[0], axB[1], possB, ampsB, [profB], np.zeros(40, int), 1e-12, 0, near=near)
	ref = ref_paint(shapeB, wcsB, possB, ampsB, profB, vmin=1e-12)
	err = np.max(np.abs(ref-exp)); out["B_expected"], out["B_ref"], out["B_ref_err"] = exp, ref, err
	say("  B: peak %.3f, reference off by %.3g = %.0f ulp of the peak" % (np.max(np.abs(exp)), err, err/np.max(np.abs(exp))/ULP))

	# ---- C ----
	rng = np.random.default_rng(3)
	possC = np.float32(pix2sky(enmap, shapeA, wcsA, rng.uniform(36, 44, 300), rng.uniform(50, 58, 300)))
	ampsC = (rng.uniform(0.5, 3, (2, 300))*rng.choice([-1, 1], (2, 300))).astype(np.float32)
	r2 = np.sort(np.concatenate([[0], rng.uniform(0, 5*arcmin, 60)]))
	prof2 = np.array([r2, np.cos(r2/(1.1*arcmin))*np.exp(-r2/(2*arcmin))]).astype(np.float32)
	idsC = (np.arange(300) % 2).astype(np.int32)
	out["C_poss"], out["C_amps"], out["C_prof2"], out["C_ids"] = possC, ampsC, prof2, idsC
	out["C_expected"] = model_paint(axA[0], axA[1], possC, ampsC, [gauss, prof2], idsC, 1e-6, 0, near=near)
	say("  smallest relative distance of a pixel from a cut radius: %.2e" % min(near))
	assert min(near) > 2e-6, "a pixel sits on a cut radius: change the seed"

	# ---- R and D ----
	rng = np.random.default_rng(5)
	possD = np.float32(pix2sky(enmap, shapeA, wcsA, rng.uniform(8, 72, 12), rng.uniform(8, 104, 12)))
	out["D_poss"] = possD
	ramp = np.array([[0, np.pi/180], [0, 1]], np.float32)
	r64 = np.array([dist64(axA[0], axA[1], possD[0, i], possD[1, i]) for i in range(12)])
	ref_derr = 0
	for i in range(12):
		m = ref_paint(shapeA, wcsA, possD[:, i:i+1], np.ones((1, 1), np.float32), ramp, vmin=1e-12)[0]
		ok = r64[i] < np.float64(ramp[0, 1])*(1-1e-3)
		ref_derr = max(ref_derr, np.max(np.abs(np.float64(m)*np.float64(ramp[0, 1])-r64[i])[ok]))
	out["R_r64_sub"] = r64.reshape(12, -1)[:, ::7]; out["R_ref_err"] = ref_derr
	delta = 2*ref_derr; out["D_delta"] = delta
	say("  R: the reference's distance error %.3g rad = %.0f ulp of the pixel size at most; guard band delta = %.3g rad" % (ref_derr, np.max(ref_derr/np.maximum(r64, pixA))/ULP, delta))
	mapD = rng.random((2, 80, 112)).astype(np.float32)*2-1
	out["D_map_seed"] = 5; out["D_map_head"] = mapD[:, 0, :8]
	def radial_case(tag, shape, wcs, ax, poss, m, bins):
		sums, asum, cnt, mask = model_radial(ax[0], ax[1], poss, m, bins, delta)
		ref = np.asarray(pointsrcs.radial_sum(enmap.ndmap(m, wcs), np.float64(poss), bins))
		out[tag+"_bins"], out[tag+"_expected"], out[tag+"_asum"], out[tag+"_cnt"], out[tag+"_mask"], out[tag+"_ref"] = np.float32(bins), sums, asum, cnt, mask, ref
		frac = mask.mean()
		tol = 4*cnt[:, None, :]*2.0**-24*asum
		good = ~mask[:, None, :-1] & np.ones(sums.shape, bool)[..., :-1]
		worst = np.max(np.where(good, np.abs(ref-sums)[..., :-1]/np.maximum(tol[..., :-1], 1e-30), 0))
		say("  %s: %.0f %% of the (object, bin) pairs marked; reference on the unmarked ones, last bin left out: %.2f of the bound; its last bin is off by %.3g on sums of scale %.3g" % (
			tag, 100*frac, worst, np.max(np.abs(ref-sums)[..., -1]), np.max(np.abs(sums[..., -1]))))
		assert frac <= 0.30, "too many pairs in the guard band: change the seed"
		assert worst <= 1, "the reference disagrees with the model outside the guard band"
	radial_case("D1", shapeA, wcsA, axA, possD, mapD, np.arange(9)*arcmin)
	radial_case("D2", shapeA, wcsA, axA, possD, mapD, np.array([0, .7, 1.1, 2, 3.3, 4, 6.5])*arcmin)
	# ---- E ----
	rng = np.random.default_rng(9)
	possE = np.float32([np.concatenate([rng.uniform(-1.2, 1.2, 4), [0.2, -0.5, 1.0]]), np.concatenate([rng.uniform(-3, 3, 4), [np.pi-2e-3, -np.pi+0.02, np.pi]])])
	mapE = rng.random((1, 90, 180)).astype(np.float32)*2-1
	out["E_poss"] = possE; out["E_map_seed"] = 9; out["E_map_head"] = mapE[:, 0, :8]
	radial_case("E", shapeB, wcsB, axB, possE, mapE, np.arange(7)*5*np.pi/180)

	# ---- beams ----
	out["beam_sigma"] = np.array(sigma); out["beam_gauss"] = pointsrcs.expand_beam(sigma, nsigma=5)
	out["beam_rmax"] = pointsrcs.expand_beam(sigma, nsigma=4, rmax=7*arcmin)
	out["nsig_rmax"] = np.array([pointsrcs.nsigma2rmax(np.float64(gauss), n) for n in (3, 5)])
	srcs = np.concatenate([np.float64(possA[:, :6]).T, np.float64(ampsA[:, :6]).T], 1)
	out["S_srcs"] = srcs

	# ---- F ----
	win = {}
	rng = np.random.default_rng(13)
	m = rng.standard_normal((3, 40, 56))
	_, wcsF = enmap.slice_geometry(fshape, fwcs, (slice(10000, 10040), slice(300, 356)))
	win["F_map"] = m
	for order in (0, 1):
		for p in (1, -1):
			win["F_o%d_p%+d" % (order, p)] = np.asarray(enmap.apply_window(enmap.ndmap(m.copy(), wcsF), pow=p, order=order))
	wy, wx = enmap.calc_window((40, 56), order=1, scale=2); win["F_wy"], win["F_wx"] = wy, wx

	if write:
		np.savez_compressed(os.path.join(HERE, "pointsrcs.npz"), **out)
		np.savez_compressed(os.path.join(HERE, "pointsrcs_window.npz"), **win)
		for f in ("pointsrcs.npz", "pointsrcs_window.npz"): say("  %s: %d bytes" % (f, os.path.getsize(os.path.join(HERE, f))))
	return rep

if __name__ == "__main__":
	main()
