"""Generate tests/golden/analysis.npz and analysis_uht.npz: what the REFERENCE's analysis.NmatConstcov / NmatConstcorr matched filters, FinderSimple and
MeasurerSimple give on a small two-frequency patch, and the discrete choices they make on the way (scipy.ndimage.label's output, the grown
labels), for tests/test_analysis.py.

Run:  python tests/golden/make_analysis.py      (needs /root/reference, cython, gcc and scipy; never run on the GPU box)

The reference is imported through _ref_harness.py on its numpy FFT engine, with its distances extension compiled into a temporary
directory as make_distances.py does.  Only arrays are saved.

The sky (analysis_inputs, shared with the test, which rebuilds everything but the noise from formulas): [2, 64, 96] pixels of 0.5 arcmin,
rows 10768:10832 (dec 0, case E) or 4768:4832 (dec -50 deg, case S) and columns 1200:1296 of the 0.5 arcmin full-sky geometry; Gaussian
beams of 1.4 and 1.1 arcmin FWHM; white noise of unit variance modulated by an ivar with a ripple and a 5 x 5 hole; an inverse noise
spectrum with a knee and a cross term; eight painted sources: two 2.4 pixels apart (one label), one just below snmin, one 1.5 pixels from
the patch edge.

Also: matched_filter_constcov, _white, _constcorr_lowcorr (with and without high_acc) and _constcorr_smoothivar over the reference's UHT
on the flat (F: 12 deg band at 1.5 deg) and the curved (C: 30 x 60 full sky, lmax 24, the long-double oracle as ducc0) geometry of
make_uharm.py, one map with a source, an ivar with a ripple and a hole, a Gaussian beam and a knee-shaped inverse noise spectrum.

Asserted here, so that the reference alone decides every discrete choice:
  no pixel has |snr_tot - snlim| < 1e-6 snlim;
  no pixel's exact (method="simple") distance from the labels lies within 4 x the largest |cellgrid - simple| of finder.grow, the largest
    being taken over the pixels of that case within 2 finder.grow of a label, and the two methods grow the same labels; finder.grow is
    0.89 arcmin, between two neighbour distances of both patches;
  no catalogue position has a fractional pixel part within 1e-6 of 0.5 (the order-0 reads);
  a raster-order flood fill (the one of tests/test_labels.py) gives scipy's labels.
"""
import sys, os, types, tempfile
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..")); sys.path.insert(0, HERE); sys.path.insert(0, os.path.join(HERE, ".."))
import _ref_harness as H
import make_distances as MD

arcmin = np.pi/180/60
ROWS = {"E": 10768, "S": 4768}
SNMIN = 5.0
GROW = 0.89*arcmin      # finder.grow: between the neighbour distances 0.814 and 0.964 arcmin of the patch at dec -50 and 0.707 and 1.0 arcmin of the one at dec 0

def analysis_inputs(shape, pixsize, l, posmap, seed):
	"""everything the cases feed the filters, from the geometry's numbers: shape (ny, nx), the mean pixel area, |l| of the 2-D fourier
	bins [ny, nx] and the positions [{dec,ra}, ny, nx].  Returns dict(map, ivar, iN, beam, srcs)."""
	ny, nx = shape
	yy, xx = np.mgrid[:ny, :nx]
	sig = np.array([1.4, 1.1])*arcmin/(8*np.log(2))**0.5
	beam = np.exp(-0.5*l[None]**2*sig[:, None, None]**2)
	ivar = np.array([1+0.3*np.sin(yy/7.0)*np.cos(xx/11.0), 0.8+0.2*np.cos(yy/5.0+xx/9.0)])
	ivar[:, 40:45, 20:25] = 0
	knee = 1.0/(1+(np.maximum(l, 1e-3)/3000.0)**-3)
	iN = np.zeros((2, 2, ny, nx))
	iN[0, 0] = knee; iN[1, 1] = 0.9*knee; iN[0, 1] = iN[1, 0] = -0.1*knee
	iN[:, :, 0, 0] = 0
	rng = np.random.default_rng(seed)
	noise = rng.standard_normal((2, ny, nx))
	with np.errstate(divide="ignore"): noise = np.where(ivar > 0, noise*np.where(ivar > 0, ivar, 1)**-0.5, 0)
	#            y      x     amplitude
	srcs = np.array([[12.3, 15.6, 9.0], [13.1, 17.9, 7.0], [30.7, 60.2, 14.0], [50.2, 80.4, 6.0], [20.6, 40.3, 1.65],
		[1.5, 50.3, 8.0], [45.3, 10.8, 5.0], [33.4, 90.1, 4.0]])
	dec, ra = posmap
	sky = np.zeros((2, ny, nx))
	for y, x, amp in srcs:
		iy, ix = int(y), int(x)
		d0 = dec[iy, ix]+(y-iy)*(dec[min(iy+1, ny-1), ix]-dec[iy, ix] if iy+1 < ny else dec[iy, ix]-dec[iy-1, ix])
		r0 = ra[iy, ix]+(x-ix)*(ra[iy, ix+1]-ra[iy, ix] if ix+1 < nx else ra[iy, ix]-ra[iy, ix-1])
		r2 = (dec-d0)**2+((ra-r0)*np.cos(d0))**2
		sky += amp*np.array([1.0, 0.8])[:, None, None]*np.exp(-0.5*r2[None]/sig[:, None, None]**2)
	return dict(map=sky+noise, ivar=ivar, iN=iN, beam=beam, srcs=srcs)

def numpy1_solve():
	"""np.linalg.solve(a, b) with b one axis short of a as a stack of vectors, numpy 1's rule, which the reference's solve_mapsys is
	written for (numpy 2 reads such a b as a stack of matrices and refuses the shapes)"""
	solve = np.linalg.solve
	def solve1(a, b):
		a, b = np.asarray(a), np.asarray(b)
		return solve(a, b[..., None])[..., 0] if b.ndim == a.ndim-1 else solve(a, b)
	np.linalg.solve = solve1

def uht_inputs(shape, lmax, sigma, seed):
	"""map, ivar [ny, nx] and the l profiles of the beam and of the inverse noise power for the UHT filter cases"""
	ny, nx = shape
	yy, xx = np.mgrid[:ny, :nx]
	rng = np.random.default_rng(seed)
	ivar = 1+0.3*np.sin(yy/3.0)*np.cos(xx/5.0)
	ivar[ny//2+2:ny//2+4, nx//3:nx//3+2] = 0
	m = rng.standard_normal(shape)+6*np.exp(-0.5*((yy-ny//2)**2+(xx-nx//2)**2)/1.5**2)
	l = np.arange(lmax+1.0)
	return dict(map=m, ivar=ivar, lbeam=np.exp(-0.5*l*(l+1)*sigma**2), linv=1/(1+((l+1)/(0.3*lmax))**-2.5))

def uht_filters(analysis, u, m, ivar, B, iC):
	"""every UHT filter case: name -> (rho, kappa)"""
	return {"constcov": analysis.matched_filter_constcov(m, B, iC, u), "white": analysis.matched_filter_white(m, B, ivar, u),
		"lowcorr": analysis.matched_filter_constcorr_lowcorr(m, B, ivar, iC, u), "lowcorr_acc": analysis.matched_filter_constcorr_lowcorr(m, B, ivar, iC, u, high_acc=True),
		"smoothivar": analysis.matched_filter_constcorr_smoothivar(m, B, ivar, iC, u)}

def geo_numbers(shape, wcs):
	return np.concatenate([np.array([shape[-2], shape[-1]], float), np.array(wcs.wcs.cdelt, float), np.array(wcs.wcs.crval, float), np.array(wcs.wcs.crpix, float)])

def main(write=True):
	tmp = tempfile.mkdtemp(prefix="pixell_analysis_")
	distances = MD.build_distances(tmp)
	sys.modules["pixell.distances"] = distances
	from oracle import sht_oracle as so
	ns = H.load_reference(so)
	import pixell
	pixell.distances = distances
	ns.fft.set_engine("numpy")
	numpy1_solve()
	from pixell import analysis
	from scipy import ndimage
	from test_labels import flood
	enmap = ns.enmap
	out, rep = {}, []
	def say(s): rep.append(s); print(s)
	# ---- the UHT filters on the flat and the curved geometry of make_uharm.py
	from pixell import uharm
	for tag, (shape, wcs), mode, lmax, sigma in (("F", enmap.band_geometry(np.deg2rad(12), res=np.deg2rad(1.5)), "flat", None, np.deg2rad(2.5)),
			("C", enmap.fullsky_geometry(shape=(30, 60)), "curved", 24, np.deg2rad(6.0))):
		shape = tuple(int(v) for v in shape[-2:])
		u = uharm.UHT(shape, wcs, mode=mode, lmax=lmax)
		inp = uht_inputs(shape, u.lmax, sigma, 31)
		out[tag+"_geo"] = geo_numbers(shape, wcs)
		for key, val in inp.items(): out["%s_%s" % (tag, key)] = val
		B, iC = u.lprof2hprof(inp["lbeam"]), u.lprof2hprof(inp["linv"])
		for name, (rho, kappa) in uht_filters(analysis, u, enmap.ndmap(inp["map"], wcs), enmap.ndmap(inp["ivar"], wcs), B, iC).items():
			out["%s_%s_rho" % (tag, name)], out["%s_%s_kappa" % (tag, name)] = np.asarray(rho), np.asarray(kappa)
			assert np.all(np.isfinite(rho)) and np.all(np.isfinite(kappa)), (tag, name)
		say("  %s: UHT filters recorded, %s mode, lmax %d" % (tag, mode, u.lmax))
	fshape, fwcs = enmap.fullsky_geometry(res=0.5*arcmin)
	for tag, row in ROWS.items():
		shape, wcs = enmap.slice_geometry(fshape, fwcs, (slice(row, row+64), slice(1200, 1296)))
		shape = tuple(int(v) for v in shape[-2:])
		out[tag+"_geo"] = geo_numbers(shape, wcs)
		l, pos = np.asarray(enmap.modlmap(shape, wcs)), np.asarray(enmap.posmap(shape, wcs))
		inp = analysis_inputs(shape, enmap.pixsize(shape, wcs), l, pos, 2024)
		out[tag+"_map"] = inp["map"]
		m = lambda a: enmap.ndmap(np.array(a), wcs)
		cc = analysis.NmatConstcorr(m(inp["iN"]), m(inp["ivar"]))
		if tag == "E":
			cv = analysis.NmatConstcov(m(inp["iN"]), m(np.ones(shape)))
			rho, kappa = cv.matched_filter(m(inp["map"]), m(inp["beam"]))
			out["E_cov_rho"], out["E_cov_kappa"] = np.asarray(rho), np.asarray(kappa)[:, :, :, :1]      # (constant along x)
			assert np.all(np.asarray(kappa) == np.asarray(kappa)[:, :, :, :1])
			rho, kappa = cc.matched_filter(m(inp["map"]), m(inp["beam"]))
			out["E_corr_rho"], out["E_corr_kappa"] = np.asarray(rho), np.asarray(kappa)[[0, 0, 1], [0, 1, 1]]
		finder = analysis.FinderSimple(cc, m(inp["beam"]), scaling=np.array([1.0, 0.8]))
		finder.grow = GROW
		res = finder(m(inp["map"]), snmin=SNMIN)
		snr, snlim = np.asarray(res.snr), float(res.snlim)
		gap = np.min(np.abs(snr-snlim))
		say("  %s: %d sources, S/N %s; nearest |snr - snlim| = %.3g" % (tag, len(res.cat), np.round(res.cat.snr, 2), gap))
		assert gap > 1e-6*snlim, "a pixel sits on the threshold"
		lab, nlabel = ndimage.label(snr >= snlim)
		assert nlabel == len(res.cat)
		fl, fn = flood(snr >= snlim)
		assert fn == nlabel and np.array_equal(fl, lab), "the flood fill and scipy disagree"
		lm = enmap.ndmap(lab.astype(np.int32), wcs)
		dcg, gcg = lm.labeled_distance_transform(rmax=finder.grow0)
		dsi, gsi = enmap.labeled_distance_transform(lm, rmax=finder.grow0, method="simple")
		near_grow = np.asarray(dsi) <= 2*finder.grow      # (where a pixel can change sides; further out the reference's error grows with the distance)
		cgerr = float(np.max(np.abs(np.asarray(dcg)-np.asarray(dsi))[near_grow]))
		margin = float(np.min(np.abs(np.asarray(dsi)-finder.grow)))
		say("  %s: cellgrid off by %.3g rad; nearest exact distance to grow = %.3g rad" % (tag, cgerr, margin))
		assert margin > 4*cgerr and margin > 1e-9, "a distance sits on finder.grow"
		grown = np.asarray(gcg)*(np.asarray(dcg) <= finder.grow)
		assert np.array_equal(grown, np.asarray(gsi)*(np.asarray(dsi) <= finder.grow)), "cellgrid and simple grow differently"
		pixs = np.array(ndimage.center_of_mass(snr**2, grown, np.arange(1, nlabel+1))).T
		frac = np.abs(pixs-np.floor(pixs)-0.5)
		assert frac.min() > 1e-6, "a position sits on a pixel border"
		# what the case is about: the pair is one label, the faint source is missed, the edge source is found
		srcs = inp["srcs"]
		near = lambda k: np.hypot(pixs[0]-srcs[k, 0], pixs[1]-srcs[k, 1]).min()
		assert lab[12, 16] == lab[13, 18] != 0 and near(4) > 3 and near(5) < 1 and 3.0 < snr[21, 40] < SNMIN, (near(4), near(5), snr[21, 40])
		cat = res.cat
		for key in ("ra", "dec", "snr", "flux_tot", "dflux_tot", "flux", "dflux"): out["%s_cat_%s" % (tag, key)] = np.asarray(cat[key])
		out[tag+"_snr"], out[tag+"_snlim"], out[tag+"_labels"], out[tag+"_grown"] = snr, snlim, lab.astype(np.int32), grown.astype(np.int32)
		# the measurer at the found positions, shifted by a fraction of a pixel
		icat = cat.copy(); icat.ra = icat.ra+0.11*arcmin; icat.dec = icat.dec-0.07*arcmin
		mpix = enmap.sky2pix(shape, wcs, [icat.dec, icat.ra])
		assert np.abs(mpix-np.floor(mpix)-0.5).min() > 1e-6
		mcat = analysis.MeasurerSimple(cc, m(inp["beam"]), scaling=np.array([1.0, 0.8]))(m(inp["map"]), icat).cat
		for key in ("ra", "dec", "snr", "flux_tot", "dflux_tot", "flux", "dflux"): out["%s_mcat_%s" % (tag, key)] = np.asarray(mcat[key])
	if write:
		for name, keep in (("analysis.npz", lambda k: k[0] in "ES"), ("analysis_uht.npz", lambda k: k[0] in "FC")):      # (two files: each below the size a committed file may have)
			f = os.path.join(HERE, name)
			np.savez_compressed(f, **{k: v for k, v in out.items() if keep(k)})
			say("  %s: %d bytes" % (name, os.path.getsize(f)))
	return rep

if __name__ == "__main__":
	main()
