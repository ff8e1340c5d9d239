"""The operator entry points on device arrays that are not C-contiguous.  pixell_amd/_arrays.py promises that torch tensors are "used
where they are"; many wrappers compute raw addresses from a tensor's shape (enmap._rotate_pairs, calc_ps2d, lbin, almops.bank_*,
lensing._deflect ...), some after a .contiguous() of their own, some trusting the caller.  Every other test hands them C-contiguous
tensors.  Here one table of entry points (ROWS) runs each on four forms of one argument at a time:

  contiguous   the reference run
  permuted     the same values over storage in reversed axis order (dense, what clone() keeps)
  sliced       the same values as a step-2 view inside a larger tensor of zeros
  expanded     a stride-0 view of the leading axis, for inputs whose leading entries may be equal; compared with the contiguous run on
               the same (repeated) values

and asserts that (1) the result is BITWISE that of the contiguous run -- it is the same kernel on the same values -- and (2) the
argument's whole storage is bitwise what it was.  enmap.fft at and above the dense-route threshold, where a view and its contiguous
copy take different kernels, is in test_fft_layouts.py (case 13).

Four rows cannot be bitwise on the GPU, whatever the layout: enmap.lbin, enmap.rbin (pxm_lbin, pxm_bin_index: float64 atomic adds into
LDS and global histograms) and pointsrcs.radial_sum, radial_bin (float32 atomic adds per bin) sum in the order the hardware serves the
atomics, so two runs on the SAME contiguous tensor differ in the last bits (measured on the MI355X: lbin 2.6e-16, radial_sum 1.9e-7 of
the largest value).  Their simulator twins, where one thread runs after the other, stay bitwise.  Their GPU twins bound the difference
by what two orders of one sum can differ by: every order of a sum of n terms is within (n-1) u sum|v_i| of the exact sum (u = 2^-53 or
2^-24, the accumulator's unit roundoff), so two of them are within 2 n u sum|v_i| of each other.  n and sum|v_i| are taken per output
bin -- the entry point's own pixel counts and its result on |map| -- so the bound is some 1e-13 (lbin) and 1e-5 (radial_sum) of a
bin's content, where an addressing fault moves whole pixels between bins.  The wrappers hand these kernels a contiguous copy, so the
property under test, that the kernel reads the view's values, is asserted no less.

(The Legendre analysis behind map2alm, map2wave and the healpix and point adjoints adds into its moments with atomics as well, but at
these sizes -- 12 ring pairs, one wave per m -- with one addition per row: bitwise, as test_pass_seams.py relies on.)

OUT_ROWS gives caller-supplied outputs as views: each is either filled, the returned object being (a map of) the view and nothing
outside it written, or refused with ValueError.  Which of the two is pinned per row; nothing may be written to a silent copy.

Sizes: a 24 x 40 full-sky geometry, lmax 20, 3 components, 50 points, unless a kernel needs more."""
import numpy as np
import pytest
import torch
from pixell_amd import enmap, curvedsky, almops, interpol, lensing, pointsrcs, reproject, uharm, wavelets, multimap, distances, sht
from pixell_amd import _arrays as A

NY, NX, LMAX, NC, NPT = 24, 40, 20, 3, 50
SHAPE, WCS = enmap.fullsky_geometry(shape=(NY, NX))
AINFO = curvedsky.alm_info(lmax=LMAX)
NELEM = AINFO.nelem
# a small patch for the flat-sky rows (UHT in flat mode)
PSHAPE, PWCS = (NY, NX), enmap.CarWCS(cdelt=[-0.05, 0.05], crval=[0.0, 0.0], crpix=[NX/2+0.5, NY/2+0.5])

def ident(t): return t
def cuda(t): return t.cuda()
def host(x):
	if isinstance(x, (enmap.dmap, multimap.dmaps)): x = x.tensor
	return np.array(x.detach().cpu().numpy()) if A.is_tensor(x) else np.array(x)
def flat(res):
	"""a result as a list of host arrays"""
	if isinstance(res, (tuple, list)): return [a for r in res for a in flat(r)]
	return [host(res)]
def same(got, ref):
	got, ref = flat(got), flat(ref)
	return len(got) == len(ref) and all(g.shape == r.shape and g.dtype == r.dtype and np.array_equal(g, r, equal_nan=g.dtype.kind in "fc") for g, r in zip(got, ref))
def bits(t): return host(torch.view_as_real(t) if t.is_complex() else t).tobytes()

def as_form(form, v, dev):
	"""(view, base) holding the values v in the given form"""
	v = np.ascontiguousarray(v); nd = v.ndim
	if form == "contiguous":
		t = dev(torch.from_numpy(v.copy())); return t, t
	if form == "permuted":
		rev = tuple(range(nd))[::-1]
		base = dev(torch.from_numpy(np.ascontiguousarray(v.transpose(rev))))
		return base.permute(*rev), base
	if form == "sliced":
		base = dev(torch.zeros(tuple(2*n+1 for n in v.shape), dtype=torch.from_numpy(v).dtype))
		t = base[tuple(slice(1, 2*n, 2) for n in v.shape)]
		t.copy_(torch.from_numpy(v).to(t.device)); return t, base
	if form == "expanded":
		base = dev(torch.from_numpy(v[:1].copy())); return base.expand(*v.shape), base
	raise ValueError(form)

RNG = np.random.default_rng(31)
def rn(*shape): return RNG.standard_normal(shape)
def cn(*shape): return RNG.standard_normal(shape)+1j*RNG.standard_normal(shape)

# ---- the inputs: made once, shared, never written to ----------------------------------------------------------------------------
MAP = rn(NC, NY, NX); HARM = cn(NC, NY, NX); HARM2 = cn(NC, NY, NX)
ALM = cn(NC, NELEM); ALM[:, :LMAX+1] = ALM[:, :LMAX+1].real
ANGLE = rn(NY, NX)
DEC = RNG.uniform(-1.4, 1.4, NPT); RA = RNG.uniform(-3.0, 3.0, NPT)
POS = np.array([DEC, RA]); PIXPOS = np.array([RNG.uniform(0, NY-1, NPT), RNG.uniform(0, NX-1, NPT)])
MASK = (RNG.random((NY, NX)) > 0.1).astype(np.uint8)
LFILTER = 1.0/(1.0+np.arange(LMAX+1.0))
PHI_ALM = 1e-3*ALM[0]/(1.0+np.arange(NELEM))
GRAD = 1e-2*rn(2, NPT); POS3 = np.array([DEC, RA, RNG.uniform(0, 1, NPT)])
BINS = np.linspace(0, 0.5, 6)
BANK_LMAXS, BANK_LS = [8, 14, 20], [10, 14, 20]
BANK_FILTERS = [np.cos(0.05*(i+1)*np.arange(LMAX+1.0)) for i in range(3)]
BANK_ALMS = [cn(NC, almops.tri_nelem(L)) for L in BANK_LS]
PROFILE = np.array([np.linspace(0, 0.3, 40), np.exp(-0.5*(np.linspace(0, 0.3, 40)/0.06)**2)])
AMPS = RNG.uniform(0.5, 2.0, (NC, NPT)).astype(np.float32)
COORDS = np.array([RNG.uniform(-1.0, 1.0, 8), RNG.uniform(-3.0, 3.0, 8)]).T.copy()      # [8, {dec,ra}]
LOC = np.array([np.pi/2-DEC, np.mod(RA, 2*np.pi)]).T.copy()                             # [npts, {theta,phi}]
NSIDE = 4; HMAP = rn(NC, 12*NSIDE**2)
UHT = uharm.UHT(PSHAPE, PWCS, mode="flat")
_wt = {}
def wavelet_transform():
	"""one curved-sky wavelet transform of the geometry, made when first needed"""
	if "wt" not in _wt: _wt["wt"] = wavelets.WaveletTransform(uharm.UHT(SHAPE, WCS, mode="curved", lmax=LMAX), basis=wavelets.ButterTrim(step=2, lmin=4, lmax=LMAX))
	return _wt["wt"]
_wave = {}
def wave_values():
	if "w" not in _wave: _wave["w"] = host(wavelet_transform().map2wave(enmap.ndmap(MAP, WCS)))
	return _wave["w"]
def wave_of(t):
	wt = wavelet_transform()
	return multimap.dmaps(t, wt.geometries)

def dm(t, wcs=WCS): return enmap.dmap(t, wcs)
def new_map(t, dtype=torch.float64): return dm(torch.zeros((NC, NY, NX), dtype=dtype, device=t.device))

# ---- input rows: (name, {argument: values}, call(tensors) -> result, [(argument to vary, may be expanded)]) ----------------------------------
ROWS = [
	("enmap.map2harm", dict(m=MAP), lambda a: enmap.map2harm(dm(a["m"])), [("m", True)]),
	("enmap.harm2map", dict(h=HARM), lambda a: enmap.harm2map(dm(a["h"])), [("h", True)]),
	("enmap.harm2map(keep_imag=True)", dict(h=HARM), lambda a: enmap.harm2map(dm(a["h"]), keep_imag=True), [("h", True)]),
	("enmap.map2harm_adjoint", dict(h=HARM), lambda a: enmap.map2harm_adjoint(dm(a["h"])), [("h", True)]),
	("enmap.harm2map_adjoint", dict(m=MAP), lambda a: enmap.harm2map_adjoint(dm(a["m"])), [("m", True)]),
	("enmap.calc_ps2d", dict(h=HARM), lambda a: enmap.calc_ps2d(dm(a["h"])), [("h", True)]),
	("enmap.calc_ps2d, [:, None] x [None, :]", dict(h=HARM, g=HARM2), lambda a: enmap.calc_ps2d(dm(a["h"][:, None]), dm(a["g"][None, :])), [("h", True), ("g", True)]),
	("enmap.lbin", dict(m=MAP), lambda a: enmap.lbin(dm(a["m"], PWCS)), [("m", True)], lambda v, dev: bin_bound(enmap.lbin, v, dev)),
	("enmap.rbin", dict(m=MAP), lambda a: enmap.rbin(dm(a["m"], PWCS)), [("m", True)], lambda v, dev: bin_bound(enmap.rbin, v, dev)),
	("enmap.rotate_pol", dict(m=MAP, ang=ANGLE), lambda a: enmap.rotate_pol(dm(a["m"]), a["ang"]), [("m", True), ("ang", True)]),
	("enmap.at", dict(m=MAP, pos=POS), lambda a: enmap.at(dm(a["m"]), a["pos"]), [("m", True), ("pos", False)]),
	("enmap.distance_transform", dict(mask=MASK), lambda a: enmap.distance_transform(dm(a["mask"])), [("mask", True)]),
	("curvedsky.alm2cl", dict(alm=ALM), lambda a: curvedsky.alm2cl(a["alm"]), [("alm", True)]),
	("curvedsky.almxfl", dict(alm=ALM), lambda a: curvedsky.almxfl(a["alm"], LFILTER), [("alm", True)]),
	("curvedsky.rotate_alm", dict(alm=ALM), lambda a: curvedsky.rotate_alm(a["alm"], 0.3, 0.7, -0.4), [("alm", True)]),
	("curvedsky.alm2map", dict(alm=ALM), lambda a: curvedsky.alm2map(a["alm"], new_map(a["alm"])), [("alm", True)]),
	("curvedsky.map2alm", dict(m=MAP), lambda a: curvedsky.map2alm(dm(a["m"]), lmax=LMAX), [("m", True)]),
	("almops.bank_split", dict(alm=ALM), lambda a: AINFO.bank_split(a["alm"], BANK_FILTERS, BANK_LMAXS, BANK_LS), [("alm", True)]),
	("almops.bank_merge", dict(a0=BANK_ALMS[0], a1=BANK_ALMS[1], a2=BANK_ALMS[2]), lambda a: AINFO.bank_merge([a["a0"], a["a1"], a["a2"]], BANK_FILTERS, BANK_LMAXS, BANK_LS), [("a0", True), ("a2", True)]),
	("interpol.interpol", dict(m=MAP, inds=PIXPOS), lambda a: interpol.interpol(a["m"], a["inds"]), [("m", True), ("inds", False)]),
	("interpol.spline_filter", dict(m=MAP), lambda a: interpol.spline_filter(a["m"]), [("m", True)]),
	("lensing.offset_by_grad", dict(pos=POS3, grad=GRAD), lambda a: lensing.offset_by_grad(a["pos"], a["grad"]), [("grad", False), ("pos", False)]),      # (an expanded gradient: test_expanded_gradient_is_refused)
	# (lens_map_curved takes no output map; its own bands of a larger device map are what delta_theta makes it write: four bands of 6 rows here)
	("lensing.lens_map_curved", dict(phi=PHI_ALM, cmb=ALM), lambda a: lensing.lens_map_curved((NC, NY, NX), WCS, a["phi"], a["cmb"], output="lua", delta_theta=np.pi/3), [("cmb", True), ("phi", False)]),
	("pointsrcs.radial_sum", dict(m=MAP, pos=POS), lambda a: pointsrcs.radial_sum(dm(a["m"]), a["pos"], BINS), [("m", True), ("pos", False)], lambda v, dev: radial_bound(pointsrcs.radial_sum, v, dev)),
	("pointsrcs.radial_bin", dict(m=MAP, pos=POS), lambda a: pointsrcs.radial_bin(dm(a["m"]), a["pos"], BINS), [("m", True), ("pos", False)], lambda v, dev: radial_bound(pointsrcs.radial_bin, v, dev)),
	("pointsrcs.sim_objects", dict(pos=POS, amps=AMPS), lambda a: pointsrcs.sim_objects(SHAPE, WCS, a["pos"], a["amps"], PROFILE, vmin=1e-3), [("amps", True), ("pos", False)]),
	("reproject.thumbnails", dict(m=MAP, coords=COORDS), lambda a: reproject.thumbnails(dm(a["m"]), a["coords"], r=0.3, res=0.1), [("m", True), ("coords", True)]),
	("uharm.UHT.map2harm (flat)", dict(m=MAP), lambda a: UHT.map2harm(dm(a["m"], PWCS), spin=[0, 2]), [("m", True)]),
	("uharm.UHT.harm2map (flat)", dict(h=HARM), lambda a: UHT.harm2map(dm(a["h"], PWCS), spin=[0, 2]), [("h", True)]),
	("uharm.UHT.harm2powspec (flat)", dict(h=HARM, g=HARM2), lambda a: UHT.harm2powspec(dm(a["h"], PWCS), dm(a["g"], PWCS)), [("h", True), ("g", True)]),
	("wavelets.map2wave", dict(m=MAP), lambda a: wavelet_transform().map2wave(dm(a["m"])), [("m", True)]),
	("wavelets.wave2map", dict(w=None), lambda a: wavelet_transform().wave2map(wave_of(a["w"])), [("w", True)]),
	# (multimap.mean / var are torch's own reductions, whose order of summation follows the strides: not bitwise, and no kernel of this library)
	("multimap.dmaps min / max", dict(w=None), lambda a: [multimap.min(wave_of(a["w"])), multimap.max(wave_of(a["w"]))], [("w", True)]),
	("distances.distance_from_points", dict(pts=POS, skip=MASK), lambda a: distances.distance_from_points(SHAPE, WCS, points=a["pts"], skip=a["skip"], domains=True), [("pts", False), ("skip", True)]),
	("sht.synthesis_general", dict(alm=ALM[1:], loc=LOC), lambda a: sht.synthesis_general(alm=a["alm"], loc=a["loc"], spin=2, lmax=LMAX), [("loc", False), ("alm", True)]),
	("sht.adjoint_synthesis_general", dict(m=MAP.reshape(NC, -1)[1:, :NPT], loc=LOC), lambda a: sht.adjoint_synthesis_general(map=a["m"], loc=a["loc"], spin=2, lmax=LMAX), [("loc", False), ("m", True)]),
	("curvedsky.alm2map_healpix", dict(alm=ALM), lambda a: curvedsky.alm2map_healpix(a["alm"], nside=NSIDE), [("alm", True)]),
	("curvedsky.map2alm_healpix", dict(m=HMAP), lambda a: curvedsky.map2alm_healpix(a["m"], lmax=2*NSIDE), [("m", True)]),
]

# ---- the rows whose kernels sum with floating-point atomics (the module docstring): what two orders of one sum may differ by ---------------
def bin_bound(fn, vals, dev):
	"""lbin / rbin -> (means [..., nbin], bin centres): 2 n_k 2^-53 mean_k|v| for the means, n_k the pixels of bin k; the centres are bitwise
	(made on the host, or by the first call on a geometry and kept)"""
	mean_abs, _, nhit = fn(dm(t_(np.abs(vals["m"]), dev), PWCS), return_nhit=True)
	with np.errstate(invalid="ignore"): return [2*np.asarray(nhit, float)*2.0**-53*host(mean_abs)*(1+1e-6), None]
def radial_bound(fn, vals, dev):
	"""radial_sum / radial_bin -> [nobj, ncomp, nbin] float32: 2 n 2^-24 times the entry point's result on |map|, n the pixels of the
	(object, bin) ring (its sums of a map of ones, exact in float32)"""
	pos = t_(vals["pos"], dev)
	n = host(pointsrcs.radial_sum(dm(t_(np.ones((NY, NX)), dev)), pos, BINS))      # [nobj, nbin]
	with np.errstate(invalid="ignore"): return [2*n[:, None, :]*2.0**-24*host(fn(dm(t_(np.abs(vals["m"]), dev)), pos, BINS))*(1+1e-6)]

def within(got, ref, bounds):
	"""|got - ref| <= bound elementwise (NaN where the reference is NaN: an empty bin); None: bitwise"""
	got, ref = flat(got), flat(ref)
	ok = len(got) == len(ref) == len(bounds)
	for g, r, b in zip(got, ref, bounds):
		if b is None: ok = ok and same(g, r); continue
		if not (g.shape == r.shape == b.shape and g.dtype == r.dtype): return False
		nan = np.isnan(r)
		ok = ok and np.array_equal(np.isnan(g), nan) and bool(np.all(np.abs(g.astype(np.float64)-r)[~nan] <= b[~nan]))
	return ok

def values_of(args):
	return {k: (wave_values() if v is None else v) for k, v in args.items()}

def check_row(dev, name, args, call, vary, bound=None):
	args = values_of(args)
	exact = bound is None or dev is ident      # (the simulator runs one thread after the other: bitwise everywhere, and within the bound too)
	def agree(got, ref, vals):
		if bound is not None and not within(got, ref, bound(vals, dev)): return False
		return same(got, ref) if exact else True
	def run(form, which, vals):
		ts = {}; base = None
		for k, v in vals.items():
			t, b = as_form(form if k == which else "contiguous", v, dev)
			ts[k] = t
			if k == which: base = b
		before = bits(base)
		res = call(ts)
		res = flat(res)      # (brought to the host before the storage is read back)
		assert bits(base) == before, "%s: the storage of %r (%s) changed" % (name, which, form)
		return res
	for which, may_expand in vary:
		ref = run("contiguous", which, args)
		for form in ("permuted", "sliced"):
			got = run(form, which, args)
			assert agree(got, ref, args), "%s with %r %s differs from the contiguous run: %s" % (name, which, form, worst(got, ref))
		if may_expand:
			v = args[which]
			rep = dict(args); rep[which] = np.ascontiguousarray(np.broadcast_to(v[:1], v.shape))
			ref = run("contiguous", which, rep)
			got = run("expanded", which, rep)
			assert agree(got, ref, rep), "%s with %r expanded differs from the contiguous run: %s" % (name, which, worst(got, ref))

def worst(got, ref):
	"""for the failure message: the largest difference relative to the largest reference value, per result array"""
	out = []
	for g, r in zip(flat(got), flat(ref)):
		if g.shape != r.shape: out.append("shape %s against %s" % (g.shape, r.shape)); continue
		with np.errstate(all="ignore"): out.append("%.3g" % (np.nanmax(np.abs(g.astype(np.complex128)-r.astype(np.complex128)))/max(np.nanmax(np.abs(r)), 1e-300)) if g.size else "empty")
	return ", ".join(out)

@pytest.mark.hostsim
@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_inputs_hostsim(row): check_row(ident, *row)
@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_inputs_gpu(row): check_row(cuda, *row)

# ---- output rows ---------------------------------------------------------------------------------------------------------------------
# (name, shape and dtype of the output, call(out tensor, dev) -> (returned object, reference result), "through" | "refuse").  The output
# starts as NaN so that a cell not written shows; rows that accumulate zero it themselves.
def t_(v, dev): return dev(torch.from_numpy(np.ascontiguousarray(v).copy()))
def o_alm2map(out, dev): return curvedsky.alm2map(t_(ALM, dev), dm(out)), curvedsky.alm2map(t_(ALM, dev), new_map(out))
def o_map2alm(out, dev): return curvedsky.map2alm(dm(t_(MAP, dev)), alm=out), curvedsky.map2alm(dm(t_(MAP, dev)), lmax=LMAX)
def o_almxfl(out, dev): return curvedsky.almxfl(t_(ALM, dev), LFILTER, out=out), curvedsky.almxfl(t_(ALM, dev), LFILTER)
def o_lmul_self(out, dev):
	out.copy_(t_(ALM, dev))
	return AINFO.lmul(out, LFILTER, out=out), AINFO.lmul(t_(ALM, dev), LFILTER)
def o_rotate_inplace(out, dev):
	out.copy_(t_(ALM, dev))
	return curvedsky.rotate_alm(out, 0.3, 0.7, -0.4, inplace=True), curvedsky.rotate_alm(t_(ALM, dev), 0.3, 0.7, -0.4)
def o_fft(out, dev): return enmap.fft(dm(t_(MAP, dev)), omap=dm(out)), enmap.fft(dm(t_(MAP, dev)))
def o_bank_merge(out, dev):
	alms = [t_(a, dev) for a in BANK_ALMS]
	return AINFO.bank_merge(alms, BANK_FILTERS, BANK_LMAXS, BANK_LS, out=out), AINFO.bank_merge(alms, BANK_FILTERS, BANK_LMAXS, BANK_LS)
def o_sim_objects(out, dev):
	return pointsrcs.sim_objects(SHAPE, WCS, t_(POS, dev), t_(AMPS, dev), PROFILE, omap=dm(out), vmin=1e-3), None
def o_distance_omap(out, dev): return distances.distance_from_points(SHAPE, WCS, points=t_(POS, dev), omap=dm(out)), None
def o_distance_odomains(out, dev): return distances.distance_from_points(SHAPE, WCS, points=t_(POS, dev), odomains=dm(out), domains=True), None
def o_interpol(out, dev): return interpol.interpol(t_(MAP, dev), t_(PIXPOS, dev), out=out), None
def o_wave2map(out, dev): return wavelet_transform().wave2map(wave_of(t_(wave_values(), dev)), omap=dm(out)), wavelet_transform().wave2map(wave_of(t_(wave_values(), dev)))

C128, F64, F32, I32 = torch.complex128, torch.float64, torch.float32, torch.int32
OUT_ROWS = [
	("curvedsky.alm2map(map=)", (NC, NY, NX), F64, o_alm2map, "refuse"),      # "output tensors must be contiguous"
	("curvedsky.map2alm(alm=)", (NC, NELEM), C128, o_map2alm, "refuse"),
	("curvedsky.almxfl(out=)", (NC, NELEM), C128, o_almxfl, "through"),
	("alm_info.lmul(out=self)", (NC, NELEM), C128, o_lmul_self, "through"),
	("curvedsky.rotate_alm(inplace=True)", (NC, NELEM), C128, o_rotate_inplace, "through"),
	("enmap.fft(omap=)", (NC, NY, NX), C128, o_fft, "through"),
	("alm_info.bank_merge(out=)", (NC, NELEM), C128, o_bank_merge, "through"),
	("pointsrcs.sim_objects(omap=)", (NC, NY, NX), F32, o_sim_objects, "refuse"),      # A.out_array: "omap must be C-contiguous"
	("distances.distance_from_points(omap=)", (NY, NX), F64, o_distance_omap, "refuse"),
	("distances.distance_from_points(odomains=)", (NY, NX), I32, o_distance_odomains, "refuse"),
	("interpol.interpol(out=)", (NC, NPT), F64, o_interpol, "refuse"),
	("wavelets.wave2map(omap=)", (NC, NY, NX), F64, o_wave2map, "refuse"),
]

def out_forms(shape, dtype, dev):
	"""(form, view, base): views of `shape` over storage filled with NaN (-1 for integers)"""
	fillv = -1 if dtype == I32 else complex(np.nan, np.nan) if dtype == C128 else np.nan
	nd = len(shape); rev = tuple(range(nd))[::-1]
	base = dev(torch.full(tuple(shape[k] for k in rev), fillv, dtype=dtype)); yield "permuted", base.permute(*rev), base
	base = dev(torch.full(tuple(2*n+1 for n in shape), fillv, dtype=dtype)); yield "sliced", base[tuple(slice(1, 2*n, 2) for n in shape)], base

def check_out_row(dev, name, shape, dtype, call, expect):
	for form, view, base in out_forms(shape, dtype, dev):
		assert not view.is_contiguous()
		before = bits(base)
		try: ret, ref = call(view, dev)
		except ValueError as e:
			assert expect == "refuse", "%s refused a %s output: %s" % (name, form, e)
			assert bits(base) == before, "%s refused a %s output after writing to it" % (name, form)
			continue
		assert expect == "through", "%s took a %s output that it used to refuse: pin the new behaviour" % (name, form)
		rt = ret.tensor if isinstance(ret, (enmap.dmap, multimap.dmaps)) else ret
		assert rt is view or (rt.data_ptr() == view.data_ptr() and tuple(rt.stride()) == tuple(view.stride()) and tuple(rt.shape) == tuple(view.shape)), "%s: the returned object is not the %s output" % (name, form)
		assert same(view, ref), "%s: the %s output does not hold the result (%s)" % (name, form, worst(view, ref))
		# nothing outside the view was written
		mask = torch.zeros(tuple(base.shape), dtype=torch.bool)
		torch.as_strided(mask, tuple(view.shape), tuple(view.stride()), view.storage_offset()).fill_(True)
		rest = host(base)[~mask.numpy()]
		assert np.all(np.isnan(rest.real)) and (rest.dtype.kind != "c" or np.all(np.isnan(rest.imag))), "%s wrote outside its %s output" % (name, form)

@pytest.mark.hostsim
@pytest.mark.parametrize("name,shape,dtype,call,expect", OUT_ROWS, ids=[r[0] for r in OUT_ROWS])
def test_outputs_hostsim(name, shape, dtype, call, expect): check_out_row(ident, name, shape, dtype, call, expect)
@pytest.mark.gpu
@pytest.mark.parametrize("name,shape,dtype,call,expect", OUT_ROWS, ids=[r[0] for r in OUT_ROWS])
def test_outputs_gpu(name, shape, dtype, call, expect): check_out_row(cuda, name, shape, dtype, call, expect)

# ---- the helper that trusted its docstring ------------------------------------------------------------------------------------------------
def check_rotate_pairs_refuses(dev):
	"""enmap._rotate_pairs computes component addresses from the shape: a dense permuted map is refused, not rotated in the wrong places"""
	view, base = as_form("permuted", HARM, dev); before = bits(base)
	with pytest.raises(ValueError): enmap._rotate_pairs(dm(view), [0, 2], False, True)
	assert bits(base) == before
def check_expanded_gradient(dev):
	"""a stride-0 gradient (both components one array) is refused by pxm_deflect, which says so; nothing is computed from overlapping components"""
	from pixell_amd import _lib
	grad, base = as_form("expanded", np.broadcast_to(GRAD[:1], GRAD.shape), dev); before = bits(base)
	with pytest.raises(_lib.PxsError, match="overlap"): lensing.offset_by_grad(t_(POS3, dev), grad)
	assert bits(base) == before
@pytest.mark.hostsim
def test_expanded_gradient_is_refused_hostsim(): check_expanded_gradient(ident)
@pytest.mark.gpu
def test_expanded_gradient_is_refused_gpu(): check_expanded_gradient(cuda)

@pytest.mark.hostsim
def test_rotate_pairs_refuses_hostsim(): check_rotate_pairs_refuses(ident)
@pytest.mark.gpu
def test_rotate_pairs_refuses_gpu(): check_rotate_pairs_refuses(cuda)
