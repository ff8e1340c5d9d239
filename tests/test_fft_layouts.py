"""The N-d FFT engine (pixell_amd.fft -> pxf_fft_nd) on tensors that are NOT C-contiguous: permuted, sliced, offset, expanded and
negative-stride views, in place and out of place, every dtype pair.  pixell_amd/fft.py promises that "tensors are used with their own
strides"; every other test hands the library contiguous tensors (numpy views are staged contiguously before the library sees them), so
the stride planner -- fft_axis in csrc/api_fft.hip, launch_pass and FftContext::exec in csrc/fft.hip -- is otherwise only ever walked
on a handful of its combinations.

Every case
  * compares with numpy.fft (scipy.fft.dctn / dstn for the r2r kinds) in long double on the values read back from the input view, on
    max|got - ref| / max|ref| at the bounds of test_fft_fuzz.py: 2e-13 when input and output are double precision, 2e-5 otherwise;
  * asserts that the cells of the output's storage outside the output view are still NaN (the storage is made of NaN) and
  * that the whole storage of the input is bitwise what it was, unless the transform is in place.
plan_model() restates in Python what fft_axis does with the shape and the strides (drop singletons, merge, tile dim, o1 / o2, host
loop) and what launch_pass / exec derive from them (load_inner_fast, store_inner_fast, tile_i; LDS, four-step or Bluestein).  Every
named case asserts from the model that its layout reaches the branch it is named for, so a layout that stops reaching it fails.

  branch                                    named case
  merge of the line dims / no merge         1a / 1b
  tile dim is not the last line dim,
  load_inner_fast != store_inner_fast       2
  >= 2 host-loop dims                       3 (one axis and three)
  four-step, tile_i = 1, n_o1, n_o2 > 1     4a; tile_i = 1 on a transposed matrix 4b
  Bluestein with strided lines              5 (c2c, r2c, c2r through the dtype pairs)
  multi-axis c2r through the scratch pass   6
  r2r, all eight kinds                      7
  in place: c2c, FFTW-padded r2c and c2r    8
  dtype pairs, different layouts            9 (and every case from 1 to 5)
  stride-0 input                            10
  negative strides (C ABI)                  11
  both chunk branches of exec (o1_per,
  i_per) under a layout                     12
  enmap.fft / ifft / dct on interleaved
  maps, below and at the dense route        13
A seeded fuzz over make_view follows.  The simulator runs one thread per workgroup and shows index logic only; the GPU twins check
the kernels themselves (a read / write hazard between the load and the store phase of one in-place call shows only there).

Worst double-precision relative error per test, MI355X (simulator in brackets), against the bound of 2e-13: cases 1a 2.3e-16, 1b 2.3e-16,
2 1.7e-16, 3 2.0e-16 / 2.7e-16, 4a 2.6e-16, 4b 2.8e-16, 5 5.5e-16 (6.2e-16), 6 3.5e-16, 7 3.6e-16, 8 2.9e-16 / 3.0e-16, 9 2.6e-16, 10 1.6e-16,
11 1.5e-16, 12 2.5e-16, 13 6.3e-16, fuzz 9.2e-16 over 300 transforms (5.8e-16 over 60); single precision 7.3e-8 at worst against 2e-5.
Every test prints its own figure.  The whole file takes 11 s on the GPU (the fuzz 6 s) and 10 s in the simulator."""
import os, re, ctypes, itertools
import numpy as np
import pytest
import torch
import scipy.fft as sfft
from pixell_amd import fft as pfft, enmap, sht, _lib
from pixell_amd import _arrays as A

TOL64, TOL32 = 2e-13, 2e-5      # test_fft_fuzz.py
NAN = float("nan")
F32, F64, C64, C128 = np.dtype(np.float32), np.dtype(np.float64), np.dtype(np.complex64), np.dtype(np.complex128)
# (in, out) of case 9; the kind follows from them as in pixell_amd.fft: real -> complex is r2c, complex -> real c2r
PAIRS = [(C128, C128), (F32, C128), (C64, C128), (C128, C64), (F64, C64), (C128, F32), (C64, F64)]
R2R = ["DCT-I", "DCT-II", "DCT-III", "DCT-IV", "DST-I", "DST-II", "DST-III", "DST-IV"]
R2R_KIND = {k: 3+i for i, k in enumerate(R2R)}

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pixell_amd", "csrc")
def kconst(fname, name):
	with open(os.path.join(CSRC, fname)) as f: m = re.search(r"\bconstexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, f.read())
	assert m, "%s: no constant %s" % (fname, name)
	return int(m.group(1))
NLOC = kconst("fft_dev.hpp", "FFT_NLOC_MAX")      # longest line of one LDS pass

def ident(t): return t
def cuda(t): return t.cuda()
def tdt(dt): return getattr(torch, np.dtype(dt).name)
def host(t): return np.array(t.detach().cpu().numpy())      # (a copy: a host tensor's numpy() shares its memory)
def is_double(dt): return np.dtype(dt) in (F64, C128)
def cplx(dt): return np.dtype(dt).kind == "c"

# ---- views over NaN storage -----------------------------------------------------------------------------------------------------
def nan_tensor(shape, dtype):
	t = torch.empty(tuple(int(n) for n in shape), dtype=tdt(dtype))
	t.fill_(complex(NAN, NAN) if cplx(dtype) else NAN)      # (torch.full(..., nan) of a complex dtype leaves the imaginary part 0)
	return t

def make_view(rng, shape, dtype, dev, perm=None, steps=None, offs=None, tails=None, max_storage=None):
	"""(view, base): base a fresh C-contiguous tensor of NaN, view of `shape` over an axis permutation of it (storage dim k holds axis
	perm[k]) with step steps[a], offs[a] cells before and tails[a] cells after the view along axis a; what is None is drawn from rng:
	a random permutation, steps of 1 to 3, 0 to 2 cells.  max_storage: steps are lowered until the storage has at most that many cells."""
	nd = len(shape)
	perm = [int(p) for p in (rng.permutation(nd) if perm is None else perm)]
	steps = [int(s) for s in (rng.integers(1, 4, nd) if steps is None else steps)]
	offs = [int(s) for s in (rng.integers(0, 3, nd) if offs is None else offs)]
	tails = [int(s) for s in (rng.integers(0, 3, nd) if tails is None else tails)]
	ext = lambda: [offs[a]+(shape[a]-1)*steps[a]+1+tails[a] for a in range(nd)]
	while max_storage is not None and np.prod(ext(), dtype=np.int64) > max_storage:
		big = [a for a in range(nd) if steps[a] > 1]
		if big: steps[max(big, key=lambda a: ext()[a])] -= 1
		else:
			a = max(range(nd), key=lambda a: offs[a]+tails[a]); assert offs[a]+tails[a] > 0, (shape, max_storage)
			offs[a] = tails[a] = 0
	e = ext()
	base = dev(nan_tensor([e[a] for a in perm], dtype))
	v = base.permute(*[perm.index(a) for a in range(nd)])
	v = v[tuple(slice(offs[a], offs[a]+(shape[a]-1)*steps[a]+1, steps[a]) for a in range(nd))]
	assert tuple(v.shape) == tuple(shape)
	return v, base

CONTIG = dict(steps=0, offs=0, tails=0)      # (marks a C-contiguous layout in the case tables)
def view_of(rng, shape, dtype, dev, layout, max_storage=None):
	"""make_view under a layout of a case table: keys perm / steps / offs / tails; a scalar stands for every axis; "rev": reversed storage order"""
	nd = len(shape)
	if layout is CONTIG: return make_view(rng, shape, dtype, dev, perm=range(nd), steps=[1]*nd, offs=[0]*nd, tails=[0]*nd)
	kw = {}
	for k, v in layout.items(): kw[k] = (None if v is None else list(range(nd))[::-1] if isinstance(v, str) and v == "rev" else [v]*nd if np.isscalar(v) else list(v))
	return make_view(rng, shape, dtype, dev, max_storage=max_storage, **kw)

def fill(view, values): view.copy_(torch.from_numpy(np.ascontiguousarray(values)).to(view.device))
def rvals(rng, shape, dtype):
	x = rng.standard_normal(shape)
	if cplx(dtype): x = x+1j*rng.standard_normal(shape)
	return x.astype(dtype)
def bits(base): return host(torch.view_as_real(base) if base.is_complex() else base).tobytes()

def untouched_is_nan(base, *views):
	"""the cells of base's storage outside the views are NaN (both parts of a complex cell).  The mask of the cells a view covers is
	made with as_strided on a bool tensor of base's shape; where a real view lies in complex storage (or the reverse: the in-place
	r2c / c2r) everything is counted in real cells."""
	if base.is_complex() and any(not v.is_complex() for v in views): base = torch.view_as_real(base)
	assert base.is_contiguous()
	mask = torch.zeros(tuple(base.shape), dtype=torch.bool)
	for v in views:
		if v.is_complex() and not base.is_complex(): v = torch.view_as_real(v)
		assert v.is_complex() == base.is_complex()
		torch.as_strided(mask, tuple(v.shape), tuple(v.stride()), v.storage_offset()-base.storage_offset()).fill_(True)
	rest = host(base)[~mask.numpy()]
	return bool(np.all(np.isnan(rest.real)) and (rest.dtype.kind != "c" or np.all(np.isnan(rest.imag))))

# ---- the reference ------------------------------------------------------------------------------------------------------------------
def reference(kind, x, axes, oshape):
	"""long double numpy.fft / scipy.fft of the host values x; unnormalised in both directions, as pixell_amd.fft"""
	nd = x.ndim; ax = tuple(a % nd for a in axes)
	x = x.astype(np.clongdouble if x.dtype.kind == "c" else np.longdouble)
	if kind == "fft": return np.fft.fftn(x, axes=ax)
	if kind == "ifft": return np.fft.ifftn(x, axes=ax)*np.prod([x.shape[a] for a in ax])
	if kind == "rfft": return np.fft.rfftn(x, axes=ax)
	if kind == "irfft":
		s = [oshape[a] for a in ax]
		return np.fft.irfftn(x, s=s, axes=ax)*np.prod(s)
	t = 1+R2R.index(kind) % 4
	return (sfft.dctn if kind.startswith("DCT") else sfft.dstn)(x, type=t, axes=ax)

def transform(kind, x, out, axes):
	if kind == "fft": return pfft.fft(x, out, axes=axes)
	if kind == "ifft": return pfft.ifft(x, out, axes=axes)
	if kind == "rfft": return pfft.rfft(x, out, axes=axes)
	if kind == "irfft": return pfft.irfft(x, out, n=out.shape[axes[-1]], axes=axes)
	return pfft.dct(x, out, axes=axes, type=kind)

class Worst:
	"""the worst double-precision relative error of one test, printed at its end as test_fft_fuzz does"""
	def __init__(self, name): self.name, self.d64, self.d32, self.n = name, 0.0, 0.0, 0
	def add(self, d, dbl):
		self.n += 1
		if dbl: self.d64 = max(self.d64, d)
		else: self.d32 = max(self.d32, d)
	def report(self): print("\n[fft layouts] %s: %d transforms, worst relative error %.2e (double precision), %.2e (single)" % (self.name, self.n, self.d64, self.d32))

def check(what, kind, x, xbase, out, obase, axes, worst, inplace=False):
	"""one transform x -> out (views of xbase, obase) against the reference, with the two storage assertions"""
	xh = host(x); before = bits(xbase)
	idt, odt = A.np_dtype(x), A.np_dtype(out)
	got = transform(kind, x, out, list(axes))
	assert got is out, what
	oh = host(out)
	ref = reference(kind, xh, axes, tuple(out.shape))
	assert oh.shape == ref.shape, (what, oh.shape, ref.shape)
	d = float(np.max(np.abs(oh-ref))/max(float(np.max(np.abs(ref))), 1e-300))
	dbl = is_double(idt) and is_double(odt)
	assert d < (TOL64 if dbl else TOL32), ("against numpy.fft in long double", what, d)      # (NaN fails too)
	worst.add(d, dbl)
	assert untouched_is_nan(obase, out, *([x] if inplace else [])), ("cells outside the output view were written", what)
	if not inplace: assert bits(xbase) == before, ("the input's storage changed", what)
	return d

def kind_of(idt, odt, inverse=False):
	if cplx(odt): return ("ifft" if inverse else "fft") if cplx(idt) else "rfft"
	return "irfft"
def half(shape, axes):
	s = list(shape); a = axes[-1] % len(shape); s[a] = s[a]//2+1
	return tuple(s)

def hermitian(rng, shape, axes, dtype):
	"""a half spectrum of the real shape, consistent with a real signal"""
	return np.fft.rfftn(rng.standard_normal(shape), axes=tuple(a % len(shape) for a in axes)).astype(dtype)

def run_layout(rng, dev, what, shape, axes, lin, lout, idt, odt, worst, inverse=False, max_storage=None):
	"""the transform of the kind (idt, odt) imply, over `axes` of the (real-domain) `shape`, from a view of layout lin to one of layout lout"""
	kind = kind_of(idt, odt, inverse)
	ishape = half(shape, axes) if kind == "irfft" else tuple(shape)
	oshape = half(shape, axes) if kind == "rfft" else tuple(shape)
	x, xb = view_of(rng, ishape, idt, dev, lin, max_storage); out, ob = view_of(rng, oshape, odt, dev, lout, max_storage)
	fill(x, hermitian(rng, shape, axes, idt) if kind == "irfft" else rvals(rng, ishape, idt))
	what = (what, kind, tuple(shape), tuple(axes), idt.name, odt.name, tuple(x.stride()), tuple(out.stride()))
	check(what, kind, x, xb, out, ob, axes, worst)
	return x, out

# ---- the model of fft_axis / launch_pass ------------------------------------------------------------------------------------------
def lpf(n):
	big, q = 1, 2
	while q*q <= n:
		while n % q == 0: big = q; n //= q
		q += 1
	return max(big, n)
def split_two(n):
	"""split_two of fft.hip: n1*n2 = n, both <= FFT_NLOC_MAX"""
	best = best8 = -1
	for a in range(1, int(np.sqrt(n))+2):
		if a*a > n or n % a: continue
		b = n//a
		if b > NLOC: continue
		best = a
		if a % 8 == 0 and b % 8 == 0 and 4*a >= b: best8 = a
	if best < 0: return None
	if best8 > 0: best = best8
	return best, n//best
def supported(n): return n >= 1 and (n <= NLOC or split_two(n) is not None)      # (the cap on the number of factors is not reached below 2048)
def good_size(n):
	m = max(n, 1)
	while True:
		r = m
		for p in (2, 3, 5):
			while r % p == 0: r //= p
		if r == 1 and supported(m): return m
		m += 1

def axis_model(n, dims, is_e, os_e, plain=True):
	"""fft_axis for one n-point pass over the line dims [(n, is, os)] (strides in elements), then what launch_pass / exec derive"""
	if not supported(n) or (plain and lpf(n) > 128):
		M = good_size(2*n-1); lines = 1; d1, d2 = list(dims), list(dims)
		for k in range(len(dims)-1, -1, -1):
			d1[k] = (dims[k][0], dims[k][1], lines*M); d2[k] = (dims[k][0], lines*M, dims[k][2]); lines *= dims[k][0]
		return dict(n=n, route="bluestein", M=M, sub=[axis_model(M, d1, is_e, 1, False), axis_model(M, d2, 1, os_e, False)])
	d = [list(x) for x in dims if x[0] > 1]
	before = len(d); k = 0
	while k+1 < len(d):
		if d[k][1] == d[k+1][1]*d[k+1][0] and d[k][2] == d[k+1][2]*d[k+1][0]: d[k+1][0] *= d[k][0]; del d[k]
		else: k += 1
	m = dict(n=n, route="lds" if n <= NLOC else "fourstep", line_dims=before, merged=before-len(d), tile_is_last=True,
		n_i=1, is_i=0, os_i=0, n_o1=1, n_o2=1, is_e=is_e, os_e=os_e)
	if d:
		best = 0
		for k in range(1, len(d)):
			if abs(d[k][1]) < abs(d[best][1]): best = k
		m.update(n_i=d[best][0], is_i=d[best][1], os_i=d[best][2], tile_is_last=best == len(d)-1); del d[best]
	if d: m["n_o1"] = d.pop()[0]
	if d: m["n_o2"] = d.pop()[0]
	m["host"] = [x[0] for x in d]
	adjacent = abs(m["is_i"]) < abs(is_e)
	if m["route"] == "lds": m.update(load_inner_fast=adjacent, store_inner_fast=abs(m["os_i"]) < abs(os_e), tile_i=0)
	else: m.update(load_inner_fast=None, store_inner_fast=None, tile_i=int(adjacent))      # (the four-step passes set their own)
	return m

def plan_model(kind, shape, ist, ost, axes):
	"""the axis passes of pxf_fft_nd (kind 0 c2c, 1 r2c, 2 c2r, 3..10 r2r) over the real-domain shape, each as axis_model sees it;
	"scratch": the pass writes the dense scratch of the multi-axis c2r"""
	nd = len(shape); axes = [a % nd for a in axes]; last = axes[-1]
	rshape = list(shape); cshape = list(shape)
	if kind in (1, 2): cshape[last] = shape[last]//2+1
	cs = [0]*nd; acc = 1
	for k in range(nd-1, -1, -1): cs[k] = acc; acc *= cshape[k]
	passes = []; sstride = list(ist)
	for t in range(len(axes)):
		pre = kind == 2 and t < len(axes)-1
		real_axis = kind >= 3 or (kind == 1 and t == 0) or (kind == 2 and not pre)
		ax = (axes[len(axes)-2-t] if pre else last) if kind == 2 else axes[len(axes)-1-t]
		shp = rshape if real_axis else cshape
		os_ = cs if pre else list(ost)
		n = shape[ax]
		if kind >= 3: n = 2*(n-1) if kind == 3 else 2*(n+1) if kind == 7 else 2*n
		m = axis_model(n, [(shp[k], sstride[k], os_[k]) for k in range(nd) if k != ax], sstride[ax], os_[ax], plain=kind < 3)
		m.update(axis=ax, scratch=pre); passes.append(m)
		sstride = os_
	return passes

def model_of(kind, x, out, axes):
	code = {"fft": 0, "ifft": 0, "rfft": 1, "irfft": 2}.get(kind, R2R_KIND.get(kind))
	shape = tuple(out.shape) if code == 2 else tuple(x.shape)
	return plan_model(code, shape, x.stride(), out.stride(), axes)

def test_model_constants():
	"""the constant is found, and the model's length rules are those of the library where the library can be asked"""
	assert NLOC > 0
	lib = _lib.load()
	for n in (1, 2, 30, 2048, 2049, 2053, 2400, 4096, 4106, 11200, 16384, 2*2053, 2048*2048, 2048*2049):
		assert bool(lib.pxf_fft_supported(n)) == supported(n), n
	for n in (1, 7, 2049, 4105, 16385): assert int(lib.pxf_fft_good_size(n)) == good_size(n), n

# ---- the named cases 1 to 5: (name, shape, axes, input layout, output layout, what the model must show) ----------------------------------
STEP2 = dict(perm=None, steps=2, offs=0, tails=0)
def c_order(nd, **kw): return dict(perm=list(range(nd)), offs=0, tails=0, **kw)

def expect_merge(ps):
	p, = ps; assert p["line_dims"] == 3 and p["merged"] == 2 and p["host"] == [] and p["n_i"] == 4*5*6 and p["n_o1"] == 1, p
def expect_no_merge(ps):
	p, = ps; assert p["line_dims"] == 3 and p["merged"] == 0 and (p["n_i"], p["n_o1"], p["n_o2"]) == (6, 5, 4), p
def expect_tile_dim(ps):
	p, = ps
	assert not p["tile_is_last"] and p["merged"] == 0 and p["n_i"] == 6 and p["n_o1"] == 5, p
	assert abs(p["is_e"]) == 1 and p["load_inner_fast"] is False and p["store_inner_fast"] is True, p      # the axis is the fastest in memory on input, the slowest on output
def expect_host_loop(ps):
	for p in ps: assert len(p["host"]) >= 2 and p["merged"] == 0 and p["n_o1"] > 1 and p["n_o2"] > 1, p
def expect_four_step_4d(ps):
	p, = ps; assert p["route"] == "fourstep" and p["tile_i"] == 1 and p["merged"] == 0 and (p["n_i"], p["n_o1"], p["n_o2"]) == (5, 4, 3), p
def expect_four_step_t(ps):
	p, = ps; assert p["route"] == "fourstep" and p["tile_i"] == 1 and p["n_i"] == 3 and abs(p["is_i"]) == 1, p
def expect_bluestein(ps):
	p, = ps
	assert p["route"] == "bluestein" and p["M"] >= 2*2053-1 and p["M"] > NLOC, p
	a, b = p["sub"]      # the two chirp transforms: strided lines into the dense scratch and out of it, both four-step at this length
	assert a["route"] == b["route"] == "fourstep" and a["merged"] == 0 and b["merged"] == 0 and a["n_i"] > 1 and a["n_o1"] > 1, p

LAY_4D = c_order(4, steps=[2, 1, 2, 2])      # [3, 2400, 4, 5]: C order, the three line dims in steps of 2 (none merges), the axis' lines adjacent
NAMED = [
	("1a merge", (4, 5, 6, 30), [-1], CONTIG, CONTIG, expect_merge),
	("1b no merge", (4, 5, 6, 30), [-1], CONTIG, c_order(4, steps=[1, 2, 1, 1]), expect_no_merge),
	("2 tile dim", (30, 6, 5), [0], dict(perm="rev", steps=1, offs=0, tails=0), CONTIG, expect_tile_dim),
	("3 host loop, one axis", (3, 2, 4, 3, 2, 27), [-1], c_order(6, steps=[2, 2, 2, 2, 2, 1]), c_order(6, steps=[2, 2, 2, 2, 2, 1]), expect_host_loop),
	("3 host loop, three axes", (3, 2, 4, 3, 2, 27), [1, 3, 5], c_order(6, steps=2), dict(perm=list(range(6)), steps=2, offs=1, tails=1), expect_host_loop),
	("4a four-step, lines adjacent", (3, 2400, 4, 5), [1], LAY_4D, LAY_4D, expect_four_step_4d),
	("4b four-step, transposed", (3, 4096), [-1], dict(perm="rev", steps=1, offs=0, tails=0), dict(perm="rev", steps=1, offs=1, tails=0), expect_four_step_t),
	("5 Bluestein, strided lines", (3, 2053, 4), [1], dict(perm=[2, 0, 1], steps=[2, 1, 1], offs=[0, 1, 0], tails=0), dict(perm=[1, 2, 0], steps=[1, 2, 2], offs=0, tails=[1, 0, 2]), expect_bluestein),
]

def run_named(dev, case):
	name, shape, axes, lin, lout, expect = case
	rng = np.random.default_rng(11); worst = Worst("case "+name)
	for idt, odt in PAIRS:
		x, out = run_layout(rng, dev, name, shape, axes, lin, lout, idt, odt, worst)
		if idt == odt == C128:
			ps = model_of("fft", x, out, axes); print("\n[fft layouts] case %s, model: %s" % (name, ps)); expect(ps)
			run_layout(rng, dev, name, shape, axes, lin, lout, idt, odt, worst, inverse=True)
		elif cplx(idt) and cplx(odt): expect(model_of("fft", x, out, axes))      # (the same layout in elements of another width)
		elif name.startswith("5"): assert model_of(kind_of(idt, odt), x, out, axes)[0]["route"] == "bluestein"      # r2c, c2r of the 2053-point axis
	worst.report()

@pytest.mark.hostsim
@pytest.mark.parametrize("case", NAMED, ids=[c[0] for c in NAMED])
def test_named_hostsim(case): run_named(ident, case)
@pytest.mark.gpu
@pytest.mark.parametrize("case", NAMED, ids=[c[0] for c in NAMED])
def test_named_gpu(case): run_named(cuda, case)

# ---- 6. multi-axis c2r through the scratch pass --------------------------------------------------------------------------------------
def run_c2r_scratch(dev):
	rng = np.random.default_rng(12); worst = Worst("case 6 multi-axis c2r")
	for n, axes, (idt, odt) in itertools.product((31, 30), ([0, 2], [1, 2]), ((C128, F64), (C128, F32), (C64, F64))):
		shape = (5, 12, n)
		for lin, lout in ((dict(perm=[1, 2, 0], steps=[1, 2, 1], offs=[1, 0, 2], tails=0), dict(perm=[2, 0, 1], steps=[2, 1, 3], offs=0, tails=[0, 1, 1])), (STEP2, CONTIG)):
			x, out = run_layout(rng, dev, "6", shape, axes, lin, lout, idt, odt, worst)
			ps = model_of("irfft", x, out, axes)
			assert len(ps) == 2 and ps[0]["scratch"] and ps[0]["axis"] == axes[0] and not ps[1]["scratch"] and ps[1]["axis"] == 2, ps
			assert ps[1]["is_e"] == 1 and ps[1]["n"] == n, ps      # the real axis is read out of the dense scratch
	worst.report()
@pytest.mark.hostsim
def test_c2r_scratch_hostsim(): run_c2r_scratch(ident)
@pytest.mark.gpu
def test_c2r_scratch_gpu(): run_c2r_scratch(cuda)

# ---- 7. r2r --------------------------------------------------------------------------------------------------------------------------
def run_r2r(dev):
	rng = np.random.default_rng(13); worst = Worst("case 7 r2r")
	shape = (3, 20, 27)
	lays = [(dict(perm=[2, 0, 1], steps=1, offs=0, tails=0), dict(perm=[1, 2, 0], steps=[1, 2, 1], offs=[0, 1, 0], tails=[2, 0, 0])),      # permuted
		(c_order(3, steps=[2, 1, 3]), dict(perm=[0, 1, 2], steps=[1, 3, 2], offs=[1, 2, 0], tails=[0, 1, 2]))]      # sliced
	for kind, axes, (lin, lout), dt in itertools.product(R2R, ([-2, -1], [0]), lays, (F64, F32)):
		x, xb = view_of(rng, shape, dt, dev, lin); out, ob = view_of(rng, shape, dt, dev, lout)
		fill(x, rvals(rng, shape, dt))
		check(("7", kind, axes, dt.name, tuple(x.stride()), tuple(out.stride())), kind, x, xb, out, ob, axes, worst)
		ps = model_of(kind, x, out, axes)
		assert [p["axis"] for p in ps] == [a % 3 for a in axes[::-1]] and all(p["route"] == "lds" and p["merged"] == 0 for p in ps), ps
	worst.report()
@pytest.mark.hostsim
def test_r2r_hostsim(): run_r2r(ident)
@pytest.mark.gpu
def test_r2r_gpu(): run_r2r(cuda)

# ---- 8. in place ---------------------------------------------------------------------------------------------------------------------
def run_inplace_c2c(dev):
	rng = np.random.default_rng(14); worst = Worst("case 8 in-place c2c")
	shape = (6, 12, 30)
	for lay, axes, dt, kind in itertools.product((dict(perm=[2, 0, 1], steps=1, offs=0, tails=0), c_order(3, steps=[2, 3, 2]), dict(perm=[1, 2, 0], steps=[2, 1, 2], offs=[1, 0, 2], tails=1)),
			([-1], [1], [0, 1, 2]), (C128, C64), ("fft", "ifft")):
		x, xb = view_of(rng, shape, dt, dev, lay)
		fill(x, rvals(rng, shape, dt))
		check(("8 c2c", kind, axes, dt.name, tuple(x.stride())), kind, x, xb, x, xb, axes, worst, inplace=True)
	worst.report()

def padded(rng, dev, shape, cdt):
	"""FFTW's in-place r2c layout: (c, r, base), c a complex tensor [..., nh] of NaN, r = the first n reals of each of its lines"""
	n = shape[-1]; nh = n//2+1
	c, base = make_view(rng, tuple(shape[:-1])+(nh,), cdt, dev, perm=range(len(shape)), steps=[1]*len(shape), offs=[1]+[0]*(len(shape)-1), tails=[1]+[0]*(len(shape)-1))
	r = torch.view_as_real(c).reshape(tuple(shape[:-1])+(2*nh,))[..., :n]
	assert r.data_ptr() == c.data_ptr() and r.stride(-1) == 1 and r.stride(-2) == 2*nh
	return c, r, base

def run_inplace_real(dev):
	"""pxf_fft_nd anticipates this use: its dense route excludes in == out for real input"""
	rng = np.random.default_rng(15); worst = Worst("case 8 in-place r2c / c2r")
	for shape, axes, cdt in itertools.product(((6, 30), (3, 7, 31), (2, 4096), (3, 5, 2400)), ([-1], [-2, -1]), (C128, C64)):
		rdt = F64 if cdt == C128 else F32
		c, r, base = padded(rng, dev, shape, cdt)
		fill(r, rvals(rng, shape, rdt))
		check(("8 r2c", shape, axes, cdt.name), "rfft", r, base, c, base, axes, worst, inplace=True)
		route = "fourstep" if shape[-1] > NLOC else "lds"
		assert model_of("rfft", r, c, axes)[0]["route"] == route
		c, r, base = padded(rng, dev, shape, cdt)
		fill(c, hermitian(rng, shape, axes, cdt))
		check(("8 c2r", shape, axes, cdt.name), "irfft", c, base, r, base, axes, worst, inplace=True)
		assert model_of("irfft", c, r, axes)[-1]["route"] == route
	worst.report()
@pytest.mark.hostsim
def test_inplace_c2c_hostsim(): run_inplace_c2c(ident)
@pytest.mark.gpu
def test_inplace_c2c_gpu(): run_inplace_c2c(cuda)
@pytest.mark.hostsim
def test_inplace_real_hostsim(): run_inplace_real(ident)
@pytest.mark.gpu
def test_inplace_real_gpu(): run_inplace_real(cuda)

# ---- 9. dtype pairs between two different random layouts ------------------------------------------------------------------------------
def run_pairs(dev):
	rng = np.random.default_rng(16); worst = Worst("case 9 dtype pairs")
	for (idt, odt), (shape, axes) in itertools.product(PAIRS, (((5, 12, 30), [-1]), ((5, 12, 30), [0, 2]), ((4, 7, 9, 13), [1, 2, 3]), ((3, 2304), [1]))):
		x, out = run_layout(rng, dev, "9", shape, axes, {}, {}, idt, odt, worst)      # ({}: everything drawn)
		assert tuple(x.stride()) != tuple(out.stride())
	worst.report()
@pytest.mark.hostsim
def test_dtype_pairs_hostsim(): run_pairs(ident)
@pytest.mark.gpu
def test_dtype_pairs_gpu(): run_pairs(cuda)

# ---- 10. stride-0 input -------------------------------------------------------------------------------------------------------------
def run_expanded(dev):
	rng = np.random.default_rng(17); worst = Worst("case 10 stride-0 input")
	for idt, odt in PAIRS[:5]:
		for axes in ([-1], [0], [0, 1]):
			xb = dev(torch.from_numpy(rvals(rng, (30,), idt))); x = xb.expand(5, 30)
			assert tuple(x.stride()) == (0, 1)
			oshape = half((5, 30), axes) if not cplx(idt) else (5, 30)
			out, ob = make_view(rng, oshape, odt, dev)
			check(("10", axes, idt.name, odt.name, tuple(out.stride())), kind_of(idt, odt), x, xb, out, ob, axes, worst)
			if axes == [0] and cplx(idt):
				p, = model_of("fft", x, out, axes); assert p["is_e"] == 0 and p["is_i"] == 1 and p["load_inner_fast"] is False, p      # the transform runs along the stride-0 axis
	worst.report()
@pytest.mark.hostsim
def test_expanded_input_hostsim(): run_expanded(ident)
@pytest.mark.gpu
def test_expanded_input_gpu(): run_expanded(cuda)

# ---- 11. negative strides through the C ABI -------------------------------------------------------------------------------------------
def run_negative(dev):
	rng = np.random.default_rng(18); worst = Worst("case 11 negative strides")
	R, n = 6, 40
	I64 = ctypes.c_int64
	for idt, odt in ((C128, C128), (C64, C128), (C128, C64)):
		xh = rvals(rng, (R, n), idt)
		x = dev(torch.from_numpy(xh)); before = bits(x)
		y = dev(nan_tensor((R+2, n), odt))      # a row of NaN on either side of the rows written
		isz, osz = idt.itemsize, odt.itemsize
		# input element (i, j) is x[R-1-i, n-1-j]; output element (i, k) goes to y[1+i, n-1-k]
		aptr = x.data_ptr()+((R-1)*n+n-1)*isz; bptr = y.data_ptr()+(n+n-1)*osz
		_lib.check(_lib.load().pxf_fft_nd(2, (I64*2)(R, n), (I64*2)(-n, -1), (I64*2)(n, -1), 1, (ctypes.c_int*1)(1), 0, 1, 1.0,
			A.DT[idt], A.DT[odt], aptr, bptr, A.device_index(), A.current_stream()))
		yh = host(y)
		ref = np.fft.fft(xh[::-1, ::-1].astype(np.clongdouble), axis=-1)[:, ::-1]      # the FFT of the flipped array, stored flipped along the axis
		d = float(np.max(np.abs(yh[1:-1]-ref))/np.max(np.abs(ref))); dbl = is_double(idt) and is_double(odt)
		assert d < (TOL64 if dbl else TOL32), (idt, odt, d)
		worst.add(d, dbl)
		assert np.all(np.isnan(yh[[0, -1]].real)) and np.all(np.isnan(yh[[0, -1]].imag)) and bits(x) == before
		p, = plan_model(0, (R, n), (-n, -1), (n, -1), [1])
		assert p["is_i"] == -n and p["is_e"] == -1 and p["load_inner_fast"] is False and p["merged"] == 0, p
	worst.report()
@pytest.mark.hostsim
def test_negative_strides_hostsim(): run_negative(ident)
@pytest.mark.gpu
def test_negative_strides_gpu(): run_negative(cuda)

# ---- 12. the chunk seams of the four-step engine under a layout ------------------------------------------------------------------------
def run_chunks(dev, monkeypatch):
	"""case 4a's layout with PXS_FFT_TEMP_MB set so that exec splits the lines in its o1_per branch (n_i <= lines_budget < n_i n_o1)
	and in its i_per branch (lines_budget < n_i); the split result is the whole one bit for bit, as in check_fft_passes of test_pass_seams.py"""
	rng = np.random.default_rng(19); worst = Worst("case 12 chunk seams")
	shape, axes = (3, 2400, 4, 5), [1]
	x, xb = view_of(rng, shape, C128, dev, LAY_4D); fill(x, rvals(rng, shape, C128))
	p, = model_of("fft", x, x, axes); expect_four_step_4d([p])
	n_i, n_o1, n_o2 = p["n_i"], p["n_o1"], p["n_o2"]
	def once():
		out, ob = view_of(rng, shape, C128, dev, LAY_4D)
		check(("12", os.environ.get("PXS_FFT_TEMP_MB")), "fft", x, xb, out, ob, axes, worst)
		return host(out), sht.fft_passes()
	whole, pw = once()
	assert (pw["n"], pw["first"], pw["last"]) == (n_o2, n_i*n_o1, n_i*n_o1), pw      # at the default budget: one pass per o2
	for branch, mb in (("o1_per", 0.6), ("i_per", 0.12)):
		budget = int(mb*(1 << 20)); lb = max(1, budget//(16*p["n"]))      # lines_budget of FftContext::exec
		if branch == "o1_per":
			assert n_i <= lb < n_i*n_o1, (lb, p)
			o1_per, i_per = min(n_o1, max(1, lb//n_i)), n_i
		else:
			assert lb < n_i, (lb, p)
			o1_per, i_per = 1, lb
		want = (n_o2*-(-n_o1//o1_per)*-(-n_i//i_per), o1_per*i_per, (n_o1-(-(-n_o1//o1_per)-1)*o1_per)*(n_i-(-(-n_i//i_per)-1)*i_per))
		assert want[0] > n_o2 and want[2] < want[1], want      # more passes than the whole run, and a smaller last one
		monkeypatch.setenv("PXS_FFT_TEMP_MB", repr(mb))
		try: split, ps = once()
		finally: monkeypatch.delenv("PXS_FFT_TEMP_MB")
		print("\n[fft layouts] case 12, %s branch at %g MB (%d lines): passes %s" % (branch, mb, lb, ps))
		assert ps["n"] > 1 and (ps["n"], ps["first"], ps["last"]) == want, (ps, want)
		assert np.array_equal(split, whole), branch
	worst.report()
@pytest.mark.hostsim
def test_chunk_seams_hostsim(monkeypatch): run_chunks(ident, monkeypatch)
@pytest.mark.gpu
def test_chunk_seams_gpu(monkeypatch): run_chunks(cuda, monkeypatch)

# ---- 13. enmap.fft / ifft / dct on pixel-interleaved maps --------------------------------------------------------------------------------
def run_enmap(dev):
	"""a [ny, nx, 3] tensor seen as [3, ny, nx], and its [1:] slice.  256 x 270 is above the 65 536 pixels of the dense route: the
	contiguous copy goes through the chain stages and the view through the generic engine, and each is compared with the reference"""
	rng = np.random.default_rng(20); worst = Worst("case 13 enmap")
	for ny, nx in ((24, 40), (256, 270)):
		_, wcs = enmap.fullsky_geometry(shape=(ny, nx))
		for dt in (F64, C128, F32):
			base = dev(torch.from_numpy(rvals(rng, (ny, nx, 3), dt)))
			for v in (base.permute(2, 0, 1), base.permute(2, 0, 1)[1:]):
				assert not v.is_contiguous()
				xh = host(v).astype(np.clongdouble if cplx(dt) else np.longdouble); before = bits(base)
				tol = TOL64 if is_double(dt) else TOL32
				refs = {"fft": np.fft.fftn(xh, axes=(-2, -1))/np.sqrt(ny*nx), "ifft": np.fft.ifftn(xh, axes=(-2, -1))*np.sqrt(ny*nx)}
				if not cplx(dt): refs["dct"] = sfft.dctn(xh, type=1, axes=(-2, -1))/np.sqrt((2*ny-1)*(2*nx-1))
				for name, ref in refs.items():
					if name == "ifft" and not cplx(dt): continue
					forms = [("view", v)]+([("contiguous", v.contiguous())] if ny*nx >= 65536 else [])
					for form, t in forms:
						got = getattr(enmap, name)(enmap.dmap(t, wcs))
						assert isinstance(got, enmap.dmap) and got.wcs is wcs
						d = float(np.max(np.abs(host(got.tensor)-ref))/np.max(np.abs(ref)))
						assert d < tol, ("enmap."+name, form, ny, nx, dt.name, tuple(v.shape), d)
						worst.add(d, is_double(dt))
				assert bits(base) == before
	worst.report()
@pytest.mark.hostsim
def test_enmap_interleaved_hostsim(): run_enmap(ident)
@pytest.mark.gpu
def test_enmap_interleaved_gpu(): run_enmap(cuda)

# ---- the fuzz --------------------------------------------------------------------------------------------------------------------------
LENGTHS = [1, 2, 3, 5, 7, 8, 12, 13, 16, 27, 30, 61, 64, 100, 131]
LONG = [2400, 11200, 16384, 2053]      # four-step (two of them above the 10240 points an LDS line holds) and Bluestein
MAX_ELEMS = 300000
def run_fuzz(dev, ncases, seed):
	rng = np.random.default_rng(seed); worst = Worst("fuzz")
	seen = {}
	for case in range(ncases):
		nd = int(rng.integers(1, 7)); nax = int(rng.integers(1, min(nd, 3)+1))
		axes = [int(a) for a in rng.permutation(nd)[:nax]]
		kind = str(rng.choice(["fft", "ifft", "rfft", "irfft", "inplace", "r2r"]))
		shape = [int(rng.choice(LENGTHS)) for _ in range(nd)]
		if kind != "r2r" and rng.random() < 0.3: shape[axes[int(rng.integers(0, nax))]] = int(rng.choice(LONG))      # (r2r stays at 1500 points or fewer)
		while np.prod(shape, dtype=np.int64) > MAX_ELEMS:
			k = max((k for k in range(nd) if shape[k] not in LONG), key=lambda k: shape[k]); shape[k] = max(1, shape[k]//2)
		dbl = rng.random() < 0.7
		rdt, cdt = (F64, C128) if dbl else (F32, C64)
		if rng.random() < 0.3: axes = [a-nd for a in axes]
		what = (case, kind, tuple(shape), tuple(axes), rdt.name)
		mk = lambda shp, dt: make_view(rng, tuple(shp), dt, dev, max_storage=8*MAX_ELEMS)
		if kind == "inplace":
			x, xb = mk(shape, cdt); fill(x, rvals(rng, shape, cdt))
			check(what, "fft" if rng.random() < 0.5 else "ifft", x, xb, x, xb, axes, worst, inplace=True)
			continue
		if kind == "r2r":
			kind = str(rng.choice(R2R))
			if kind == "DCT-I": shape = [max(n, 2) if k in [a % nd for a in axes] else n for k, n in enumerate(shape)]      # (DCT-I needs two points)
			idt = odt = rdt; ishape = oshape = tuple(shape)
		elif kind in ("fft", "ifft"): idt = odt = cdt; ishape = oshape = tuple(shape)
		elif kind == "rfft": idt, odt = rdt, cdt; ishape, oshape = tuple(shape), half(shape, axes)
		else: idt, odt = cdt, rdt; ishape, oshape = half(shape, axes), tuple(shape)
		x, xb = mk(ishape, idt); out, ob = mk(oshape, odt)
		fill(x, hermitian(rng, shape, axes, idt) if kind == "irfft" else rvals(rng, ishape, idt))
		check(what+(kind, tuple(x.stride()), tuple(out.stride())), kind, x, xb, out, ob, axes, worst)
		for p in model_of(kind, x, out, axes): seen[p["route"]] = seen.get(p["route"], 0)+1
	worst.report(); print("[fft layouts] fuzz: axis passes by route %s" % seen)
	assert all(seen.get(r, 0) > 0 for r in ("lds", "fourstep", "bluestein")), seen
	return worst

@pytest.mark.hostsim
def test_layout_fuzz_hostsim(): run_fuzz(ident, 60, 21)
@pytest.mark.gpu
def test_layout_fuzz_gpu(): run_fuzz(cuda, 300, 22)
