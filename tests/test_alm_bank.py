"""almops.bank_split / bank_merge (include/pxsht.h pxa_bank_split / pxa_bank_merge, csrc/bank.hip) against the per-scale composition they
replace: curvedsky.transfer_alm + alm_info.lmul, in the same dtype.

split is one multiply per element, so it must agree with the composition bit for bit (np.array_equal; a zero may differ in sign), and the
rows lmax_i < l <= L_i must be exactly zero.  merge adds nscale products per element: the composition rounds every product and every
sum, the kernel may contract them into fmas; both stay within nscale u sum_i |f_i a_i| of the exact sum (u = eps/2, to first order), so
they differ by at most nscale eps sum_i |f_i a_i| -- with prior contents (accumulate) that is one more term.  Shapes: lmax 0 and 1 (degenerate rows),
37 (not a multiple of anything), 300 (more than one 256-lane block per row, pairs across block boundaries for complex64); scales with
lmax_i = 0, lmax_i = lmax, L_i > lmax_i and two scales sharing one L; layouts with mmax < lmax and with stride 2 (rectangular);
complex64 meets odd and even row starts in every triangular layout."""
import numpy as np
import pytest
from pixell_amd import almops, curvedsky

def scales_of(lmax):
	"""(lmax_i, L_i): lmax_i = 0; lmax_i = lmax; two scales that share an L above their own band limits"""
	Lc = lmax//2+3
	return [0, lmax, lmax//3, lmax//2], [0, lmax, Lc, Lc]

def layout(kind, lmax):
	if kind == "tri": return curvedsky.alm_info(lmax=lmax)
	if kind == "mmax": return curvedsky.alm_info(lmax=lmax, mmax=lmax//2)
	if kind == "rect2": return curvedsky.alm_info(lmax=lmax, stride=2, layout="rect")
	raise ValueError(kind)

def rand_c(rng, shape, dtype):
	return (rng.standard_normal(shape)+1j*rng.standard_normal(shape)).astype(dtype)

def filters_of(rng, lmaxs, lmax):
	return [rng.standard_normal(lmax+1)+0.1 for _ in lmaxs]

def inside(L, lmax_i):
	"""mask over the triangular layout of L: True where l <= lmax_i"""
	info = curvedsky.alm_info(lmax=L)
	mask = np.zeros(info.nelem, bool)
	for m in range(min(lmax_i, L)+1): mask[info.lm2ind(np.arange(m, lmax_i+1), m)] = True
	return mask

def split_reference(ainfo, alm, filters, lmaxs):
	res = []
	for f, li in zip(filters, lmaxs):
		small = curvedsky.alm_info(lmax=li)
		a = curvedsky.transfer_alm(ainfo, alm, small)
		res.append(np.asarray(small.lmul(a, f[:li+1])))
	return res

def check_split(lmax, kind, npre, dtype, seed=0, scales=None):
	"""scales: (lmaxs, Ls) in place of scales_of(lmax); entries 2 and 3 must share an L"""
	rng = np.random.default_rng(seed)
	ainfo = layout(kind, lmax); lmaxs, Ls = scales_of(lmax) if scales is None else scales
	alm = rand_c(rng, (npre, ainfo.nelem) if npre > 1 else (ainfo.nelem,), dtype)
	filters = filters_of(rng, lmaxs, lmax)
	got = ainfo.bank_split(alm, filters, lmaxs, Ls)
	want = split_reference(ainfo, alm, filters, lmaxs)
	assert len(got) == len(lmaxs)
	assert got[2].base is not None and got[2].base is got[3].base       # the scales that share L are views of one allocation
	for g, w, li, L in zip(got, want, lmaxs, Ls):
		assert g.dtype == dtype and g.shape == alm.shape[:-1]+(almops.tri_nelem(L),)
		mask = inside(L, li)
		back = curvedsky.transfer_alm(curvedsky.alm_info(lmax=L), g, curvedsky.alm_info(lmax=li))
		assert np.array_equal(back, w)
		assert np.all(g[..., ~mask] == 0)
		assert np.all(np.isfinite(g.view(g.real.dtype)))

def merge_reference(ainfo, alms, filters, lmaxs, Ls, prior, absolute=False):
	out = prior.copy()
	for a, f, li, L in zip(alms, filters, lmaxs, Ls):
		small = curvedsky.alm_info(lmax=li)
		s = curvedsky.transfer_alm(curvedsky.alm_info(lmax=L), a, small)
		if absolute: s = (np.abs(s)*np.abs(f[small_l(small)])).astype(a.dtype)
		else: s = np.asarray(small.lmul(s, f[:li+1]))
		curvedsky.transfer_alm(small, s, ainfo, out, op=np.add)
	return out

def small_l(info):
	l = np.zeros(info.nelem, int)
	for m in range(info.mmax+1): l[info.lm2ind(np.arange(m, info.lmax+1), m)] = np.arange(m, info.lmax+1)
	return l

def check_merge(lmax, kind, npre, dtype, seed=1, scales=None):
	rng = np.random.default_rng(seed)
	ainfo = layout(kind, lmax); lmaxs, Ls = scales_of(lmax) if scales is None else scales
	pre = (npre,) if npre > 1 else ()
	alms = [rand_c(rng, pre+(almops.tri_nelem(L),), dtype) for L in Ls]
	filters = filters_of(rng, lmaxs, lmax)
	eps = np.finfo(dtype).eps; n = len(lmaxs)
	zero = np.zeros(pre+(ainfo.nelem,), dtype)
	got = ainfo.bank_merge(alms, filters, lmaxs, Ls)
	assert got.dtype == dtype and got.shape == zero.shape
	want = merge_reference(ainfo, alms, filters, lmaxs, Ls, zero)
	mag = merge_reference(ainfo, alms, filters, lmaxs, Ls, zero, absolute=True).real
	err = np.abs(got.astype(np.complex128)-want.astype(np.complex128))
	assert np.all(err <= n*eps*mag), (np.max(err), np.max(mag))
	assert np.array_equal(ainfo.bank_merge(alms, filters, lmaxs, Ls), got)          # bitwise repeatable
	# accumulate: onto prior contents, which count as one more term of the sum
	prior = rand_c(rng, zero.shape, dtype)
	out = prior.copy()
	res = ainfo.bank_merge(alms, filters, lmaxs, Ls, out=out, accumulate=True)
	assert res is out
	want = merge_reference(ainfo, alms, filters, lmaxs, Ls, prior)
	err = np.abs(out.astype(np.complex128)-want.astype(np.complex128))
	assert np.all(err <= (n+1)*eps*(mag+np.abs(prior))), (np.max(err), np.max(mag))
	# overwrite: prior contents of the layout's elements do not survive
	out2 = prior.copy(); ainfo.bank_merge(alms, filters, lmaxs, Ls, out=out2)
	sel = np.zeros(ainfo.nelem, bool)
	for m in range(ainfo.mmax+1): sel[ainfo.lm2ind(np.arange(m, lmax+1), m)] = True
	assert np.array_equal(out2[..., sel], got[..., sel])

CASES = [(lmax, kind, npre) for lmax in (0, 1, 37) for kind in ("tri", "mmax", "rect2") for npre in (1, 3) if not (kind == "mmax" and lmax == 0)]
CASES += [(300, "tri", 1), (300, "tri", 3), (300, "mmax", 1)]
DTYPES = [np.complex128, np.complex64]

def run_all(fn):
	for lmax, kind, npre in CASES:
		for dtype in DTYPES: fn(lmax, kind, npre, dtype)

@pytest.mark.hostsim
def test_bank_split_hostsim(): run_all(check_split)
@pytest.mark.hostsim
def test_bank_merge_hostsim(): run_all(check_merge)
@pytest.mark.gpu
def test_bank_split_gpu(): run_all(check_split)
@pytest.mark.gpu
def test_bank_merge_gpu(): run_all(check_merge)

def test_bank_argument_errors():
	ainfo = curvedsky.alm_info(lmax=4)
	alm = np.zeros(ainfo.nelem, np.complex128)
	with pytest.raises(ValueError): almops.bank_split(ainfo, alm, [np.ones(5)], [5])             # lmax_i beyond the input's
	with pytest.raises(ValueError): almops.bank_split(ainfo, alm, [np.ones(5)], [3], Ls=[2])     # L_i below lmax_i
	with pytest.raises(ValueError): almops.bank_merge(ainfo, [np.zeros(3, np.complex128)], [np.ones(5)], [3])     # not the layout of L_i

@pytest.mark.gpu
def test_bank_tensors_on_a_side_stream_gpu():
	"""device tensors, issued on a side stream: the same bits as numpy inputs staged on the default stream"""
	import torch
	rng = np.random.default_rng(2)
	lmax = 300; ainfo = curvedsky.alm_info(lmax=lmax); lmaxs, Ls = scales_of(lmax)
	filters = filters_of(rng, lmaxs, lmax)
	for dtype in DTYPES:
		alm = rand_c(rng, (3, ainfo.nelem), dtype)
		want = ainfo.bank_split(alm, filters, lmaxs, Ls)
		wmerge = ainfo.bank_merge(want, filters, lmaxs, Ls)
		torch.cuda.synchronize()
		s = torch.cuda.Stream()
		talm = torch.from_numpy(alm).cuda()
		torch.cuda.synchronize()
		with torch.cuda.stream(s):
			got = ainfo.bank_split(talm, filters, lmaxs, Ls)
			gmerge = ainfo.bank_merge(got, filters, lmaxs, Ls)
		s.synchronize()
		assert all(isinstance(g, torch.Tensor) and g.is_cuda for g in got) and gmerge.is_cuda
		for g, w in zip(got, want): assert np.array_equal(g.cpu().numpy(), w)
		assert np.array_equal(gmerge.cpu().numpy(), wmerge)
