"""alm post-processing on the GPU: alm2cl, lmul (almxfl), l-dependent matrix products.

Host mirror of cython/cmisc.pyx:8-110 (alm2cl) and :159-274 (lmul / lmatmul) of the reference, as
reached through alm_info.alm2cl / alm_info.lmul (pixell/curvedsky.py:451-474).  Same argument
meaning, broadcasting and error behaviour; the arithmetic runs in include/pxsht.h pxa_alm2cl /
pxa_lmatmul.  numpy inputs are staged through device memory, torch CUDA tensors are used in place
and the result is then a CUDA tensor.  No CPU fallback.
"""
import ctypes
import numpy as np
from . import _lib, _arrays as A
from ._arrays import device_index, current_stream
from .sht import _Buf

def _flat2(x):
	"""[..., n] -> contiguous [npre, n] (view when possible)"""
	n = x.shape[-1]
	if A.is_tensor(x): return x.contiguous().reshape(-1, n)
	return np.ascontiguousarray(x).reshape(-1, n)

def _mstart_buf(ainfo):
	return _Buf(np.ascontiguousarray(ainfo.mstart[:ainfo.mmax+1], dtype=np.uint64))

def alm2cl(ainfo, alm, alm2=None, cl_dtype=None):
	"""cmisc.alm2cl (cython/cmisc.pyx:8-110): cross spectrum of alm and alm2 (which broadcast); the
	result has the broadcast leading shape + (lmax+1,).  Each distinct pair of rows is computed once."""
	if not A.is_tensor(alm): alm = np.asarray(alm)
	same = alm2 is None or alm2 is alm
	if same: alm2 = alm
	elif not A.is_tensor(alm2): alm2 = np.asarray(alm2)
	if A.is_tensor(alm) != A.is_tensor(alm2): raise ValueError("alm and alm2 must both be numpy arrays or both torch tensors")
	ctype = np.result_type(A.np_dtype(alm), A.np_dtype(alm2))
	if ctype not in (np.dtype(np.complex64), np.dtype(np.complex128)):
		raise ValueError("alm2cl requires complex64 or complex128 arrays")
	rtype = np.dtype(np.float32) if ctype == np.dtype(np.complex64) else np.dtype(np.float64)
	cl_dtype = rtype if cl_dtype is None else np.dtype(cl_dtype)
	if cl_dtype not in (np.dtype(np.float32), np.dtype(np.float64)): raise ValueError("cl dtype must be float32 or float64")
	if ctype == np.dtype(np.complex128) and cl_dtype == np.dtype(np.float32):
		raise ValueError("float32 spectra of double precision alm are not supported")   # cmisc.pyx:84
	alm = A.astype(alm, ctype); alm2 = alm if same else A.astype(alm2, ctype)
	if alm.shape[-1] < ainfo.nelem or alm2.shape[-1] < ainfo.nelem: raise ValueError("alm too short for this alm_info")
	pshape = np.broadcast_shapes(tuple(alm.shape[:-1]), tuple(alm2.shape[:-1]))
	# row index of each broadcast element in the flattened inputs
	i1 = np.broadcast_to(np.arange(int(np.prod(alm.shape[:-1], dtype=int))).reshape(alm.shape[:-1]), pshape).reshape(-1)
	i2 = np.broadcast_to(np.arange(int(np.prod(alm2.shape[:-1], dtype=int))).reshape(alm2.shape[:-1]), pshape).reshape(-1)
	f1 = _flat2(alm); f2 = f1 if same else _flat2(alm2)
	b1 = _Buf(f1); b2 = b1 if same else _Buf(f2)
	npre = len(i1); nl = ainfo.lmax+1
	cl = A.empty((npre, nl), cl_dtype, like=alm)
	bc = _Buf(cl, writeback=True)
	if bc.tmp is not None and not _lib.is_hostsim(): bc.tmp = A.empty((npre, nl), cl_dtype); bc.ptr = bc.tmp.data_ptr()
	ms = _mstart_buf(ainfo)
	lib = _lib.load(); dev = device_index(); st = current_stream()
	csz = ctype.itemsize; rsz = cl_dtype.itemsize; n1 = f1.shape[-1]; n2 = f2.shape[-1]
	done = {}
	copies = []
	for i in range(npre):
		key = (int(i1[i]), int(i2[i])) if not same else tuple(sorted((int(i1[i]), int(i2[i]))))
		if key in done: copies.append((i, done[key])); continue
		done[key] = i
		_lib.check(lib.pxa_alm2cl(ainfo.lmax, ainfo.mmax, ms.ptr, ainfo.stride, b1.ptr + int(i1[i])*n1*csz, b2.ptr + int(i2[i])*n2*csz,
			A.DT[ctype], bc.ptr + i*nl*rsz, A.DT[cl_dtype], dev, st))
	tgt = bc.tmp if bc.tmp is not None else cl
	for i, j in copies: tgt[i] = tgt[j]
	bc.finish()
	return cl.reshape(tuple(pshape)+(nl,))

def lmul(ainfo, alm, lfun, out=None):
	"""cmisc.lmul (cython/cmisc.pyx:159-197): res[...,lm] = lfun[...,l] alm[...,lm] with broadcasting of the
	leading axes, or, for lfun[a,b,l] with alm[b,lm], the matrix product res[a,lm] = sum_b lfun[a,b,l] alm[b,lm].
	lfun shorter than lmax+1 counts as zero beyond its end."""
	tens = A.is_tensor(alm)
	if not tens: alm = np.asarray(alm)
	ctype = np.result_type(A.np_dtype(alm), np.complex64)
	if ctype not in (np.dtype(np.complex64), np.dtype(np.complex128)): raise ValueError("lmul requires complex64 or complex128 arrays")
	alm = A.astype(alm, ctype)
	if alm.shape[-1] < ainfo.nelem: raise ValueError("alm too short for this alm_info")
	# the filter is small: keep it on the host in f64 and upload once per call
	lfun = np.asarray(A.host(lfun), dtype=np.float64)
	if ctype == np.dtype(np.complex64): lfun = lfun.astype(np.float32).astype(np.float64)   # the reference casts the filter to the alm's real type
	if out is not None and (A.np_dtype(out) != ctype or A.is_tensor(out) != tens):
		raise ValueError("lmul's out argument must be contiguous along last axis, and have the same dtype as alm")
	lib = _lib.load(); dev = device_index(); st = current_stream(); ms = _mstart_buf(ainfo)
	nalm = alm.shape[-1]; csz = ctype.itemsize
	if lfun.ndim == 3 and alm.ndim == 2:
		N, M, nl = lfun.shape
		if M != alm.shape[0]: raise ValueError("lmul: matrix shape %s does not match alm shape %s" % (str(lfun.shape), str(alm.shape)))
		if M > 8: raise ValueError("lmul: at most 8 input components")
		if out is None: out = A.empty((N, nalm), ctype, like=alm); _zero(out)
		bi = _Buf(_flat2(alm)); bo = _Buf(out, writeback=True); bl = _Buf(np.ascontiguousarray(lfun))
		_lib.check(lib.pxa_lmatmul(N, M, ainfo.lmax, ainfo.mmax, ms.ptr, ainfo.stride, bi.ptr, nalm, bo.ptr, nalm, A.DT[ctype], bl.ptr, nl, dev, st))
		bo.finish()
		return out
	try:
		pre = np.broadcast_shapes(tuple(alm.shape[:-1]), lfun.shape[:-1])
	except ValueError:
		raise ValueError("lmul's alm and lfun's dimensions must either broadcast (when ignoring the last dimension), or have shape compatible with a matrix product (again ignoring the last dimension)")
	npre = int(np.prod(pre, dtype=int)); nl = lfun.shape[-1]
	ia = np.broadcast_to(np.arange(int(np.prod(alm.shape[:-1], dtype=int))).reshape(alm.shape[:-1]), pre).reshape(-1)
	il = np.broadcast_to(np.arange(int(np.prod(lfun.shape[:-1], dtype=int))).reshape(lfun.shape[:-1]), pre).reshape(-1)
	fa = _flat2(alm); fl = np.ascontiguousarray(lfun).reshape(-1, nl)
	if out is not None and tuple(out.shape) != tuple(pre)+(nalm,): raise ValueError("lmul: out has the wrong shape")
	bl = _Buf(fl)
	# work[npre, nalm] starts as the (broadcast) input rows and is scaled in place, like the reference's
	# `out[:] = aflat` followed by lmul_dp on each row
	if _lib.is_hostsim():
		work = np.ascontiguousarray(A.host(fa)[ia]); ptr = work.ctypes.data
	else:
		torch = A.torch()
		dev_in = fa if tens else A.to_gpu(fa if fa.flags.writeable else fa.copy())
		work = dev_in[torch.as_tensor(np.array(ia), device=dev_in.device)]          # gather = fresh contiguous copy (np.array: broadcast index views are read-only)
		ptr = work.data_ptr()
	for i in range(npre):
		row = ptr + i*nalm*csz
		_lib.check(lib.pxa_lmatmul(1, 1, ainfo.lmax, ainfo.mmax, ms.ptr, ainfo.stride, row, nalm, row, nalm, A.DT[ctype], bl.ptr + int(il[i])*nl*8, nl, dev, st))
	shape = tuple(pre)+(nalm,)
	if tens:
		if _lib.is_hostsim(): work = A.torch().as_tensor(work)
		if out is None: return work.reshape(shape)
		out.copy_(work.reshape(shape)); return out
	work = A.host(work)
	if out is None: return work.reshape(shape)
	out[...] = work.reshape(shape); return out

def _zero(x):
	if A.is_tensor(x): x.zero_()
	else: x[...] = 0

def rotate_alm(alm, lmax, psi, theta, phi, inplace=False):
	"""Euler-angle (zyz) rotation of alm[..., nelem] in the triangular layout (mmax = lmax), every leading component in one
	launch sequence of include/pxsht.h pxa_rotate_alm (FP64 arithmetic for complex64 and complex128 alike).  numpy alm are staged
	through the device and the result is numpy; torch CUDA tensors are used where they are, on the current stream.  inplace: the
	result is written into `alm`, which is returned; otherwise `alm` is left as it is and a new array is returned."""
	tens = A.is_tensor(alm)
	if not tens: alm = np.asarray(alm)
	ctype = A.np_dtype(alm)
	if ctype not in (np.dtype(np.complex64), np.dtype(np.complex128)): raise ValueError("rotate_alm requires complex64 or complex128 alm")
	lmax = int(lmax)
	nelem = (lmax+1)*(lmax+2)//2
	if lmax < 0 or alm.ndim < 1 or alm.shape[-1] != nelem:
		raise ValueError("rotate_alm: alm of %d elements is not the triangular layout of lmax %d (%d elements)" % (alm.shape[-1] if alm.ndim else 0, lmax, nelem))
	shape = tuple(alm.shape); npre = int(np.prod(shape[:-1], dtype=int))
	psi, theta, phi = float(psi), float(theta), float(phi)
	if npre == 0: return alm if inplace else (alm.clone() if tens else alm.copy())
	lib = _lib.load(); dtc = A.DT[ctype]
	def run(src_ptr, dst_ptr, dev, st):
		_lib.check(lib.pxa_rotate_alm(lmax, npre, src_ptr, nelem, dst_ptr, nelem, dtc, psi, theta, phi, dev, st))
	if _lib.is_hostsim():
		# (host pointers: the simulator runs the kernels on the CPU)
		if tens:
			src = alm.contiguous(); dst = src if inplace else A.torch().empty_like(src)
			run(src.data_ptr(), dst.data_ptr(), 0, None)
			if inplace and dst is not alm: alm.copy_(dst); return alm
			return dst
		work = alm if (inplace and alm.flags.c_contiguous and alm.dtype.isnative) else np.array(alm, dtype=ctype, order="C")
		run(work.ctypes.data, work.ctypes.data, 0, None)
		if inplace and work is not alm: alm[...] = work; return alm
		return work
	torch = A.torch()
	if tens:
		A.require_gpu(alm)
		with torch.cuda.device(alm.device):
			st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
			src = alm.contiguous()
			dst = src if inplace else torch.empty_like(src, memory_format=torch.contiguous_format)
			run(src.data_ptr(), dst.data_ptr(), alm.device.index, st)
		if inplace and dst is not alm: alm.copy_(dst); return alm
		return dst
	dev = device_index(); st = current_stream()
	work = A.to_gpu(np.array(alm, dtype=ctype, order="C"))
	run(work.data_ptr(), work.data_ptr(), dev, st)
	res = A.host(work).reshape(shape)
	if inplace: alm[...] = res; return alm
	return res

# ---------------------------------------------------------------------------------------
# the alm filter bank (include/pxsht.h pxa_bank_split / pxa_bank_merge; csrc/bank.hip)
# ---------------------------------------------------------------------------------------
def tri_nelem(L): return (int(L)+1)*(int(L)+2)//2

def _filter_table(filters, lmaxs, nl, ctype):
	"""f64[nscale, nl]: row i is filters[i] up to lmaxs[i] (zero beyond, or where filters[i] is shorter); rounded to float for complex64 alm"""
	tab = np.zeros((len(lmaxs), nl))
	for i, f in enumerate(filters):
		f = np.asarray(A.host(f), dtype=np.float64).reshape(-1)
		n = min(len(f), int(lmaxs[i])+1, nl)
		tab[i, :n] = f[:n]
	if ctype == np.dtype(np.complex64): tab = tab.astype(np.float32).astype(np.float64)
	return tab

def _bank_tables(lmaxs, Ls, ptrs, pitches):
	n = len(lmaxs)
	return ((ctypes.c_int*n)(*[int(v) for v in lmaxs]), (ctypes.c_int*n)(*[int(v) for v in Ls]),
		(ctypes.c_void_p*n)(*[int(p) for p in ptrs]), (ctypes.c_int64*n)(*[int(v) for v in pitches]))

def _to_kind(x, tens):
	"""the result as the caller's kind: tensors stay, device copies of numpy inputs come back"""
	return x if tens else A.host(x)

def bank_split_groups(ainfo, alm, table, lmaxs, groups):
	"""pxa_bank_split with the outputs laid out for batched transforms.  alm: [pre..., >= ainfo.nelem] device array (tensor; numpy in
	the simulator), complex; table: f64[nscale, nl] (numpy); groups: [(L, [scale indices])].  Returns one uninitialised-then-filled array
	[len(indices), pre..., tri_nelem(L)] per group: scale `indices[k]` is row k, band-limited to lmaxs[...] and zero up to L."""
	ctype = A.np_dtype(alm); pre = tuple(alm.shape[:-1]); npre = int(np.prod(pre, dtype=int))
	if alm.shape[-1] < ainfo.nelem: raise ValueError("alm too short for this alm_info")
	flat = _flat2(alm); csz = ctype.itemsize
	outs = [A.empty((len(idx),)+pre+(tri_nelem(L),), ctype, like=flat) for L, idx in groups]
	if npre == 0: return outs
	order = [(i, L, A.ptr(o)+k*npre*tri_nelem(L)*csz) for (L, idx), o in zip(groups, outs) for k, i in enumerate(idx)]
	tabs = _bank_tables([lmaxs[i] for i, L, p in order], [L for i, L, p in order], [p for i, L, p in order], [tri_nelem(L) for i, L, p in order])
	bt = _Buf(np.ascontiguousarray(table[[i for i, L, p in order]])); ms = _mstart_buf(ainfo)
	_lib.check(_lib.load().pxa_bank_split(len(order), *tabs, npre, ainfo.lmax, ainfo.mmax, ms.ptr, ainfo.stride, A.ptr(flat), flat.shape[-1], A.DT[ctype],
		bt.ptr, table.shape[-1], device_index(), current_stream()))
	return outs

def bank_merge_groups(ainfo, arrays, table, lmaxs, groups, out, accumulate=False):
	"""pxa_bank_merge, the transpose: arrays[g] is [len(indices), pre..., tri_nelem(L)] for groups[g] = (L, indices) (contiguous device arrays);
	out [pre..., ainfo.nelem] (contiguous, same kind) receives sum_i table[i] * scale i, added to its content if `accumulate`"""
	ctype = A.np_dtype(out); pre = tuple(out.shape[:-1]); npre = int(np.prod(pre, dtype=int))
	if out.shape[-1] < ainfo.nelem: raise ValueError("out too short for this alm_info")
	if npre == 0: return out
	csz = ctype.itemsize
	order = [(i, L, A.ptr(a)+k*npre*tri_nelem(L)*csz) for (L, idx), a in zip(groups, arrays) for k, i in enumerate(idx)]
	order.sort(key=lambda t: t[0])                  # summed in ascending scale index
	tabs = _bank_tables([lmaxs[i] for i, L, p in order], [L for i, L, p in order], [p for i, L, p in order], [tri_nelem(L) for i, L, p in order])
	bt = _Buf(np.ascontiguousarray(table[[i for i, L, p in order]])); ms = _mstart_buf(ainfo)
	_lib.check(_lib.load().pxa_bank_merge(len(order), *tabs, npre, ainfo.lmax, ainfo.mmax, ms.ptr, ainfo.stride, A.ptr(out), out.shape[-1], A.DT[ctype],
		bt.ptr, table.shape[-1], int(bool(accumulate)), device_index(), current_stream()))
	return out

def _bank_args(ainfo, filters, lmaxs, Ls, ctype):
	lmaxs = [int(v) for v in lmaxs]
	Ls = list(lmaxs) if Ls is None else [int(v) for v in Ls]
	if len(filters) != len(lmaxs) or len(Ls) != len(lmaxs): raise ValueError("filters, lmaxs and Ls must have one entry per scale")
	if any(l < 0 or l > ainfo.lmax or L < l for l, L in zip(lmaxs, Ls)): raise ValueError("every scale needs 0 <= lmax_i <= min(ainfo.lmax, L_i)")
	groups = [(L, [i for i, v in enumerate(Ls) if v == L]) for L in sorted(set(Ls))]
	return lmaxs, Ls, groups, _filter_table(filters, lmaxs, ainfo.lmax+1, ctype)

def bank_split(ainfo, alm, filters, lmaxs, Ls=None):
	"""The filter bank of a wavelet analysis in one kernel launch: for every scale i a copy of alm[..., nelem] (layout ainfo) multiplied by
	filters[i][l], truncated to lmaxs[i] and stored in the triangular layout of band limit Ls[i] >= lmaxs[i] (default lmaxs[i]; the rows
	lmaxs[i] < l <= Ls[i] are zero).  What transfer_alm + alm_info.lmul give scale by scale, without their index arrays and with the input
	read once.  Returns a list of arrays [..., tri_nelem(Ls[i])]; scales that share L are views of one allocation.  numpy alm are staged
	through the device, torch CUDA tensors are used in place on the current stream and the results are tensors."""
	tens = A.is_tensor(alm)
	if not tens: alm = np.asarray(alm)
	ctype = np.result_type(A.np_dtype(alm), np.complex64)
	if ctype not in (np.dtype(np.complex64), np.dtype(np.complex128)): raise ValueError("bank_split requires complex64 or complex128 arrays")
	lmaxs, Ls, groups, table = _bank_args(ainfo, filters, lmaxs, Ls, ctype)
	outs = bank_split_groups(ainfo, A.put(alm, ctype), table, lmaxs, groups)
	res = [None]*len(lmaxs)
	for (L, idx), o in zip(groups, outs):
		o = _to_kind(o, tens)
		for k, i in enumerate(idx): res[i] = o[k]
	return res

def bank_merge(ainfo, alms, filters, lmaxs, Ls=None, out=None, accumulate=False):
	"""The transpose of bank_split: out[..., lm] = (out[..., lm] if accumulate) + sum_i filters[i][l] alms[i][..., lm] over the scales with
	l <= lmaxs[i], in one launch and in ascending i (bitwise repeatable).  alms[i]: [..., tri_nelem(Ls[i])]; out: [..., ainfo.nelem] in the
	layout ainfo (allocated if None).  numpy arrays are staged, torch CUDA tensors used in place."""
	if len(alms) == 0: raise ValueError("bank_merge needs at least one scale")
	tens = A.is_tensor(alms[0])
	if any(A.is_tensor(a) != tens for a in alms) or (out is not None and A.is_tensor(out) != tens): raise ValueError("alms and out must all be numpy arrays or all torch tensors")
	if not tens: alms = [np.asarray(a) for a in alms]
	ctype = np.result_type(np.complex64, *[A.np_dtype(a) for a in alms])
	if ctype not in (np.dtype(np.complex64), np.dtype(np.complex128)): raise ValueError("bank_merge requires complex64 or complex128 arrays")
	lmaxs, Ls, _, table = _bank_args(ainfo, filters, lmaxs, Ls, ctype)
	pre = tuple(alms[0].shape[:-1])
	for a, L in zip(alms, Ls):
		if tuple(a.shape) != pre+(tri_nelem(L),): raise ValueError("bank_merge: scale arrays must be [pre..., (L_i+1)(L_i+2)/2] with common pre-dimensions")
	if out is None:
		if accumulate: raise ValueError("bank_merge: accumulate needs out")
		out = A.empty(pre+(ainfo.nelem,), ctype, like=alms[0]); _zero(out)       # (elements outside the layout, e.g. of a strided one, are defined too)
	elif A.np_dtype(out) != ctype or tuple(out.shape[:-1]) != pre: raise ValueError("bank_merge: out must have the alms' dtype and pre-dimensions")
	direct = (tens and out.is_contiguous()) or (not tens and _lib.is_hostsim() and out.flags.c_contiguous)
	work = out if direct else A.put(out, ctype)
	arrays = [A.put(a, ctype)[None] for a in alms]             # every scale a group of its own: [1, pre..., nelem]
	bank_merge_groups(ainfo, arrays, table, lmaxs, [(L, [i]) for i, L in enumerate(Ls)], work, accumulate=accumulate)
	if work is not out:
		if tens: out.copy_(work)
		else: out[...] = _to_kind(work, False)
	return out
