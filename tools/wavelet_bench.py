"""Time the wavelet transform and its filter bank on the GPU.  Device-resident scalar map on the full-sky Fejer-1 grid (--ny rows, 2 ny
columns), UHT(mode="curved", lmax=--lmax), default basis; device events, warm-up first, the two variants of the bank alternating in one run.
  bank:       almops.bank_split_groups + bank_merge_groups (one launch each) against the per-scale composition they replace
              (curvedsky.transfer_alm + alm_info.lmul, both directions), on the transform's own scales.  Bytes from shapes:
              16 (N + sum_i N_i) each way for complex128 (N_i: the triangular layout of the scale's group band limit), against the
              HBM peak (8.0 TB/s spec, 6.29 TB/s measured for a float4 copy).
  transform:  first and second call of map2wave + wave2map (plans built / reused), steady-state times, SHT calls and plans.
    python tools/wavelet_bench.py [--ny 21600] [--lmax 10000] [--reps 3] [--out profiles/wavelet_bench.json]"""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path: sys.path.insert(0, ROOT)
HBM_SPEC_TBS, HBM_COPY_TBS = 8.0, 6.29

def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--ny", type=int, default=21600)
	ap.add_argument("--lmax", type=int, default=10000)
	ap.add_argument("--reps", type=int, default=3)
	ap.add_argument("--out", default=None)
	a = ap.parse_args()
	import torch
	assert torch.cuda.is_available(), "wavelet_bench needs a GPU"
	from pixell_amd import enmap, uharm, wavelets, curvedsky, almops, sht, _lib
	assert not _lib.is_hostsim()
	def timed(fn, reps):
		e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
		torch.cuda.synchronize(); t0 = time.perf_counter(); e0.record()
		for _ in range(reps): fn()
		e1.record(); torch.cuda.synchronize()
		return e0.elapsed_time(e1)/reps, (time.perf_counter()-t0)*1e3/reps
	shape, wcs = enmap.fullsky_geometry(shape=(a.ny, 2*a.ny))
	uht = uharm.UHT(shape, wcs, mode="curved", lmax=a.lmax)
	wt = wavelets.WaveletTransform(uht)
	res = dict(tool="tools/wavelet_bench.py", device=torch.cuda.get_device_name(0), shape=list(shape), lmax=wt.basis.lmax, lmaxs=[int(v) for v in wt.basis.lmaxs],
		geometries=[list(s) for s, w in wt.geometries], reps=a.reps)
	print(json.dumps(res), flush=True)
	# ---- the bank alone, on a random alm
	ainfo = wt.ainfo; N = ainfo.nelem; lmaxs = [int(v) for v in wt.basis.lmaxs]
	g = torch.Generator(device="cuda").manual_seed(1)
	alm = torch.randn((1, N), dtype=torch.complex128, device="cuda", generator=g)
	groups = [(L, idx) for L, idx, geo in wt._groups(range(wt.nlevel))]
	table = almops._filter_table([wt.filters[i]/wt.norms[i] for i in range(wt.nlevel)], lmaxs, ainfo.lmax+1, np.dtype(np.complex128))
	out = torch.empty_like(alm)
	state = {}
	def fused():
		state["s"] = almops.bank_split_groups(ainfo, alm, table, lmaxs, groups)
		almops.bank_merge_groups(ainfo, state["s"], table, lmaxs, groups, out)
	def split_only(): state["s"] = almops.bank_split_groups(ainfo, alm, table, lmaxs, groups)
	def merge_only(): almops.bank_merge_groups(ainfo, state["s"], table, lmaxs, groups, out)
	def composed():
		oalm = torch.zeros_like(alm)
		for i, li in enumerate(lmaxs):
			small = curvedsky.alm_info(lmax=li)
			s = curvedsky.transfer_alm(ainfo, alm, small)
			small.lmul(s, table[i, :li+1], s)
			small.lmul(s, table[i, :li+1], s)
			curvedsky.transfer_alm(small, s, ainfo, oalm, op=lambda x, y: x+y)
		state["c"] = oalm
	fused(); composed()                                   # warm-up: code objects, memory pool
	rows = []
	for rep in range(a.reps):                             # alternating
		f = timed(fused, 1); c = timed(composed, 1)
		rows.append(dict(rep=rep, fused_ms=round(f[0], 3), fused_host_ms=round(f[1], 3), composed_ms=round(c[0], 3), composed_host_ms=round(c[1], 3)))
		print(json.dumps(rows[-1]), flush=True)
	sp = timed(split_only, a.reps)[0]; me = timed(merge_only, a.reps)[0]
	nbytes = 16*(N+sum(len(idx)*almops.tri_nelem(L) for L, idx in groups))
	res["bank"] = dict(rows=rows, split_ms=round(sp, 3), merge_ms=round(me, 3), bytes_each_way=nbytes, split_TBs=round(nbytes/sp/1e9, 3), merge_TBs=round(nbytes/me/1e9, 3),
		hbm_spec_TBs=HBM_SPEC_TBS, hbm_copy_TBs=HBM_COPY_TBS, agree=float((out-state["c"]).abs().max()/state["c"].abs().max()))
	print(json.dumps(res["bank"]), flush=True)
	del alm, out, state; torch.cuda.empty_cache()
	# ---- the transform
	made, calls = [], []
	Base = sht.Plan
	class Counted(Base):
		def __init__(self, h): made.append(1); Base.__init__(self, h)
	sht.Plan = Counted
	for name in ("alm2map", "map2alm"):
		def wrap(orig):
			def fn(*args, **kw): calls.append(1); return orig(*args, **kw)
			return fn
		setattr(curvedsky, name, wrap(getattr(curvedsky, name)))
	m = enmap.dmap(torch.randn(shape, dtype=torch.float64, device="cuda", generator=g), wcs)
	st = {}
	def both(): st["w"] = wt.map2wave(m); st["b"] = wt.wave2map(st["w"])
	first = timed(both, 1); plans_first, calls_first = len(made), len(calls)
	second = timed(both, 1); plans_second = len(made)-plans_first
	fwd = timed(lambda: st.__setitem__("w", wt.map2wave(m)), a.reps); bwd = timed(lambda: st.__setitem__("b", wt.wave2map(st["w"])), a.reps)
	res["transform"] = dict(first_call_ms=round(first[1], 1), second_call_ms=round(second[1], 1), plans_first_call=plans_first, plans_second_call=plans_second,
		sht_calls_per_pair=calls_first, map2wave_ms=round(fwd[0], 2), wave2map_ms=round(bwd[0], 2), plans_owned=len(wt.pin))
	print(json.dumps(res["transform"]), flush=True)
	if a.out:
		with open(a.out, "w") as fh: json.dump(res, fh, indent=1)

if __name__ == "__main__":
	main()
