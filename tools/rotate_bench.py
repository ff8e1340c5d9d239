"""Time curvedsky.rotate_alm on the GPU: complex128 alm resident on the device (torch CUDA tensors, in place), lmax 2000 / 4000 / 10000,
ncomp 1 and 3.  Call time from device events around `--reps` back-to-back calls after one warm-up call.  The flop count is the algorithm's
(DESIGN.md section 8): two passes over every (row m, column k) pair of every l, (l+1)^2 of them, each a recurrence step (2 multiplies + 1
FMA = 4 flop) and one FMA per component (2 flop): (4 + 2 ncomp) flop, against 78.6 TFLOP/s of FP64 (vector) peak.
    python tools/rotate_bench.py [--lmax 2000 4000 10000] [--ncomp 1 3] [--reps 3] [--out profiles/rotate_bench.json]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path: sys.path.insert(0, ROOT)
FP64_PEAK_TFLOPS = 78.6

def flops(lmax, ncomp):
	s = sum((l + 1)**2 for l in range(lmax + 1))
	return 2*s*(4 + 2*ncomp)

def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--lmax", type=int, nargs="+", default=[2000, 4000, 10000])
	ap.add_argument("--ncomp", type=int, nargs="+", default=[1, 3])
	ap.add_argument("--reps", type=int, default=3)
	ap.add_argument("--out", default=None)
	a = ap.parse_args()
	import torch
	assert torch.cuda.is_available(), "rotate_bench needs a GPU"
	from pixell_amd import curvedsky, _lib
	assert not _lib.is_hostsim()
	rows = []
	for lmax in a.lmax:
		for nc in a.ncomp:
			n = (lmax + 1)*(lmax + 2)//2
			g = torch.Generator(device="cuda").manual_seed(1)
			alm = torch.randn((nc, n), dtype=torch.complex128, device="cuda", generator=g)
			alm[:, :lmax + 1] = alm[:, :lmax + 1].real.to(torch.complex128)
			ang = curvedsky.euler_angs[("gal", "equ")]
			curvedsky.rotate_alm(alm, *ang, inplace=True)          # warm-up (code objects, memory pool)
			torch.cuda.synchronize()
			e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
			t0 = time.perf_counter(); e0.record()
			for _ in range(a.reps): curvedsky.rotate_alm(alm, *ang, inplace=True)
			e1.record(); torch.cuda.synchronize(); wall = (time.perf_counter() - t0)/a.reps
			ms = e0.elapsed_time(e1)/a.reps
			f = flops(lmax, nc)
			row = dict(lmax=lmax, ncomp=nc, dtype="complex128", ms_per_call=round(ms, 3), host_wall_ms_per_call=round(wall*1e3, 3),
				flop=f, tflops=round(f/(ms*1e-3)/1e12, 2), frac_fp64_peak=round(f/(ms*1e-3)/1e12/FP64_PEAK_TFLOPS, 4))
			print(json.dumps(row), flush=True)
			rows.append(row)
			del alm; torch.cuda.empty_cache()
	if a.out:
		with open(a.out, "w") as fh:
			json.dump(dict(tool="tools/rotate_bench.py", reps=a.reps, device=torch.cuda.get_device_name(0), fp64_peak_tflops=FP64_PEAK_TFLOPS,
				flop_model="2 passes x sum_l (l+1)^2 x (4 + 2 ncomp)", rows=rows), fh, indent=1)

if __name__ == "__main__":
	main()
