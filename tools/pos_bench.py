"""Time sht.synthesis_general / adjoint_synthesis_general (curvedsky.alm2map_pos) on the GPU, everything resident on the device (torch CUDA
tensors).  Cases: lmax 4000 T/Q/U (spin 0 + spin 2) f64 eps 1e-10 at 5400 x 10800 jittered pixel centres of an F1 band (a stand-in for the
positions of lens_map_curved), and lmax 2000 T/Q/U at 1e7 uniformly random points.  Device-event ms per call after one warm-up call:
the point plan alone (binning + sort), forward and adjoint on a made plan (T and QU share it, as in curvedsky.alm2map_pos), the same
with the plan made inside the call, and the floor: sht.synthesis_2d / adjoint_synthesis_2d onto the same CC grid.  The split per stage
(CC synthesis, 2-D FFTs, grid kernels, interpolation / spreading) comes from the plan's own stage timers (sht.points_profile: device
events around each stage, one timed call per direction).
    python tools/pos_bench.py [--cases lens rand] [--reps 2] [--out profiles/pos_bench.json]"""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path: sys.path.insert(0, ROOT)

def timed(fn, reps):
	import torch
	fn(); torch.cuda.synchronize()
	e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
	e0.record()
	for _ in range(reps): fn()
	e1.record(); torch.cuda.synchronize()
	return e0.elapsed_time(e1)/reps

def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--cases", nargs="+", default=["lens", "rand"])
	ap.add_argument("--reps", type=int, default=2)
	ap.add_argument("--out", default=None)
	a = ap.parse_args()
	import torch
	assert torch.cuda.is_available(), "pos_bench needs a GPU"
	from pixell_amd import sht, _lib
	assert not _lib.is_hostsim()
	rows = []
	g = torch.Generator(device="cuda").manual_seed(1)
	for case in a.cases:
		if case == "lens":
			lmax, ny, nx = 4000, 5400, 10800
			jit = 0.3*np.pi/10800
			th = ((torch.arange(ny, device="cuda", dtype=torch.float64) + 0.5 + 2700)*np.pi/10800)[:, None].expand(ny, nx)
			ph = ((torch.arange(nx, device="cuda", dtype=torch.float64) + 0.5)*2*np.pi/21600)[None, :].expand(ny, nx)
			th = (th + jit*torch.randn((ny, nx), generator=g, device="cuda", dtype=torch.float64)).clamp(0, np.pi)
			ph = ph + jit*torch.randn((ny, nx), generator=g, device="cuda", dtype=torch.float64)
			loc = torch.stack([th.reshape(-1), ph.reshape(-1)], 1).contiguous(); del th, ph
			desc = "5400 x 10800 jittered F1 band pixel centres (rows 2700-8099 of 10800)"
		else:
			lmax, n = 2000, 10**7
			u = torch.rand((n, 2), generator=g, device="cuda", dtype=torch.float64)
			loc = torch.stack([torch.arccos(1 - 2*u[:, 0]), 2*np.pi*u[:, 1]], 1).contiguous(); del u
			desc = "1e7 uniformly random points"
		npts = loc.shape[0]; nalm = (lmax + 1)*(lmax + 2)//2
		alm = torch.randn((3, nalm), generator=g, device="cuda", dtype=torch.complex128)
		alm[:, :lmax + 1] = alm[:, :lmax + 1].real.to(torch.complex128)
		mp = torch.zeros((3, npts), device="cuda", dtype=torch.float64)
		kw = dict(loc=loc, lmax=lmax, epsilon=1e-10)
		def fwd(plan=None):
			if plan is None: plan = sht.points_plan(loc, lmax, epsilon=1e-10)
			sht.synthesis_general(alm=alm[:1], map=mp[:1], spin=0, plan=plan, **kw); sht.synthesis_general(alm=alm[1:], map=mp[1:], spin=2, plan=plan, **kw)
		def adj(plan=None):
			if plan is None: plan = sht.points_plan(loc, lmax, epsilon=1e-10)
			sht.adjoint_synthesis_general(map=mp[:1], alm=alm[:1], spin=0, plan=plan, **kw); sht.adjoint_synthesis_general(map=mp[1:], alm=alm[1:], spin=2, plan=plan, **kw)
		def plan():
			sht.points_plan(loc, lmax, epsilon=1e-10)
		nt, nph = sht.points_grid_shape(lmax, lmax)
		cc = torch.zeros((3, nt, nph), device="cuda", dtype=torch.float64)
		def floor_fwd():
			sht.synthesis_2d(alm=alm[:1], map=cc[:1], spin=0, lmax=lmax, geometry="CC"); sht.synthesis_2d(alm=alm[1:], map=cc[1:], spin=2, lmax=lmax, geometry="CC")
		def floor_adj():
			sht.adjoint_synthesis_2d(alm=alm[:1], map=cc[:1], spin=0, lmax=lmax, geometry="CC"); sht.adjoint_synthesis_2d(alm=alm[1:], map=cc[1:], spin=2, lmax=lmax, geometry="CC")
		t_plan = timed(plan, a.reps)
		t_fwd_call = timed(fwd, a.reps); t_adj_call = timed(adj, a.reps)
		p = sht.points_plan(loc, lmax, epsilon=1e-10)
		t_fwd = timed(lambda: fwd(p), a.reps); t_adj = timed(lambda: adj(p), a.reps)
		t_ffl = timed(floor_fwd, a.reps); t_afl = timed(floor_adj, a.reps)
		split = {}
		for name, fn in (("forward", fwd), ("adjoint", adj)):
			sht.points_profile(p); fn(p); torch.cuda.synchronize()
			split[name] = {k: round(v, 3) for k, v in sht.points_profile_read(p).items() if k != "plan"}
			sht.points_profile(p, False)
		plan_host_ms = sht.points_profile_read(p)["plan"]
		row = dict(case=case, desc=desc, lmax=lmax, npts=npts, comps="T,Q,U (spin 0 + spin 2)", map_dtype="float64", epsilon=1e-10,
			kernel_width=p.query("kernel_width"), fine_grid=[p.query("fine_ntheta"), p.query("fine_nphi")], cc_grid=[nt, nph],
			ms_points_plan=round(t_plan, 2), ms_points_plan_host_wall=round(plan_host_ms, 2),
			ms_forward=round(t_fwd, 2), ms_adjoint=round(t_adj, 2), ms_forward_with_plan=round(t_fwd_call, 2), ms_adjoint_with_plan=round(t_adj_call, 2),
			ms_stage_split=split,
			ms_cc_synthesis_floor=round(t_ffl, 2), ms_cc_adjoint_synthesis_floor=round(t_afl, 2),
			taps=int(npts)*p.query("kernel_width")**2)
		del p
		print(json.dumps(row), flush=True)
		rows.append(row)
		del loc, alm, mp, cc; sht.clear_plans(); torch.cuda.empty_cache()
	if a.out:
		with open(a.out, "w") as fh:
			json.dump(dict(tool="tools/pos_bench.py", reps=a.reps, device=torch.cuda.get_device_name(0),
				note="forward / adjoint: two API calls (spin 0, spin 2) on one made point plan; *_with_plan: the plan made inside, once for both; "
				"ms_stage_split: the plan's stage timers over one forward / adjoint (T + QU); floor: the CC-grid transforms alone", rows=rows), fh, indent=1)

if __name__ == "__main__":
	main()
