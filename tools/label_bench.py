#!/usr/bin/env python
"""labels.label and labels.stats at the headline size: the 21600 x 43200 full-sky geometry with 1e5 discs of 2 arcmin radius painted by
pointsrcs.sim_objects and thresholded.  Each step is timed with events, next to one device-to-device copy, timed in the same run, of the
bytes the step must move at the least (label: the mask read and the labels written; stats: the labels read).
usage: tools/label_bench.py [reps]            runs the two steps one after the other, each in a process of its own under a time limit
       tools/label_bench.py --step label|stats [reps]   one step, one JSON line"""
import sys, os, json, subprocess
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEP_LIMIT = 300      # seconds per step

def driver(reps):
	for step in ("label", "stats"):
		rc = subprocess.call(["timeout", "-k", "10", str(STEP_LIMIT), sys.executable, os.path.abspath(__file__), "--step", step, str(reps)])
		if rc != 0:
			print(json.dumps({"step": step, "failed": rc})); return rc      # (nothing more is started on the GPU after a failure)
	return 0

def step(name, reps):
	import numpy as np, torch
	from pixell_amd import enmap, pointsrcs, labels
	ny, nx, nobj, r0 = 21600, 43200, 100000, 2*np.pi/180/60
	shape, wcs = enmap.fullsky_geometry(shape=(ny, nx))
	rng = np.random.default_rng(1)
	poss = np.array([np.arcsin(rng.uniform(-np.sin(1.48), np.sin(1.48), nobj)), rng.uniform(-np.pi, np.pi, nobj)])
	prof = np.array([[0, r0, r0*1.001], [1.0, 1.0, 0.0]])
	sky = pointsrcs.sim_objects(shape, wcs, torch.as_tensor(poss, device="cuda"), torch.ones(nobj, dtype=torch.float32, device="cuda"), prof, vmin=0.5, op="max")
	mask = (sky.tensor > 0.5).to(torch.uint8)
	del sky
	def timed(fn):
		fn(); torch.cuda.synchronize()
		a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
		a.record()
		for _ in range(reps): fn()
		b.record(); torch.cuda.synchronize()
		return a.elapsed_time(b)/reps
	def copy_ms(nbytes):
		"""one device-to-device copy that reads and writes nbytes in all"""
		src = torch.empty(nbytes//2, dtype=torch.uint8, device="cuda"); dst = torch.empty_like(src)
		return timed(lambda: dst.copy_(src))
	res = dict(step=name, shape=[ny, nx], nobj=nobj, foreground=float(mask.float().mean()), reps=reps)
	if name == "label":
		lab, n = labels.label(mask)
		res["nlabel"] = n
		res["ms"] = round(timed(lambda: labels.label(mask)), 3)
		res["min_bytes"] = mask.numel()*(1+4)
	else:
		lab, n = labels.label(mask)
		g = torch.Generator(device="cuda"); g.manual_seed(2)
		v = torch.randn((ny, nx), generator=g, device="cuda", dtype=torch.float64); w = v*v
		res["nlabel"] = n
		res["ms"] = round(timed(lambda: labels.stats(lab, values=v, weights=w, nlabel=n)), 3)
		res["min_bytes"] = lab.numel()*4
		del v, w
	res["copy_ms"] = round(copy_ms(res["min_bytes"]), 3)
	res["ratio"] = round(res["ms"]/res["copy_ms"], 2)
	print(json.dumps(res))

if __name__ == "__main__":
	args = sys.argv[1:]
	if args[:1] == ["--step"]: step(args[1], int(args[2]) if len(args) > 2 else 3)
	else: sys.exit(driver(int(args[0]) if args else 3))
