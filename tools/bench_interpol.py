"""Times interpol.spline_filter, enmap.project and enmap.at on the device; prints one JSON line per operation.

  python tools/bench_interpol.py                 a 21600 x 43200 float64 map: its spline_filter; its projection onto the 1' full-sky geometry
                                                 (10800 x 21600) at order 3 with and without the prefilter and at order 1; at() for 10^6
                                                 uniform random positions at orders 3 and 1
  python tools/bench_interpol.py --res 2         the same on a 2' map (16 times fewer pixels), projected onto the 4' geometry

Each operation runs once to warm up (code objects, torch's allocator) and `--reps` times between device events; all times and the median
are reported.  spline_filter's time includes taking its scratch and output maps from torch's caching allocator.  algorithmic_GB: what the
filter has to move, a read and a write of the float64 map per axis (4 x the map); hbm_frac: that over the time, over 8 TB/s."""
import argparse, json, os, sys
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

HBM = 8.0e12
arcmin = np.pi/180/60

def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--res", type=float, default=0.5, help="pixel size of the map in arcminutes; it is projected onto twice that")
	ap.add_argument("--npoint", type=int, default=1000000)
	ap.add_argument("--reps", type=int, default=8)
	args = ap.parse_args()
	import torch
	from pixell_amd import enmap, interpol, _lib
	assert torch.cuda.is_available() and not _lib.is_hostsim(), "this benchmark needs a GPU"
	def timed(fn):
		fn(); torch.cuda.synchronize()
		ts = []
		for _ in range(args.reps):
			a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
			a.record(); r = fn(); b.record(); b.synchronize()
			ts.append(a.elapsed_time(b)); del r
		return ts
	def say(what, ts, **kw):
		print(json.dumps(dict(what=what, median_ms=float(np.median(ts)), ms=[round(t, 4) for t in ts], **kw)), flush=True)
	shape, wcs = enmap.fullsky_geometry(res=args.res*arcmin)
	oshape, owcs = enmap.fullsky_geometry(res=2*args.res*arcmin)
	ny, nx = shape
	g = torch.Generator(device="cuda"); g.manual_seed(1)
	m = enmap.dmap(torch.randn((ny, nx), dtype=torch.float64, device="cuda", generator=g), wcs)
	ts = timed(lambda: interpol.spline_filter(m, border="grid-wrap"))
	gb = 4*ny*nx*8/1e9
	say("spline_filter %dx%d f64" % (ny, nx), ts, algorithmic_GB=gb, hbm_frac=gb*1e9/(float(np.median(ts))*1e-3)/HBM)
	ip = interpol.interpolator(m, npre=0, order=3, border="constant")
	say("project -> %dx%d, order 3, prefiltered interpolator" % oshape, timed(lambda: enmap.project(m, oshape, owcs, ip=ip)))
	pos = torch.stack([torch.asin(torch.rand(args.npoint, dtype=torch.float64, device="cuda", generator=g)*2-1),
		(torch.rand(args.npoint, dtype=torch.float64, device="cuda", generator=g)*2-1)*np.pi])
	say("at, %d random positions, order 3, prefiltered interpolator" % args.npoint, timed(lambda: enmap.at(m, pos, ip=ip)))
	del ip
	torch.cuda.empty_cache()
	say("project -> %dx%d, order 3, filter included" % oshape, timed(lambda: enmap.project(m, oshape, owcs, order=3)))
	say("project -> %dx%d, order 1" % oshape, timed(lambda: enmap.project(m, oshape, owcs, order=1)))
	say("at, %d random positions, order 1" % args.npoint, timed(lambda: enmap.at(m, pos, order=1)))

if __name__ == "__main__":
	main()
