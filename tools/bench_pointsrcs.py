"""Times pointsrcs.sim_objects and pointsrcs.radial_sum on the device; prints one JSON line.

  python tools/bench_pointsrcs.py                       10^6 Gaussian sources (FWHM 1.4', vmin = 1e-3 min|amp|) into the 21600 x 43200
                                                         float32 map, and radial_sum of 10^5 objects x 20 bins of 0.5'
  python tools/bench_pointsrcs.py --res 2 --nsrc 62500 --nrad 6250     the same densities on a 2' map (16 times fewer pixels)

Each operation runs once to warm up (library scratch, torch allocator) and `--reps` times between device events; the median is
reported.  evals: pixels inside the discs (paint) or inside the outermost bin (radial_sum), counted from the cut radii and the pixel
areas -- the work the result needs, not the pixels the kernels look at.  bytes: for the paint, the 16 x 16 tiles that end up non-zero
read and written once plus the object records; for the radial sums, the box pixels read once.  hbm_frac: bytes / time over 8 TB/s."""
import argparse, json, os, sys
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

HBM = 8.0e12
arcmin = np.pi/180/60

def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--res", type=float, default=0.5, help="pixel size in arcminutes")
	ap.add_argument("--nsrc", type=int, default=1000000)
	ap.add_argument("--nrad", type=int, default=100000)
	ap.add_argument("--nbin", type=int, default=20)
	ap.add_argument("--reps", type=int, default=3)
	args = ap.parse_args()
	import torch
	from pixell_amd import enmap, pointsrcs
	shape, wcs = enmap.fullsky_geometry(res=args.res*arcmin)
	ny, nx = shape
	pix = args.res*arcmin
	rng = np.random.default_rng(0)
	def catalogue(n):
		return np.array([np.arcsin(rng.uniform(-1, 1, n)), rng.uniform(-np.pi, np.pi, n)], np.float32)
	def timed(fn):
		fn(); torch.cuda.synchronize()
		ts = []
		for _ in range(args.reps):
			a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
			a.record(); fn(); b.record(); b.synchronize()
			ts.append(a.elapsed_time(b)*1e-3)
		return float(np.median(ts))
	res = dict(shape=[ny, nx], nsrc=args.nsrc, nrad=args.nrad, nbin=args.nbin)
	# ---- paint ----
	sigma = 1.4*arcmin/(8*np.log(2))**0.5
	rs = np.linspace(0, 10*sigma, 500)
	prof = np.array([rs, np.exp(-0.5*(rs/sigma)**2)], np.float32)
	poss = catalogue(args.nsrc)
	amps = rng.uniform(0.5, 3, (1, args.nsrc)).astype(np.float32)
	vmin = 1e-3*float(amps.min())
	dposs, damps = torch.as_tensor(poss, device="cuda"), torch.as_tensor(amps, device="cuda")
	omap = enmap.dmap(torch.zeros((1, ny, nx), dtype=torch.float32, device="cuda"), wcs)
	t = timed(lambda: pointsrcs.sim_objects(shape, wcs, dposs, damps, prof, omap=omap, vmin=vmin))
	k = np.searchsorted(-prof[1], -(np.float32(vmin)/amps[0]), side="right")-1      # the last sample with b >= vmin/amp (b decreases)
	rcut = prof[0][np.minimum(np.maximum(k, 0)+1, prof.shape[1]-1)]
	evals = float(np.sum(np.pi*np.float64(rcut)**2/(pix*pix*np.maximum(np.cos(np.float64(poss[0])), pix))))
	tiles = int((omap.tensor[0, :ny//16*16, :nx//16*16].reshape(ny//16, 16, nx//16, 16) != 0).any(3).any(1).sum())
	nbytes = tiles*256*4*2+args.nsrc*16
	res["paint"] = dict(seconds=t, evals=evals, evals_per_s=evals/t, tiles_touched=tiles, bytes=nbytes, hbm_frac=nbytes/t/HBM)
	del omap
	# ---- radial sums ----
	m = enmap.dmap(torch.rand((1, ny, nx), dtype=torch.float32, device="cuda"), wcs)
	bins = np.arange(args.nbin+1)*0.5*arcmin
	rposs = catalogue(args.nrad); drposs = torch.as_tensor(rposs, device="cuda")
	t = timed(lambda: pointsrcs.radial_sum(m, drposs, bins))
	c = np.maximum(np.cos(np.float64(rposs[0])), pix)
	evals = float(np.sum(np.pi*bins[-1]**2/(pix*pix*c)))
	box = float(np.sum((2*bins[-1]/pix+2)*np.minimum(2*bins[-1]/(pix*c)+2, nx)))
	res["radial_sum"] = dict(seconds=t, evals=evals, evals_per_s=evals/t, box_pixels=box, bytes=box*4, hbm_frac=box*4/t/HBM)
	print(json.dumps(res))

if __name__ == "__main__":
	main()
