"""Times reproject.map2healpix / healpix2map with method="spline" on the device; prints one JSON line per operation.

  python tools/bench_reproject.py                a [3, 10800, 21600] float32 dmap (1' full sky) -> nside 2048 with rot="equ,gal", order 1, and back
  python tools/bench_reproject.py --res 4 --nside 512      the same 16 times smaller

The fused calls alternate with the unfused composition of functions that do not need csrc/healpix.hip: the centres of the healpix pixels
from the ring tables, the rotation and the closed-form angle formed with torch, then enmap.at and enmap.rotate_pol.  (There is no such
composition for healpix -> CAR: nothing else reads a healpix map at positions.)  Each operation runs once to warm up and `--reps` times
between device events around work that ends in a synchronise; all times and the median are reported.  must_move_GB: the output written
once plus the input read once (CAR -> healpix: no more than the taps ask for); hbm_frac: that over the median time, over 8 TB/s.  The
reads are gathers, so this sits well below a streaming kernel's share."""
import argparse, json, os, sys
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

HBM = 8.0e12
arcmin = np.pi/180/60

def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--res", type=float, default=1.0, help="pixel size of the CAR map in arcminutes")
	ap.add_argument("--nside", type=int, default=2048)
	ap.add_argument("--reps", type=int, default=5)
	args = ap.parse_args()
	import torch
	from pixell_amd import curvedsky, enmap, reproject, _lib
	assert torch.cuda.is_available() and not _lib.is_hostsim(), "this benchmark needs a GPU"
	def timed(fn):
		fn(); torch.cuda.synchronize()
		ts = []
		for _ in range(args.reps):
			a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
			a.record(); r = fn(); b.record(); b.synchronize()
			ts.append(a.elapsed_time(b)); del r
		return ts
	def say(what, ts, gb=None, **kw):
		if gb is not None: kw.update(must_move_GB=gb, hbm_frac=gb*1e9/(float(np.median(ts))*1e-3)/HBM)
		print(json.dumps(dict(what=what, median_ms=float(np.median(ts)), ms=[round(t, 4) for t in ts], **kw)), flush=True)
	shape, wcs = enmap.fullsky_geometry(res=args.res*arcmin)
	ny, nx = shape
	nside, npix = args.nside, 12*args.nside**2
	g = torch.Generator(device="cuda"); g.manual_seed(1)
	m = enmap.dmap(torch.randn((3, ny, nx), dtype=torch.float32, device="cuda", generator=g), wcs)
	rot = "equ,gal"

	# the unfused composition
	ri = curvedsky.get_ring_info_healpix(nside)
	nphi = torch.as_tensor(ri.nphi.astype(np.int64), device="cuda")
	def unfused():
		ring = torch.repeat_interleave(torch.arange(len(ri.theta), device="cuda"), nphi)
		k = torch.arange(npix, device="cuda")-torch.as_tensor(ri.offsets.astype(np.int64), device="cuda")[ring]
		dec = np.pi/2-torch.as_tensor(ri.theta, device="cuda")[ring]
		ra = torch.as_tensor(ri.phi0, device="cuda")[ring]+2*np.pi*k.double()/nphi[ring].double()      # (float64: an integer tensor times a Python float is float32)
		M = torch.as_tensor(reproject._rotmat(rot), device="cuda")
		n = torch.stack([torch.cos(dec)*torch.cos(ra), torch.cos(dec)*torch.sin(ra), torch.sin(dec)])
		e = torch.stack([-torch.sin(ra), torch.cos(ra), torch.zeros_like(ra)])
		V, E = M @ n, M @ e
		ce = V[0]*E[1]-V[1]*E[0]; cn = (V[0]**2+V[1]**2)*E[2]-V[2]*(V[0]*E[0]+V[1]*E[1])
		pos = torch.stack([torch.atan2(V[2], torch.hypot(V[0], V[1])), torch.atan2(V[1], V[0])])
		v = enmap.at(m, pos, order=1, border="constant")
		return enmap.rotate_pol(v, -torch.atan2(cn, ce), axis=-2)
	fused = lambda: reproject.map2healpix(m, nside=nside, rot=rot, method="spline", order=1)
	gb = (3*npix*4+min(3*ny*nx*4, 4*3*npix*4))/1e9
	a, b = fused(), unfused()
	print(json.dumps(dict(what="fused - unfused", max_abs=float((a-b).abs().max()), above_1e_5=int(((a-b).abs() > 1e-5).sum()), of=int(a.numel()))), flush=True)
	del a, b
	for rep in range(2):
		say("map2healpix spline order 1 rot %s, [3, %d, %d] f32 -> nside %d, fused" % (rot, ny, nx, nside), timed(fused), gb)
		say("the same unfused: torch positions and angle, enmap.at, enmap.rotate_pol", timed(unfused))
	heal = fused()
	torch.cuda.empty_cache()
	gb = (3*ny*nx*4+3*npix*4)/1e9
	say("healpix2map spline order 1, nside %d -> [3, %d, %d] f32, fused" % (nside, ny, nx), timed(lambda: reproject.healpix2map(heal, shape, wcs, method="spline", order=1)), gb)
	say("the same with rot gal,equ", timed(lambda: reproject.healpix2map(heal, shape, wcs, rot="gal,equ", method="spline", order=1)), gb)
	say("the same, order 0", timed(lambda: reproject.healpix2map(heal, shape, wcs, method="spline", order=0)), gb)

if __name__ == "__main__":
	main()
