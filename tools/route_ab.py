"""A/B of two builds of the library, route by route: the same seeded calls through each (one fresh process per library, selected with
PIXELL_AMD_LIB), outputs dumped and compared.  The case list reaches every value of the route enum of csrc/sht_plan.hpp, both directions.

  PIXELL_AMD_LIB=<lib> PXS_CHAIN_VERBOSE=1 python tools/route_ab.py run OUT.npz [--split | --fft] 2> OUT.log
  python tools/route_ab.py compare A.npz B.npz B.log     # B.log: the verbose log of a build that prints its routes
  python tools/route_ab.py merge SIM_TABLE GPU_TABLE...   # compare outputs -> the table of profiles/route_refactor_ab.txt

Maps must agree bit for bit; alm bit for bit with the deterministic option (and on the simulator), to 1e-13 relative rms with the
default atomic sums on the GPU (the bound of tests/test_streams.py); scratch_bytes, analysis_form and theta_line must be equal.
--fft: the generic N-d FFT engine instead (csrc/fft.hip, api_fft.hip), which has no atomic sums: every output bit for bit, everywhere."""
import os, sys, json
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path: sys.path.insert(0, ROOT)

def cases(split):
	from pixell_amd import sht
	rng = np.random.default_rng(1234)
	def ralm(lmax, nc, nb=None, dt=np.complex128):
		n = (lmax+1)*(lmax+2)//2; sh = (nc, n) if nb is None else (nb, nc, n)
		return (rng.standard_normal(sh)+1j*rng.standard_normal(sh)).astype(dt)
	def rmap(*sh, dt=np.float64): return rng.standard_normal(sh).astype(dt)
	def grid(name, g, nt, nph, lmax, spin, what, analysis=None, nb=None, mode="STANDARD", adt=np.complex128, mdt=np.float64, env=None):
		"""what: syn | adj (adjoint synthesis) | ana | adjana"""
		nca, ncm = sht._ncomp(spin, mode)
		alm = ralm(lmax, nca, nb, adt); m = rmap(*(((nb,) if nb else ())+(ncm, nt, nph)), dt=mdt)
		kw = dict(spin=spin, lmax=lmax, geometry=g, phi0=0.2, return_plan=True)
		def run():
			for k, v in (env or {}).items(): os.environ[k] = v
			try:
				if what == "syn": p = sht.synthesis_2d(alm=alm, map=m, mode=mode, **kw); out = m
				elif what == "adj": p = sht.adjoint_synthesis_2d(alm=alm, map=m, mode=mode, **kw); out = alm
				elif what == "ana": p = sht.analysis_2d(alm=alm, map=m, analysis=analysis, **kw); out = alm
				else: p = sht.adjoint_analysis_2d(alm=alm, map=m, analysis=analysis, **kw); out = m
			finally:
				for k in (env or {}): del os.environ[k]
			return out, p
		return name, run
	def rings(name, kw, lmax, spin, what, mode="STANDARD"):
		nca, ncm = sht._ncomp(spin, mode)
		npix = int(np.max(kw["ringstart"].astype(np.int64))+np.max(kw["nphi"].astype(np.int64))*abs(kw.get("pixstride", 1)))
		alm = ralm(lmax, nca); m = rmap(ncm, npix)
		def run():
			if what == "syn": out = sht.synthesis(alm=alm, map=m, spin=spin, lmax=lmax, mode=mode, **kw); p = sht.synthesis.last_plan
			else: out = sht.adjoint_synthesis(alm=alm, map=m, spin=spin, lmax=lmax, mode=mode, **kw); p = sht.adjoint_synthesis.last_plan
			return out, p
		return name, run
	def healpix(nside):
		i = np.arange(1, 4*nside); north = np.minimum(i, 4*nside-i); cap = north < nside
		nphi = np.where(cap, 4*north, 4*nside).astype(np.uint64)
		z = np.where(cap, 1-north**2/(3.0*nside**2), (4*nside-2.0*north)/(3*nside))*np.where(i <= 2*nside, 1, -1)
		phi0 = np.where(cap, np.pi/(4*north), np.where((north-nside) % 2 == 0, np.pi/(4*nside), 0.0))
		rs = np.concatenate([[0], np.cumsum(nphi)[:-1]]).astype(np.uint64)
		return dict(theta=np.arccos(z), nphi=nphi, phi0=phi0, ringstart=rs)
	def band(n=96, r0=9, nr=70, nph=200):
		return dict(theta=(r0+np.arange(nr)+0.5)*np.pi/n, nphi=np.full(nr, nph, np.uint64), phi0=np.full(nr, -0.4), ringstart=np.arange(nr, dtype=np.uint64)*nph)
	def points(name, adjoint):
		lmax = 20; loc = np.stack([rng.uniform(0, np.pi, 50), rng.uniform(0, 2*np.pi, 50)], 1)
		alm = ralm(lmax, 2); m = rmap(2, 50)
		def run():
			plan = sht.points_plan(loc, lmax)
			if adjoint: out = sht.adjoint_synthesis_general(map=m, loc=loc, spin=2, lmax=lmax, alm=alm, plan=plan)
			else: out = sht.synthesis_general(alm=alm, loc=loc, spin=2, lmax=lmax, map=m, plan=plan)
			return out, plan.grid
		return name, run
	if split:      # PXS_BATCH_GB=1 (set by the caller for this process): 64 scalar maps of 21 MB of scratch each go in several passes
		return [grid("batch64 split syn s0", "F1", 540, 1080, 511, 0, "syn", nb=64), grid("batch64 split ana s0", "F1", 540, 1080, 511, 0, "ana", nb=64),
			grid("batch24 split adj s2", "F1", 540, 1080, 511, 2, "adj", nb=24), grid("batch24 split adjana s2", "F1", 540, 1080, 511, 2, "adjana", nb=24),
			# 800 rings against ~390 of the CC grid: through the CC grid, 35 MB (spin 0) and 70 MB (spin 2) of scratch per map
			grid("batch40 split syn s0 cc", "F1", 800, 1600, 383, 0, "syn", nb=40), grid("batch40 split adj s0 cc", "F1", 800, 1600, 383, 0, "adj", nb=40),
			grid("batch16 split syn s2 cc", "F1", 800, 1600, 383, 2, "syn", nb=16), grid("batch16 split adj s2 cc", "F1", 800, 1600, 383, 2, "adj", nb=16)]
	F = ("F1", 24, 48, 20)        # direct for both spins
	G = ("F1", 32, 64, 20)        # between the thresholds: spin 0 direct, spin 2 through the CC grid
	H = ("F1", 64, 128, 20)       # through the CC grid for both spins; >= 2 lmax + 2 rings
	U = ("F1", 26, 64, 12)        # ring chain planned, 2 ntheta = 4 x 13: no theta chain
	N = ("F1", 64, 32, 20)        # mmax >= nphi/2: no ring chain
	cs = []
	for nm, g in (("F", F), ("G", G), ("H", H), ("U", U), ("N", N)):
		for spin in (0, 2):
			for what in ("syn", "adj"): cs.append(grid("%s %s s%d" % (what, nm, spin), *g, spin, what))
	cs += [rings("%s band s%d" % (w, s), band(), 24, s, w) for s in (0, 2) for w in ("syn", "adj")]
	cs += [rings("%s healpix s%d" % (w, s), healpix(4), 14, s, w) for s in (0, 2) for w in ("syn", "adj")]
	# 16 ring lengths: 16 (spin 0) and 32 (spin 2) FFT jobs, so the ring FFTs fork to the side streams (sht_general.hip); nside 4 never does
	cs += [rings("%s healpix16 s%d" % (w, s), healpix(16), 32, s, w) for s in (0, 2) for w in ("syn", "adj")]
	for what in ("ana", "adjana"):
		cs += [grid("%s DH s0" % what, "DH", 22, 44, 10, 0, what), grid("%s F2 s2" % what, "F2", 21, 44, 10, 2, what),
			grid("%s H weights s0" % what, *H, 0, what, analysis="weights"), grid("%s H weights s2" % what, *H, 2, what, analysis="weights"),
			grid("%s CC65 ducc0 s2" % what, "CC", 65, 120, 30, 2, what), grid("%s N weights s0" % what, *N, 0, what, analysis="weights"),
			grid("%s F default s0" % what, *F, 0, what), grid("%s H default s2" % what, *H, 2, what),
			grid("%s F interpolant s0" % what, *F, 0, what, analysis="interpolant"), grid("%s H interpolant s2" % what, *H, 2, what, analysis="interpolant"),
			grid("%s U default s0" % what, *U, 0, what), grid("%s N default s2" % what, *N, 2, what), grid("%s U interpolant s2" % what, *U, 2, what, analysis="interpolant")]
	cs += [grid("adjana F interpolant s0 ADJ_ANA_FUSED=0", *F, 0, "adjana", analysis="interpolant", env={"PXS_ADJ_ANA_FUSED": "0"}),
		grid("adjana H interpolant s2 ADJ_ANA_FUSED=0", *H, 2, "adjana", analysis="interpolant", env={"PXS_ADJ_ANA_FUSED": "0"}),
		grid("adjana F default s0 ADJ_ANA_FUSED=0", *F, 0, "adjana", env={"PXS_ADJ_ANA_FUSED": "0"})]
	cs += [grid("%s DERIV1 %s" % (w, nm), *g, 1, w, mode="DERIV1") for nm, g in (("F", F), ("H", H)) for w in ("syn", "adj")]
	cs += [rings("%s band DERIV1" % w, band(), 24, 1, w, mode="DERIV1") for w in ("syn", "adj")]
	for what in ("syn", "adj", "ana", "adjana"):
		cs += [grid("%s H s2 f32/c64" % what, *H, 2, what, adt=np.complex64, mdt=np.float32), grid("%s F s0 f32/c128" % what, *F, 0, what, mdt=np.float32),
			grid("%s H s0 batch5" % what, *H, 0, what, nb=5), grid("%s G s2 batch3" % what, *G, 2, what, nb=3), grid("%s U s0 batch2" % what, *U, 0, what, nb=2)]
	cs += [points("alm2map_pos s2", False), points("alm2map_pos adjoint s2", True)]
	return cs

def fft_cases():
	"""pixell_amd.fft on seeded arrays: single-pass lines (the direct-DFT radix pass at 7 and 61, 2048 the longest), four-step lines (2304 the
	shortest), chirp-z by the min-prime rule (131) and for want of a factorisation (4099), every kind, strided views, the budget seam"""
	import torch
	from pixell_amd import fft as pfft, _lib
	rng = np.random.default_rng(4321)
	dev = "cpu" if _lib.is_hostsim() else "cuda"
	def arr(*sh, dt=np.complex128):
		x = rng.standard_normal(sh)+(1j*rng.standard_normal(sh) if np.dtype(dt).kind == "c" else 0)
		return torch.from_numpy(x.astype(dt)).to(dev)
	def out(*sh, dt=np.complex128): return torch.zeros(sh, dtype=getattr(torch, np.dtype(dt).name), device=dev)
	cs = []
	def case(name, fn, env=None):
		def run():
			for k, v in (env or {}).items(): os.environ[k] = v
			try: o = fn().cpu().numpy()
			except _lib.PxsError as e: o = np.array([e.code])      # (a refusal is an outcome too: the same code from both builds)
			finally:
				for k in (env or {}): del os.environ[k]
			return o, None
		cs.append(("fft "+name, run))
	for n in (1, 2, 7, 36, 61, 131, 216, 2048, 2304, 4099, 10800):
		x = arr(3, n)
		case("c2c forward n=%d" % n, lambda x=x: pfft.fft(x)); case("c2c backward n=%d" % n, lambda x=x: pfft.ifft(x))
	for n in (9, 16):
		x = arr(3, n, dt=np.float64); h = arr(3, n//2+1); h2 = arr(6, n//2+1)
		case("r2c n=%d" % n, lambda x=x: pfft.rfft(x)); case("c2r n=%d" % n, lambda h=h, n=n: pfft.irfft(h, n=n))
		case("c2r two axes 6 x %d" % n, lambda h2=h2, n=n: pfft.irfft(h2, n=n, axes=[-2, -1]))
	x = arr(2, 5, 12); case("middle axis of (2, 5, 12)", lambda x=x: pfft.fft(x, axes=[1]))
	x = arr(8, 21)[::2, 1::3]; case("non-contiguous input view", lambda x=x: pfft.fft(x))
	x = arr(4, 10); o = out(4, 20)
	def strided_out(x=x, o=o): pfft.fft(x, o[:, ::2]); return o      # (the whole base array: what lies between must stay untouched)
	case("output into a strided view", strided_out)
	x = arr(4, 6, 10); case("three axes", lambda x=x: pfft.fft(x, axes=[0, 1, 2]))
	x = arr(3, 36, dt=np.complex64); case("c2c complex64", lambda x=x: pfft.fft(x))
	x = arr(3, 16, dt=np.float32); case("r2c float32", lambda x=x: pfft.rfft(x))
	# 3000: the extended length 6000 is a four-step line; DCT-I and DST-I extend to 2 (n -+ 1), which has it at 3001 and 2999 and is refused
	# at 3000 (5998 = 2 x 2999, 6002 = 2 x 3001: no chirp-z for r2r)
	kinds = ("DCT-I", "DCT-II", "DCT-III", "DCT-IV", "DST-I", "DST-II", "DST-III", "DST-IV")
	for n, t in [(n, t) for n in (5, 16, 31, 3000) for t in kinds]+[(3001, "DCT-I"), (2999, "DST-I")]:
		case("%s n=%d" % (t, n), lambda x=arr(2, n, dt=np.float64), t=t: pfft.dct(x, type=t))
	x = arr(24, 40, dt=np.float64); case("real 2-D, generic engine", lambda x=x: pfft.fft(x, axes=[-2, -1]), env={"PXS_FFT2_FAST_MINPIX": "-1"})
	x = arr(40, 2304); case("four-step in passes of 14 lines", lambda x=x: pfft.fft(x), env={"PXS_FFT_TEMP_MB": "0.5"})
	return cs

def run(out, split, fft=False):
	from pixell_amd import sht, _lib
	res = {}; meta = {"hostsim": bool(_lib.is_hostsim()), "version": _lib.load().pxs_version().decode(), "cases": []}
	for det in ((False,) if fft else (False, True)):
		sht.set_deterministic(det); sht.clear_plans()
		for name, fn in (fft_cases() if fft else cases(split)):
			key = name+(" [det]" if det else "")
			os.write(2, ("CASE %s\n" % key).encode())
			o, plan = fn()
			if not _lib.is_hostsim():
				import torch; torch.cuda.synchronize()
			res[key] = np.array(o, copy=True)
			info = plan.info() if plan is not None else dict(scratch_bytes=0, nring_syn=0, nring_ana=0)      # (the FFT cases have no plan)
			meta["cases"].append(dict(name=key, scratch=info["scratch_bytes"], nring_syn=info["nring_syn"], nring_ana=info["nring_ana"],
				form=plan.query("analysis_form") if plan is not None else 0, line=plan.query("theta_line") if plan is not None else 0,
				alm=bool(plan is not None and np.iscomplexobj(o))))
	np.savez(out, **{k.replace("/", "|"): v for k, v in res.items()})
	with open(out+".json", "w") as f: json.dump(meta, f)

def routes_of(log):
	"""{case: [route lines]} from a PXS_CHAIN_VERBOSE log with the CASE markers of run()"""
	out = {}; cur = None
	for line in open(log, errors="replace"):
		if line.startswith("CASE "): cur = line[5:].strip(); out[cur] = []
		elif cur and "[pxsht]" in line and " route " in line:
			w = line.split(); s = "%s%s %s" % (w[3].rstrip(","), "^T" if "adjoint 1" in line else "", line.split("passes of ")[1].strip() if "passes of " in line else "")
			if s.strip() not in out[cur]: out[cur].append(s.strip())
	return out

def compare(a, b, log):
	A, B = np.load(a), np.load(b); ma, mb = json.load(open(a+".json")), json.load(open(b+".json"))
	rts = routes_of(log) if log else {}
	sim = mb["hostsim"]; bad = 0; rows = []
	assert len(ma["cases"]) == len(mb["cases"]), "the two dumps hold %d and %d cases" % (len(ma["cases"]), len(mb["cases"]))
	for ca, cb in zip(ma["cases"], mb["cases"]):
		assert ca["name"] == cb["name"]
		k = ca["name"]; x, y = A[k.replace("/", "|")], B[k.replace("/", "|")]
		bit = x.tobytes() == y.tobytes()
		err = float(np.sqrt(np.sum(np.abs(x.astype(np.complex128)-y)**2)/max(np.sum(np.abs(x.astype(np.complex128))**2), 1e-300)))
		need_bits = (not ca["alm"]) or sim or k.endswith("[det]")
		ok = (bit if need_bits else err <= 1e-13) and ca["scratch"] == cb["scratch"] and ca["form"] == cb["form"] and ca["line"] == cb["line"]
		bad += not ok
		rows.append("%-46s %-34s %-9s %-9.1e scratch %10d %s form %d line %d  %s" % (k, "; ".join(rts.get(k, ["?"])), "bitwise" if bit else "differs", err, cb["scratch"],
			"=" if ca["scratch"] == cb["scratch"] else "!= %d" % ca["scratch"], cb["form"], cb["line"], "ok" if ok else "FAIL"))
	print("# %s (%s)  vs  %s (%s): %d cases, %d failed" % (a, ma["version"], b, mb["version"], len(rows), bad))
	print("\n".join(rows))
	return bad

def merge(sim_table, gpu_tables):
	"""one row per case from the compare outputs of the simulator and of the GPU (cases run on the GPU only: simulator column -)"""
	import re
	def rows(f):
		pat = r"(.{46}) (.{34}) (\S+)\s+(\S+)\s+scratch\s+(\d+) (=|!= \d+) form (\d) line (\d)\s+(\S+)"
		return [[x.strip() for x in re.match(pat, l).groups()] for l in open(f) if not l.startswith("#")]
	sim = {r[0]: r for r in rows(sim_table)}; bad = 0
	agree = lambda x: "-" if x is None else ("bitwise" if x[2] == "bitwise" else "%s %s" % (x[2], x[3]))
	print("%-46s %-26s %-20s %-20s %12s %-8s %s" % ("case", "route (^T: adjoint) passes", "simulator", "GPU", "scratch", "=parent", "form line"))
	for t in gpu_tables:
		for r in rows(t):
			s = sim.get(r[0]); ok = r[8] == "ok" and (s is None or s[8] == "ok"); bad += not ok
			print("%-46s %-26s %-20s %-20s %12s %-8s %s %s  %s" % (r[0], r[1], agree(s), agree(r), r[4], "yes" if r[5] == "=" and (s is None or s[5] == "=") else "NO", r[6], r[7], "ok" if ok else "FAIL"))
	return bad

if __name__ == "__main__":
	if sys.argv[1] == "run": run(sys.argv[2], "--split" in sys.argv, "--fft" in sys.argv)
	elif sys.argv[1] == "merge": sys.exit(1 if merge(sys.argv[2], sys.argv[3:]) else 0)
	else: sys.exit(1 if compare(sys.argv[2], sys.argv[3], sys.argv[4] if len(sys.argv) > 4 else None) else 0)
