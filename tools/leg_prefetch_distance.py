#!/usr/bin/env python
"""Distance between the scalar row loads of the VALU Legendre kernels' loops and the wait that drains them, read off the gfx950 assembly.
usage: tools/leg_prefetch_distance.py pixell_amd/csrc/leg_s0.hip pixell_amd/csrc/leg_spin.hip   (compiles with hipcc -S; needs no GPU)
       tools/leg_prefetch_distance.py leg_s0.s leg_spin.s                                       (listings made before)
For every innermost loop of leg_{syn,ana}_{s0,spin}<K> that holds scalar loads and FP64 FMAs (the flush of the analysis, inside a trip, holds neither; its waits, on
its own LDS reads in one trip of eight, are counted with the trip's): the FMAs of one trip, every s_load_dwordx2/4/8/16 with the number of
v_fma_f64 / v_fmac_f64 between it and the first s_waitcnt on lgkmcnt after it (through the back edge if the trip ends first), and every such wait of the trip.
The loops with the most FMAs per trip run four full steps: the phase-C loops, and where the compiler unrolls it, the pair loop of phase B, which lies inside the loop
of phase B's 4-step tests ("4 steps" instead of "phase C": the mark is the nesting as the listing shows it, which block placement can blur)."""
import subprocess, sys, re, os, tempfile

def listing(path):
	if not path.endswith((".hip", ".cpp")): return open(path).read()
	with tempfile.TemporaryDirectory() as d:
		out = os.path.join(d, "k.s")
		subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-S", path, "-o", out], stderr=subprocess.DEVNULL)
		return open(out).read()

def kernels(text):
	cur, body = None, []
	for line in text.splitlines():
		m = re.match(r"^(_ZN3pxs\w+):", line)
		if m: cur, body = m.group(1), []
		elif cur is not None:
			body.append(line)
			if line.startswith(".Lfunc_end"): yield cur, body; cur = None      # (a kernel may end in several s_endpgm)

def demangle(n): return re.sub(r"\(.*", "", subprocess.run(["c++filt", n], capture_output=True, text=True).stdout.strip())

FMA = re.compile(r"^\s*v_fma(c)?_f64(_e32|_e64|_dpp)?\s"); LOAD = re.compile(r"^\s*(s_load_dwordx(2|4|8|16))\s+(s\[\d+:\d+\])"); WAIT = re.compile(r"^\s*s_waitcnt\b.*lgkmcnt")

def loops(body):
	label = {}
	for i, l in enumerate(body):
		m = re.match(r"^(\.LBB\d+_\d+):", l)
		if m: label[m.group(1)] = i
	regs = []
	for i, l in enumerate(body):
		m = re.match(r"^\s*s_cbranch_\w+\s+(\.LBB\d+_\d+)", l) or re.match(r"^\s*s_branch\s+(\.LBB\d+_\d+)", l)
		if m and m.group(1) in label and label[m.group(1)] < i: regs.append((label[m.group(1)], i, m.group(1)))
	# the loops that hold FMAs and row loads and no other such loop (a loop of the flush inside a trip holds neither)
	work = [r for r in regs if any(FMA.match(l) for l in body[r[0]:r[1]+1]) and any(LOAD.match(l) for l in body[r[0]:r[1]+1])]
	inner = [r for r in work if not any(o[:2] != r[:2] and r[0] <= o[0] and o[1] <= r[1] for o in work)]
	# (nested: the loop lies inside another loop of the kernel -- the pair loop of phase B inside the loop of its 4-step tests)
	return [r + (any(o[:2] != r[:2] and o[0] <= r[0] and r[1] <= o[1] for o in regs),) for r in {x[:2]: x for x in inner}.values()]

def report(name, body):
	rows = []
	for a, b, lab, nested in sorted(loops(body)):
		trip = body[a:b+1]
		nf = sum(1 for l in trip if FMA.match(l))
		if nf == 0 or not any(LOAD.match(l) for l in trip): continue
		loads = []
		for i, l in enumerate(trip):
			m = LOAD.match(l)
			if not m: continue
			d, k, n = 0, i + 1, 0
			while n < 2*len(trip):      # (through the back edge once at most)
				x = trip[k % len(trip)]
				if WAIT.match(x): break
				if FMA.match(x): d += 1
				k += 1; n += 1
			loads.append((m.group(1), m.group(3), d))
		waits = sum(1 for l in trip if WAIT.match(l))
		rows.append((lab, nf, waits, loads, nested))
	if not rows: return
	top = max(r[1] for r in rows)
	print(name)
	for lab, nf, waits, loads, nested in rows:
		print("  loop %-10s %-8s %3d FMAs per trip, %d waits on lgkmcnt; FMAs from request to drain: min %d" % (lab, "phase C" if nf == top and not nested else "4 steps" if nf == top else "", nf, waits, min(d for _, _, d in loads)))
		for op, reg, d in loads: print("      %-17s %-10s %4d" % (op, reg, d))

for path in sys.argv[1:]:
	for n, body in kernels(listing(path)):
		d = demangle(n)
		if re.search(r"pxs::leg_(syn|ana)_(s0|spin)<\d+>$", d): report(d.replace("void ", ""), body)
