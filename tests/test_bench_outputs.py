"""bench.py --dump-outputs: what the timed path computed in its last step, as .npy files (a fixed, seeded sample where an output is large),
so that two builds can be compared output for output; and a plain run (no --full) is the headline loop alone."""
import json, os, subprocess, sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
import bench

def test_dump_index_is_fixed_and_in_bounds():
	assert bench.dump_index(1000, k=1000) is None
	a = bench.dump_index(3*21600*43200); b = bench.dump_index(3*21600*43200)
	assert np.array_equal(a, b) and a.dtype.kind == "i"
	assert 0.99*bench.DUMP_SAMPLE < len(a) <= bench.DUMP_SAMPLE and a[0] >= 0 and a[-1] < 3*21600*43200 and bool(np.all(np.diff(a) > 0))

def test_dump_outputs_files(tmp_path):
	torch = pytest.importorskip("torch")
	small = torch.arange(12, dtype=torch.float64).reshape(3, 4)*(1+2j)
	big = torch.arange(bench.DUMP_SAMPLE+5, dtype=torch.float64)
	bench.dump_outputs(str(tmp_path), {"alm": small, "map": big})
	alm = np.load(tmp_path/"alm.npy")
	assert alm.dtype == np.float64 and alm.shape == (3, 4, 2) and not (tmp_path/"alm_index.npy").exists()
	np.testing.assert_array_equal(alm[..., 0]+1j*alm[..., 1], small.numpy())
	m = np.load(tmp_path/"map.npy"); idx = np.load(tmp_path/"map_index.npy")
	assert m.dtype == np.float64 and idx.dtype == np.float64 and m.shape == idx.shape
	np.testing.assert_array_equal(m, idx)          # the sample of arange is its own index
	assert sum(os.path.getsize(p) for p in tmp_path.iterdir()) < 64 << 20

@pytest.mark.gpu
def test_plain_run_dumps_last_step(tmp_path):
	"""C1, 3 timed steps: the line holds the contract fields and nothing from --full; the dumped alm is the map2alm of the last step,
	i.e. the seeded input alm back to round-trip accuracy, and the map its synthesis"""
	import torch
	env = dict(os.environ); env.pop("WORLD_SIZE", None); env.pop("RANK", None); env.pop("LOCAL_RANK", None)
	p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "c1", "--steps", "3", "--warmup", "1",
		"--dump-outputs", str(tmp_path)], env=env, capture_output=True, text=True, timeout=600)
	lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
	assert p.returncode == 0 and len(lines) == 1, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
	r = json.loads(lines[0])
	assert r["steps"] == 3 and r["warmup"] == 1 and r["ms_per_step"] > 0 and r["value"] > 0
	assert r["unit"] == "round-trips/s" and r["higher_is_better"] is True and r["dtype"] == "f64"
	for k in ("configs", "cpu_baseline", "h2d_inclusive", "fft", "accuracy"): assert k not in r, k
	assert r["analysis_other_forms"] is None
	cfg = bench.CONFIGS["c1"]
	alm = np.load(tmp_path/"alm.npy")
	assert alm.dtype == np.float64 and alm.shape == (1, bench.nalm(cfg["lmax"]), 2)
	ref = bench.make_alm(cfg, 1000, torch.device("cuda", 0)).cpu().numpy()
	got = alm[..., 0]+1j*alm[..., 1]
	assert np.sqrt(np.mean(np.abs(got-ref)**2)/np.mean(np.abs(ref)**2)) < 1e-10
	m, idx = np.load(tmp_path/"map.npy"), np.load(tmp_path/"map_index.npy")
	ny, nx = cfg["shape"]
	assert m.dtype == np.float64 and m.shape == idx.shape and idx[-1] < ny*nx and np.isfinite(m).all() and np.abs(m).max() > 0
