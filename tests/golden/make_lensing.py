"""Generate tests/golden/lensing.npz by running the REFERENCE's pixell.lensing / enmap.rotate_pol (pure numpy) in this container.

Run:  python tests/golden/make_lensing.py      (needs /root/reference; never run on the GPU box)

The reference is imported through _ref_harness.py with the repo's long-double oracle mounted as ducc0.sht.experimental.  Only inputs and
expected outputs are saved:
  d_<geo>_*      lensing.offset_by_grad on 10-degree grids (CC, Fejer-1, CC flipped in y, CC flipped in x): positions, gradients
                 (1e-3 * random, with a zero, a dec-only and an ra-only gradient planted), outputs with pol=True; on CC also pol=False, a
                 psi0 component, a float32 gradient and geodesic=False with gradients planted that carry points over the poles
  g_*            the same on the 1-degree CC grid of the reference's test_offset (every 12th row kept; the gradient is regenerated
                 by the test from its seed, g_grad_head pins the generator)
  pw_*           lensing.pole_wrap
  r_*            enmap.rotate_pol: a batch of two T/Q/U maps, spin 0, 1, 2, float64 and float32
  e_*            end to end at lmax 16 on the 10-degree CC grid: expected lensed map = the reference's offset_by_grad applied to the
                 oracle's DERIV1 map, the oracle's exact synthesis on one-pixel rings at those positions, the reference's rotate_pol
  m_*            the reference's test_lensing shape: 1-degree CC, lmax 400, alm from lensing.rand_alm(seed=1).  The spectrum up to
                 lmax is kept and every 64th element of phi_alm: the test draws the alm itself (the legacy generator is bit-exact,
                 m_phi_sub and lens_unlensed.npz pin it) -- the whole phi_alm is 1.3 MB.  Expected map as in e_*, every 4th row.
  a_*            lensing.rand_alm with and without phi_seed

Comparison with the reference's recorded tests/data/MM_lensed_071123.fits (np.isclose share per component, printed by this script).
As run for the committed fixtures (every 4th row, 46 of 181 rows, the two pole rows among them; the oracle takes 8 minutes for them,
--full evaluates every row in four times that):
  isclose share per component: all rows [1. 1. 1.], pole rows left out [1. 1. 1.]
  max |diff| / rms per component: [4.7e-12 5.5e-11 5.5e-11]
Every evaluated pixel is close, so the recorded rows are kept as lensing_recorded.npz (every 4th row) and a GPU test pins the result
to them with the reference's own np.isclose, pole rows left out.
"""
import sys, os, types, time
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, HERE)
from oracle import sht_oracle as so
import _ref_harness as H
from make_golden import read_fits_f64

deg = np.pi/180

def geo_numbers(shape, wcs):
	return np.array([shape[-2], shape[-1]], float), np.array(wcs.wcs.cdelt, float), np.array(wcs.wcs.crval, float), np.array(wcs.wcs.crpix, float)

def planted_grad(rng, shape):
	g = 1e-3*rng.random((2,)+tuple(shape[-2:]))
	g[:, 3, 3] = 0; g[:, 4, 5] = [7e-4, 0]; g[:, 5, 7] = [0, -6e-4]; g[:, 9, 0] = [-5e-4, 0]; g[:, 0, 2] = 0; g[:, -1, 4] = [3e-4, 0]
	return g

def exact_points(alm, dec, ra, lmax, spin):
	"""the oracle's synthesis on rings of one pixel at (dec, ra)"""
	n = dec.size
	kw = dict(theta=np.pi/2-dec.reshape(-1), nphi=np.ones(n, np.int64), phi0=ra.reshape(-1), ringstart=np.arange(n, dtype=np.int64), lmax=lmax)
	out = []
	for s, i1, i2 in [(0, 0, 1), (2, 1, 3)] if spin == [0, 2] else [(0, i, i+1) for i in range(len(alm))]:
		out.append(np.asarray(so.synthesis(alm=alm[i1:i2], spin=s, **kw), np.float64))
	return np.concatenate(out).reshape((len(alm),)+dec.shape)

def main():
	sht = types.ModuleType("sht_exp")
	for name in ["synthesis_2d", "adjoint_synthesis_2d", "analysis_2d", "adjoint_analysis_2d", "synthesis", "adjoint_synthesis", "get_gridweights"]:
		setattr(sht, name, getattr(so, name))
	ns = H.load_reference(sht)
	enmap, curvedsky, powspec, lensing = ns.enmap, ns.curvedsky, ns.powspec, ns.lensing
	import warnings; warnings.simplefilter("ignore")
	rng = np.random.default_rng(2024)
	out = {}
	ps_cmb, ps_lens = powspec.read_camb_scalar("/root/reference/tests/data/test_scalCls.dat")

	# ---- offset_by_grad on 10-degree grids ----
	for key, variant, sel in [("cc", "cc", None), ("f1", "fejer1", None), ("ccy", "cc", (slice(None, None, -1), slice(None))), ("ccx", "cc", (slice(None), slice(None, None, -1)))]:
		shape, wcs = enmap.fullsky_geometry(res=10*deg, variant=variant)
		if sel is not None: shape, wcs = enmap.slice_geometry(shape, wcs, sel)
		shape = tuple(int(v) for v in shape)
		pos = np.asarray(enmap.posmap(shape, wcs))
		grad = planted_grad(rng, shape)
		out["d_%s_geo" % key] = np.concatenate(geo_numbers(shape, wcs))
		out["d_%s_pos" % key] = pos; out["d_%s_grad" % key] = grad
		out["d_%s_out" % key] = lensing.offset_by_grad(pos, grad, pol=True)
		if key != "cc": continue
		out["d_cc_out_nopol"] = lensing.offset_by_grad(pos, grad, pol=False)
		psi0 = rng.uniform(-1, 1, pos.shape[1:])
		out["d_cc_psi0"] = psi0
		out["d_cc_out_psi0"] = lensing.offset_by_grad(np.concatenate([pos, psi0[None]]), grad)
		g32 = grad.astype(np.float32)
		out["d_cc_grad32"] = g32
		out["d_cc_out32"] = lensing.offset_by_grad(pos, g32.astype(np.float64), pol=True)
		gn = grad.copy()
		gn[:, 1, 3] = [-0.3, 1e-4]; gn[:, -2, 6] = [0.25, -2e-4]; gn[:, 2, 9] = [-0.36, 0]      # over the south / north / south pole (rows 1, 17, 2 are 10, 10, 20 degrees from one; row 0 is the southern one)
		out["d_cc_grad_ng"] = gn
		out["d_cc_out_ng"] = lensing.offset_by_grad(pos, gn, geodesic=False, pol=True)
	pw = np.array([[1.7, -1.6, 0.3, np.pi/2, -1.9], [0.1, 6.0, -2.0, 1.0, 3.0]])
	out["pw_in"] = pw; out["pw_out"] = lensing.pole_wrap(pw)

	# ---- the same on the reference test's 1-degree CC grid ----
	shape1, wcs1 = enmap.fullsky_geometry(res=1*deg, variant="cc")
	shape1 = tuple(int(v) for v in shape1)
	pos1 = np.asarray(enmap.posmap(shape1, wcs1))
	g1 = 1e-3*np.random.default_rng(11).random((2,)+shape1)
	out["g_geo"] = np.concatenate(geo_numbers(shape1, wcs1))
	out["g_grad_head"] = g1[:, 0, :8].copy()
	out["g_out12"] = lensing.offset_by_grad(pos1, g1, pol=True)[:, ::12]

	# ---- rotate_pol ----
	m = rng.standard_normal((2, 3, 19, 36)); ang = rng.uniform(-np.pi, np.pi, (19, 36))
	out["r_map"] = m; out["r_ang"] = ang
	for s in (0, 1, 2):
		out["r_out_s%d" % s] = np.asarray(enmap.rotate_pol(m, ang, spin=s))
		out["r_out32_s%d" % s] = np.asarray(enmap.rotate_pol(m.astype(np.float32), ang, spin=s)).astype(np.float32)

	# ---- end to end, lmax 16, CC 10 degrees ----
	shape, wcs = enmap.fullsky_geometry(res=10*deg, variant="cc")
	shape = tuple(int(v) for v in shape)
	lmax = 16; ai = curvedsky.alm_info(lmax)
	def ralm(n, scale):
		a = (rng.standard_normal((n, ai.nelem))+1j*rng.standard_normal((n, ai.nelem)))*scale
		a[:, :lmax+1] = a[:, :lmax+1].real
		return a
	cmb = ralm(3, 1.0); phi = ralm(1, 2e-4)[0]; phi[0] = 0
	grad = enmap.zeros((2,)+shape, wcs)
	curvedsky.alm2map(phi, grad, deriv=True)
	raw = lensing.offset_by_grad(enmap.posmap(shape, wcs), grad, pol=True)
	ex = exact_points(cmb, np.asarray(raw[0]), np.asarray(raw[1]), lmax, [0, 2])
	out["e_cmb"] = cmb; out["e_phi"] = phi; out["e_grad"] = np.asarray(grad)
	out["e_lensed"] = np.asarray(enmap.rotate_pol(ex, np.asarray(raw[2])))

	# ---- rand_alm ----
	nl = 25
	A = rng.standard_normal((4, 4, nl)); ps4 = np.einsum("ikl,jkl->ijl", A, A)+0.1*np.eye(4)[:, :, None]
	out["a_ps"] = ps4
	p, c, _ = lensing.rand_alm(ps4, seed=3, ncomp=3); out["a_phi"] = p; out["a_cmb"] = c
	p, c, _ = lensing.rand_alm(ps4, seed=3, phi_seed=4, ncomp=3); out["a_phi_ps"] = p; out["a_cmb_ps"] = c
	p, c, _ = lensing.rand_alm(ps4, seed=5, ncomp=1, dtype=np.float32); out["a_phi_sp"] = p; out["a_cmb_sp"] = c

	# ---- the reference's test_lensing: 1-degree CC, lmax 400, rand_alm(seed=1) ----
	data = "/root/reference/tests/data/"
	lmax = 400
	ps_in = np.zeros((4, 4, ps_cmb.shape[-1])); ps_in[0, 0] = ps_lens; ps_in[1:, 1:] = ps_cmb
	phi_alm, cmb_alm, ainfo = lensing.rand_alm(ps_in, lmax=lmax, seed=1, ncomp=3)
	out["m_ps"] = ps_in[:, :, :lmax+1].copy(); out["m_phi_sub"] = phi_alm[::64].copy()
	grad = enmap.zeros((2,)+shape1, wcs1)
	t0 = time.time(); curvedsky.alm2map(phi_alm, grad, deriv=True)
	raw = np.asarray(lensing.offset_by_grad(pos1, grad, pol=True))
	full = "--full" in sys.argv          # every row (for the comparison with the recorded map): four times the oracle time
	step = 1 if full else 4
	ex = exact_points(cmb_alm, raw[0, ::step], raw[1, ::step], lmax, [0, 2])
	lensed = np.asarray(enmap.rotate_pol(ex, raw[2, ::step]))
	print("lmax 400 expected map: %.0f s" % (time.time()-t0))
	out["m_lensed4"] = lensed[:, ::4] if full else lensed
	gold, _ = read_fits_f64(data+"MM_lensed_071123.fits")
	ok = np.isclose(lensed, gold[:, ::step])
	inner = ok[:, 1:-1] if full else ok[:, 1:]
	print("MM_lensed vs this pipeline (rows ::%d): isclose share per component: all rows %s, pole rows left out %s" % (step, ok.mean((1, 2)), inner.mean((1, 2))))
	print("   max |diff| / rms per component:", np.max(np.abs(lensed-gold[:, ::step]), (1, 2))/np.sqrt(np.mean(gold**2, (1, 2))))
	np.savez_compressed(os.path.join(HERE, "lensing.npz"), **out)
	np.savez_compressed(os.path.join(HERE, "lensing_recorded.npz"), lensed4=gold[:, ::4])
	print("lensing.npz written: %.0f kB" % (os.path.getsize(os.path.join(HERE, "lensing.npz"))/1e3))

if __name__ == "__main__":
	main()
