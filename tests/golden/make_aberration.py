"""Generate tests/golden/aberration.npz by running the REFERENCE's pixell.aberration in this container.

Run:  python tests/golden/make_aberration.py      (needs /root/reference; never run on the GPU box)

The reference is imported through _ref_harness.py with the repo's long-double oracle mounted as ducc0.sht.experimental, and with these
stand-ins for what it needs beyond that, all written here:
  numba                              njit is the identity (both call forms)
  ducc0.nufft.u2nu                   the direct trigonometric sum in numpy
  ducc0.misc.get_deflected_angles    the reference's own lensing.offset_by_grad(..., geodesic=True, pol=True) on (-d_theta, d_phi); its third
                                     output is the spin-2 phase, twice the angle the basis turns by, so gamma = half of it
  ducc0.sht.rotate_alm               oracle synthesis at the rotated positions of a CC grid followed by oracle analysis on that grid (exact
                                     for these tiny alm)
  pixell.fft                         the reference's own numpy engine
  astropy.coordinates / .units       empty modules (pixell.coordinates imports them; nothing of it is called)
Only inputs and expected outputs are saved (beta = 0.05 throughout, so that every effect is far above the tolerances):
  bf_<dir>_dpos / _mod     calc_boost_field(beta, dir, modulation=True) for dir_equ and the pole
  alm, alm2                T/E/B alm of lmax 8: the test maps are their synthesis on the Fejer-1 24 x 48 grid (full) and on its rows 2 .. 21 (band)
  ab_full, ab_band         boost_map(modulation=None): the aberrated map, every 3rd pixel; full: boundary="fullsky", band: boundary="periodic"
  ab_full2                 the same for alm2, every 23rd pixel (an Aberrator used twice)
  bo_<geo>_<mode>_<d>      boost_map with modulation T2lin / lin2T / T2T, dipole off (d = 0) and on (1), every 23rd pixel
  mo_*                     apply_modulation alone on small float32 and float64 maps, every mode, dipole off and on
  mo_spread_<dtype>        per mode and dipole: max |reference - long double| / max |long double|, the long-double evaluation of the same
                           formulas being made here
  cov_resid                the covariance check of tests/test_aberration.py (sign of the rotation), evaluated with the stand-ins above:
                           max |X - Y| / max |X|

The continuation over the pole (boundary="fullsky") is made here, not by the reference: its interpol_map writes
np.roll(imap[...,::-1], nx//2, -1), which reverses the map's columns where the rows beyond a pole are the rows before it in reverse
order, half a turn away.  The generator builds that doubled map itself and hands it to the reference's interpol_map as a periodic
one.  The covariance check tells the two apart: it holds to rounding with this continuation and fails at the 17 % level with the
reference's own (cov_resid_literal).

As run for the committed fixture (13 seconds):
  covariance residual (CPU stand-ins): 1.35e-13; with the reference's own doubling: 1.66e-01
  modulation spread float64 (T2lin, lin2T, T2T, lin2lin; dipole off, on): 1.1e-12 8.0e-15 9.5e-13 6.7e-15 5.8e-17 1.2e-16 1.2e-12 9.0e-15
  modulation spread float32:                                              2.7e-08 3.8e-08 3.1e-08 3.0e-08 3.1e-08 3.5e-08 4.7e-08 2.9e-08
  file size: 81224 bytes
"""
import sys, os, types
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, HERE)
from oracle import sht_oracle as so
import _ref_harness as H

BETA = 0.05
MODES = ("T2lin", "lin2T", "T2T")
SUB, SUB_AB = 23, 3      # every SUB-th pixel of the modulated maps, every SUB_AB-th of the aberrated ones

def load():
	sht = types.ModuleType("sht_exp")
	for name in ["synthesis_2d", "adjoint_synthesis_2d", "analysis_2d", "adjoint_analysis_2d", "synthesis", "adjoint_synthesis", "get_gridweights"]:
		setattr(sht, name, getattr(so, name))
	def njit(*a, **k):
		if len(a) == 1 and callable(a[0]) and not k: return a[0]
		return lambda f: f
	sys.modules["numba"] = types.ModuleType("numba"); sys.modules["numba"].njit = njit
	ns = H.load_reference(sht)
	import ducc0
	for name in ("astropy.coordinates", "astropy.units"): sys.modules[name] = types.ModuleType(name)
	sys.modules["astropy"].coordinates = sys.modules["astropy.coordinates"]; sys.modules["astropy"].units = sys.modules["astropy.units"]
	ducc0.nufft.u2nu = u2nu
	ducc0.misc = types.ModuleType("ducc0.misc"); sys.modules["ducc0.misc"] = ducc0.misc
	ducc0.misc.get_deflected_angles = lambda **kw: get_deflected_angles(ns.lensing, **kw)
	ducc0.sht.rotate_alm = rotate_alm
	ns.fft.set_engine("numpy")      # (enmap.fft of the reference's interpol_map: ducc0.fft is absent)
	from pixell import aberration
	ns.aberration = aberration
	ns.interpol_map = aberration.interpol_map
	return ns

def doubled_interpol(ns):
	"""aberration.interpol_map with the map continued over the pole by the generator: row ny + r is row ny - 1 - r half a turn away.  The
	reference writes np.roll(imap[...,::-1], nx//2, -1), which reverses x, not y (see the covariance residuals below)."""
	def interpol_map(imap, pixs, epsilon=None, nthread=None, ydouble=False):
		if not ydouble: return ns.interpol_map(imap, pixs, epsilon=epsilon, nthread=nthread)
		ny, nx = imap.shape[-2:]
		dmap = ns.enmap.zeros(imap.shape[:-2]+(2*ny, nx), imap.wcs, imap.dtype)
		dmap[..., :ny, :] = imap
		dmap[..., ny:, :] = np.roll(imap[..., ::-1, :], nx//2, -1)
		return ns.interpol_map(dmap, pixs, epsilon=epsilon, nthread=nthread)
	return interpol_map

def kfreq(n):
	j = np.arange(n)
	return np.where(j <= (n-1)//2, j, j-n)

def u2nu(*, grid, coord, forward, epsilon, nthreads, periodicity, fft_order):
	assert fft_order and not forward
	n1, n2 = grid.shape
	e1 = np.exp(2j*np.pi*np.outer(coord[:, 0], kfreq(n1))/periodicity[0])
	e2 = np.exp(2j*np.pi*np.outer(coord[:, 1], kfreq(n2))/periodicity[1])
	return np.einsum("pa,ab,pb->p", e1, grid, e2)

def get_deflected_angles(lensing, *, theta, phi0, nphi, dphi, ringstart, nthreads, calc_rotation, deflect):
	npix = int(np.sum(nphi))
	ipos = np.zeros((2, npix))
	for r in range(len(theta)):
		sl = slice(int(ringstart[r]), int(ringstart[r])+int(nphi[r]))
		ipos[0, sl] = np.pi/2-theta[r]; ipos[1, sl] = phi0[r]+np.arange(int(nphi[r]))*dphi[r]
	grad = np.array([-deflect[:, 0], deflect[:, 1]])
	opos = lensing.offset_by_grad(ipos, grad, geodesic=True, pol=True)
	return np.array([np.pi/2-opos[0], opos[1], 0.5*opos[2]]).T

def rotate_alm(alm, lmax, psi, theta, phi, nthreads=0):
	"""f'(n) = f(R^-1 n), R = R_z(phi) R_y(theta) R_z(psi): f at the turned positions of a CC grid, analysed on that grid"""
	nt, nph = lmax+2, 2*lmax+2
	th = np.arange(nt)*np.pi/(nt-1); ph = np.arange(nph)*2*np.pi/nph
	T, P = np.meshgrid(th, ph, indexing="ij")
	n = np.array([np.sin(T)*np.cos(P), np.sin(T)*np.sin(P), np.cos(T)]).reshape(3, -1)
	def rz(a): return np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
	def ry(a): return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
	m = (rz(phi) @ ry(theta) @ rz(psi)).T @ n
	t2, p2 = np.arctan2(np.hypot(m[0], m[1]), m[2]), np.arctan2(m[1], m[0])
	npt = t2.size
	vals = so.synthesis(alm=np.asarray(alm)[None], spin=0, theta=t2, nphi=np.ones(npt, np.int64), phi0=p2, ringstart=np.arange(npt, dtype=np.int64), lmax=lmax)
	out = so.analysis_2d(map=np.asarray(vals, np.float64).reshape(1, nt, nph), spin=0, lmax=lmax, geometry="CC")
	return np.asarray(out, np.complex128)[0]

# ---- the modulation in long double ---------------------------------------------------------------------------------------------------
def modulate_ld(utils, m, a, mode, dipole, spin0, T0, freq, unit):
	ld = np.longdouble
	h, c, k = ld(utils.h), ld(utils.c), ld(utils.k)
	f, T0, unit = ld(freq), ld(T0), ld(unit)
	V = 2*h*f*f*f/c**2*ld(1e26)
	def planck(T): return V/np.expm1(h*f/(k*T))
	def iplanck(I): return h*f/k/np.log1p(V/I)
	x0 = h*f/(k*T0)
	scale = 2*x0**4*k**3*T0**2/(h**2*c**2)/(4*np.sinh(x0/2)**2)*ld(1e26)
	m = np.asarray(m).astype(ld); a = np.asarray(a).astype(ld)
	out = np.empty_like(m)
	def t2lin(v, a, mono): return (planck(a*(v*unit+T0))-(planck(T0) if mono else planck(a*T0)))/scale/unit
	def lin2t(v, a, mono): return (iplanck(v*unit*scale+(planck(T0) if mono else planck(T0/a)))*a-ld(utils.T_cmb))/unit
	for ci in range(m.shape[0]):
		mono = bool(dipole and spin0[ci])
		if mode == "T2T": out[ci] = m[ci]*a+((a-1)*(T0/unit) if dipole and ci == 0 else 0)
		elif mode == "T2lin": out[ci] = t2lin(m[ci], a, mono)
		elif mode == "lin2T": out[ci] = lin2t(m[ci], a, mono)
		else: out[ci] = t2lin(lin2t(m[ci], 1+0*a, mono), a, mono)
	return out

def main():
	ns = load()
	enmap, curvedsky, ab, utils = ns.enmap, ns.curvedsky, ns.aberration, ns.utils
	def covariance(alm):
		"""the check of tests/test_aberration.py: aberrating towards d the sky turned to d = turning to d the sky aberrated towards the pole"""
		d, pole = ab.dir_equ, np.array([0.0, np.pi/2])
		shape, wcs = enmap.fullsky_geometry(shape=(24, 48), dims=(3,))
		rot = lambda a: curvedsky.rotate_alm(a.copy(), 0, np.pi/2-d[1], d[0])
		X = ab.aberrate_map(curvedsky.alm2map(rot(alm), enmap.zeros(shape, wcs)), dir=d, beta=BETA, boundary="fullsky")
		P = ab.aberrate_map(curvedsky.alm2map(alm, enmap.zeros(shape, wcs)), dir=pole, beta=BETA, boundary="fullsky")
		Y = curvedsky.alm2map(rot(curvedsky.map2alm(P, lmax=20)), enmap.zeros(shape, wcs))
		return float(np.abs(np.asarray(X)-np.asarray(Y)).max()/np.abs(np.asarray(X)).max())
	import warnings; warnings.simplefilter("ignore")
	rng = np.random.default_rng(77)
	out = {}
	pole = np.array([0.0, np.pi/2])
	for key, d in (("equ", ab.dir_equ), ("pole", pole)):
		alm, malm = ab.calc_boost_field(BETA, d, modulation=True)
		out["bf_%s_dpos" % key] = alm; out["bf_%s_mod" % key] = malm
	# ---- maps ----
	lmax = 8
	ai = curvedsky.alm_info(lmax)
	def draw():
		a = (rng.standard_normal((3, ai.nelem))+1j*rng.standard_normal((3, ai.nelem)))*100
		a[:, :lmax+1] = a[:, :lmax+1].real
		for l, m in ((0, 0), (1, 0), (1, 1)): a[1:, ai.lm2ind(l, m)] = 0
		return a
	alm, alm2 = draw(), draw()
	cov_literal = covariance(alm)
	ab.interpol_map = doubled_interpol(ns)
	cov = covariance(alm)
	out["alm"] = alm; out["alm2"] = alm2
	shape, wcs = enmap.fullsky_geometry(shape=(24, 48), dims=(3,))
	full = curvedsky.alm2map(alm, enmap.zeros(shape, wcs))
	full2 = curvedsky.alm2map(alm2, enmap.zeros(shape, wcs))
	band = full[:, 2:22]
	assert band.shape == (3, 20, 48)
	out["geo_full"] = np.concatenate([[24, 48], wcs.wcs.cdelt, wcs.wcs.crval, wcs.wcs.crpix])
	out["geo_band"] = np.concatenate([[20, 48], band.wcs.wcs.cdelt, band.wcs.wcs.crval, band.wcs.wcs.crpix])
	sub = lambda m, step: np.asarray(m).reshape(3, -1)[:, ::step].copy()
	for key, m, bnd in (("full", full, "fullsky"), ("band", band, "periodic")):
		res = ab.boost_map(m.copy(), beta=BETA, modulation=None, boundary=bnd)
		out["ab_"+key] = sub(res, SUB_AB)
		assert np.array_equal(np.asarray(res), np.asarray(ab.boost_map(m.copy(), beta=BETA, modulation=None, dipole=True, boundary=bnd)))
		for mode in MODES:
			for dip in (0, 1):
				out["bo_%s_%s_%d" % (key, mode, dip)] = sub(ab.boost_map(m.copy(), beta=BETA, modulation=mode, dipole=bool(dip), boundary=bnd), SUB)
	out["ab_full2"] = sub(ab.aberrate_map(full2.copy(), beta=BETA, boundary="fullsky"), SUB)
	# ---- the modulation alone ----
	mshape, mwcs = enmap.fullsky_geometry(shape=(6, 8), dims=(3,))
	m64 = 300*rng.standard_normal(mshape); a64 = 1+BETA*rng.uniform(-1, 1, mshape[-2:])
	out["mo_map"] = m64; out["mo_A"] = a64
	spreads = {}
	for dt, tag in ((np.float64, "64"), (np.float32, "32")):
		spread = []
		for mode in MODES+("lin2lin",):
			for dip in (0, 1):
				m = enmap.ndmap(m64.astype(dt), mwcs); a = enmap.ndmap(a64.astype(dt), mwcs)
				res = np.asarray(ab.apply_modulation(m.copy(), a, mode=mode, dipole=bool(dip)))
				assert res.dtype == dt
				out["mo_%s_%s_%d" % (tag, mode, dip)] = res
				truth = modulate_ld(utils, m, a, mode, dip, [True, False, False], utils.T_cmb, 150e9, 1e-6)
				spread.append(float(np.abs(res-truth).max()/np.abs(truth).max()))
		spreads[tag] = np.array(spread); out["mo_spread_"+tag] = spreads[tag]
	out["cov_resid"] = np.array(cov); out["cov_resid_literal"] = np.array(cov_literal)
	path = os.path.join(HERE, "aberration.npz")
	np.savez(path, **out)
	print("covariance residual (CPU stand-ins): %.2e; with the reference's own doubling: %.2e" % (cov, cov_literal))
	for tag in ("64", "32"): print("modulation spread float%s:" % tag, " ".join("%.1e" % v for v in spreads[tag]))
	print("file size: %d bytes" % os.path.getsize(path))

if __name__ == "__main__":
	main()
