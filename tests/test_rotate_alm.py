"""curvedsky.rotate_alm / sht.rotate_alm (curvedsky.py:714-740 of the reference; ducc0.sht.rotate_alm): Euler-angle rotation of alm.
The convention is pinned without any Wigner formula: the rotated alm evaluated at n must equal the original evaluated at R^-1 n,
R = R_z(phi) R_y(theta) R_z(psi), both through one-pixel rings of sht.synthesis (and, in the simulator, of the long-double oracle).
Small sizes run in the test-only host simulator, the same bodies and the full sizes on the GPU."""
import numpy as np
import pytest
from pixell_amd import curvedsky, sht
from oracle import sht_oracle as so

def Rz(a): c, s = np.cos(a), np.sin(a); return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])
def Ry(a): c, s = np.cos(a), np.sin(a); return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
def rotmat(psi, theta, phi): return Rz(phi) @ Ry(theta) @ Rz(psi)
def nalm(lmax): return (lmax+1)*(lmax+2)//2
def lvals(lmax): return np.concatenate([np.arange(m, lmax+1) for m in range(lmax+1)])
def mvals(lmax): return np.concatenate([np.full(lmax+1-m, m) for m in range(lmax+1)])

def rand_alm(lmax, ncomp=1, seed=0, dtype=np.complex128):
	rng = np.random.default_rng(seed)
	a = rng.standard_normal((ncomp, nalm(lmax))) + 1j*rng.standard_normal((ncomp, nalm(lmax)))
	a[:, :lmax+1] = a[:, :lmax+1].real               # m = 0 of a real field
	return a.astype(dtype)

def rand_dirs(n, seed=1):
	v = np.random.default_rng(seed).standard_normal((n, 3)); return v/np.linalg.norm(v, axis=1)[:, None]

def to_angles(v): return np.arccos(np.clip(v[:, 2], -1, 1)), np.arctan2(v[:, 1], v[:, 0])

def evaluate(alm, lmax, v, oracle=False):
	"""f(n_i) for the spin-0 alm[1, nelem] at the unit vectors v[n, 3]: one ring of one pixel per direction"""
	th, ph = to_angles(v); n = len(th)
	kw = dict(alm=np.asarray(alm, np.complex128).reshape(1, -1), theta=th, nphi=np.ones(n, np.int64), phi0=ph, ringstart=np.arange(n, dtype=np.int64),
		lmax=lmax, spin=0, map=np.zeros((1, n)))
	return (so if oracle else sht).synthesis(**kw)[0]

ANGLES = [(0.3, 1.1, -0.7), (2.5, 1e-7, -1.3), (-0.4, np.pi - 1e-6, 0.9), (-2.0, -0.8, -3.0), (0.0, np.pi, 0.0)]

# --------------------------------------------------------------------------------------------------------------------------------
def point_eval_body(lmax, npts, angles=ANGLES, oracle=False, tol=1e-11):
	a = rand_alm(lmax, seed=lmax)
	v = rand_dirs(npts, seed=lmax + 1)
	for psi, theta, phi in angles:
		r = curvedsky.rotate_alm(a, psi, theta, phi)
		R = rotmat(psi, theta, phi)
		src = v @ R                                           # rows: R^-1 n = R^T n
		for orc in ([False, True] if oracle else [False]):
			f1 = evaluate(r, lmax, v, orc); f0 = evaluate(a, lmax, src, orc)
			err = np.max(np.abs(f1 - f0))/np.sqrt(np.mean(f0**2))
			assert err < tol, "lmax %d angles %s oracle %s: %.2e" % (lmax, (psi, theta, phi), orc, err)

def convention_body(lmax=64):
	eq = curvedsky.euler_angs[("gal", "equ")]
	R = rotmat(*eq)
	for v, (ra, dec) in [(np.array([0, 0, 1.0]), (192.859, 27.128)), (np.array([1.0, 0, 0]), (266.405, -28.936))]:
		w = R @ v
		got_ra = np.degrees(np.arctan2(w[1], w[0])) % 360; got_dec = np.degrees(np.arcsin(w[2]))
		assert abs(got_ra - ra) < 0.01 and abs(got_dec - dec) < 0.01
	np.testing.assert_allclose(curvedsky.euler_angs[("equ", "gal")], -eq[::-1])
	np.testing.assert_allclose(rotmat(*curvedsky.euler_angs[("equ", "gal")]) @ R, np.eye(3), atol=1e-14)
	# a Gaussian beam on the pole, rotated gal -> equ, peaks at the galactic pole's equatorial position
	sigma = np.radians(4.0); l = np.arange(lmax+1)
	a = np.zeros((1, nalm(lmax)), np.complex128)
	a[0, :lmax+1] = np.exp(-0.5*l*(l+1)*sigma**2)*np.sqrt((2*l+1)/(4*np.pi))
	check_peak(curvedsky.rotate_alm(a, *eq), lmax, np.radians(192.859), np.radians(27.128), evaluate(a, lmax, np.array([[0, 0, 1.0]]))[0])

def check_peak(alm, lmax, ra, dec, peak, step=np.radians(0.5), tol=1e-3):
	c = np.array([np.cos(dec)*np.cos(ra), np.cos(dec)*np.sin(ra), np.sin(dec)])
	e1 = np.cross([0, 0, 1.0], c); e1 /= np.linalg.norm(e1); e2 = np.cross(c, e1)
	ang = np.linspace(0, 2*np.pi, 8, endpoint=False)
	ring = np.cos(step)*c + np.sin(step)*(np.cos(ang)[:, None]*e1 + np.sin(ang)[:, None]*e2)
	vals = evaluate(alm, lmax, np.vstack([c, ring]))
	assert abs(vals[0] - peak) < tol*abs(peak), (vals[0], peak)
	assert np.all(vals[1:] < vals[0])

def prof2alm_body():
	# the reference's prof2alm(dir=[ra, dec]) is rotate_alm(prof2alm(p), 0, pi/2 - dec, ra) (curvedsky.py:578)
	n = 49
	theta = so.grid_theta("CC", n)
	prof = np.exp(-0.5*(theta/np.radians(8.0))**2)
	alm = curvedsky.prof2alm(prof)
	lmax = curvedsky.nalm2lmax(alm.shape[-1])
	peak = evaluate(alm, lmax, np.array([[0, 0, 1.0]]))[0]
	for ra, dec in [(1.2, 0.4), (-2.0, -1.1), (0.3, 0.0)]:
		check_peak(curvedsky.rotate_alm(alm, 0, np.pi/2 - dec, ra), lmax, ra, dec, peak)

def closed_forms_body(lmax, ncomp=3, tol=1e-10, big=False):
	"""theta = pi -> (-1)^l conj(a); theta = 0 -> e^{-im(psi+phi)} a; rotation followed by its inverse -> a; spectra unchanged"""
	if big:
		import torch
		g = torch.Generator(device="cuda").manual_seed(5)
		a = torch.randn((ncomp, nalm(lmax)), dtype=torch.complex128, device="cuda", generator=g)
		a[:, :lmax+1] = a[:, :lmax+1].real.to(torch.complex128)
		xp = torch; ls = torch.as_tensor(lvals(lmax), device="cuda"); ms = torch.as_tensor(mvals(lmax), dtype=torch.float64, device="cuda")
		amax = float(a.abs().max())
		def mx(x): return float(x.abs().max())
	else:
		a = rand_alm(lmax, ncomp, seed=3); xp = np; ls = lvals(lmax); ms = mvals(lmax); amax = np.max(np.abs(a))
		def mx(x): return float(np.max(np.abs(x)))
	sgn = 1 - 2*(ls % 2)
	r = curvedsky.rotate_alm(a, 0.0, np.pi, 0.0)
	assert mx(r - sgn*a.conj()) < tol*amax
	r = curvedsky.rotate_alm(a, 0.4, 0.0, -1.3)
	assert mx(r - xp.exp(-1j*ms*(0.4 - 1.3))*a) < tol*amax
	for psi, theta, phi in [(0.3, 1.1, -0.7), tuple(curvedsky.euler_angs[("gal", "equ")])]:
		r = curvedsky.rotate_alm(a, psi, theta, phi)
		back = curvedsky.rotate_alm(r, -phi, -theta, -psi)
		assert mx(back - a) < tol*amax, mx(back - a)/amax
		ainfo = curvedsky.alm_info(lmax)
		cl0 = ainfo.alm2cl(a[:, None], a[None, :]); cl1 = ainfo.alm2cl(r[:, None], r[None, :])
		for i, j in [(0, 0), (1, 1), (2, 2), (0, 1)][:(4 if ncomp >= 3 else 1)]:
			c0, c1 = cl0[i, j], cl1[i, j]
			scale = xp.sqrt(cl0[i, i]*cl0[j, j])
			assert mx((c1 - c0)/scale) < 1e-11, (i, j, mx((c1 - c0)/scale))

def api_body(lmax=24):
	a = rand_alm(lmax, 6, seed=11)
	ang = (0.7, 2.1, -0.3)
	ref = np.stack([curvedsky.rotate_alm(a[i], *ang) for i in range(6)])
	assert ref.shape == a.shape and ref.dtype == np.complex128
	same = lambda x, y: np.testing.assert_allclose(x, y, rtol=0, atol=1e-13)     # batching changes no arithmetic of a component
	same(curvedsky.rotate_alm(a[:3], *ang), ref[:3])
	same(curvedsky.rotate_alm(a.reshape(2, 3, -1), *ang), ref.reshape(2, 3, -1))
	same(sht.rotate_alm(a[0], lmax, *ang), ref[0])
	same(sht.rotate_alm(a[:3], lmax, *ang, nthreads=4), ref[:3])
	for method in ["auto", "ducc0", "healpy"]:
		np.testing.assert_array_equal(curvedsky.rotate_alm(a[0], *ang, lmax=lmax, method=method, nthread=3), ref[0])
	# complex64 in, complex64 out, FP64 arithmetic inside
	s = curvedsky.rotate_alm(a[:3].astype(np.complex64), *ang)
	assert s.dtype == np.complex64
	assert np.max(np.abs(s - ref[:3])) < 1e-5*np.max(np.abs(ref[:3]))
	# inplace or not
	b = a[:3].copy(); b0 = b.copy()
	r = curvedsky.rotate_alm(b, *ang)
	assert r is not b and np.array_equal(b, b0)
	r = curvedsky.rotate_alm(b, *ang, inplace=True)
	assert r is b; same(b, ref[:3])
	nc = np.asfortranarray(a[:3].T).T.copy(order="F")         # not C-contiguous, written in place all the same
	r = curvedsky.rotate_alm(nc, *ang, inplace=True)
	assert r is nc; same(nc, ref[:3])
	# layouts and names the rotation does not accept
	with pytest.raises(ValueError): curvedsky.rotate_alm(a[0], *ang, lmax=lmax - 1)
	with pytest.raises(ValueError): curvedsky.rotate_alm(a[0, :-1], *ang)
	with pytest.raises(ValueError): curvedsky.rotate_alm(np.zeros((lmax+1)**2, np.complex128), *ang)
	with pytest.raises(ValueError): curvedsky.rotate_alm(a[0], *ang, method="libsharp")
	with pytest.raises(ValueError): curvedsky.rotate_alm(a[0], *ang, method=None)
	with pytest.raises(ValueError): sht.rotate_alm(a[0], lmax + 1, *ang)

def tensor_body(lmax=24, device="cuda"):
	import torch
	a = rand_alm(lmax, 3, seed=12); ang = (-1.1, 0.6, 2.2)
	ref = curvedsky.rotate_alm(a, *ang)
	t = torch.from_numpy(a.copy()).to(device)
	r = curvedsky.rotate_alm(t, *ang)
	assert torch.is_tensor(r) and r.device == t.device and r is not t
	np.testing.assert_array_equal(r.cpu().numpy(), ref)
	assert np.array_equal(t.cpu().numpy(), a)
	r = curvedsky.rotate_alm(t, *ang, inplace=True)
	assert r is t and np.array_equal(t.cpu().numpy(), ref)
	r = sht.rotate_alm(torch.from_numpy(a[0].astype(np.complex64)).to(device), lmax, *ang)
	assert r.dtype == torch.complex64 and np.max(np.abs(r.cpu().numpy() - ref[0])) < 1e-5*np.max(np.abs(ref[0]))

# --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.hostsim
def test_point_evaluation_hostsim(): point_eval_body(40, 120, oracle=True)
@pytest.mark.hostsim
def test_convention_hostsim(): convention_body()
@pytest.mark.hostsim
def test_prof2alm_direction_hostsim(): prof2alm_body()
@pytest.mark.hostsim
def test_closed_forms_hostsim(): closed_forms_body(48)
@pytest.mark.hostsim
def test_api_hostsim(): api_body()
@pytest.mark.hostsim
def test_tensor_hostsim(): tensor_body(device="cpu")

@pytest.mark.gpu
def test_point_evaluation_gpu(): point_eval_body(40, 300)
@pytest.mark.gpu
def test_point_evaluation_gpu_lmax2000(): point_eval_body(2000, 300)
@pytest.mark.gpu
def test_point_evaluation_gpu_lmax10000():
	# near the identity both evaluations use (almost) the same rings, so the one-pixel-ring synthesis errors cancel: the rotation's own
	# error (measured 1.3e-11).  At generic angles the two sides are evaluated on different rings and the comparison carries the
	# synthesis error at lmax 10000 as well (measured 4.6e-10, median 9e-12; profiles/r07_rotate_accuracy_lmax10000.txt)
	point_eval_body(10000, 200, angles=[ANGLES[1]], tol=3e-11)
	point_eval_body(10000, 200, angles=[ANGLES[0], ANGLES[2]], tol=1e-9)
@pytest.mark.gpu
def test_convention_gpu(): convention_body()
@pytest.mark.gpu
def test_prof2alm_direction_gpu(): prof2alm_body()
@pytest.mark.gpu
def test_closed_forms_gpu(): closed_forms_body(48)
@pytest.mark.gpu
def test_closed_forms_gpu_lmax10000(): closed_forms_body(10000, big=True)
@pytest.mark.gpu
def test_api_gpu(): api_body()
@pytest.mark.gpu
def test_tensor_gpu(): tensor_body()
