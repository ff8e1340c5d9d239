"""The transform families of pixell_amd.curvedsky -- cyl rings, healpix rings, points -- where no other test looks: DERIV1 adjoints,
map2alm_raw_general(deriv=True) and the write-back into alm whose slices are strided views.  Under ordered sums every call is compared
BITWISE with the same result composed here from sht.synthesis / adjoint_synthesis / synthesis_general / adjoint_synthesis_general, one
library call per pre-index and spin group, as the reference's loops make them (curvedsky.py:910-924, 936-960, 1067-1084, 1098-1115).

The sign rule of the gradient maps [d/ddec, d/dra / cos dec], written out:
  * forward (alm -> map): the library returns d/dtheta; component 0 of the OUTPUT is negated after the call, in every family;
  * adjoint, cyl and healpix: NO sign is applied, the input map goes to the library as it is (so this is not the transpose of the
    forward call) and is left as it was;
  * adjoint, points: component 0 of a COPY of the input is negated before the call -- the exact transpose -- and the input is left as
    it was.
The reference negates the caller's map after the adjoint call instead; the difference is deliberate."""
import numpy as np
import pytest
from pixell_amd import curvedsky, enmap, sht, _lib, wcs as wcsutils

LMAX = 8; NELEM = (LMAX+1)*(LMAX+2)//2
SIGN = np.array([-1.0, 1.0])[:, None]                     # on [2, pixels]: d/dtheta <-> d/ddec
GROUPS = [(0, slice(0, 1)), (2, slice(1, 3))]             # spin=[0, 2] on three components

def _put(kind, x):
	"""a contiguous array of the kind under test: numpy, or a tensor where the library reads tensors"""
	x = np.ascontiguousarray(x)
	if kind == "numpy": return x
	import torch
	t = torch.from_numpy(x.copy())
	return t if _lib.is_hostsim() else t.cuda()

def _host(x):
	x = getattr(x, "tensor", x)
	return x.detach().cpu().numpy() if type(x).__module__.startswith("torch") else np.asarray(x)

def _same(a, b): return _host(a).shape == _host(b).shape and np.array_equal(_host(a), _host(b))

def _rand_alm(rng, shape): return rng.standard_normal(shape)+1j*rng.standard_normal(shape)

class _Cyl:
	"""the rows of a CAR map as rings, the way alm2map_cyl hands them to the library: the ring tables of the map flipped into ducc's
	orientation, the stored order expressed as a descending ringstart / negative pixel stride"""
	signed_adjoint = False
	def __init__(self, shape, wcs):
		self.pix = tuple(shape[-2:]); self.wcs = wcs; ny, nx = self.pix
		flip = curvedsky.analyse_geometry(shape, wcs).flip
		rinfo = curvedsky.get_ring_info(*curvedsky.flip_geometry(shape, wcs, flip))
		rows = np.arange(ny)[::-1] if flip[0] else np.arange(ny)
		self.kw = dict(theta=rinfo.theta, nphi=rinfo.nphi, phi0=rinfo.phi0, ringstart=(rows*nx+(nx-1 if flip[1] else 0)).astype(np.uint64),
			pixstride=-1 if flip[1] else 1, lmax=LMAX)
	def syn(self, alm, **k): return sht.synthesis(alm=alm, **k, **self.kw).reshape((-1,)+self.pix)
	def adj(self, m, **k): return sht.adjoint_synthesis(map=m.reshape(m.shape[0], -1), **k, **self.kw)
	def alm2map(self, kind, alm, m, **k):
		return curvedsky.alm2map_cyl(alm, enmap.ndmap(m, self.wcs) if kind == "numpy" else enmap.dmap(m, self.wcs), spin=[0, 2], **k)

class _Healpix:
	signed_adjoint = False
	def __init__(self, nside):
		r = curvedsky.get_ring_info_healpix(nside); self.pix = (12*nside**2,)
		self.kw = dict(theta=r.theta, nphi=r.nphi, phi0=r.phi0, ringstart=r.offsets, lmax=LMAX)
	def syn(self, alm, **k): return sht.synthesis(alm=alm, **k, **self.kw)
	def adj(self, m, **k): return sht.adjoint_synthesis(map=m, **k, **self.kw)
	def alm2map(self, kind, alm, m, **k): return curvedsky.alm2map_healpix(alm, m, spin=[0, 2], **k)

class _Points:
	signed_adjoint = True
	def __init__(self, kind, npts):
		r = np.random.RandomState(5); self.pix = (npts,)
		self.loc = _put(kind, np.stack([np.arccos(r.uniform(-1, 1, npts)), r.uniform(0, 2*np.pi, npts)], -1))
	def syn(self, alm, **k): return sht.synthesis_general(alm=alm, loc=self.loc, lmax=LMAX, **k)
	def adj(self, m, **k): return sht.adjoint_synthesis_general(map=m, loc=self.loc, lmax=LMAX, **k)
	def alm2map(self, kind, alm, m, **k): return curvedsky.alm2map_raw_general(alm, m, self.loc, spin=[0, 2], **k)

def _family(name, kind):
	shape, wcs = enmap.fullsky_geometry(shape=(12, 20))
	if name == "cyl_full": return _Cyl(shape, wcs)
	if name == "cyl_band": return _Cyl(*wcsutils.slice_geometry(shape, wcs, (slice(3, 10), slice(None))))
	if name == "healpix": return _Healpix(4)
	return _Points(kind, 37)

def direct_body(name, kind):
	"""alm2map of the family: DERIV1 forward and adjoint, and the adjoint of spin groups into a strided alm"""
	fam = _family(name, kind); rng = np.random.RandomState(11)
	# forward with deriv, two pre-dimension entries: the output's declination component is negated after the call
	alm = _rand_alm(rng, (2, NELEM)); out = _put(kind, rng.standard_normal((2, 2)+fam.pix))
	res = fam.alm2map(kind, _put(kind, alm), out, deriv=True)
	for i in range(2):
		want = _host(fam.syn(_put(kind, alm[i][None]), spin=1, mode="DERIV1"))*SIGN.reshape((2,)+(1,)*len(fam.pix))
		assert _same(out[i], want) and _same(_host(res)[i], want)
	# adjoint with deriv into an alm whose rows are every other element of their memory: the sign rule of the module docstring
	m = rng.standard_normal((2, 2)+fam.pix); base0 = _rand_alm(rng, (2, 2*NELEM))
	base = _put(kind, base0); md = _put(kind, m)
	res = fam.alm2map(kind, base[:, ::2], md, deriv=True, adjoint=True)
	for i in range(2):
		m_in = m[i]*SIGN.reshape((2,)+(1,)*len(fam.pix)) if fam.signed_adjoint else m[i]
		want = fam.adj(_put(kind, m_in), spin=1, mode="DERIV1")
		assert _same(base[i, ::2], _host(want)[0]) and _same(_host(res)[i], _host(want)[0])
	assert _same(md, m) and _same(base[:, 1::2], base0[:, 1::2])               # the input map and the memory between the elements: untouched
	# adjoint of the spin groups into an alm that is every other component of its memory: a group's slice is strided, the library
	# writes a contiguous staging copy and the result is written back through the view
	m = rng.standard_normal((2, 3)+fam.pix); base0 = _rand_alm(rng, (2, 6, NELEM))
	base = _put(kind, base0); md = _put(kind, m)
	res = fam.alm2map(kind, base[:, ::2], md, adjoint=True)
	for i in range(2):
		for s, sel in GROUPS:
			want = fam.adj(_put(kind, m[i, sel]), spin=s)
			assert _same(base[i, ::2][sel], want) and _same(_host(res)[i, sel], want)
	assert _same(md, m) and _same(base[:, 1::2], base0[:, 1::2])

def solver_deriv_body(kind):
	"""map2alm_raw_general(deriv=True), forward and adjoint, niter 0 and 1, against the Jacobi iteration written out:
	x_0 = B y, x_1 = x_0 + B (y - F x_0) with F the synthesis and B the weighted adjoint synthesis (adjoint: F and B the transposes)"""
	fam = _family("points", kind); rng = np.random.RandomState(12); npts = fam.pix[0]
	w0 = np.linspace(0.5, 1.5, npts); w = _put(kind, w0); sg = _put(kind, SIGN)
	def Y(a):  return fam.syn(a, spin=1, mode="DERIV1")
	def YT(m): return fam.adj(m, spin=1, mode="DERIV1")
	for niter in (0, 1):
		m = rng.standard_normal((2, 2, npts)); alm = _put(kind, _rand_alm(rng, (2, NELEM)))
		res = curvedsky.map2alm_raw_general(_put(kind, m), fam.loc, alm, deriv=True, niter=niter, weights=w0)
		for i in range(2):
			y = _put(kind, m[i])*sg                                     # d/ddec -> d/dtheta, on a copy
			x = YT(y*w)
			for _ in range(niter): x = x+YT((y-Y(x))*w)
			assert _same(alm[i], _host(x)[0]) and _same(_host(res)[i], _host(x)[0])
		a = _rand_alm(rng, (2, NELEM)); out = _put(kind, rng.standard_normal((2, 2, npts)))
		res = curvedsky.map2alm_raw_general(out, fam.loc, _put(kind, a), deriv=True, adjoint=True, niter=niter, weights=w0)
		for i in range(2):
			y = _put(kind, a[i][None])
			x = Y(y)*w
			for _ in range(niter): x = x+Y(y-YT(x))*w
			assert _same(out[i], x*sg) and _same(_host(res)[i], x*sg)

FAMILIES = ["cyl_full", "cyl_band", "healpix", "points"]; KINDS = ["numpy", "device"]

def _ordered(body, *args):
	sht.set_deterministic(True)      # (the Legendre analysis of an adjoint repeats bit for bit only with ordered sums)
	try: body(*args)
	finally: sht.set_deterministic(None)

@pytest.mark.hostsim
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", FAMILIES)
def test_direct_sim(name, kind): _ordered(direct_body, name, kind)

@pytest.mark.hostsim
@pytest.mark.parametrize("kind", KINDS)
def test_solver_deriv_sim(kind): _ordered(solver_deriv_body, kind)

@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", FAMILIES)
def test_direct_gpu(name, kind): _ordered(direct_body, name, kind)

@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_solver_deriv_gpu(kind): _ordered(solver_deriv_body, kind)
