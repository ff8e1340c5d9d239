"""The VALU Legendre analysis with more ring pairs per lane: leg_ana_spin<6>, which the host's rule (leg_ana_k, legendre.hip) takes where the ring set gives at
least 8 waves per m at the default K = 4 (spin 0 stays at K = 8: asserted), and plan option "leg_ana_k", which forces a K for tests (plan query "leg_ana_k": the K
of the last analysis).  A larger K changes the pair map (leg_pair_of), the wave count and with it the partial-moment layout, first[], the seeds and the blocks per
m; what it must not change is the result.  Tolerance 1e-11 (test_grid_gpu's).  TEST_K: spin 2 K = 6, the new kernel; spin 0 K = 8, forced the same way.
Legendre-only calls on explicit equidistant ring sets with nphi = 8 (cases, reference -- the C port of the long-double oracle on a mirror-symmetric subset of the
rings -- and helpers of tests/test_leg_wave_blocks.py):
  30 pairs             one wave, its first K - 1 blocks hold no pair at all
  64 K + 5 pairs       389 / 517 pairs: two waves, the polar one holds five pairs and K - 1 blocks of padding
  2700 pairs           the rule selects K = 6 for spin 2 by itself (8 waves per m with it, 11 at K = 4) and K = 8 for spin 0 (GPU only; asserted through the query)
mmax = lmax throughout and mmax < lmax once.  The recording call, two seeded calls and a plan without seeds agree bit for bit in the ordered mode and to rounding
with atomic adds.  A K without a compiled kernel raises.
Polar rings: a map that is nonzero on the 64 most polar ring pairs only, against the port on those 128 rings.  A wave starts all its blocks when its most equatorial
one goes live, and what the LEG_LIVE rule drops is below 2^-100 of the largest input value: every moment agrees with the port to 1e-11 of the
largest moment, and where the port's moment is below 2^-100 of the largest input value the kernel's is within 2^-90 of it -- the bound of
tests/test_leg_live_start.py (check_single) with the two sides exchanged.  (2^-90 of the input on EVERY moment is not a bound a sum in doubles can meet: a moment
of order 1 carries 2^-53 of rounding.)
Counters: with profiling on, the FP64 flops of a seeded launch equal 128 x the FMAs per lane that the rule of tools/leg_live_count.cpp gives for the ring set, the
pair map and K -- restated here in numpy (live_steps, executed_fmas): coefficients as LegTables::build_host makes them, start values as the kernels', the 4-step test.
CC grids through the whole route (analysis_2d = what map2alm calls, adjoint_synthesis_2d), so that N_cc, the resampling and the weights reach the kernels under a
forced K and under the rule: the analysis of a band-limited map returns its alm; the adjoint synthesis of white noise on a ring subset is the port's.  CC 130 x 264,
lmax 128, K forced (one padded wave); CC 3602 x 80, lmax 3600, mmax 32 (GPU only): the Legendre ring set has 1793 pairs or more and the rule picks K = 6 for spin 2.
Host-simulator twins (PXS_K_SMALL_OFF=1) at lmax 40."""
import functools
import numpy as np
import pytest
from pixell_amd import sht
from oracle import sht_oracle as so
from test_leg_wave_blocks import case, ring_kw, rel, relrms, port_adj, run_adj, TOL, NPH

TEST_K = {0: 8, 2: 6}
OTHER_K = {0: 4, 2: 4}
RULE_K = {0: 8, 2: 6}      # what leg_ana_k selects on the large ring sets

def forced(c, K):
	"""the cached plan of the case's ring calls, its analysis K forced (0: the rule)"""
	kw = ring_kw(np.array(c["th"]), c["lmax"])
	p = sht.ring_plan(kw["theta"], kw["nphi"], kw["phi0"], kw["ringstart"], c["lmax"], c["lmax"], kw["mstart"], 1, 1)
	p.set_option("leg_ana_k", K)
	return p

def check_adj(c, K):
	p = forced(c, K)
	oa = sht.adjoint_synthesis(map=c["pix"].reshape(c["nc"], -1), spin=c["spin"], **ring_kw(np.array(c["th"]), c["lmax"]))
	assert sht.adjoint_synthesis.last_plan is p and (K == 0 or p.query("leg_ana_k") == K)
	e = relrms(oa, c["ra"])
	print("spin %d, %d rings, lmax %d, K %d: adjoint synthesis %.3e" % (c["spin"], c["nr"], c["lmax"], K, e))
	assert np.all(np.isfinite(oa)) and e < TOL
	assert np.max(np.abs(oa-c["ra"])) < 1e-8*np.sqrt(np.mean(np.abs(c["ra"])**2))
	return oa

@functools.lru_cache(maxsize=None)
def polar_case(lmax, nr, spin):
	"""white noise on the 64 most polar ring pairs of the equidistant set and the port's adjoint synthesis of it"""
	c = case("eq", lmax, nr, spin); idx = np.concatenate([np.arange(64), nr-64+np.arange(64)])
	pix = np.zeros((c["nc"], nr, NPH)); pix[:, idx] = np.random.default_rng(41+spin).standard_normal((c["nc"], 128, NPH))
	ra = port_adj(pix[:, idx], spin, lmax, c["th"][idx]); ra.setflags(write=False); pix.setflags(write=False)
	return c, pix, ra

def body_polar(spin, lmax):
	K = TEST_K[spin]; c, pix, ra = polar_case(lmax, 2*(64*K+5), spin)
	p = forced(c, K)
	oa = sht.adjoint_synthesis(map=np.array(pix).reshape(c["nc"], -1), spin=spin, **ring_kw(np.array(c["th"]), lmax))
	assert sht.adjoint_synthesis.last_plan is p and p.query("leg_ana_k") == K
	big = np.max(np.abs(pix)); d = np.abs(oa-ra); tiny = np.abs(ra) < 2.0**-100*big
	print("spin %d K %d: max |moment - port| / max |moment| %.3e; %d of %d moments below 2^-100 of the input, largest difference there %.3e of the input" % (
		spin, K, np.max(d)/np.max(np.abs(ra)), int(tiny.sum()), tiny.size, np.max(d[tiny])/big if tiny.any() else -1))
	assert np.all(np.isfinite(oa)) and np.max(d) < TOL*np.max(np.abs(ra))
	assert tiny.sum() >= 16, "the case does not reach the range the test is about"
	assert np.max(d[tiny]) <= 2.0**-90*big

def body_sizes(spin, lmax, big):
	K = TEST_K[spin]
	for nr in (60, 2*(64*K+5)): check_adj(case("eq", lmax, nr, spin), K)
	if big:
		c = case("eq", lmax, 5400, spin)
		check_adj(c, 0); assert sht.adjoint_synthesis.last_plan.query("leg_ana_k") == RULE_K[spin], "the rule's K at 11 waves per m"
		check_adj(c, OTHER_K[spin]); check_adj(c, K)

def body_mmax(spin, lmax, mmax):
	"""mmax < lmax: the alm of m <= mmax are those of the full transform"""
	K = TEST_K[spin]; c = case("eq", lmax, 2*(64*K+5), spin)
	kw = ring_kw(np.array(c["th"]), lmax); kw["mstart"] = so._tri_mstart(lmax, mmax)
	p = sht.ring_plan(kw["theta"], kw["nphi"], kw["phi0"], kw["ringstart"], lmax, mmax, kw["mstart"], 1, 1); p.set_option("leg_ana_k", K)
	oa = sht.adjoint_synthesis(map=c["pix"].reshape(c["nc"], -1), spin=spin, mmax=mmax, **kw)
	assert sht.adjoint_synthesis.last_plan is p and p.query("leg_ana_k") == K
	n = oa.shape[1]; assert n < c["ra"].shape[1]
	e = relrms(oa, c["ra"][:, :n]); print("spin %d mmax %d of %d: %.3e" % (spin, mmax, lmax, e))
	assert e < TOL

def body_seeds(spin, lmax, monkeypatch):
	K = TEST_K[spin]; c = case("eq", lmax, 2*(64*K+5), spin)
	def run():
		forced(c, K); out = [run_adj(c) for rep in range(3)]
		assert sht.adjoint_synthesis.last_plan.query("leg_ana_k") == K
		return out
	for ordered in (True, False):
		monkeypatch.setattr(sht, "_deterministic", ordered); monkeypatch.setenv("PXS_SEED_MIN_LMAX", "0"); sht.clear_plans()
		try:
			res = run()
			monkeypatch.setenv("PXS_SEED_GB", "0"); sht.clear_plans()
			plain = run()
		finally:
			monkeypatch.delenv("PXS_SEED_GB", raising=False); sht.clear_plans()
		assert relrms(res[0], c["ra"]) < TOL
		for a in res[1:]+plain:
			if ordered: assert np.array_equal(a, res[0]), "ordered adjoint synthesis: a seeded call differs from the recording one or from the plan without seeds"
			else: assert relrms(a, res[0]) < 1e-14

def body_uncompiled(spin):
	c = case("eq", 40, 60, spin); sht.clear_plans()
	forced(c, 5)
	with pytest.raises(Exception, match="ring pairs per lane"): run_adj(c)
	forced(c, 0); run_adj(c)      # the plan is usable afterwards
	sht.clear_plans()

# ---- the rule of tools/leg_live_count.cpp: where the waves leave phase A, and what a seeded launch executes ----
LD = np.longdouble
SC_BIG, SC_SMALL, LEG_LIVE = 2.0**400, 2.0**-800, 2.0**-140

def pow_scaled(x, n):
	"""x^n as mant 2^e, mant in [0.5, 1): pow_scaled of legendre_dev.hpp, elementwise"""
	rm = np.full(x.shape, 0.5); re = np.ones(x.shape, np.int64); bm, be = np.frexp(x); be = be.astype(np.int64)
	while n:
		if n & 1: rm, d = np.frexp(rm*bm); re = re+be+d
		bm, d = np.frexp(bm*bm); be = 2*be+d
		n >>= 1
	return rm, re

def to_scaled(mant, e):
	s = np.where(e >= 0, (e+400)//800, -((-e+400)//800)); s = np.minimum(s, 0)
	v = np.ldexp(mant, (e-800*s).astype(np.int64)); s = np.where(mant == 0, 0, s)
	return np.where(mant == 0, 0.0, v), s

def step_coefs(spin, lmax, m):
	"""(a, b) of every step of this m, as LegTables::build_host computes them (long double, rounded to double)"""
	if spin == 0:
		n = (lmax-m)//2+1
		def eps(l): l = LD(l); return LD(0) if l <= m else np.sqrt((l*l-LD(m)*m)/(4*l*l-1))
		ca, cb = np.zeros(n), np.zeros(n); a_prev, a_cur = LD(0), LD(1)
		for k in range(n):
			lp = m+2*k+1
			e2 = eps(lp+1)**2+eps(lp)**2; f = eps(lp)*eps(lp-1); d = eps(lp+1)*eps(lp+2)
			a_next = a_cur/d if k == 0 else -f*a_prev/d
			ak = a_cur/(a_next*d); ca[k] = float(ak); cb[k] = float(-ak*e2)
			a_prev, a_cur = a_cur, a_next
		return ca, cb
	s = spin; l0 = max(m, s); n = lmax-l0+1
	def Sf(l): l = LD(l); return np.sqrt((l*l-LD(m)*m)*(l*l-LD(s)*s))
	ca, cb = np.zeros(max(n, 0)), np.zeros(max(n, 0)); b_prev, b_cur = LD(0), LD(1)
	for l in range(l0, lmax+1):
		L = LD(l); q = np.sqrt((2*L+3)/(2*L+1))*(2*L+1)
		A = q*(L+1)/Sf(l+1); B = q*LD(m)*LD(s)/(L*Sf(l+1))
		C = np.sqrt((2*L+3)/(2*L-1))*(L+1)*Sf(l)/(L*Sf(l+1)) if l > l0 else LD(0)
		b_next = A*b_cur if l == l0 else C*b_prev
		ca[l-l0] = float(A*b_cur/b_next); cb[l-l0] = float(B*b_cur/b_next)
		b_prev, b_cur = b_cur, b_next
	return ca, cb

def live_steps(spin, lmax, theta_n, m):
	"""per ring pair (northern theta): is it alive at this m, and the 4-step test at which one of its chains is live (a large number: at none); n: the steps of the m"""
	th = theta_n.astype(LD); cth, sth = np.cos(th).astype(float), np.sin(th).astype(float); sh2, ch2 = np.sin(th/2).astype(float), np.cos(th/2).astype(float)
	ofs = max(100.0, 0.01*lmax); s = spin; npairs = len(th)
	ca, cb = step_coefs(spin, lmax, m); n = len(ca)
	if spin == 0:
		alive = m <= lmax*sth+ofs
		v, sc = to_scaled(*pow_scaled(sth, m)); v2 = [v]; scs = [sc]; sgn = [1.0]; x = cth*cth
	else:
		t1 = lmax*sth+ofs; b = -2.0*s*np.abs(cth); c = float(s*s)-t1*t1; discr = b*b-4*c
		mlim = np.where(discr <= 0, float(lmax), np.minimum(float(lmax), 0.5*(-b+np.sqrt(np.maximum(discr, 0)))))
		alive = m <= mlim+0.5; v2, scs = [], []; sgn = [1.0, -1.0]; x = cth
		for h in (0, 1):
			es = (m-s if h else m+s) if m >= s else (s-m if h else s+m); ec = (m+s if h else m-s) if m >= s else (s+m if h else s-m)
			m1, e1 = pow_scaled(sh2, es); m2, e2 = pow_scaled(ch2, ec)
			mt, d = np.frexp(m1*m2); v, sc = to_scaled(mt, e1+e2+(m if m >= s else 0)+d)
			if m < s and h and ((s-m) & 1): v = -v
			v2.append(v); scs.append(sc)
	v2 = [np.where(alive, v, 0.0) for v in v2]; scs = [np.where(alive, sc, 0) for sc in scs]; v1 = [np.zeros(npairs) for v in v2]
	NEVER = 1 << 30; ktrue = np.full(npairs, NEVER); k = 0
	while True:
		lv = np.zeros(npairs, bool)
		for v, sc in zip(v2, scs): lv |= (sc == 0) & (np.abs(v) >= LEG_LIVE)
		ktrue = np.where(lv & alive & (ktrue == NEVER), k, ktrue)
		if k+4 > n or np.all((ktrue < NEVER) | ~alive): break
		with np.errstate(over="ignore", invalid="ignore"):
			for i in range(4):
				for h in range(len(v2)):
					cf = ca[k+i]*x+sgn[h]*cb[k+i]
					nx = cf*v2[h]+v1[h] if spin == 0 else cf*v2[h]-v1[h]
					v1[h], v2[h] = v2[h], nx
			for h in range(len(v2)):
				up = (scs[h] < 0) & (np.abs(v2[h]) > SC_BIG)
				v1[h] = np.where(up, v1[h]*SC_SMALL, v1[h]); v2[h] = np.where(up, v2[h]*SC_SMALL, v2[h]); scs[h] = scs[h]+up
		k += 4
	return alive, ktrue, n

def executed_fmas(spin, lmax, theta, K):
	"""FMAs per lane of a seeded VALU analysis launch: sum over m and waves with an alive pair of (steps - start step) x K x (6 | 12); waves of 64 K consecutive
	pairs, pole first, the padding in front of pair 0 (leg_pair_of)"""
	npairs = len(theta)//2; per = 64*K; nwave = (npairs+per-1)//per; pad = nwave*per-npairs; total = 0
	for m in range(lmax+1):
		alive, ktrue, n = live_steps(spin, lmax, theta[:npairs], m)
		if n <= 0: continue
		kend = 4*(n//4)
		for w in range(nwave):
			a, b = max(0, w*per-pad), min(npairs, (w+1)*per-pad)
			if not alive[a:b].any(): continue
			k0 = min(kend, int(ktrue[a:b][alive[a:b]].min()))
			total += (n-k0)*K*(12 if spin else 6)
	return total

def body_counters(spin, lmax, monkeypatch):
	K = TEST_K[spin]; c = case("eq", lmax, 2*(64*K+5), spin)
	monkeypatch.setenv("PXS_SEED_MIN_LMAX", "0"); sht.clear_plans()
	p = forced(c, K); run_adj(c)      # records the seeds
	p.profile(True); p.profile_flops()
	run_adj(c); got = p.profile_flops()[1]
	p.profile(False); sht.clear_plans()
	want = 128*executed_fmas(spin, lmax, np.array(c["th"]), K)
	other = 128*executed_fmas(spin, lmax, np.array(c["th"]), OTHER_K[spin])
	print("spin %d K %d: executed flops %.0f, the rule's %d (K %d: %d)" % (spin, K, got, want, OTHER_K[spin], other))
	assert other != want, "the ring set does not tell the two pair maps apart"
	assert got == want

# ---- CC grids through the whole route ----
def port_adj_grid(pix, spin, lmax, t, nph, phi0):
	"""test_leg_wave_blocks.port_adj for rings of nph pixels from phi0 on"""
	from oracle import sht_port
	ms = so._tri_mstart(lmax, lmax)
	L = np.fft.fft(pix, axis=2)[:, :, np.arange(lmax+1) % nph]*np.exp(-1j*np.arange(lmax+1)*phi0)[None, None, :]
	cols = sht_port.leg(spin, lmax, np.arange(lmax+1), t, leg=np.transpose(L, (2, 0, 1)))
	out = np.zeros((pix.shape[0], so.nalm(lmax)), complex)
	for m in range(lmax+1): out[:, int(ms[m])+m:int(ms[m])+lmax+1] = cols[m, :, m:]
	out[:, :lmax+1] = out[:, :lmax+1].real
	return out

@functools.lru_cache(maxsize=None)
def grid_case(nt, nph, lmax, spin):
	nc = 1 if spin == 0 else 2
	th = np.asarray(so.grid_info("CC", nt)["theta"], np.float64)
	idx = np.concatenate([np.arange(8), np.arange(8, nt//2, max(1, nt//24)), [nt//2]]); sub = np.unique(np.concatenate([idx, nt-1-idx]))
	pix = np.zeros((nc, nt, nph)); pix[:, sub] = np.random.default_rng(7+spin).standard_normal((nc, len(sub), nph))
	ra = port_adj_grid(pix[:, sub], spin, lmax, th[sub], nph, 0.3); ra.setflags(write=False)
	return dict(alm=so.rand_alm_simple(lmax, nc, 3, spin=(spin,)), pix=pix, ra=ra)

def body_grid(spin, nt, nph, lmax, K):
	nc = 1 if spin == 0 else 2; c = grid_case(nt, nph, lmax, spin)
	kw = dict(spin=spin, lmax=lmax, mstart=so._tri_mstart(lmax, lmax), geometry="CC", phi0=0.3, return_plan=True)
	m = np.zeros((nc, nt, nph)); p = sht.synthesis_2d(alm=c["alm"], map=m, **kw)      # the band-limited map
	p.set_option("leg_ana_k", K)
	back = np.zeros_like(c["alm"]); assert sht.analysis_2d(alm=back, map=m, **kw) is p and p.query("leg_ana_k") == K
	oa = np.zeros_like(c["alm"]); assert sht.adjoint_synthesis_2d(alm=oa, map=np.array(c["pix"]), **kw) is p and p.query("leg_ana_k") == K
	e1, e2 = relrms(back, c["alm"]), relrms(oa, c["ra"])
	print("CC %d x %d lmax %d spin %d K %d: analysis of the band-limited map %.3e  adjoint synthesis of white noise %.3e" % (nt, nph, lmax, spin, K, e1, e2))
	assert e1 < TOL and e2 < TOL

def body_grid_rule(spin):
	"""CC 3602 x 80, lmax 3600, mmax 32: the rule's K on the Legendre ring set of the route; the analysis of the band-limited map returns the alm"""
	nt, nph, lmax, mmax = 3602, 80, 3600, 32; nc = 1 if spin == 0 else 2
	ms = so._tri_mstart(lmax, mmax); n = int(ms[mmax])+lmax+1
	rng = np.random.default_rng(9+spin); alm = rng.standard_normal((nc, n))+1j*rng.standard_normal((nc, n)); alm[:, :lmax+1] = alm[:, :lmax+1].real
	for mm in range(mmax+1): alm[:, int(ms[mm])+mm:int(ms[mm])+max(mm, spin)] = 0
	kw = dict(spin=spin, lmax=lmax, mmax=mmax, mstart=ms, geometry="CC", phi0=0.3, return_plan=True)
	m = np.zeros((nc, nt, nph)); p = sht.synthesis_2d(alm=alm, map=m, **kw)
	back = np.zeros_like(alm); assert sht.analysis_2d(alm=back, map=m, **kw) is p
	ncc = p.query("ncc_circle"); nr_leg = ncc//2+1 if ncc > 0 else nt
	print("spin %d: Legendre ring set %d rings, K %d, analysis of the band-limited map %.3e" % (spin, nr_leg, p.query("leg_ana_k"), relrms(back, alm)))
	assert (nr_leg+1)//2 >= 1793 and p.query("leg_ana_k") == RULE_K[spin]
	assert relrms(back, alm) < TOL
	p.set_option("leg_ana_k", OTHER_K[spin]); b2 = np.zeros_like(alm); sht.analysis_2d(alm=b2, map=m, **kw)
	assert p.query("leg_ana_k") == OTHER_K[spin] and relrms(b2, back) < 1e-13

@pytest.fixture
def fresh():
	sht.clear_plans()
	yield
	sht.clear_plans()

@pytest.mark.gpu
@pytest.mark.parametrize("spin", [0, 2])
def test_sizes_gpu(fresh, spin): body_sizes(spin, 200, True)

@pytest.mark.gpu
@pytest.mark.parametrize("spin", [0, 2])
def test_polar_pairs_only_gpu(fresh, spin): body_polar(spin, 200)

@pytest.mark.gpu
@pytest.mark.parametrize("spin", [0, 2])
def test_mmax_below_lmax_gpu(fresh, spin): body_mmax(spin, 200, 131)

@pytest.mark.gpu
@pytest.mark.parametrize("spin", [0, 2])
def test_seed_modes_gpu(spin, monkeypatch): body_seeds(spin, 200, monkeypatch)

@pytest.mark.gpu
@pytest.mark.parametrize("spin", [0, 2])
def test_counters_gpu(spin, monkeypatch): body_counters(spin, 200, monkeypatch)

@pytest.mark.gpu
@pytest.mark.parametrize("spin", [0, 2])
def test_uncompiled_k_raises_gpu(spin): body_uncompiled(spin)

@pytest.mark.gpu
@pytest.mark.parametrize("spin", [0, 2])
def test_cc_grid_forced_k_gpu(fresh, spin): body_grid(spin, 130, 264, 128, TEST_K[spin])

@pytest.mark.gpu
@pytest.mark.parametrize("spin", [0, 2])
def test_cc_grid_rule_k_gpu(fresh, spin): body_grid_rule(spin)

@pytest.fixture
def sim(monkeypatch):
	monkeypatch.setenv("PXS_K_SMALL_OFF", "1"); sht.clear_plans()
	yield
	sht.clear_plans()

@pytest.mark.hostsim
@pytest.mark.parametrize("spin", [0, 2])
def test_sizes_hostsim(sim, spin): body_sizes(spin, 40, False)

@pytest.mark.hostsim
@pytest.mark.parametrize("spin", [0, 2])
def test_polar_pairs_only_hostsim(sim, spin): body_polar(spin, 64)

@pytest.mark.hostsim
@pytest.mark.parametrize("spin", [0, 2])
def test_mmax_below_lmax_hostsim(sim, spin): body_mmax(spin, 40, 23)

@pytest.mark.hostsim
@pytest.mark.parametrize("spin", [0, 2])
def test_seed_modes_hostsim(sim, spin, monkeypatch): body_seeds(spin, 40, monkeypatch)

@pytest.mark.hostsim
@pytest.mark.parametrize("spin", [0, 2])
def test_counters_hostsim(sim, spin, monkeypatch): body_counters(spin, 40, monkeypatch)

@pytest.mark.hostsim
@pytest.mark.parametrize("spin", [0, 2])
def test_uncompiled_k_raises_hostsim(sim, spin): body_uncompiled(spin)

@pytest.mark.hostsim
@pytest.mark.parametrize("spin", [0, 2])
def test_cc_grid_forced_k_hostsim(sim, spin): body_grid(spin, 42, 88, 40, TEST_K[spin])
