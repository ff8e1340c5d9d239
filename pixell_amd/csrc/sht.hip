// SHT plans and pipelines (C-ABI pxs_* of include/pxsht.h) for gfx950.
//
//   synthesis        alm --Legendre--> leg[m][ring] --transpose*phase--> h[ring][m] --c2r ring FFT--> map
//   adjoint synth.   map --r2c ring FFT (pruned to m<=mmax)--> h[ring][m] --transpose*phase--> leg --Legendre^T--> alm
//   analysis_2d      map --ring FFT--> leg on the map's rings --theta resampling--> leg on a minimal
//                    Clenshaw-Curtis grid (lmax+2.. rings) incl. exact |sin| quadrature --Legendre^T--> alm
//   adj. analysis    the exact transpose of the above
//
// The theta resampling between the two grids is exact for the band limit (sht_unfused.hip says how); the fused chains of fftchain.hip
// run it, the ring FFTs and their transposes wherever their planners take the sizes.
// flip_y / flip_x (curvedsky.map2buffer, curvedsky.py:1384-1411) are negative strides here.
#include "sht_plan.hpp"
#include <cmath>
#include <algorithm>

static const char* const ROUTE_NAMES[] = {"direct", "via-cc", "via-cc-unfused", "via-cc-unfused-h", "ring-weights", "cc-weights", "chain", "unfused"};

Route::Scratch Route::scratch(const pxs_plan* p, int nb) const {
	Scratch s; const size_t nct = (size_t)nb*nc, nm = (size_t)p->mmax + 1, c16 = sizeof(double2);
	s.leg = c16*nct*nm*ld_leg_alloc; s.leg2 = c16*nct*nm*ld_leg2; s.h = c16*nct*nr_h*ld_h;
	if (to_map) s.almt = sizeof(double)*4*(tb->nrows + 4)*nb; else s.mom = sizeof(double)*4*std::max<long>(tb->nrows, 1)*nb;
	if (theta_fused && !line) FftChain::theta_scratch(theta, form->tp, (int)nm, (int)nct, s.c1, s.c2);
	if (reserve_chain) p->chain->ring_scratch(p->nring, (int)nct, !to_map, s.r1, p->mmax);
	return s;
}

namespace {

void plan_common(pxs_plan* p, int lmax, int mmax, const uint64_t* mstart, int64_t lstride, int device) {
	PXS_REQUIRE(lmax >= 0 && mmax >= 0 && mmax <= lmax, "need 0 <= mmax <= lmax");
	PXS_REQUIRE(mstart != nullptr, "mstart is required");
	PXS_HIP(hipSetDevice(device));
	p->device = device; p->lmax = lmax; p->mmax = mmax; p->lstride = lstride;
	std::vector<uint64_t> ms(mstart, mstart+mmax+1);
	p->d_mstart = upload(ms);
	p->fc = &fft_context(device);
	{	// scratch for the per-wave partial moments of the analysis: 16 GiB where the device has room (MI355X: 288 GB),
		// never more than 1/8 of what is free now.  Measured at config 3: 4 GiB 448.8, 8 GiB 442.7, 16 GiB 438.0, 24 GiB 437.7 ms.
		size_t fr = 0, tot = 0;
		if (hipMemGetInfo(&fr, &tot) == hipSuccess && fr > 0) p->wk.part_budget = std::min<size_t>(size_t(2) << 30, std::max<size_t>(fr/8, size_t(256) << 20));      // (ordered analysis only: <= 2 GB of partial moments, m in chunks)
		env_budget("PXS_PART_GB", 30, p->wk.part_budget);      // (0: one m per pass)
		{ const char* d = getenv("PXS_DETERMINISTIC"); p->wk.deterministic = d && atoi(d) != 0; }      // default of pxs_plan_option("deterministic")
	}
	env_budget("PXS_RESAMPLE_MB", 20, p->resample_chunk_bytes);
	{ const char* e = getenv("PXS_ANALYSIS"); if (e) { const std::string v(e); p->ana_weights = v == "weights" ? 1 : (v == "ducc0" ? 2 : (v == "interpolant" ? 0 : p->ana_weights)); } }
	if (p->general) return;      // per-ring lengths and phases: see GenRings::setup
	std::string why;
	if (!FftContext::supported(p->nphi, &why)) throw Error(PXS_ERR_UNSUPPORTED, why);
	// e^{-i m phi0}
	std::vector<double2> ph(mmax+1);
	for (int m = 0; m <= mmax; m++) { LDb a = (LDb)m*(LDb)p->phi0; ph[m] = make_double2((double)cosl(a), (double)(-sinl(a))); }
	p->phase = upload(ph);
	p->chain.reset(new FftChain(p->fc));
	p->chain_rings = 2L*mmax < p->nphi && p->chain->plan_rings(p->nphi);      // (two real rings per complex transform: no aliased rings)
	if (getenv("PXS_CHAIN_VERBOSE")) fprintf(stderr, "[pxsht] ring chain nphi=%d mmax=%d: %s\n", p->nphi, mmax, p->chain_rings ? p->chain->describe().c_str() : "off");
}

// the theta tables and the two forms of the analysis of a plan whose rings are (rows of) a 2-D grid
void setup_resampling(pxs_plan* p) {
	ThetaTables& t = p->th; AnaForm &ai = p->ana_interp, &af = p->ana_fine;
	af.fine = true;
	if (p->nfull == 0) p->nfull = p->nring;
	GridInfo gi = grid_info(p->geometry, p->nfull);
	t.N = gi.N; t.mir_c = gi.c;
	const int lmax = p->lmax;
	t.Ncc = FftContext::good_size(std::max<long>(2L*lmax + 2, 4));
	if (t.Ncc & 1) t.Ncc = FftContext::good_size(t.Ncc + 1);
	while (t.Ncc & 1) t.Ncc = FftContext::good_size(t.Ncc + 1);
	{	// ducc0's own N_cc = 2 good_size_complex(lmax + 1) where the FFT engine takes it and twice it (the fused chains decide for themselves below)
		const long nd = FftChain::ducc_ncc(lmax);
		if (nd >= 4 && FftContext::supported(nd) && FftContext::supported(2*nd)) t.Ncc = nd;
	}
	ai.M = FftContext::good_size(t.N + 2L*lmax + 2);
	if (p->chain_rings) {	// the fused theta chains need N, M and Ncc to share a modulus: let their planner pick M and Ncc
		ai.tp = FftChain::plan_theta(t.N, lmax);
		if (ai.tp.ok) { t.Ncc = ai.tp.Ncc; ai.M = ai.tp.M; }
		if (getenv("PXS_CHAIN_VERBOSE")) fprintf(stderr, "[pxsht] theta chain N=%ld lmax=%d: ok=%d g=%ld bN=%ld g2=%ld (M=%ld) ac=%ld (Ncc=%ld) | syn gs=%ld bs=%ld aNs=%ld\n",
			t.N, lmax, (int)ai.tp.ok, ai.tp.g, ai.tp.bN, ai.tp.g2, ai.tp.M, ai.tp.ac, ai.tp.Ncc, ai.tp.gs, ai.tp.bs, ai.tp.aNs);
	}
	t.ncc = (int)(t.Ncc/2 + 1);
	std::string why;
	if (!FftContext::supported(t.N, &why)) throw Error(PXS_ERR_UNSUPPORTED, why);
	// CC ring set
	std::vector<LDb> th(t.ncc);
	for (int j = 0; j < t.ncc; j++) th[j] = 2*PIl*j/t.Ncc;
	th[t.ncc-1] = PIl;
	p->rs_cc.build(th); p->rs_cc.upload_all();
	// shift phases e^{-i k theta0}, k = 0..N/2
	const LDb th0 = (LDb)gi.c*PIl/gi.N;
	std::vector<double2> ps(t.N/2 + 1);
	for (long k = 0; k <= t.N/2; k++) { LDb a = (LDb)k*th0; ps[k] = make_double2((double)cosl(a), (double)(-sinl(a))); }
	t.ph_shift = upload(ps);
	{ std::vector<double2> pu(ps.size()); for (size_t k = 0; k < ps.size(); k++) pu[k] = make_double2(ps[k].x, -ps[k].y); t.ph_up = upload(pu); }
	// synthesis: Legendre on the minimal CC grid + exact Fourier upsampling in theta pays once the map has clearly more rings
	// (measured: at nring / ncc = 1.33 -- C2, C4 -- the detour pays for spin 2, profiles/r06_syn_via_cc_c2.txt, and costs 11 ms per 64
	// scalar maps at C4: the two thresholds of round 4, profiles/README.md)
	// (a band: what counts is the ring-pair slots of its own rings, unpaired rings take a whole slot)
	{ const long rings = p->band ? 2L*p->rs_map.npairs : p->nring;
	  p->syn_via_cc = rings > t.ncc + t.ncc/4;
	  p->syn_via_cc0 = rings > t.ncc + t.ncc/2; }
	// sigma_i = sum_{|q|<=Ks} s_q e^{i q theta_i} on the M grid, via one device FFT
	const long Ks = lmax + t.N/2;
	PXS_REQUIRE(2*Ks < ai.M, "internal: fine grid too small");
	std::vector<double2> spec(ai.M, make_double2(0, 0));
	for (long q = 0; q <= Ks; q++) { double s = abs_sin_coef(q); spec[q].x = s; if (q > 0) spec[ai.M - q].x = s; }
	DevBuf dspec = upload(spec);
	ai.sigma.alloc(sizeof(double2)*ai.M);
	FftDims d;
	FftLoad ld; ld.ptr = dspec.p; FftStore st; st.ptr = ai.sigma.p;
	p->fc->exec(nullptr, ai.M, false, d, ld, st);
	PXS_HIP(hipStreamSynchronize(nullptr));
	// CC weights incl. all FFT normalisations: (pi/nphi)(2pi/Ncc) eps_j / (N M)
	std::vector<double2> w(t.ncc);
	for (int j = 0; j < t.ncc; j++) {
		LDb e = (j == 0 || j == t.ncc-1) ? 1 : 2;
		w[j] = make_double2((double)((PIl/p->nphi)*(2*PIl/t.Ncc)*e/((LDb)t.N*(LDb)ai.M)), 0.0);
	}
	ai.wcc = upload(w);
	{	// the same weights for the fused adjoint of the analysis (TH_TO_CC_ADJ): halved off the two pole rings
		std::vector<double2> wh(w); for (int j = 1; j + 1 < t.ncc; j++) wh[j].x *= 0.5;
		ai.whalf = upload(wh); }
	{	// weights of the transposed theta upsampling (TH_FROM_CC_ADJ): 1/N_cc, half at the two pole rings
		std::vector<double2> wa(t.ncc);
		for (int j = 0; j < t.ncc; j++) wa[j] = make_double2(((j == 0 || j == t.ncc-1) ? 0.5 : 1.0)/(double)t.Ncc, 0.0);
		t.wadj = upload(wa); }
	if (FftContext::supported(2*t.Ncc)) {	// the fine-CC form: M = 2 N_cc (through the fused chains: = g * (2 ac))
		if (ai.tp.ok && FftChain::sub_ok_theta(2*ai.tp.ac)) { af.tp = ai.tp; af.tp.g2 = 2*ai.tp.ac; af.tp.M = 2*t.Ncc; } else af.tp.ok = false;
		const long Mf = af.M = 2*t.Ncc; const int nf = (int)(Mf/2 + 1);
		const std::vector<double> gw = grid_weights("CC", nf);
		// table on the circle: (Mf / 2 pi) x the weight of the full-circle rule int g |sin| = sum_i t_i g(theta_i): ring weight
		// (sum over the rings = 2) at both images of a ring, twice that at the two poles, which the circle holds once
		std::vector<double2> sg(Mf);
		for (long i = 0; i < Mf; i++) {
			const long r = std::min(i, Mf - i);
			const LDb wr = (LDb)gw[r]/(2*PIl)*((r == 0 || r == Mf/2) ? 2 : 1);
			sg[i] = make_double2((double)(wr*(LDb)Mf/(2*PIl)), 0.0);
		}
		af.sigma = upload(sg);
		{ std::vector<double> sh((size_t)nf); for (int i = 0; i < nf; i++) sh[i] = sg[i].x; af.sig_half = upload(sh); }      // sg[i] = sg[Mf - i], real
		const double f = (double)ai.M/(double)Mf;       // the FFT normalisation 1/(N M) of the weights, for this M
		std::vector<double2> wf(w), whf(w);
		for (int j = 0; j < t.ncc; j++) { wf[j].x *= f; whf[j].x *= (j == 0 || j == t.ncc-1) ? f : 0.5*f; }
		af.wcc = upload(wf); af.whalf = upload(whf);
	}
}

int ncomp_of(int spin, int mode, bool alm_side) {
	if (mode == PXS_MODE_DERIV1) return alm_side ? 1 : 2;
	return spin == 0 ? 1 : 2;
}

// ring FFT of the nb maps of a pass: user map -> leg[c][m][ring] * e^{-i m phi0}, rows of the route's ld_leg
void map2leg(pxs_plan* p, hipStream_t st, const Route& r, const MapArg& m, int nb, double2* leg) {
	const int nc = nb*r.nc, ncb = nb > 1 ? r.nc : 0;
	{	StageScope stage(p->prof, st, PXS_STAGE_RING_FFT);
		PXS_REQUIRE(p->chain_rings || (ncb == 0 && (p->general || r.ld_leg == p->nring)), "internal: only the ring chain takes batches and padded rows");
		if (p->general) gen_map2leg(p, st, m, nc, leg, r.ld_leg);
		else if (p->chain_rings) p->chain->map2leg(st, p->map_desc(m, ncb), nc, p->mmax, leg, r.ld_leg, p->phase.as<double2>(), 1.0);
		else unfused_map2leg(p, st, m, nc, leg);
	}
	PXS_HIP(hipGetLastError());
}

// the nb maps of a pass: leg[c][m][ring] * e^{+i m phi0} -> hbuf[c][ring][m] -> c2r ring FFT -> user map
// (leg: rows of stride ldleg; null: the route's theta stage has written hbuf already.  hbuf: the route's ld_h and nr_h, sized by reserve_call)
void leg2map(pxs_plan* p, hipStream_t st, const Route& r, const double2* leg, long ldleg, const MapArg& m, int nb) {
	const int nc = nb*r.nc, ncb = nb > 1 ? r.nc : 0;
	{	StageScope stage(p->prof, st, PXS_STAGE_RING_FFT);
		PXS_REQUIRE(p->chain_rings || (ncb == 0 && !(p->general && !leg)), "internal: only the ring chain takes batches");
		if (p->general) gen_leg2map(p, st, leg, ldleg, m, nc);
		else {
			if (leg) leg_to_h(p, st, leg, ldleg, r.ld_h, nc);
			// (the CC detour of a band plan: h holds all nfull rings of the grid, the map's rings start at row0)
			const bool full_h = r.nr_h > p->nring;
			if (p->chain_rings) p->chain->h2map(st, p->hbuf.as<double2>() + (full_h ? (size_t)p->row0*r.ld_h : 0), r.ld_h, p->map_desc(m, ncb), nc, p->mmax, full_h ? r.nr_h : 0);
			else unfused_h2map(p, st, m, nc);
		}
	}
	PXS_HIP(hipGetLastError());
}

} // namespace

extern "C" {

int pxs_plan_grid2d(pxs_plan** plan, const char* geometry, int ntheta, int nphi, double phi0,
                    int flip_y, int flip_x, int lmax, int mmax, const uint64_t* mstart, int64_t lstride, int device)
{
	PXS_TRY
	PXS_REQUIRE(plan && geometry && ntheta > 0 && nphi > 0, "pxs_plan_grid2d: bad arguments");
	GridInfo gi = grid_info(geometry, ntheta);
	if (!gi.ok) throw Error(PXS_ERR_UNSUPPORTED, std::string("unsupported 2d geometry '") + geometry + "' (supported: CC, F1, MW, MWflip, DH, F2)");
	std::unique_ptr<pxs_plan> p(new pxs_plan());
	p->is_grid = true; p->geometry = geometry; p->nring = ntheta; p->nphi = nphi; p->phi0 = phi0;
	p->ring_stride = flip_y ? -(long)nphi : (long)nphi;
	p->pix_stride = flip_x ? -1 : 1;
	p->ring_off0 = (flip_y ? (long)(ntheta-1)*nphi : 0) + (flip_x ? (long)nphi-1 : 0);
	plan_common(p.get(), lmax, mmax, mstart, lstride, device);
	p->rs_map.build(grid_theta(geometry, ntheta)); p->rs_map.upload_all();
	if (grid_weights_only(geometry)) {	// quadrature weights per pixel for the analysis (pxs_analysis)
		p->wring = ring_weight_table(geometry, ntheta, nphi);
	} else if (lmax <= grid_maxlmax(geometry, ntheta)) setup_resampling(p.get());
	*plan = p.release();
	PXS_CATCH
}

int pxs_plan_rings(pxs_plan** plan, int nring, const double* theta, const uint64_t* nphi,
                   const double* phi0, const uint64_t* ringstart, int64_t pixstride,
                   int lmax, int mmax, const uint64_t* mstart, int64_t lstride, int device)
{
	PXS_TRY
	PXS_REQUIRE(plan && nring > 0 && theta && nphi && phi0 && ringstart, "pxs_plan_rings: bad arguments");
	std::unique_ptr<pxs_plan> p(new pxs_plan());
	p->is_grid = false; p->nring = nring; p->nphi = (int)nphi[0]; p->phi0 = phi0[0];
	p->ring_off0 = (long)ringstart[0];
	p->ring_stride = nring > 1 ? (long)ringstart[1] - (long)ringstart[0] : (long)nphi[0];
	// equal rings at equal spacing (every CAR map) take the fused / paired ring FFTs; anything else (healpix, profile rings,
	// masked ring subsets) the general path: per-ring length, phase and offset
	for (int r = 0; r < nring; r++)
		if ((long)nphi[r] != p->nphi || std::fabs(phi0[r] - phi0[0]) > 1e-13 || (long)ringstart[r] != p->ring_off0 + r*p->ring_stride) p->general = true;
	if (!FftContext::supported(p->nphi)) p->general = true;          // equal rings of a length with a prime factor > 2048: Bluestein lives on the general path
	{ const char* e = getenv("PXS_GENERAL_RINGS"); if (e && atoi(e) != 0) p->general = true; }      // (tests: the general path on uniform rings)
	p->pix_stride = pixstride;
	plan_common(p.get(), lmax, mmax, mstart, lstride, device);
	if (p->general) p->gen.setup(device, nring, nphi, phi0, ringstart);
	std::vector<LDb> th(nring);
	for (int r = 0; r < nring; r++) th[r] = theta[r];
	p->rs_map.build(th); p->rs_map.upload_all();
	// Rows of a Fejer-1 grid (a declination band of a CAR map, curvedsky.py:843-873): theta_r = (row0 + r + 1/2) pi / n.  Synthesis
	// and its adjoint can then run their Legendre stage on the ~lmax+2 CC rings of that grid instead of the band's own ring-pair
	// slots (an unpaired ring costs a whole slot): the band figures of profiles/README.md.
	if (!p->general && p->chain_rings && nring >= 2) {
		const LDb d = th[1] - th[0];
		const long n = d > 0 ? (long)llroundl(PIl/d) : 0;
		const long k0 = n > 0 ? (long)llroundl(th[0]*n/PIl - 0.5L) : -1;
		bool ok = n > nring && k0 >= 0 && k0 + nring <= n && lmax <= n - 1 && n < (1L << 30) && FftContext::supported(2*n);
		for (int r = 0; ok && r < nring; r++) ok = fabsl(th[r] - ((LDb)(k0 + r) + 0.5L)*PIl/n) < 1e-11L;
		if (ok) {
			p->band = true; p->geometry = "F1"; p->nfull = (int)n; p->row0 = (int)k0;
			setup_resampling(p.get());
			if (!p->chain_theta()) { p->band = false; p->nfull = 0; p->row0 = 0; p->th.ncc = 0; }     // (no fused theta chain for this size: stay on the band's own rings)
		}
	}
	*plan = p.release();
	PXS_CATCH
}

int pxs_plan_points(pxs_plan** plan, const pxs_plan* g, int64_t npts, const double* d_loc, double epsilon, int device, void* stream)
{
	PXS_TRY
	PXS_REQUIRE(plan && g && npts >= 0 && (d_loc || npts == 0), "pxs_plan_points: bad arguments");
	PXS_REQUIRE(g->is_grid && g->geometry == "CC" && !g->pts && g->phi0 == 0 && g->ring_stride == g->nphi && g->pix_stride == 1,
		"pxs_plan_points: needs an unflipped CC grid plan with phi0 = 0");
	PXS_REQUIRE(g->nring >= g->lmax + 2 && g->nphi % 2 == 0 && g->nphi >= 2*g->mmax + 2, "pxs_plan_points: the CC grid needs ntheta >= lmax + 2 and an even nphi >= 2 mmax + 2");
	PXS_REQUIRE(FftContext::supported(2L*g->nring - 2) && FftContext::supported(g->nphi), "pxs_plan_points: CC grid sizes the FFT engine cannot transform");
	PXS_REQUIRE(epsilon >= 1e-13 && epsilon <= 0.1, "pxs_plan_points: epsilon must lie in [1e-13, 0.1]");
	PXS_REQUIRE(device == g->device, "pxs_plan_points: the grid plan lives on another device");
	PXS_HIP(hipSetDevice(device));
	std::unique_ptr<pxs_plan> p(new pxs_plan());
	p->device = device; p->lmax = g->lmax; p->mmax = g->mmax; p->lstride = g->lstride; p->pgrid = const_cast<pxs_plan*>(g);
	p->pts = points_create(g->nring, g->nphi, g->lmax, g->mmax, device, (long)npts, d_loc, epsilon, (hipStream_t)stream);
	*plan = p.release();
	PXS_CATCH
}

int pxm_plan_map_points(pxs_plan** plan, int ny, int nx, int ydouble, int64_t npts, const double* d_pix, double epsilon, int device, void* stream)
{
	PXS_TRY
	PXS_REQUIRE(plan && ny >= 1 && nx >= 1 && npts >= 0 && (d_pix || npts == 0), "pxm_plan_map_points: bad arguments");
	PXS_REQUIRE(ny < (1 << 30) && nx < (1 << 30), "pxm_plan_map_points: map too large");
	PXS_REQUIRE(FftContext::supported(ydouble ? 2L*ny : ny) && FftContext::supported(nx), "pxm_plan_map_points: map sizes the FFT engine cannot transform");
	PXS_REQUIRE(epsilon >= 1e-13 && epsilon <= 0.1, "pxm_plan_map_points: epsilon must lie in [1e-13, 0.1]");
	PXS_HIP(hipSetDevice(device));
	std::unique_ptr<pxs_plan> p(new pxs_plan());
	p->device = device;
	p->pts = mappoints_create(ny, nx, ydouble, device, (long)npts, d_pix, epsilon, (hipStream_t)stream);
	*plan = p.release();
	PXS_CATCH
}

int pxm_map_points(pxs_plan* p, int ncomp, const void* d_maps, int map_dtype, int64_t map_cstride, void* d_out, int out_dtype, int64_t out_cstride, void* stream)
{
	PXS_TRY
	PXS_REQUIRE(p && p->pts && points_from_map(p->pts), "pxm_map_points needs a plan of pxm_plan_map_points");
	PXS_REQUIRE(ncomp >= 0 && (ncomp == 0 || (d_maps && d_out)), "pxm_map_points: bad arguments");
	PXS_REQUIRE((map_dtype == PX_F32 || map_dtype == PX_F64) && (out_dtype == PX_F32 || out_dtype == PX_F64), "pxm_map_points: maps and values must be float32 or float64");
	std::lock_guard<std::mutex> plan_lock(p->call_mu);
	PXS_HIP(hipSetDevice(p->device));
	hipStream_t st = (hipStream_t)stream;
	PlanUse use(p, st);
	mappoints_run(p->pts, ncomp, d_maps, map_dtype, (long)map_cstride, d_out, out_dtype, (long)out_cstride, st);
	PXS_CATCH
}

void pxs_plan_destroy(pxs_plan* plan) { delete plan; }

int pxs_plan_option(pxs_plan* p, const char* name, int64_t value) {
	PXS_TRY
	PXS_REQUIRE(p && name, "pxs_plan_option: null argument");
	std::lock_guard<std::mutex> plan_lock(p->call_mu);
	if (p->pts) {      // a points plan: its spreading is always ordered; the Legendre stage follows the grid plan's own option
		const std::string n(name);
		PXS_REQUIRE((n == "deterministic" || n == "profile") && (value == 0 || value == 1), "pxs_plan_option: a points plan takes 'deterministic' or 'profile' (0 or 1)");
		if (n == "deterministic") p->wk.deterministic = value != 0;
		else points_profile(p->pts, value != 0);
		return 0;
	}
	if (std::string(name) == "analysis") {
		PXS_REQUIRE(value >= 0 && value <= 2, "pxs_plan_option: analysis takes 0 (interpolant), 1 (weights) or 2 (ducc0)");
		p->ana_weights = (int)value;
	} else if (std::string(name) == "deterministic") {      // analysis sums in a fixed order: bitwise repeatable results (default 0: atomic adds, repeatable to ~1e-14)
		PXS_REQUIRE(value == 0 || value == 1, "pxs_plan_option: deterministic takes 0 or 1");
		p->wk.deterministic = value != 0;
	} else if (std::string(name) == "build_tables") {      // build the recurrence tables of spin `value` now rather than in the first transform (cold-start accounting of bench.py)
		PXS_REQUIRE(value >= 0 && value <= p->lmax + 1, "pxs_plan_option: build_tables takes a spin");
		PXS_HIP(hipSetDevice(p->device));
		(void)p->table((int)value);
	} else if (std::string(name) == "leg_max_batch") {      // upper bound on the maps of one Legendre launch (8 x as many for the MFMA form); 0: the grid limit alone
		PXS_REQUIRE(value >= 0 && value <= (1 << 20), "pxs_plan_option: leg_max_batch takes 0 (no bound) or a number of maps");
		p->wk.max_batch = (int)value;
	} else if (std::string(name) == "leg_ana_k") {      // ring pairs per lane of the VALU analysis kernels; 0: the host's rule -- for tests (a value without a compiled kernel fails at the launch)
		PXS_REQUIRE(value >= 0 && value <= 64, "pxs_plan_option: leg_ana_k takes 0 (the host's rule) or a number of ring pairs per lane");
		p->wk.ana_k = (int)value;
	} else throw Error(PXS_ERR_ARG, std::string("pxs_plan_option: unknown option '") + name + "'");
	PXS_CATCH
}

// the interpolating form of the analysis (fused chains or the unfused engine): the fine-CC form (the default; the weights option
// on a grid below 2 lmax + 2 rings takes it too), else the interpolant form
static const AnaForm& ana_form(const pxs_plan* p) { return p->ana_weights != 0 && p->ana_fine.M > 0 ? p->ana_fine : p->ana_interp; }

// THE fused theta operation of a route, on nct components of the plan's buffers: leg <-> leg2 (analysis side), leg2 -> h (synthesis
// side), with the tables of the route's form; wring: optional weight per ring of the map
static void run_theta(pxs_plan* p, hipStream_t st, const Route& r, int nct, int spin, const double2* wring) {
	const ThetaTables& t = p->th; const AnaForm& f = *r.form;
	const bool to_h = r.theta == TH_FROM_CC || r.theta == TH_TO_CC_ADJ, mid = r.theta == TH_TO_CC || r.theta == TH_TO_CC_ADJ;      // mid: over the form's fine circle
	ThetaCall c;
	c.tp = &f.tp; c.nc = nct; c.nm = p->mmax + 1; c.spin = spin; c.lmax = p->lmax; c.mir_c = t.mir_c;
	c.map = (to_h ? p->hbuf : p->leg).as<double2>(); c.ldmap = to_h ? r.ld_h : r.ld_leg; c.nr = to_h ? r.nr_h : r.nr_th;
	c.cc = p->leg2.as<double2>(); c.ldcc = r.ld_leg2; c.ncc = t.ncc;
	c.ph = (r.theta == TH_FROM_CC ? t.ph_up : t.ph_shift).as<double2>();
	if (mid) { c.sigma = f.sigma.as<double2>(); c.sig_half = f.sig_half.as<double>(); }
	if (r.theta != TH_FROM_CC) c.wcc = (r.theta == TH_TO_CC ? f.wcc : r.theta == TH_TO_CC_ADJ ? f.whalf : t.wadj).as<double2>();
	c.wring = wring;
	if (to_h) { c.tab = p->phase.as<double2>(); c.scale = mid ? 2.0 : 1.0/(double)t.Ncc; }
	p->chain->theta(st, r.theta, c);
}
static Route route_of(const pxs_plan* p, bool analysis, int spin, int mode, bool adjoint, const LegTables* tb);
static Route analysis_route_now(const pxs_plan* p) { return route_of(p, true, 0, PXS_MODE_STANDARD, false, nullptr); }      // pxs_analysis under the plan's current option
// The chain stage shapes of the plan's standard calls (analysis under its current option, synthesis of spin 0 and spin 2), each once:
// a dry run (FftChain::dry_begin) through the routes and the theta call of the calls themselves.
static std::vector<ChainShape> chain_shapes(const pxs_plan* cp) {
	pxs_plan* p = const_cast<pxs_plan*>(cp);
	std::vector<ChainShape> all, out;
	if (!p->chain || !p->chain_rings) return out;
	std::lock_guard<std::mutex> plan_lock(p->call_mu);
	FftChain::MapDesc md; memset(&md, 0, sizeof(md)); md.dtype = PX_F64; md.cstride = (long)p->nring*p->nphi; md.ring_stride = p->nphi; md.pix_stride = 1; md.nring = p->nring; md.nphi = p->nphi;
	p->chain->dry_begin(&all);
	try {
		for (int which = 0; which < 3; which++) {
			const bool ana = which == 0; const int spin = which == 2 ? 2 : 0;
			const Route r = route_of(p, ana, spin, PXS_MODE_STANDARD, false, nullptr);
			if (!r.reserve_chain) continue;
			if (ana) p->chain->map2leg(nullptr, md, r.nc, p->mmax, nullptr, r.ld_leg, nullptr, 1.0);
			else p->chain->h2map(nullptr, nullptr, r.ld_h, md, r.nc, p->mmax, 0);
			if (r.theta_fused && !r.line) run_theta(p, nullptr, r, r.nc, spin, nullptr);      // (no ring weights: a query builds no tables)
		}
	} catch (...) { p->chain->dry_end(); throw; }
	p->chain->dry_end();
	for (const ChainShape& c : all) {
		bool seen = false;
		for (const ChainShape& o : out) seen = seen || (o.sid == c.sid && o.na == c.na && o.nb == c.nb && o.T == c.T);
		if (!seen) out.push_back(c);
	}
	return out;
}
int pxs_plan_query(const pxs_plan* p, const char* name, int64_t* value) {
	PXS_TRY
	PXS_REQUIRE(name && value, "pxs_plan_query: null argument");
	const std::string n(name);
	if (n.compare(0, 7, "passes_") == 0) {      // passes of the most recent call at a memory-budget seam (include/pxsht.h), as its launch loop counted them
		std::string seam = n.substr(7); int which = 0;      // 0: how many, 1 / 2 / 3: size of the first / the one before the last / the last
		static const char* const sufs[3] = {"_first", "_prev", "_last"};
		for (int i = 0; i < 3 && !which; i++) {
			const size_t k = strlen(sufs[i]);
			if (seam.size() > k && seam.compare(seam.size() - k, k, sufs[i]) == 0) { seam.resize(seam.size() - k); which = i + 1; }
		}
		const PassLog* l = nullptr;
		if (seam == "fft") { int dev = p ? p->device : 0; if (!p) PXS_HIP(hipGetDevice(&dev)); l = &fft_context(dev).pass_lines; }      // device-wide: plan may be NULL
		else {
			PXS_REQUIRE(p && !p->pts, "pxs_plan_query: the passes of this seam belong to a grid or ring plan");
			if (seam == "batch") l = &p->pass_batch; else if (seam == "resample") l = &p->pass_resample;
			else if (seam == "leg_m") l = &p->wk.pass_m; else if (seam == "leg_valu") l = &p->wk.pass_valu; else if (seam == "leg_mm") l = &p->wk.pass_mm;
			else if ((seam == "theta" || seam == "ring") && p->chain) l = seam == "theta" ? &p->chain->pass_theta : &p->chain->pass_ring;
		}
		if (!l) throw Error(PXS_ERR_ARG, std::string("pxs_plan_query: unknown name '") + name + "'");
		*value = which == 0 ? l->n : which == 1 ? l->first : which == 2 ? l->prev : l->last;
		return 0;
	}
	PXS_REQUIRE(p, "pxs_plan_query: null argument");
	if (p->pts) *value = points_query(p->pts, n);
	else if (n == "analysis_form") { const Route r = analysis_route_now(p); *value = (r.kind == R_RING_WEIGHTS || r.kind == R_CC_WEIGHTS) ? 1 : (r.form->fine ? 2 : 0); }
	else if (n == "leg_executed_flops_ana") {      // wave count less what was not executed (legendre_dev.hpp, PXS_COUNT_AT): blocks of the analysis kernels from their own start; reset with pxs_profile_flops
		double sum = 0;
		if (p->wk.count.p) {
			PXS_HIP(hipSetDevice(p->device)); PXS_HIP(hipDeviceSynchronize());
			std::vector<double> c(p->wk.count.bytes/sizeof(double)); PXS_HIP(hipMemcpy(c.data(), p->wk.count.p, p->wk.count.bytes, hipMemcpyDeviceToHost));
			for (size_t i = 1; i + 2 < c.size(); i += 4) sum += (c[i] - c[i + 2])*128.0;
		}
		*value = (int64_t)sum;
	}
	else if (n == "leg_ana_k") *value = p->wk.last_ana_k;      // ring pairs per lane of the VALU launches of the most recent Legendre analysis on the plan (0: none yet)
	else if (n == "ncc_circle") *value = p->th.ncc > 0 ? p->th.Ncc : 0;
	else if (n == "ducc_ncc_circle") *value = FftChain::ducc_ncc(p->lmax);
	else if (n == "theta_line") *value = analysis_route_now(p).line ? 1 : 0;      // 1: its theta resampling runs as ONE kernel per call (thetaline.hip), 0: as the stage chain
	else if (n == "chain_stages" || n == "chain_static") {      // distinct chain stage shapes of the plan's standard calls / those with a compile-time-planned kernel
		int64_t k = 0;
		for (const ChainShape& c : chain_shapes(p)) {
			if (getenv("PXS_CHAIN_VERBOSE")) fprintf(stderr, "[pxsht] plan stage %d: na=%d nb=%d T=%d static %d\n", c.sid, c.na, c.nb, c.T, c.is_static ? 1 : 0);
			k += (n == "chain_stages" || c.is_static) ? 1 : 0;
		}
		*value = k;
	}
	else if (n == "chain_static_table") *value = p->chain ? p->chain->static_check(0) : 0;      // entries of the compiled table, each checked against the FFT engine's plan of its lengths (throws on a mismatch)
	else throw Error(PXS_ERR_ARG, std::string("pxs_plan_query: unknown name '") + name + "'");
	PXS_CATCH
}

int pxs_plan_info(const pxs_plan* p, int* nsyn, int* nana, int64_t* scratch) {
	if (!p) return PXS_ERR_ARG;
	// rings of the Legendre stage of a spin-2 synthesis (the call's route) and of the interpolating analysis
	if (nsyn) *nsyn = route_of(p, false, 2, PXS_MODE_STANDARD, false, nullptr).rs->nring;
	if (nana) *nana = p->th.ncc > 0 ? p->th.ncc : p->nring;      // (the CC grid where the plan has one, whatever the analysis option: what this has always reported)
	if (scratch) *scratch = (int64_t)(p->leg.bytes + p->leg2.bytes + p->hbuf.bytes + p->b1.bytes + p->b2.bytes + p->wk.almt.bytes + p->wk.part.bytes + p->wk.mom.bytes);
	return 0;
}

/* planner of the fused theta chains (diagnostics / tests): out = {ok, g, bN, g2, M, ac, Ncc, gs, bs, aNs} */
int pxs_debug_theta_plan(int64_t N, int lmax, int64_t* out) {
	const ThetaPlan t = FftChain::plan_theta(N, lmax);
	const int64_t v[10] = {t.ok, t.g, t.bN, t.g2, t.M, t.ac, t.Ncc, t.gs, t.bs, t.aNs};
	for (int i = 0; i < 10; i++) out[i] = v[i];
	return 0;
}

/* diagnostics (tools/chain_lab.py): average ms of one fused-chain stage group of the plan on scratch data.
 * kind 0: map2leg (MA1, MA2), 1: h2map (MS1, MS2), 2: TH_TO_CC (RA1-5), 3: TH_FROM_CC (RS1-3), 4: TH_FROM_CC_ADJ */
int pxs_debug_chain(pxs_plan* p, int kind, int nc, int spin, int reps, double* ms) {
	PXS_TRY
	PXS_REQUIRE(p && ms && nc >= 1 && reps >= 1 && kind >= 0 && kind <= 4, "pxs_debug_chain: bad arguments");
	PXS_REQUIRE(p->chain_rings && (kind < 2 || p->chain_theta()), "pxs_debug_chain: the plan has no fused chain for this stage");
	PXS_HIP(hipSetDevice(p->device));
	std::lock_guard<std::mutex> plan_lock(p->call_mu);
	PlanUse use(p, nullptr);      // (runs on the NULL stream, on the plan's scratch)
	const size_t nm = (size_t)p->mmax + 1, nr = (size_t)p->nring, c16 = sizeof(double2);
	const long ldm = FftChain::pad8(p->nring), ldc = p->ld_cc(), ldh = p->ld_h();
	DevBuf dmap;
	if (kind < 2) { dmap.alloc(sizeof(double)*(size_t)nc*nr*p->nphi); PXS_HIP(hipMemset(dmap.p, 0, dmap.bytes)); }
	p->leg.ensure(c16*nc*nm*ldm); p->leg2.ensure(c16*nc*nm*std::max<long>(ldc, 8)); p->hbuf.ensure(c16*nc*nr*ldh);
	PXS_HIP(hipMemset(p->leg.p, 0, p->leg.bytes)); PXS_HIP(hipMemset(p->leg2.p, 0, p->leg2.bytes)); PXS_HIP(hipMemset(p->hbuf.p, 0, p->hbuf.bytes));
	hipStream_t st = nullptr;
	Route r;      // the theta stage groups: a route by hand, on the whole-grid strides
	r.ld_leg = ldm; r.nr_th = p->nring; r.ld_leg2 = ldc; r.ld_h = ldh; r.nr_h = p->nring;
	r.theta = kind == 2 ? TH_TO_CC : (kind == 3 ? TH_FROM_CC : TH_FROM_CC_ADJ);
	r.form = kind == 2 && ana_form(p).tp.ok ? &ana_form(p) : &p->ana_interp;      // (TH_TO_CC: the form the plan's analysis option selects, where the chains hold it)
	auto run = [&]() {
		const FftChain::MapDesc md = p->map_desc(MapArg{dmap.p, PX_F64, (long)nr*p->nphi, 0});
		if (kind == 0) p->chain->map2leg(st, md, nc, p->mmax, p->leg.as<double2>(), ldm, p->phase.as<double2>(), 1.0);
		else if (kind == 1) p->chain->h2map(st, p->hbuf.as<double2>(), ldh, md, nc, p->mmax);
		else run_theta(p, st, r, nc, spin, nullptr);
	};
	run(); PXS_HIP(hipStreamSynchronize(st));
	hipEvent_t e0, e1; PXS_HIP(hipEventCreate(&e0)); PXS_HIP(hipEventCreate(&e1));
	PXS_HIP(hipEventRecord(e0, st));
	for (int i = 0; i < reps; i++) run();
	PXS_HIP(hipEventRecord(e1, st)); PXS_HIP(hipEventSynchronize(e1));
	float t = 0; PXS_HIP(hipEventElapsedTime(&t, e0, e1));
	(void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
	*ms = (double)t/reps;
	PXS_CATCH
}

int pxs_profile(pxs_plan* p, int enable) {
	PXS_TRY
	PXS_REQUIRE(p, "pxs_profile: null plan");
	p->prof.enabled = enable != 0;
	if (enable && !p->wk.count.p) { PXS_HIP(hipSetDevice(p->device)); p->wk.count.alloc(4*1024*sizeof(double)); /* PXS_NCOUNT slots of four sums: legendre_dev.hpp */ PXS_HIP(hipMemset(p->wk.count.p, 0, p->wk.count.bytes)); }
	p->wk.count_on = enable != 0;
	PXS_CATCH
}

int pxs_profile_flops(pxs_plan* p, double* flops, int reset) {
	PXS_TRY
	PXS_REQUIRE(p && flops, "pxs_profile_flops: null argument");
	flops[0] = flops[1] = 0;
	if (!p->wk.count.p) return 0;
	PXS_HIP(hipSetDevice(p->device));
	PXS_HIP(hipDeviceSynchronize());
	std::vector<double> c(p->wk.count.bytes/sizeof(double)); PXS_HIP(hipMemcpy(c.data(), p->wk.count.p, p->wk.count.bytes, hipMemcpyDeviceToHost));
	for (size_t i = 0; i + 3 < c.size(); i += 4) { flops[0] += c[i]*128.0; flops[1] += c[i+1]*128.0; }     // FMA instructions per lane x 64 lanes x 2 flops (the wave counts of a slot: legendre_dev.hpp, PXS_COUNT_AT)
	if (reset) PXS_HIP(hipMemset(p->wk.count.p, 0, p->wk.count.bytes));
	PXS_CATCH
}

int pxs_profile_read(pxs_plan* p, double* ms, int* counts, int reset) {
	PXS_TRY
	PXS_REQUIRE(p && ms && counts, "pxs_profile_read: null argument");
	p->prof.read(ms, counts, PXS_NSTAGE, reset != 0);
	PXS_CATCH
}

// THE route decision of a call: every test of what the plan can do is here and nowhere else.
// analysis: pxs_analysis (else pxs_synthesis); tb: the recurrence tables of the spin (null: a query, which sizes nothing)
static Route route_of(const pxs_plan* p, bool analysis, int spin, int mode, bool adjoint, const LegTables* tb) {
	Route r;
	const int nr = p->nring;
	const bool th = p->chain_theta();
	const long ldm = p->ld_map(), ldc = p->ld_cc(), ldh = p->ld_h();
	r.to_map = analysis ? adjoint : !adjoint; r.tb = tb;
	r.nc = analysis ? (spin == 0 ? 1 : 2) : ncomp_of(spin, mode, false); r.deriv1 = mode == PXS_MODE_DERIV1;
	r.rs = &p->rs_map; r.nr_th = nr; r.form = &p->ana_interp;
	auto use_h = [&](int rows) { r.nr_h = rows; r.ld_h = ldh; };
	if (!analysis) {
		// Legendre stage on the minimal CC grid + exact Fourier resampling in theta where the map has clearly more rings (the thresholds of
		// setup_resampling): grids, and bands of F1 grids (their rows outside the band are zero)
		const bool cc = (p->is_grid || (p->band && th)) && (spin == 0 ? p->syn_via_cc0 : p->syn_via_cc) && p->th.ncc > 0;
		// (the adjoint takes the detour through the fused chain only; tools/adj_bench.py times it, profiles/r06_adj_bench.txt)
		r.ld_leg = r.ld_leg_alloc = ldm;
		if (!cc || (adjoint && !th)) { r.kind = R_DIRECT; if (!adjoint && !p->general) use_h(nr); }
		else {
			r.rs = &p->rs_cc; r.ld_leg2 = ldc; r.nr_th = p->band ? p->nfull : nr;      // (a band: the theta stage works on every ring of its grid)
			if (adjoint) { r.kind = R_VIA_CC; r.theta = TH_FROM_CC_ADJ; r.ld_leg = r.ld_leg_alloc = p->band ? FftChain::pad8(p->nfull) : ldm; }
			else if (th) { r.kind = R_VIA_CC; r.theta = TH_FROM_CC; use_h(r.nr_th); r.ld_leg = 0; }      // (leg: unused, but sized as it always was -- a plan's scratch_bytes are part of what it reports)
			// (a grid whose ring FFTs are chained but whose theta resampling is not -- 2 ntheta with a prime factor >= 7 -- and one without any chain)
			else { r.kind = !p->chain_rings ? R_VIA_CC_UNFUSED_H : R_VIA_CC_UNFUSED; r.theta = TH_FROM_CC; use_h(nr); r.ld_leg = nr; }      // (the unfused split writes dense rows)
		}
	} else if (p->wring.p) { r.kind = R_RING_WEIGHTS; }
	// ring weights on the map's own rings: the weights option, and ducc0's route on CC grids with >= 2 lmax + 2 rings (its
	// resample_to_prepared_CC multiplies such a grid by its weights directly: need_first_resample is false for it)
	else if ((p->ana_weights == 1 || (p->ana_weights == 2 && p->geometry == "CC")) && (long)nr >= 2L*p->lmax + 2)
		r.kind = (th && p->th.ncc > 0) ? R_CC_WEIGHTS : R_RING_WEIGHTS;
	else {
		r.form = &ana_form(p);
		// (the adjoint of the interpolant form: PXS_ADJ_ANA_FUSED=0 sends it through the unfused engine; read per call, the tests switch it.
		//  Unfused also: the fine-CC form on a plan whose chains cannot hold the circle of 2 N_cc points)
		auto adj_ana_fused = [] { const char* e = getenv("PXS_ADJ_ANA_FUSED"); return e ? atoi(e) != 0 : true; };
		r.kind = (th && (r.form->fine ? r.form->tp.ok : (!adjoint || adj_ana_fused()))) ? R_CHAIN : R_UNFUSED;
	}
	if (analysis) {      // buffers of the analysis routes: map -> leg [-> leg2] -> alm, or alm -> leg -> h -> map / alm -> leg2 -> h -> map
		if (r.kind == R_RING_WEIGHTS) { r.ld_leg = ldm; if (adjoint) use_h(nr); }
		else {
			r.rs = &p->rs_cc; r.ld_leg2 = r.kind == R_UNFUSED ? p->th.ncc : ldc;
			if (!adjoint || r.kind == R_UNFUSED) r.ld_leg = r.kind == R_UNFUSED ? nr : ldm;
			if (adjoint) use_h(nr);
			r.theta = r.kind == R_CC_WEIGHTS ? (adjoint ? TH_FROM_CC : TH_FROM_CC_ADJ) : (adjoint ? TH_TO_CC_ADJ : TH_TO_CC);
		}
		r.ld_leg_alloc = r.ld_leg;
	}
	const bool unfused = r.kind == R_VIA_CC_UNFUSED || r.kind == R_VIA_CC_UNFUSED_H || r.kind == R_UNFUSED;
	r.batched = !unfused;
	r.theta_fused = r.theta != TH_NONE && !unfused;
	r.line = r.theta_fused && r.theta <= TH_FROM_CC_ADJ && FftChain::line_takes(r.form->tp, r.theta == TH_TO_CC, r.form->sig_half.as<double>());
	// the ring chain's scratch is reserved with the call (the unfused analysis leaves it to the chain's own launches, as it always did)
	r.reserve_chain = p->chain_rings && r.kind != R_UNFUSED;
	return r;
}

// per-ring weight / nphi of the ring-weights paths (DH / F2: fixed at plan time; the weights option: built on first use)
static const double2* ring_weights(pxs_plan* p) {
	if (p->wring.p) return p->wring.as<double2>();
	if (!p->th.wgrid.p) p->th.wgrid = ring_weight_table(p->geometry, p->nring, p->nphi);
	return p->th.wgrid.as<double2>();
}
// ... for the transposed theta upsampling (TH_FROM_CC_ADJ): its first stage extends the weighted ring samples to the circle
// by reflection, which holds a self-mirrored ring (the pole rings of CC, one of MW / MWflip) once and every other ring twice -- the
// zero extension it stands for is half the sum of the symmetric and the antisymmetric one, so the self-mirrored rings count double
static const double2* ring_weights_ext(pxs_plan* p) {
	const double2* w = ring_weights(p);
	if (p->geometry == "F1") return w;
	if (!p->th.wgrid_ext.p) {
		std::vector<double2> wd(p->nring);
		PXS_HIP(hipMemcpy(wd.data(), w, sizeof(double2)*p->nring, hipMemcpyDeviceToHost));
		for (int r = 0; r < p->nring; r++) if (self_mirrored(r, p->th.mir_c, p->th.N)) wd[r].x *= 2;
		p->th.wgrid_ext = upload(wd);
	}
	return p->th.wgrid_ext.as<double2>();
}

// unit weights for the transposed theta upsampling on grids with self-mirrored rings (see ring_weights_ext); null on F1 grids
static const double2* unit_weights_ext(pxs_plan* p) {
	if (p->geometry == "F1" || p->band) return nullptr;
	if (!p->th.wunit_ext.p) {
		std::vector<double2> wd(p->nring, make_double2(1, 0));
		for (int r = 0; r < p->nring; r++) if (self_mirrored(r, p->th.mir_c, p->th.N)) wd[r].x = 2;
		p->th.wunit_ext = upload(wd);
	}
	return p->th.wunit_ext.as<double2>();
}

// The nb maps of one pass of a call (nb > 1 only on the batched routes): ring FFTs of all maps in one launch each, theta chains and
// Legendre kernels map by map on the plan's scratch.  Every route is one of two stage sequences, alm -> [leg2 ->] leg / h -> map or its
// mirror image; the strides, ring sets and tables are the route's.
static void run_core(pxs_plan* p, const Route& r, int spin, int nb, const AlmArg& alm, const MapArg& map, hipStream_t st)
{
	const int nct = nb*r.nc, nr = p->nring, nm = p->mmax + 1;
	double2* leg = p->leg.as<double2>();
	switch (r.kind) {
	case R_VIA_CC_UNFUSED: case R_VIA_CC_UNFUSED_H: {      // (synthesis only; the unfused resamplers size their own b1 / b2)
		PXS_REQUIRE(nb == 1, "internal: batched call on an unfused path");
		const bool to_h = r.kind == R_VIA_CC_UNFUSED_H;
		p->leg_syn(st, r, alm, 1);
		resample_from_cc(p, st, p->leg2.as<double2>(), leg, r.nc, spin, to_h ? p->hbuf.as<double2>() : nullptr);
		leg2map(p, st, r, to_h ? nullptr : leg, r.ld_leg, map, 1);
		return; }
	case R_UNFUSED:      // analysis_2d / adjoint_analysis_2d stage by stage through the generic FFT engine
		PXS_REQUIRE(nb == 1, "internal: batched call on an unfused path");
		if (r.to_map) {
			p->leg_syn(st, r, alm, 1);
			resample_to_cc_adjoint(p, st, p->leg2.as<double2>(), leg, r.nc, spin, *r.form);
			leg2map(p, st, r, leg, r.ld_leg, map, 1);
		} else {
			map2leg(p, st, r, map, 1, leg);
			resample_to_cc(p, st, leg, p->leg2.as<double2>(), r.nc, spin, *r.form);
			p->leg_ana(st, r, alm, 1);
		}
		return;
	default: break;
	}
	// the fused routes.  Weights: of the rings in the weights forms of the analysis (R_RING_WEIGHTS: on leg itself; R_CC_WEIGHTS: folded into
	// the theta stage, self-mirrored rings doubled where it is the transposed upsampling); the adjoint of the CC-grid synthesis on grids
	// with self-mirrored rings (CC / MW / MWflip) counts those double in the reflection that stands for the zero extension
	const double2* wleg = r.kind == R_RING_WEIGHTS ? ring_weights(p) : nullptr;
	const double2* wth = r.kind == R_CC_WEIGHTS ? (r.to_map ? ring_weights(p) : ring_weights_ext(p)) : (r.kind == R_VIA_CC && !r.to_map ? unit_weights_ext(p) : nullptr);
	auto weigh = [&] { if (wleg) scale_leg_rings(st, leg, (long)nct*nm, nr, r.ld_leg, wleg); };
	auto theta = [&] { if (r.theta != TH_NONE) { StageScope stage(p->prof, st, PXS_STAGE_RESAMPLE); run_theta(p, st, r, nct, spin, wth); } };
	if (r.to_map) {
		p->leg_syn(st, r, alm, nb);
		weigh();
		theta();      // (writes h ring-major for the ring FFT)
		leg2map(p, st, r, r.theta != TH_NONE ? nullptr : leg, r.ld_leg, map, nb);
	} else {
		if (r.nr_th > nr) {      // a band through the CC grid: leg holds every ring of the grid, zero outside the band's rows
			PXS_HIP(hipMemsetAsync(p->leg.p, 0, sizeof(double2)*(size_t)nct*nm*r.ld_leg, st));
			leg += p->row0;
		}
		map2leg(p, st, r, map, nb, leg);
		weigh();
		theta();
		p->leg_ana(st, r, alm, nb);
	}
}

// Scratch of a call is sized HERE and only here, from its route, before its first launch (a plan's buffers only grow, so this
// allocates on the first call of a kind and when a later call brings a larger batch).  What is sized elsewhere, at the point of use,
// belongs to the rarely taken paths: z of the general ring sets (sht_general.hip), the packed spectra of the unfused ring FFT and
// b1 / b2 of the unfused theta resamplers, the partial moments of the deterministic analysis (legendre.hip).  A buffer that grows gives
// its old block to the arena while the launches that use it may still be queued (of the plan's previous call on another stream): the
// arena synchronises the device before that block serves anybody else (arena.hip), and a block below the arena's threshold goes
// through hipFree, which waits for the device.
static void reserve_call(pxs_plan* p, const Route& r, int nb) {
	const Route::Scratch s = r.scratch(p, nb);
	p->wk.almt.ensure(s.almt); p->wk.mom.ensure(s.mom);
	p->leg.ensure(s.leg); p->leg2.ensure(s.leg2); p->hbuf.ensure(s.h);
	if (r.reserve_chain) p->chain->reserve(std::max(s.c1, s.r1), s.c2);
}

// maps per pass of a batched call: bounded by the scratch the plan may hold (leg + leg_cc + h per map, and the chain scratch)
static int batch_chunk(const pxs_plan* p, int nbatch, int ncm) {
	if (nbatch <= 1 || !p->chain_rings) return 1;           // the unfused paths take one map at a time
	const size_t per_map = sizeof(double2)*(size_t)ncm*((size_t)(p->mmax+1)*(p->nring + (p->th.ncc > 0 ? p->th.ncc : 0))*2 + (size_t)p->nring*p->nphi);
	// scratch budget of one pass: PXS_BATCH_GB, default 64 GB (MI355X: 288 GB; 8 maps of config 5 = 56 GB, so that the batched Legendre kernels get
	// their 8-map groups there; it was 32 in rounds 2-4), never more than 40 % of what is free on the device now beyond what the plan holds already
	size_t budget_env = 0; env_budget("PXS_BATCH_GB", 30, budget_env);      // (per call; unset or 0: the default rule)
	size_t budget = budget_env ? budget_env : (size_t)64 << 30;
	if (!budget_env) {
		size_t fr = 0, tot = 0;
		const size_t held = p->leg.bytes + p->leg2.bytes + p->hbuf.bytes + (p->chain ? p->chain->scratch_bytes() : 0);
		if (hipMemGetInfo(&fr, &tot) == hipSuccess && fr > 0) budget = std::min(budget, std::max<size_t>((size_t)4 << 30, held + (size_t)(0.4*(double)fr)));
	}
	const int cap = (int)std::max<size_t>(1, std::min<size_t>((size_t)nbatch, budget/std::max<size_t>(per_map, 1)));
	if (ncm == 1 && cap >= 8 && nbatch > cap) {      // scalar maps: the batched Legendre analysis works on groups of 8 maps (leg_ana_s0_mm)
		const int cap8 = cap & ~7, npass = (nbatch + cap8 - 1)/cap8;
		return std::min(cap8, (((nbatch + npass - 1)/npass + 7)/8)*8);
	}
	const int npass = (nbatch + cap - 1)/cap;
	return (nbatch + npass - 1)/npass;      // equal passes (64 maps at 15 per pass: 13 x 4 + 12, not 15 x 4 + 4 with a last pass at 27 % of the batch dimension)
}

// a call after its argument checks (call_mu held, the plan's device selected): route, scratch, then the maps in passes
static void run_call(pxs_plan* p, bool analysis, int spin, int mode, int adjoint, int nbatch, const AlmArg& alm, const MapArg& map, hipStream_t st) {
	const Route r = route_of(p, analysis, spin, mode, adjoint != 0, &p->table(spin));
	const int chunk = r.batched ? batch_chunk(p, nbatch, r.nc) : 1;
	if (getenv("PXS_CHAIN_VERBOSE")) fprintf(stderr, "[pxsht] %s route %s, adjoint %d, spin %d, analysis option %d, %d maps in passes of %d\n", analysis ? "analysis" : "synthesis", ROUTE_NAMES[r.kind], adjoint, spin, p->ana_weights, nbatch, chunk);
	reserve_call(p, r, std::min(chunk, nbatch));
	// the pass reports are those of THIS call: a seam the call does not come by reports no pass
	p->pass_batch.begin(); p->pass_resample.begin(); p->wk.pass_m.begin(); p->wk.pass_valu.begin(); p->wk.pass_mm.begin();
	if (p->chain) { p->chain->pass_theta.begin(); p->chain->pass_ring.begin(); }
	for (int b0 = 0; b0 < nbatch; b0 += chunk) {
		p->pass_batch.add(std::min(chunk, nbatch - b0));
		run_core(p, r, spin, std::min(chunk, nbatch - b0), alm.from(b0), map.from(b0), st);
	}
}

int pxs_synthesis(pxs_plan* p, int spin, int mode, int adjoint, int nbatch,
                  void* alm, int alm_dtype, int64_t alm_cstride, int64_t alm_bstride,
                  void* map, int map_dtype, int64_t map_cstride, int64_t map_bstride, void* stream)
{
	PXS_TRY
	PXS_REQUIRE(p && alm && map, "pxs_synthesis: null argument");
	std::lock_guard<std::mutex> plan_lock(p->call_mu);
	PXS_REQUIRE(!p->pts || p->pgrid, "pxs_synthesis: a map points plan interpolates maps (pxm_map_points), it has no alm");
	PXS_REQUIRE(spin >= 0 && spin <= p->lmax + 1, "pxs_synthesis: bad spin");
	PXS_REQUIRE(mode == PXS_MODE_STANDARD || (mode == PXS_MODE_DERIV1 && spin == 1), "DERIV1 needs spin 1");
	PXS_REQUIRE(map_dtype == PX_F32 || map_dtype == PX_F64, "map must be float32 or float64");
	PXS_REQUIRE(nbatch >= 1, "pxs_synthesis: nbatch must be >= 1");
	PXS_HIP(hipSetDevice(p->device));
	hipStream_t st = (hipStream_t)stream;
	PlanUse use(p, st);      // (a points plan: its own scratch here, the grid plan's in the pxs_synthesis calls points_run makes on it)
	const AlmArg a{alm, alm_dtype, (long)alm_cstride, (long)alm_bstride}; const MapArg m{map, map_dtype, (long)map_cstride, (long)map_bstride};
	if (p->pts) points_run(p->pts, p->pgrid, spin, mode, adjoint, nbatch, a, m, st);
	else run_call(p, false, spin, mode, adjoint, nbatch, a, m, st);
	PXS_CATCH
}

int pxs_analysis(pxs_plan* p, int spin, int adjoint, int nbatch,
                 void* map, int map_dtype, int64_t map_cstride, int64_t map_bstride,
                 void* alm, int alm_dtype, int64_t alm_cstride, int64_t alm_bstride, void* stream)
{
	PXS_TRY
	PXS_REQUIRE(p && alm && map, "pxs_analysis: null argument");
	std::lock_guard<std::mutex> plan_lock(p->call_mu);
	PXS_REQUIRE(p->is_grid, "pxs_analysis needs a grid2d plan");
	PXS_REQUIRE(map_dtype == PX_F32 || map_dtype == PX_F64, "map must be float32 or float64");
	PXS_REQUIRE(nbatch >= 1, "pxs_analysis: nbatch must be >= 1");
	if (p->lmax > grid_maxlmax(p->geometry, p->nring)) throw Error(PXS_ERR_ARG, "too few rings for analysis up to requested lmax");
	PXS_HIP(hipSetDevice(p->device));
	hipStream_t st = (hipStream_t)stream;
	PlanUse use(p, st);
	run_call(p, true, spin, PXS_MODE_STANDARD, adjoint, nbatch, AlmArg{alm, alm_dtype, (long)alm_cstride, (long)alm_bstride}, MapArg{map, map_dtype, (long)map_cstride, (long)map_bstride}, st);
	PXS_CATCH
}

} // extern "C"