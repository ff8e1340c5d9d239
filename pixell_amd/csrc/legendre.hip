// Legendre stage of the SHT for gfx950: alm <-> leg[comp][m][ring].
//
// Replaces ducc0's alm2leg / leg2alm (inside ducc0.sht.experimental.*; not in the reference
// tree) as reached from pixell/curvedsky.py:907-960, 1032-1084.
//
// Design (MI355X-first).  A single map is 1-4 right-hand sides wide, too narrow for the 16x16x4 f64 MFMA: it runs on plain FP64 FMA as
// described below.  A batch of 4 or more maps shares one recurrence per ring pair and is contracted with the f64 MFMA (leg_*_mm,
// leg_s0.hip / leg_spin.hip; leg_batch_plan below says which maps go where).  The VALU kernels:
//  * one wave64 per workgroup; a lane owns K ring PAIRS (theta, pi-theta) => K independent
//    recurrence chains of ILP per lane, north/south sharing one recurrence;
//  * spin 0: Ishioka-type two-step recurrence in x^2, p_{k+1} = (a_k x^2 + b_k) p_k + p_{k-1},
//    p_k ~ lambda_{m+2k+1,m}/x: 2 FMA of recurrence serve TWO degrees l, 4 FMA accumulate;
//    spin s: scaled three-term recurrence for (s)lambda and (-s)lambda, 4 FMA + 8 FMA per l;
//  * per-step coefficients (a,b) and the pre-scaled alm are wave-uniform: they are fetched with
//    scalar loads and fed to v_fma_f64 as SGPR operands, the recurrence state and the
//    accumulators stay in VGPRs for the whole l loop;
//  * extended exponent: lambda_mm ~ sin^m(theta) underflows for large m, so a chain starts as
//    (mantissa, scale) with value = mantissa * 2^(800*scale), is advanced without accumulating
//    until some lane of the wave is live (scale 0 and |value| >= LEG_LIVE = 2^-140, legendre_dev.hpp), then advanced with
//    accumulation until all lanes are at scale 0, then runs the branch-free fast loop; a wave's 64 K pairs are consecutive, pole first, with the
//    padding in wave 0 (leg_pair_of);
//  * analysis needs the sum over rings (lanes) for every l: the 4 sums of a step are reduce-scattered over the lanes with
//    v_permlane32_swap / v_permlane16_swap, one ds_write_b64 per step parks them in a tile of 16 steps; at a flush lane j owns
//    output j, adds its 16 partial sums and the wave issues one contiguous 512-byte global_atomic_add_f64 into the moments
//    (PXS_DETERMINISTIC=1: per-wave partial moments summed in wave order by reduce_partials instead).
// Translation units: this file holds the host side (tables, seeds, dispatch), the alm pre / post kernels and the table kernels.  legendre_dev.hpp holds the
// code of the kernels that does not depend on spin or direction: the pair map, the reduction tile, and leg_ana_mm<Sys, NG, W> / leg_syn_mm<Sys, NG>, the one
// analysis and the one synthesis body of the four MFMA kernels.  leg_s0.hip and leg_spin.hip hold the 18 kernel instantiations and what differs between the MFMA
// kernels, as the policies S0Mm / SpinMm (chain, phase A, table, slots per wave, the parked ring data, the synthesis epilogue).  The four VALU kernels (leg_syn_s0,
// leg_ana_s0, leg_syn_spin, leg_ana_spin) each write the phase skeleton out, with the macros S0_* / SPIN_* at the head of their file: one driver with policies was
// built for them and is not here (leg_spin.hip and profiles/README.md say why) -- change the four copies together.  launch_leg_s0 / launch_leg_spin pick the
// kernel of (direction, form, K or ng).
#include "legendre_dev.hpp"
#include <thread>
#include <memory>
#include <functional>
#include <string>

namespace pxs {

// ring pairs per lane (K) of the VALU kernels: chosen by measurement on MI355X (profiles/r04_ktune_c3.txt, profiles/r05_dp_rate_and_k_waves.txt;
// leg_ana_spin<4>: 3 waves per SIMD, K = 6 has 2: 146.9 against 150.5 ms at config 3, before the one-drain row prefetch); k_small_grid lowers them on small ring
// sets, leg_ana_k raises the analysis ones on large ring sets
static constexpr int K_SYN0 = 4, K_ANA0 = 8, K_SYNS = 3, K_ANAS = 4;

// ---------------------------------------------------------------------------------
// alm pre / post transforms
// ---------------------------------------------------------------------------------
__device__ __forceinline__ double2 ld_alm(const void* alm, int dtype, long idx) {
	if (dtype == PX_C64) { float2 v = ((const float2*)alm)[idx]; return make_double2(v.x, v.y); }
	return ((const double2*)alm)[idx];
}
__device__ __forceinline__ void st_alm(void* alm, int dtype, long idx, double2 v) {
	if (dtype == PX_C64) ((float2*)alm)[idx] = make_float2((float)v.x, (float)v.y);
	else ((double2*)alm)[idx] = v;
}
__device__ __forceinline__ double eps_lm(int l, int m) {
	if (l <= m) return 0.0;
	double L = l, M = m;
	return sqrt((L*L - M*M)/(4.0*L*L - 1.0));
}

struct AlmK {
	int lmax, mmax, spin, deriv1, dtype;
	long nrows, cstride, lstride;
	const long* row; const double* alpha; const uint64_t* mstart;
	void* alm; double* almt; const double* mom;
	long alm_bs, almt_bs, mom_bs;      // batched calls: blockIdx.z = map; strides in alm elements / doubles
};
__device__ __forceinline__ void* alm_of_batch(const AlmK& a) { return (char*)a.alm + (size_t)(a.dtype == PX_C64 ? 8 : 16)*(size_t)blockIdx.z*(size_t)a.alm_bs; }

// Each thread takes ALM_U rows 256 apart and issues all their loads before the first store: with one row per thread a wave had 1 KB of
// loads in flight behind a chain of dependent scalar loads (alm_pre_spin 1.15 TB/s at config 3).
#define ALM_U 4
static inline dim3 alm_grid(int nrows, int nm, int nb) { return dim3((unsigned)((nrows + 256*ALM_U - 1)/(256*ALM_U)), (unsigned)nm, (unsigned)nb); }
// spin 0: almt[row(m)+k] = alpha_k * ( eps_{l+1} a_l + eps_{l+2} a_{l+2},  a_{l+1} ),  l = m+2k
__global__ __launch_bounds__(256) void alm_pre_s0(AlmK a) {
	const int m = blockIdx.y;
	const int nk = (a.lmax - m)/2 + 1;
	const int kb = blockIdx.x*(256*ALM_U) + threadIdx.x;
	if (kb >= nk) return;
	const long base = (long)a.mstart[m];
	const long row = a.row[m];
	const void* alm = alm_of_batch(a);
	double2 a0[ALM_U], a1[ALM_U], a2[ALM_U]; double al[ALM_U];
#pragma unroll
	for (int u = 0; u < ALM_U; u++) {
		const int k = kb + 256*u, l = m + 2*k;
		const bool ok = k < nk;
		a0[u] = ok ? ld_alm(alm, a.dtype, base + (long)l*a.lstride) : make_double2(0, 0);
		a1[u] = (ok && l+1 <= a.lmax) ? ld_alm(alm, a.dtype, base + (long)(l+1)*a.lstride) : make_double2(0, 0);
		a2[u] = (ok && l+2 <= a.lmax) ? ld_alm(alm, a.dtype, base + (long)(l+2)*a.lstride) : make_double2(0, 0);
		al[u] = ok ? a.alpha[row + k] : 0.0;
	}
#pragma unroll
	for (int u = 0; u < ALM_U; u++) {
		const int k = kb + 256*u, l = m + 2*k;
		if (k >= nk) break;
		const double e1 = eps_lm(l+1, m), e2 = eps_lm(l+2, m);
		double* o = a.almt + (long)blockIdx.z*a.almt_bs + 4*(row + k);
		o[0] = al[u]*(e1*a0[u].x + e2*a2[u].x); o[1] = al[u]*(e1*a0[u].y + e2*a2[u].y);
		o[2] = al[u]*a1[u].x;                   o[3] = al[u]*a1[u].y;
	}
}
// a_{m+2k} = eps_{l+1} alpha_k M1_k + eps_l alpha_{k-1} M1_{k-1};  a_{m+2k+1} = alpha_k M2_k
__global__ __launch_bounds__(256) void alm_post_s0(AlmK a) {
	const int m = blockIdx.y;
	const int nk = (a.lmax - m)/2 + 1;
	const int kb = blockIdx.x*(256*ALM_U) + threadIdx.x;
	if (kb >= nk) return;
	const long row = a.row[m];
	const long base = (long)a.mstart[m];
	void* alm = alm_of_batch(a);
	double M0[ALM_U], M1[ALM_U], M2[ALM_U], M3[ALM_U], P0[ALM_U], P1[ALM_U], al[ALM_U], alp[ALM_U];
#pragma unroll
	for (int u = 0; u < ALM_U; u++) {
		const int k = kb + 256*u;
		const bool ok = k < nk;
		const long r = row + k;
		const double* M = a.mom + (long)blockIdx.z*a.mom_bs + 4*r;
		M0[u] = ok ? M[0] : 0.0; M1[u] = ok ? M[1] : 0.0; M2[u] = ok ? M[2] : 0.0; M3[u] = ok ? M[3] : 0.0;
		al[u] = ok ? a.alpha[r] : 0.0;
		const bool prev = ok && k > 0;
		P0[u] = prev ? M[-4] : 0.0; P1[u] = prev ? M[-3] : 0.0; alp[u] = prev ? a.alpha[r-1] : 0.0;
	}
#pragma unroll
	for (int u = 0; u < ALM_U; u++) {
		const int k = kb + 256*u, l = m + 2*k;
		if (k >= nk) break;
		const double e1 = eps_lm(l+1, m), e0 = eps_lm(l, m);
		double2 v = make_double2(e1*al[u]*M0[u], e1*al[u]*M1[u]);
		if (k > 0) { v.x += e0*alp[u]*P0[u]; v.y += e0*alp[u]*P1[u]; }
		st_alm(alm, a.dtype, base + (long)l*a.lstride, v);
		if (l+1 <= a.lmax) st_alm(alm, a.dtype, base + (long)(l+1)*a.lstride, make_double2(al[u]*M2[u], al[u]*M3[u]));
	}
}
// spin s: rows l = l0..lmax; almt = beta_l * ( a+ = -(E+iB),  a- = -(-1)^s (E-iB) )
__global__ __launch_bounds__(256) void alm_pre_spin(AlmK a) {
	const int m = blockIdx.y;
	const int l0 = max(m, a.spin);
	const int lb = l0 + blockIdx.x*(256*ALM_U) + threadIdx.x;
	if (lb > a.lmax) return;
	const long base = (long)a.mstart[m], row = a.row[m];
	const void* alm = alm_of_batch(a);
	double2 E[ALM_U], B[ALM_U]; double be[ALM_U];
#pragma unroll
	for (int u = 0; u < ALM_U; u++) {
		const int l = lb + 256*u;
		const bool ok = l <= a.lmax;
		const long idx = base + (long)l*a.lstride;
		E[u] = ok ? ld_alm(alm, a.dtype, idx) : make_double2(0, 0);
		B[u] = (ok && !a.deriv1) ? ld_alm(alm, a.dtype, idx + a.cstride) : make_double2(0, 0);
		be[u] = ok ? a.alpha[row + (l - l0)] : 0.0;
	}
	const double sg = (a.spin & 1) ? -1.0 : 1.0;
#pragma unroll
	for (int u = 0; u < ALM_U; u++) {
		const int l = lb + 256*u;
		if (l > a.lmax) break;
		double2 e = E[u]; const double2 b = B[u];
		if (a.deriv1) { const double f = sqrt((double)l*(l+1.0)); e.x *= f; e.y *= f; }
		double* o = a.almt + (long)blockIdx.z*a.almt_bs + 4*(row + (l - l0));
		o[0] = -be[u]*(e.x - b.y); o[1] = -be[u]*(e.y + b.x);
		o[2] = -sg*be[u]*(e.x + b.y); o[3] = -sg*be[u]*(e.y - b.x);
	}
}
// E = -1/2 beta (mu+ + sg mu-),  B = i/2 beta (mu+ - sg mu-)
__global__ __launch_bounds__(256) void alm_post_spin(AlmK a) {
	const int m = blockIdx.y;
	const int l0 = max(m, a.spin);
	const int lb = blockIdx.x*(256*ALM_U) + threadIdx.x + min(m, l0);   // also zero-fill m <= l < l0
	if (lb > a.lmax) return;
	const long base = (long)a.mstart[m], row = a.row[m];
	void* alm = alm_of_batch(a);
	double M0[ALM_U], M1[ALM_U], M2[ALM_U], M3[ALM_U], be[ALM_U];
#pragma unroll
	for (int u = 0; u < ALM_U; u++) {
		const int l = lb + 256*u;
		const bool ok = l <= a.lmax && l >= l0;
		const long r = row + (l - l0);
		const double* M = a.mom + (long)blockIdx.z*a.mom_bs + 4*r;
		M0[u] = ok ? M[0] : 0.0; M1[u] = ok ? M[1] : 0.0; M2[u] = ok ? M[2] : 0.0; M3[u] = ok ? M[3] : 0.0;
		be[u] = ok ? a.alpha[r] : 0.0;
	}
	const double sg = (a.spin & 1) ? -1.0 : 1.0;
#pragma unroll
	for (int u = 0; u < ALM_U; u++) {
		const int l = lb + 256*u;
		if (l > a.lmax) break;
		const long idx = base + (long)l*a.lstride;
		// (rows m <= l < l0: be = 0 and the moments read as 0: E = B = 0)
		const double2 E = make_double2(-0.5*be[u]*(M0[u] + sg*M2[u]), -0.5*be[u]*(M1[u] + sg*M3[u]));
		const double2 B = make_double2(-0.5*be[u]*(M1[u] - sg*M3[u]),  0.5*be[u]*(M0[u] - sg*M2[u]));
		if (a.deriv1) { const double f = sqrt((double)l*(l+1.0)); st_alm(alm, a.dtype, idx, make_double2(f*E.x, f*E.y)); }
		else { st_alm(alm, a.dtype, idx, E); st_alm(alm, a.dtype, idx + a.cstride, B); }
	}
}

// mom[row] = sum over the waves that wrote that row.  A wave writes rows from the end of its phase A on and nothing at all
// when none of its rings is live for this m; `first` says which (36 % of the (wave, m) pairs are dead at config 3, and the
// 16 GiB partial buffer no longer needs a memset before every launch).
__global__ __launch_bounds__(256) void reduce_partials(const double* __restrict__ part, double* __restrict__ mom, const long* __restrict__ row,
		const int* __restrict__ first, int m0, int nmc, long rowbase, long rows_chunk, int nwave)
{
	const int mi = blockIdx.y;
	const long r0 = row[m0 + mi], nrow = row[m0 + mi + 1] - r0;
	const long i = (long)blockIdx.x*blockDim.x + threadIdx.x;      // 4*step + component
	if (i >= 4*nrow) return;
	const int step = (int)(i >> 2);
	const long off = (r0 - rowbase)*4 + i;
	double s = 0;
	for (int w = 0; w < nwave; w++) {
		const int f = first[w*nmc + mi];
		if (f > 0 && step >= f - 1) s += part[(long)w*rows_chunk*4 + off];
	}
	mom[r0*4 + i] = s;
}

// compact step table: (a, b) or (a, a + b) of the rows of LegTables::coef; 32 rows of padding (a tile reads 16 steps whatever nk is).  c2p: spin 0 only (null otherwise)
__global__ __launch_bounds__(256) void coef2_kernel(const double4_t* __restrict__ coef, long nrows, double2* __restrict__ c2, double2* __restrict__ c2p) {
	const long i = (long)blockIdx.x*blockDim.x + threadIdx.x;
	if (i >= nrows + 32) return;
	const double4_t c = i < nrows ? coef[i] : double4_t{0, 0, 0, 0};
	c2[i] = make_double2(c.a, c.b);
	if (c2p) c2p[i] = make_double2(c.a, c.c);
}


// ---------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------
void LegProfile::begin(hipStream_t st, int stage) {
	if (!enabled) return;
	hipEvent_t e; PXS_HIP(hipEventCreate(&e)); PXS_HIP(hipEventRecord(e, st)); open_.push_back(e);
}
void LegProfile::end(hipStream_t st, int stage) {
	if (!enabled || open_.empty()) return;
	hipEvent_t e; PXS_HIP(hipEventCreate(&e)); PXS_HIP(hipEventRecord(e, st));
	recs.push_back(Rec{open_.back(), e, stage}); open_.pop_back();
}
void LegProfile::read(double* ms, int* counts, int nstage, bool reset) {
	for (int i = 0; i < nstage; i++) { ms[i] = 0; counts[i] = 0; }
	for (auto& r : recs) {
		PXS_HIP(hipEventSynchronize(r.b));
		float t = 0; PXS_HIP(hipEventElapsedTime(&t, r.a, r.b));
		if (r.stage >= 0 && r.stage < nstage) { ms[r.stage] += t; counts[r.stage]++; }
	}
	if (reset) { for (auto& r : recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); } recs.clear(); }
}
LegProfile::~LegProfile() { for (auto& r : recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); } for (auto e : open_) (void)hipEventDestroy(e); }

void RingSet::build(const std::vector<long double>& theta) {
	const long double PIl = 3.141592653589793238462643383279502884L;
	nring = (int)theta.size();
	std::vector<char> used(nring, 0);
	ring_n.clear(); ring_s.clear(); cth.clear(); sth.clear(); sh2.clear(); ch2.clear();
	// order pairs by colatitude of the northern member (pole first)
	std::vector<int> order(nring);
	for (int i = 0; i < nring; i++) order[i] = i;
	std::stable_sort(order.begin(), order.end(), [&](int x, int y) {
		long double a = std::min(theta[x], PIl - theta[x]), b = std::min(theta[y], PIl - theta[y]); return a < b; });
	// fast path for symmetric ascending grids: partner of i is nring-1-i
	for (int oi = 0; oi < nring; oi++) {
		int i = order[oi];
		if (used[i]) continue;
		used[i] = 1;
		int partner = -1;
		int cand = nring-1-i;
		const long double tol = 1e-12L;
		if (cand != i && cand >= 0 && !used[cand] && fabsl(theta[cand] - (PIl - theta[i])) < tol) partner = cand;
		else {
			for (int j = 0; j < nring; j++) if (!used[j] && j != i && fabsl(theta[j] - (PIl - theta[i])) < tol) { partner = j; break; }
		}
		int in_ = i, is_ = partner;
		if (partner >= 0) { used[partner] = 1; if (theta[partner] < theta[i]) { in_ = partner; is_ = i; } }
		long double th = theta[in_];
		bool flipped = false;
		if (partner < 0 && th > PIl/2) { th = PIl - th; flipped = true; }   // lone southern ring: treat via its mirror
		if (flipped) { ring_n.push_back(-1); ring_s.push_back(in_); }
		else { ring_n.push_back(in_); ring_s.push_back(is_); }
		cth.push_back((double)cosl(th)); sth.push_back((double)sinl(th));
		sh2.push_back((double)sinl(th/2)); ch2.push_back((double)cosl(th/2));
	}
	npairs = (int)ring_n.size();
}
void RingSet::upload_all() {
	d_ring_n = upload(ring_n); d_ring_s = upload(ring_s); d_cth = upload(cth); d_sth = upload(sth);
	d_sh2 = upload(sh2); d_ch2 = upload(ch2);
}

void LegTables::build_host(int lmax_, int mmax_, int spin_) {
	lmax = lmax_; mmax = mmax_; spin = spin_;
	row.assign(mmax+2, 0);
	for (int m = 0; m <= mmax; m++) {
		long n = spin == 0 ? (lmax - m)/2 + 1 : std::max(0, lmax - std::max(m, spin) + 1);
		row[m+1] = row[m] + n;
	}
	nrows = row[mmax+1];
	// +4: the fast loops prefetch up to 3 rows ahead.  Uninitialised storage: every row is written below by the thread that owns its m
	// (a zero-filled std::vector costs a single-threaded first touch of 3 GB at lmax 10^4: more than the square roots)
	std::unique_ptr<double4_t[]> coef_(new double4_t[nrows + 4]); std::unique_ptr<double[]> alpha_(new double[nrows + 4]);
	double4_t* coef = coef_.get(); double* alpha = alpha_.get();
	for (long i = nrows; i < nrows + 4; i++) { coef[i] = double4_t{0, 0, 0, 0}; alpha[i] = 0.0; }
	typedef long double LDb;
	const LDb PIl = 3.141592653589793238462643383279502884L;
	// The rows of different m are independent (the sectoral start values are a short serial prefix): m is dealt cyclically to host
	// threads -- the table of a 21600-ring, lmax 10^4 plan is 7.5e7 rows of 4-6 long-double square roots, 8 s on one core.
	static const int nthr_env = [] { const char* e = getenv("PXS_TABLE_THREADS"); return e ? atoi(e) : 0; }();
	const int nthr = (int)std::max(1L, std::min<long>({(long)(nthr_env > 0 ? nthr_env : 32), (long)std::max(1u, std::thread::hardware_concurrency()), (long)mmax + 1, nrows/4096 + 1}));
	auto run_threads = [&](auto&& body) {      // body(m)
		if (nthr == 1) { for (int m = 0; m <= mmax; m++) body(m); return; }
		std::vector<std::thread> th;
		for (int t = 0; t < nthr; t++) th.emplace_back([&, t] { for (int m = t; m <= mmax; m += nthr) body(m); });
		for (auto& x : th) x.join();
	};
	if (spin == 0) {
		std::vector<LDb> cms(mmax+1);
		{ LDb cm = 1/sqrtl(4*PIl); for (int m = 0; m <= mmax; m++) { if (m > 0) cm = -cm*sqrtl((LDb)(2*m+1)/(LDb)(2*m)); cms[m] = cm; } }
		run_threads([&](int m) {
			const LDb cm = cms[m];
			auto eps = [&](int l) -> LDb { if (l <= m) return 0; LDb L = l, M = m; return sqrtl((L*L-M*M)/(4*L*L-1)); };
			const int nk = (lmax - m)/2 + 1;
			LDb a_prev = 0, a_cur = sqrtl((LDb)(2*m+3))*cm;   // alpha_{k-1}, alpha_k
			for (int k = 0; k < nk; k++) {
				const int lp = m + 2*k + 1;
				const LDb e2 = eps(lp+1)*eps(lp+1) + eps(lp)*eps(lp), f = eps(lp)*eps(lp-1), d = eps(lp+1)*eps(lp+2);
				const LDb a_next = (k == 0) ? a_cur/d : -f*a_prev/d;
				const LDb ak = a_cur/(a_next*d);
				coef[row[m]+k] = double4_t{(double)ak, (double)(-ak*e2), (double)(ak - ak*e2), 0.0};
				alpha[row[m]+k] = (double)a_cur;
				a_prev = a_cur; a_cur = a_next;
			}
		});
	} else {
		const int s = spin;
		// m < s: h(m) = (2s+1)(2s)!/((s+m)!(s-m)!) ; m >= s: c'_m^2 = g(m)/(4 pi 4^m)
		std::vector<LDb> nrm(mmax+1);
		{
			LDb h = 2*s+1; for (int i = 1; i <= s; i++) h = h*(LDb)(s+i)/(LDb)i;
			for (int m = 0; m < std::min(s, mmax+1); m++) { if (m > 0) h = h*(LDb)(s-m+1)/(LDb)(s+m); nrm[m] = sqrtl(h/(4*PIl)); }
			if (s <= mmax) {
				LDb c2 = (LDb)(2*s+1)/(4*PIl*powl(4.0L, s));
				nrm[s] = sqrtl(c2);
				for (int m = s+1; m <= mmax; m++) { c2 = c2*(LDb)(2*m+1)*(LDb)(2*m)/(4*(LDb)(m+s)*(LDb)(m-s)); nrm[m] = sqrtl(c2); }
			}
		}
		run_threads([&](int m) {
			const int l0 = std::max(m, s);
			const int nl = lmax - l0 + 1;
			if (nl <= 0) return;
			auto Sf = [&](int l) -> LDb { LDb L = l, M = m, Sp = s; return sqrtl((L*L-M*M)*(L*L-Sp*Sp)); };
			LDb b_prev = 0, b_cur = ((m & 1) ? -1 : 1)*nrm[m];
			for (int l = l0; l <= lmax; l++) {
				const LDb L = l;
				const LDb q = sqrtl((2*L+3)/(2*L+1))*(2*L+1);
				const LDb A = q*(L+1)/Sf(l+1);
				const LDb B = q*(LDb)m*(LDb)s/(L*Sf(l+1));
				const LDb C = (l > l0) ? sqrtl((2*L+3)/(2*L-1))*(L+1)*Sf(l)/(L*Sf(l+1)) : 0;
				const LDb b_next = (l == l0) ? A*b_cur : C*b_prev;
				{ const LDb ca = A*b_cur/b_next, cb = B*b_cur/b_next; coef[row[m]+(l-l0)] = double4_t{(double)ca, (double)cb, (double)(ca+cb), (double)(ca-cb)}; }
				alpha[row[m]+(l-l0)] = (double)b_cur;
				b_prev = b_cur; b_cur = b_next;
			}
		});
	}
	d_row = upload(row);
	d_coef.alloc(sizeof(double4_t)*(size_t)(nrows + 4)); PXS_HIP(hipMemcpy(d_coef.p, coef, d_coef.bytes, hipMemcpyHostToDevice));
	d_alpha.alloc(sizeof(double)*(size_t)(nrows + 4)); PXS_HIP(hipMemcpy(d_alpha.p, alpha, d_alpha.bytes, hipMemcpyHostToDevice));
	build_compact();
}


// ---- recurrence tables on the GPU in double-double arithmetic (round 5) --------------------------------------------------------------
// The tables were built on host threads in long double (75 million rows of 4-6 square roots at lmax 10^4: 0.85 s of a 1.25 s cold
// call, followed by a 3 GB pageable upload).  The rows of one m are a serial recurrence, the m are independent: one GPU thread per m in
// double-double (106-bit) arithmetic builds the same rows in place in device memory in ~10 ms; the O(mmax) sectoral start values come from
// the host in long double as (hi, lo) pairs.  build_host (PXS_TABLES_HOST=1) remains as the reference the tests compare against.
// (error-free transforms: the compiler must not contract a product into a neighbouring add -- hipcc's default -ffp-contract=fast turned
// a - x*x into fma(-x, x, a) inside these and the device tables came out with 4-7e-15 errors instead of 2e-16, tools/tables_probe.hip)
#if defined(__clang__)
#define PXS_FP_STRICT _Pragma("clang fp contract(off)")
#else
#define PXS_FP_STRICT
#endif
struct dd { double h, l; };
__host__ __device__ __forceinline__ dd dd_norm(double a, double b) {
	PXS_FP_STRICT const double s = a + b; return dd{s, b - (s - a)}; }
__host__ __device__ __forceinline__ dd dd_of(double a) {
	PXS_FP_STRICT return dd{a, 0.0}; }
__host__ __device__ __forceinline__ dd dd_add(dd a, dd b) {
	PXS_FP_STRICT
	const double s = a.h + b.h, v = s - a.h, e = (a.h - (s - v)) + (b.h - v);
	return dd_norm(s, e + (a.l + b.l));
}
__host__ __device__ __forceinline__ dd dd_neg(dd a) {
	PXS_FP_STRICT return dd{-a.h, -a.l}; }
__host__ __device__ __forceinline__ dd dd_mul(dd a, dd b) {
	PXS_FP_STRICT
	const double p = a.h*b.h, e = fma(a.h, b.h, -p);
	return dd_norm(p, e + (a.h*b.l + a.l*b.h));
}
__host__ __device__ __forceinline__ dd dd_div(dd a, dd b) {
	PXS_FP_STRICT
	const double q1 = a.h/b.h;
	dd r = dd_add(a, dd_neg(dd_mul(dd_of(q1), b)));
	const double q2 = r.h/b.h;
	r = dd_add(r, dd_neg(dd_mul(dd_of(q2), b)));
	const double q3 = r.h/b.h;
	return dd_add(dd_norm(q1, q2), dd_of(q3));
}
__host__ __device__ __forceinline__ dd dd_sqrt(dd a) {
	PXS_FP_STRICT
	if (a.h <= 0.0) return dd{0.0, 0.0};
	const double x = sqrt(a.h);
	// one Newton step in double-double: x + (a - x^2) / (2 x)
	const double p = x*x, e = fma(x, x, -p);
	const dd r = dd_add(a, dd{-p, -e});
	return dd_norm(x, r.h/(2.0*x));
}
__host__ __device__ __forceinline__ double dd_val(dd a) {
	PXS_FP_STRICT return a.h + a.l; }

// spin 0: q(l) = eps_l^2 = (l^2 - m^2) / (4 l^2 - 1) (0 for l <= m); rows as in build_host
__global__ __launch_bounds__(64) void leg_tables_s0(int lmax, int mmax, const long* __restrict__ row, const dd* __restrict__ cms, double4_t* __restrict__ coef, double* __restrict__ alpha) {
	const int m = blockIdx.x*blockDim.x + threadIdx.x;
	if (m > mmax) return;
	auto q = [&](int l) -> dd { if (l <= m) return dd{0.0, 0.0}; const double L = l, M = m; return dd_div(dd_of(L*L - M*M), dd_of(4.0*L*L - 1.0)); };
	const int nk = (lmax - m)/2 + 1;
	dd a_prev = dd{0.0, 0.0}, a_cur = dd_mul(dd_sqrt(dd_of(2.0*m + 3.0)), cms[m]);
	// sliding window of q(lp - 1) ... q(lp + 2), lp = m + 2 k + 1
	dd qm1 = q(m), q0 = q(m + 1), qp1 = q(m + 2), qp2 = q(m + 3);
	const long r0 = row[m];
	for (int k = 0; k < nk; k++) {
		const dd e2 = dd_add(qp1, q0), f = dd_sqrt(dd_mul(q0, qm1)), d = dd_sqrt(dd_mul(qp1, qp2));
		const dd a_next = (k == 0) ? dd_div(a_cur, d) : dd_neg(dd_div(dd_mul(f, a_prev), d));
		const dd ak = dd_div(a_cur, dd_mul(a_next, d));
		const dd ake = dd_mul(ak, e2);
		coef[r0 + k] = double4_t{dd_val(ak), -dd_val(ake), dd_val(dd_add(ak, dd_neg(ake))), 0.0};
		alpha[r0 + k] = dd_val(a_cur);
		a_prev = a_cur; a_cur = a_next;
		const int lp = m + 2*k + 3;      // next step
		qm1 = qp1; q0 = qp2; qp1 = q(lp + 1); qp2 = q(lp + 2);
	}
}
// spin s: rows l = max(m, s) .. lmax as in build_host
__global__ __launch_bounds__(64) void leg_tables_spin(int lmax, int mmax, int s, const long* __restrict__ row, const dd* __restrict__ nrm, double4_t* __restrict__ coef, double* __restrict__ alpha) {
	const int m = blockIdx.x*blockDim.x + threadIdx.x;
	if (m > mmax) return;
	const int l0 = max(m, s), nl = lmax - l0 + 1;
	if (nl <= 0) return;
	auto Sf = [&](int l) -> dd { const double L = l, M = m, Sp = s; return dd_sqrt(dd_mul(dd_of(L*L - M*M), dd_of(L*L - Sp*Sp))); };
	dd b_prev = dd{0.0, 0.0}, b_cur = (m & 1) ? dd_neg(nrm[m]) : nrm[m];
	const long r0 = row[m];
	dd sf = Sf(l0);
	for (int l = l0; l <= lmax; l++) {
		const double L = l;
		const dd sf1 = Sf(l + 1);
		const dd qq = dd_mul(dd_sqrt(dd_div(dd_of(2*L + 3), dd_of(2*L + 1))), dd_of(2*L + 1));
		const dd A = dd_div(dd_mul(qq, dd_of(L + 1)), sf1);
		const dd B = dd_div(dd_mul(qq, dd_of((double)m*(double)s)), dd_mul(dd_of(L), sf1));
		dd b_next;
		if (l == l0) b_next = dd_mul(A, b_cur);
		else {
			const dd C = dd_div(dd_mul(dd_mul(dd_sqrt(dd_div(dd_of(2*L + 3), dd_of(2*L - 1))), dd_of(L + 1)), sf), dd_mul(dd_of(L), sf1));
			b_next = dd_mul(C, b_prev);
		}
		const dd ca = dd_div(dd_mul(A, b_cur), b_next), cb = dd_div(dd_mul(B, b_cur), b_next);
		coef[r0 + (l - l0)] = double4_t{dd_val(ca), dd_val(cb), dd_val(dd_add(ca, cb)), dd_val(dd_add(ca, dd_neg(cb)))};
		alpha[r0 + (l - l0)] = dd_val(b_cur);
		b_prev = b_cur; b_cur = b_next; sf = sf1;
	}
}

void LegTables::build(int lmax_, int mmax_, int spin_) {
	{ const char* e = getenv("PXS_TABLES_HOST"); if (e && atoi(e) != 0) { build_host(lmax_, mmax_, spin_); return; } }
	lmax = lmax_; mmax = mmax_; spin = spin_;
	row.assign(mmax+2, 0);
	for (int m = 0; m <= mmax; m++) {
		long n = spin == 0 ? (lmax - m)/2 + 1 : std::max(0, lmax - std::max(m, spin) + 1);
		row[m+1] = row[m] + n;
	}
	nrows = row[mmax+1];
	typedef long double LDb;
	const LDb PIl = 3.141592653589793238462643383279502884L;
	// sectoral start values (a serial product over m): host, long double, handed over as (hi, lo)
	std::vector<dd> start(mmax+1);
	auto put = [&](int m, LDb v) { const double h = (double)v; start[m] = dd{h, (double)(v - (LDb)h)}; };
	if (spin == 0) {
		LDb cm = 1/sqrtl(4*PIl);
		for (int m = 0; m <= mmax; m++) { if (m > 0) cm = -cm*sqrtl((LDb)(2*m+1)/(LDb)(2*m)); put(m, cm); }
	} else {
		const int s = spin;
		LDb h = 2*s+1; for (int i = 1; i <= s; i++) h = h*(LDb)(s+i)/(LDb)i;
		for (int m = 0; m < std::min(s, mmax+1); m++) { if (m > 0) h = h*(LDb)(s-m+1)/(LDb)(s+m); put(m, sqrtl(h/(4*PIl))); }
		if (s <= mmax) {
			LDb c2 = (LDb)(2*s+1)/(4*PIl*powl(4.0L, s));
			put(s, sqrtl(c2));
			for (int m = s+1; m <= mmax; m++) { c2 = c2*(LDb)(2*m+1)*(LDb)(2*m)/(4*(LDb)(m+s)*(LDb)(m-s)); put(m, sqrtl(c2)); }
		}
	}
	d_row = upload(row);
	DevBuf d_start = upload(start);
	// (4 rows of padding: the phase-C loops of the VALU kernels request rows up to 2 past the end of an m (leg_syn_s0, leg_syn_spin) or 3 (the analysis kernels, whose
	// row sets start a step late), the pre-scaled alm (leg_almt_stride) up to 2)
	d_coef.alloc(sizeof(double4_t)*(size_t)(nrows + 4)); d_alpha.alloc(sizeof(double)*(size_t)(nrows + 4));
	// (+4 rows: the fast loops prefetch up to 3 rows ahead)
	PXS_HIP(hipMemset((char*)d_coef.p + sizeof(double4_t)*(size_t)nrows, 0, sizeof(double4_t)*4)); PXS_HIP(hipMemset((char*)d_alpha.p + sizeof(double)*(size_t)nrows, 0, sizeof(double)*4));
	const dim3 grid((unsigned)((mmax + 1 + 63)/64));
	if (spin == 0) hipLaunchKernelGGL(leg_tables_s0, grid, dim3(64), 0, (hipStream_t)0, lmax, mmax, d_row.as<long>(), d_start.as<dd>(), d_coef.as<double4_t>(), d_alpha.as<double>());
	else           hipLaunchKernelGGL(leg_tables_spin, grid, dim3(64), 0, (hipStream_t)0, lmax, mmax, spin, d_row.as<long>(), d_start.as<dd>(), d_coef.as<double4_t>(), d_alpha.as<double>());
	PXS_HIP(hipGetLastError());
	build_compact();      // (synchronises the device: d_start goes out of scope; the tables are plan state, built once)
}

// The compact step tables, built with the tables themselves: 16 bytes per row and table, i.e. half of d_coef again for the spin-s tables (0.8 GB next to 1.6 GB at lmax 10^4)
// and as much as d_coef again for the two spin-0 ones (0.4 GB each next to 0.8 GB).  They used to be filled by the first batched transform on that call's stream, which
// a first transform on another stream could overtake; now no transform ever sees them incomplete.
void LegTables::build_compact() {
	d_coef2.alloc(sizeof(double2)*(size_t)(nrows + 32));
	if (spin == 0) d_coef2p.alloc(sizeof(double2)*(size_t)(nrows + 32));
	hipLaunchKernelGGL(coef2_kernel, dim3((unsigned)((nrows + 32 + 255)/256)), dim3(256), 0, (hipStream_t)0, d_coef.as<double4_t>(), nrows, d_coef2.as<double2>(), d_coef2p.as<double2>());
	PXS_HIP(hipGetLastError());
	PXS_HIP(hipDeviceSynchronize());
}

// doubles per map of the pre-scaled alm / the moments of a batched call
static long leg_almt_stride(const LegTables& tb) { return 4*(tb.nrows + 4); }
static long leg_mom_stride(const LegTables& tb) { return 4*std::max<long>(tb.nrows, 1); }
// kernel arguments of one launch: nb maps (MFMA forms: groups of maps, make_legk_mm), `pairs` ring pairs per workgroup
static LegK make_legk(const RingSet& rs, const LegTables& tb, LegWork& wk, double2* leg, long ld, int pairs, int nb, long leg_bs) {
	LegK a; memset(&a, 0, sizeof(a));
	a.lmax = tb.lmax; a.mmax = tb.mmax; a.spin = tb.spin; a.nm = tb.mmax+1; a.npairs = rs.npairs; a.nring = rs.nring;
	a.nwave = (rs.npairs + pairs - 1)/pairs;
	a.nrows = tb.nrows; a.row = tb.d_row.as<long>(); a.coef = tb.d_coef.as<double4_t>(); a.alpha = tb.d_alpha.as<double>();
	a.ring_n = rs.d_ring_n.as<int>(); a.ring_s = rs.d_ring_s.as<int>(); a.cth = rs.d_cth.as<double>(); a.sth = rs.d_sth.as<double>();
	a.sh2 = rs.d_sh2.as<double>(); a.ch2 = rs.d_ch2.as<double>();
	a.almt = wk.almt.as<double>(); a.part = wk.part.as<double>(); a.mom = wk.mom.as<double>();
	a.leg = leg; a.ld = ld > 0 ? ld : rs.nring;
	a.ofs = std::max(100.0, 0.01*tb.lmax);
	a.nmc = a.nm; a.xcd = 1;      // (the XCD-aware block order, always: see leg_block)
	a.count = wk.count_on ? wk.count.as<double>() : nullptr;
	a.coef2 = tb.d_coef2.as<double2>(); a.coef2p = tb.d_coef2p.as<double2>();
	a.nb = nb; a.leg_bs = leg_bs; a.almt_bs = leg_almt_stride(tb); a.mom_bs = leg_mom_stride(tb);
	PXS_REQUIRE((long)8*((a.nm + 7)/8)*leg_blocks_per_m(a.nwave, nb) < (1L << 31), "internal: Legendre grid too large for one launch");
	return a;
}
// ... of an MFMA launch: nmaps maps from `leg` on in groups of 4 ng, one group per wave (synthesis) or workgroup (analysis)
static LegK make_legk_mm(const RingSet& rs, const LegTables& tb, LegWork& wk, double2* leg, long ld, int pairs, int nmaps, int ng, long leg_bs) {
	LegK a = make_legk(rs, tb, wk, leg, ld, pairs, (nmaps + 4*ng - 1)/(4*ng), leg_bs);
	a.nmaps = nmaps;
	return a;
}

// maps (MFMA forms: groups) one launch can take: all of them share one grid of 8 ceil(nm / 8) leg_blocks_per_m(nwave, nb) blocks (a large batch of
// small-ring, high-lmax maps goes out as several launches instead of tripping make_legk's grid check)
// (the spin MFMA runs used to be cut at half the spin-0 synthesis limit and at the limit of 128 pairs per workgroup: lower than the grid needs; now every form is cut by its own
// pairs per workgroup.  Out of reach at real sizes: tens of thousands of maps in one call)
// (cap: pxs_plan_option "leg_max_batch", 0 = none: a lower bound for the tests of the launch seam, which the grid limit never reaches)
static int leg_max_batch(const RingSet& rs, const LegTables& tb, int pairs, int cap) {
	const long nwave = (rs.npairs + (long)pairs - 1)/pairs, per_m = ((1L << 31) - 1)/(8L*((tb.mmax + 1 + 7)/8));      // blocks per m one grid can hold: nwave nb, or one more (leg_blocks_per_m)
	const long grid = std::max<long>(1, std::min<long>(1 << 20, (per_m - 1)/std::max<long>(nwave, 1)));
	return (int)(cap > 0 ? std::min<long>(grid, cap) : grid);
}
// seeds of (ring set, spin, direction, K): allocate on first use if the plan's budget allows; returns the mode for this launch.
// The step a seed records depends on the rule that ends phase A (LEG_LIVE).  That rule is a compile-time constant of the library, and
// seeds live in device memory of the process that recorded them, so a seed is never loaded under another rule than it was recorded
// under; the two directions of a plan record their own seeds (dir is part of the key) under the same constant.
static LegWork::Seeds* seeds_for(LegWork& wk, const RingSet& rs, const LegTables& tb, int dir, int K, LegK& a) {
	a.seed_mode = 0; a.seed_d = nullptr; a.seed_i = nullptr;
	env_budget("PXS_SEED_GB", 30, wk.seed_budget);
	if (wk.seed_budget == 0) return nullptr;
	// loading a seed costs 20 / 40 bytes per lane and m, running phase A ~0.09 lmax recurrence steps: measured on MI355X the seeds
	// win at lmax 10^4 (C3 341.8 -> 327.6 ms per round trip) and for spin 2 at lmax 4000 (C2 28.7 -> 28.0 ms), and lose for spin 0
	// at lmax 4000 (C4: leg_syn 109.1 -> 113.9 ms per 64 maps)
	{	const char* e = getenv("PXS_SEED_MIN_LMAX");
		const int lmin = e ? atoi(e) : (tb.spin == 0 ? 6000 : 3000);
		if (tb.lmax < lmin) return nullptr; }
	LegWork::Seeds& sb = wk.seeds[std::make_tuple((const void*)&rs, tb.spin, dir, K)];
	if (sb.refused) return nullptr;
	const int nd = tb.spin == 0 ? 2 : 4, ni = tb.spin == 0 ? 1 : 2;
	const size_t slots = (size_t)a.nm*a.nwave;
	if (!sb.d.p) {
		const size_t bd = sizeof(double)*slots*nd*K*64, bi = sizeof(int)*slots*(ni*K + 1)*64;
		if (wk.seed_bytes + bd + bi > wk.seed_budget) { sb.refused = true; return nullptr; }
		sb.d.alloc(bd); sb.i.alloc(bi); wk.seed_bytes += bd + bi;
	}
	a.seed_d = sb.d.as<double>(); a.seed_i = sb.i.as<int>(); a.seed_mode = sb.ready ? 2 : 1;
	return &sb;
}
// after the recording launch: later launches on OTHER streams wait for it (a plan serves one call at a time, but the next call may
// come on another stream).  The entry points of a plan now order whole calls across streams (PlanUse, sht_plan.hpp), which covers this
// too; the event stays for callers of leg_synthesis / leg_analysis that do not come through a plan's entry point.
static void seeds_written(LegWork::Seeds* sb, hipStream_t st) {
	if (!sb || sb->ready) return;
	if (!sb->written) PXS_HIP(hipEventCreateWithFlags(&sb->written, hipEventDisableTiming));
	PXS_HIP(hipEventRecord(sb->written, st)); sb->wstream = st; sb->ready = true;
}
static void seeds_wait(LegWork::Seeds* sb, hipStream_t st) {
	if (sb && sb->ready && sb->written && st != sb->wstream) PXS_HIP(hipStreamWaitEvent(st, sb->written, 0));
}

// will the next launch of this kind record seeds (first use on a plan, budget permitting)?
static bool seeds_pending(LegWork& wk, const RingSet& rs, const LegTables& tb, int dir, int K) {
	LegK probe; memset(&probe, 0, sizeof(probe)); probe.nm = tb.mmax + 1; probe.nwave = (rs.npairs + 64*K - 1)/(64*K);
	LegWork::Seeds* sb = seeds_for(wk, rs, tb, dir, K, probe);
	return sb != nullptr && !sb->ready;
}

static AlmK make_almk(const LegTables& tb, LegWork& wk, const void* alm, int dtype, long cstride, const uint64_t* d_mstart, long lstride, int deriv1, long alm_bs) {
	AlmK k; memset(&k, 0, sizeof(k));
	k.alm_bs = alm_bs; k.almt_bs = leg_almt_stride(tb); k.mom_bs = leg_mom_stride(tb);
	k.lmax = tb.lmax; k.mmax = tb.mmax; k.spin = tb.spin; k.deriv1 = deriv1; k.dtype = dtype;
	k.nrows = tb.nrows; k.cstride = cstride; k.lstride = lstride; k.row = tb.d_row.as<long>(); k.alpha = tb.d_alpha.as<double>();
	k.mstart = d_mstart; k.alm = const_cast<void*>(alm); k.almt = wk.almt.as<double>(); k.mom = wk.mom.as<double>();
	return k;
}

// Rings per lane of a small ring set.  (1) A wave of 64 K ring pairs takes the polar form of the recurrences (leg_wave_polar) only if its most equatorial ring
// stays within 71.5 degrees of the pole, so on a grid of a few hundred rings the default K leaves the rings next to the poles in the plain form (l^2 eps there):
// where a smaller compiled K makes the first wave eligible, take it.  (2) Up to 512 ring pairs (lmax ~1000) the launch is short of waves, not of work per wave
// -- (mmax + 1) x ceil(npairs / 64 K) waves for 1024 SIMDs -- and the smallest K is the fastest (profiles/r05_k_small_grids.txt: the reference's
// benchmark shape 900x1800, lmax 750: 0.365 -> 0.335 ms per round trip, its T/Q/U version 1.047 -> 0.938; at lmax 1500 the defaults are level, at 2500 ahead).
static int k_small_grid(const RingSet& rs, int kdef, std::initializer_list<int> smaller, int kmid = 0) {
#ifdef PXS_HOST_SIM
	const bool off = [] { const char* e = getenv("PXS_K_SMALL_OFF"); return e && atoi(e) != 0; }();      // (the host simulation runs small grids only: its tests switch the rule off to reach the default kernels)
#else
	constexpr bool off = false;
#endif
	if (off || rs.npairs <= 0) return kdef;
	if (rs.npairs <= 512) { int k = kdef; for (int c : smaller) k = std::min(k, c); return k; }
	// (3) up to 1400 ring pairs (lmax ~2500: 2700 rings) the synthesis kernels are still 5-12 % faster with K = 2 and the scalar analysis 2-4 % with K = 4; at lmax 4000 the defaults
	// are 20 % ahead (profiles/r05_k_mid_grids.txt)
	if (kmid > 0 && rs.npairs <= 1400) return kmid;
	// (the first wave's most equatorial pair under the kernels' pair map, leg_pair_of: the first wave is the one that holds the padding)
	auto eligible = [&](int k) { const int last = leg_wave_last_pair(rs.npairs, k, 0); return last >= 0 && rs.cth[last]*rs.cth[last] > PXS_POLAR_COS2; };
	if (eligible(kdef)) return kdef;
	for (int k : smaller) if (k < kdef && eligible(k)) return k;
	return kdef;
}
// Ring pairs per lane of the VALU analysis.  Spin s: where k_small_grid leaves the default and the ring set gives LEG_BIG_MIN_WAVES waves per m with it (1793 ring
// pairs), K_ANAS_BIG: the lane reduce-scatter of a step (10 VALU instructions whatever K is) is then shared by half as many FMAs again, at two waves per SIMD
// instead of three; on smaller ring sets the padded polar wave and the fewer, longer waves cost more than that saves.  C3: leg_ana_spin<4> 91.41 -> leg_ana_spin<6>
// 87.48 ms per launch (spreads 0.5 / 1.0), C2 leg_ana 8.72 -> 8.65.  Spin 0 keeps K_ANA0: leg_ana_s0<12> (217 VGPRs, two waves per SIMD)
// was measured without per-block starts and gained 0.4 ms of 24, inside its spread, and again with them (four more stages; the same 217 VGPRs, no scratch), behind a
// rule that took it where K_ANA0 leaves LEG_BIG_MIN_WAVES waves per m (C3): leg_ana_s0<8> 23.77 -> leg_ana_s0<12> 23.15 ms per launch at spreads of 0.13 / 0.33, C3 leg_ana
// 110.89 -> 110.35 at spreads of 0.76 / 0.54 -- under three times the spread both ways; instance and rule are out again (profiles/README.md, "Block starts").
static constexpr int K_ANAS_BIG = 6, LEG_BIG_MIN_WAVES = 8;
static int leg_ana_k(const RingSet& rs, int spin) {
	if (spin == 0) return k_small_grid(rs, K_ANA0, {4, 2}, 4);
	const int k = k_small_grid(rs, K_ANAS, {3, 2});
	return (k == K_ANAS && (rs.npairs + 64*K_ANAS - 1)/(64*K_ANAS) >= LEG_BIG_MIN_WAVES) ? K_ANAS_BIG : k;
}
// ---- batch planner ----
// A call of nb maps goes out as an ordered list of launches.  With 4 or more maps (PXS_SYN_MM_MIN / PXS_ANA_MM_MIN) the maps share one recurrence in the FP64-MFMA
// kernels (leg_*_mm): groups of 8 maps per wave (synthesis) or workgroup (analysis); a remainder of more than 4 maps as one more 8-map group, of 4 or fewer as a
// 4-map group, a lone left-over map through the VALU kernel (it costs more in a 4-map group).  An MFMA result equals the single-map call to rounding (1e-13), not
// bit for bit: the sums run in another order.  Never MFMA: the ordered (bitwise repeatable) analysis, which takes every map alone, and the spin analysis of a gradient.
// The VALU launch that records the recurrence seeds takes one map, so that only one wave writes each seed.
enum LegForm { LEG_VALU, LEG_MM8, LEG_MM4 };
struct LegLaunch { int b0, n; LegForm form; int ng; };      // maps [b0, b0 + n); ng: groups of 4 maps per wave / workgroup (MFMA forms)
static int mm_min(const char* name) { const char* e = getenv(name); const int x = e ? atoi(e) : 4; return x <= 0 ? (1 << 30) : std::max(2, x); }
static int syn_mm_min() { return mm_min("PXS_SYN_MM_MIN"); }      // (read per call, like the budgets)
static int ana_mm_min() { return mm_min("PXS_ANA_MM_MIN"); }
// seeds_pending: will a VALU launch record seeds; max_valu / max_mm8: maps one launch can take (grid limit).  seeds_pending is a callable, not a bool, because asking
// ALLOCATES the seed buffers of the VALU kernel (seeds_for): it is asked only where the parent asked, with more than one map left to the VALU kernel
static std::vector<LegLaunch> leg_batch_plan(int nb, int spin, bool analysis, int deriv1, bool deterministic, const std::function<bool()>& seeds_pending, int max_valu, int max_mm8) {
	const bool ordered = analysis && deterministic;
	const bool mm = nb >= (analysis ? ana_mm_min() : syn_mm_min()) && !ordered && !(analysis && spin > 0 && deriv1);
	std::vector<LegLaunch> plan;
	int b = 0;
	if (mm) {
		const int nmm = nb - (nb % 8 == 1 ? 1 : 0), r = nmm % 8, n8 = nmm - r;
		for (; b < n8; b += max_mm8) plan.push_back({b, std::min(max_mm8, n8 - b), LEG_MM8, 2});
		if (r > 4) plan.push_back({n8, r, LEG_MM8, 2}); else if (r > 0) plan.push_back({n8, r, LEG_MM4, 1});
		b = nmm;
	}
	if (ordered || (nb - b > 1 && seeds_pending())) for (const int e = ordered ? nb : b + 1; b < e; b++) plan.push_back({b, 1, LEG_VALU, 0});
	for (; b < nb; b += max_valu) plan.push_back({b, std::min(max_valu, nb - b), LEG_VALU, 0});
	return plan;
}
// PXS_CHAIN_VERBOSE: the launch list of the call, e.g. "[pxsht] legendre analysis spin 0, 13 maps: mm8 [0,8) mm8 [8,13)"
static void print_batch_plan(bool analysis, int spin, int nb, const std::vector<LegLaunch>& plan) {
	if (!getenv("PXS_CHAIN_VERBOSE")) return;
	std::string s;
	for (const LegLaunch& l : plan) s += std::string(l.form == LEG_VALU ? " VALU [" : l.form == LEG_MM8 ? " mm8 [" : " mm4 [") + std::to_string(l.b0) + "," + std::to_string(l.b0 + l.n) + ")";
	fprintf(stderr, "[pxsht] legendre %s spin %d, %d maps:%s\n", analysis ? "analysis" : "synthesis", spin, nb, s.c_str());
}

void leg_synthesis(hipStream_t st, const RingSet& rs, const LegTables& tb, LegWork& wk,
                   const void* alm, int alm_dtype, long alm_cstride, const uint64_t* d_mstart, long lstride,
                   double2* leg, int deriv1, LegProfile* prof, long ld, int nb, long alm_bstride, long leg_bstride)
{
	PXS_REQUIRE(alm_dtype == PX_C64 || alm_dtype == PX_C128, "alm must be complex64 or complex128");
	PXS_REQUIRE(nb >= 1, "leg_synthesis: nb must be >= 1");
	wk.almt.ensure(sizeof(double)*(size_t)leg_almt_stride(tb)*nb);
	AlmK ak = make_almk(tb, wk, alm, alm_dtype, alm_cstride, d_mstart, lstride, deriv1, alm_bstride);
	const int nm = tb.mmax+1;
	const int K = tb.spin == 0 ? k_small_grid(rs, K_SYN0, {2}, 2) : k_small_grid(rs, K_SYNS, {2}, 2);
	const int mm_pairs = tb.spin == 0 ? 64 : 32;      // ring pairs per wave of the MFMA form (spin s: one chain per half-wave)
	if (tb.spin == 0) hipLaunchKernelGGL(alm_pre_s0, alm_grid(tb.lmax/2 + 1, nm, nb), dim3(256), 0, st, ak);
	else              hipLaunchKernelGGL(alm_pre_spin, alm_grid(tb.lmax + 1, nm, nb), dim3(256), 0, st, ak);
	const std::vector<LegLaunch> plan = leg_batch_plan(nb, tb.spin, false, deriv1, wk.deterministic, [&] { return seeds_pending(wk, rs, tb, 0, K); },
		leg_max_batch(rs, tb, 64*K, wk.max_batch), 8*leg_max_batch(rs, tb, mm_pairs, wk.max_batch));
	print_batch_plan(false, tb.spin, nb, plan);
	wk.pass_valu.begin(); wk.pass_mm.begin();
	for (const LegLaunch& l : plan) {
		(l.ng ? wk.pass_mm : wk.pass_valu).add(l.n);
		double2* legl = leg + (size_t)l.b0*leg_bstride;
		LegK a = l.ng ? make_legk_mm(rs, tb, wk, legl, ld, mm_pairs, l.n, l.ng, leg_bstride) : make_legk(rs, tb, wk, legl, ld, 64*K, l.n, leg_bstride);
		a.almt += (size_t)l.b0*a.almt_bs;
		LegWork::Seeds* sb = nullptr;
		if (!l.ng) { sb = seeds_for(wk, rs, tb, 0, K, a); seeds_wait(sb, st); }
		if (prof) prof->begin(st, 0);
		(tb.spin == 0 ? launch_leg_s0 : launch_leg_spin)(false, l.ng, K, leg_grid(a), st, a);
		if (prof) prof->end(st, 0);
		seeds_written(sb, st);
	}
	PXS_HIP(hipGetLastError());
}

// one VALU analysis launch: maps [0, nb) of leg into mom (pre-zeroed unless wk.deterministic).
// Default: the waves of one m add their sums straight into mom with global_atomic_add_f64 -- the blocks of one m run back
// to back on one XCD (leg_block), so the row they share sits in that XCD's L2 while they do.  The order of those additions
// is not fixed: results repeat to rounding, not bit for bit.  pxs_plan_option("deterministic", 1) (or PXS_DETERMINISTIC=1 when the plan is made) selects the former scheme instead
// (per-wave partial moments in scratch, m in chunks that keep them below part_budget, summed in wave order by reduce_partials), for callers that need bitwise repeats.
static void leg_analysis_valu(hipStream_t st, const RingSet& rs, const LegTables& tb, LegWork& wk, int K, const double2* leg, double* mom, LegProfile* prof, long ld, int nb, long leg_bstride)
{
	const int nm = tb.mmax+1, nwave = (rs.npairs + 64*K - 1)/(64*K);
	const bool atomic = !wk.deterministic;
	std::vector<int> cuts; cuts.push_back(0);
	if (atomic) cuts.push_back(nm);
	else {
		const size_t budget = wk.part_budget;
		for (int m = 0; m < nm;) {
			int m1 = m+1;
			while (m1 < nm && (size_t)(tb.row[m1+1]-tb.row[m])*32*nwave <= budget) m1++;
			cuts.push_back(m1); m = m1;
		}
		size_t maxrows = 1;
		for (size_t c = 0; c+1 < cuts.size(); c++) maxrows = std::max<size_t>(maxrows, (size_t)(tb.row[cuts[c+1]]-tb.row[cuts[c]]));
		wk.part.ensure(sizeof(double)*4*maxrows*nwave);
		// sized once, before the first launch: growing a buffer inside the chunk loop would free memory that kernels of the
		// previous chunk may still use (and hipFree synchronises the device)
		size_t maxm = 1;
		for (size_t c = 0; c+1 < cuts.size(); c++) maxm = std::max<size_t>(maxm, (size_t)(cuts[c+1]-cuts[c]));
		wk.first.ensure(sizeof(int)*(size_t)nwave*maxm);
	}
	LegWork::Seeds* seeds = nullptr;
	wk.pass_m.begin();
	for (size_t c = 0; c+1 < cuts.size(); c++) {
		const int m0 = cuts[c], m1 = cuts[c+1];
		const long rows = tb.row[m1]-tb.row[m0];
		if (rows <= 0) continue;
		wk.pass_m.add(m1 - m0);
		LegK a = make_legk(rs, tb, wk, const_cast<double2*>(leg), ld, 64*K, nb, leg_bstride);
		a.mom = mom; a.m0 = m0; a.rowbase = tb.row[m0]; a.rows_chunk = rows; a.nmc = m1-m0; a.atomic = atomic ? 1 : 0;
		seeds = seeds_for(wk, rs, tb, 1, K, a); seeds_wait(seeds, st);
		if (atomic) { a.part = mom; a.rowbase = 0; a.rows_chunk = 0; a.first = nullptr; }
		else {
			PXS_HIP(hipMemsetAsync(wk.first.p, 0, sizeof(int)*(size_t)nwave*(m1-m0), st));
			a.first = wk.first.as<int>();
		}
		if (prof) prof->begin(st, 1);
		const dim3 grid = leg_grid(a);
		(tb.spin == 0 ? launch_leg_s0 : launch_leg_spin)(true, 0, K, grid, st, a);
		if (prof) prof->end(st, 1);
		if (atomic) continue;
		const long maxrow = tb.row[m0+1] - tb.row[m0];       // rows per m shrink with m
		hipLaunchKernelGGL(reduce_partials, dim3((unsigned)((4*maxrow+255)/256), m1-m0), dim3(256), 0, st, (const double*)wk.part.p,
			mom, tb.d_row.as<long>(), (const int*)wk.first.p, m0, m1-m0, tb.row[m0], rows, a.nwave);
	}
	seeds_written(seeds, st);
}

void leg_analysis(hipStream_t st, const RingSet& rs, const LegTables& tb, LegWork& wk,
                  const double2* leg, void* alm, int alm_dtype, long alm_cstride, const uint64_t* d_mstart, long lstride,
                  int deriv1, LegProfile* prof, long ld, int nb, long alm_bstride, long leg_bstride)
{
	PXS_REQUIRE(alm_dtype == PX_C64 || alm_dtype == PX_C128, "alm must be complex64 or complex128");
	PXS_REQUIRE(nb >= 1, "leg_analysis: nb must be >= 1");
	const int K = wk.ana_k > 0 ? wk.ana_k : leg_ana_k(rs, tb.spin);
	wk.last_ana_k = K;
	const int nm = tb.mmax+1;
	const int mm_pairs = (tb.spin == 0 ? 64 : 32)*MM_WAVES;      // ring pairs per workgroup of the MFMA form
	const std::vector<LegLaunch> plan = leg_batch_plan(nb, tb.spin, true, deriv1, wk.deterministic, [&] { return seeds_pending(wk, rs, tb, 1, K); },
		leg_max_batch(rs, tb, 64*K, wk.max_batch), 8*leg_max_batch(rs, tb, mm_pairs, wk.max_batch));
	print_batch_plan(true, tb.spin, nb, plan);
	const size_t nmom = (size_t)leg_mom_stride(tb);
	wk.mom.ensure(sizeof(double)*nmom*nb);
	if (!wk.deterministic) PXS_HIP(hipMemsetAsync(wk.mom.p, 0, sizeof(double)*nmom*nb, st));      // (the ordered scheme writes every row it reads)
	wk.pass_valu.begin(); wk.pass_mm.begin();
	for (const LegLaunch& l : plan) {
		(l.ng ? wk.pass_mm : wk.pass_valu).add(l.n);
		const double2* legl = leg + (size_t)l.b0*leg_bstride;
		double* mom = wk.mom.as<double>() + nmom*l.b0;
		if (!l.ng) { leg_analysis_valu(st, rs, tb, wk, K, legl, mom, prof, ld, l.n, leg_bstride); continue; }
		LegK a = make_legk_mm(rs, tb, wk, const_cast<double2*>(legl), ld, mm_pairs, l.n, l.ng, leg_bstride);
		a.mom = mom; a.part = mom; a.atomic = 1;
		if (prof) prof->begin(st, 1);
		(tb.spin == 0 ? launch_leg_s0 : launch_leg_spin)(true, l.ng, K, leg_grid(a), st, a);
		if (prof) prof->end(st, 1);
	}
	AlmK ak = make_almk(tb, wk, alm, alm_dtype, alm_cstride, d_mstart, lstride, deriv1, alm_bstride);
	if (tb.spin == 0) hipLaunchKernelGGL(alm_post_s0, alm_grid(tb.lmax/2 + 1, nm, nb), dim3(256), 0, st, ak);
	else              hipLaunchKernelGGL(alm_post_spin, alm_grid(tb.lmax + 1, nm, nb), dim3(256), 0, st, ak);
	PXS_HIP(hipGetLastError());
}

} // namespace pxs
