// Spin-0 Legendre kernels for gfx950 (design notes: head of legendre.hip): leg_syn_s0 / leg_ana_s0 (one wave per workgroup, K ring pairs per lane, plain
// v_fma_f64) and the FP64-MFMA forms of batched calls, leg_syn_s0_mm / leg_ana_s0_mm.  Replaces ducc0's alm2leg / leg2alm for spin 0 as reached from
// pixell/curvedsky.py:907-960, 1032-1084.
#include "legendre_dev.hpp"

namespace pxs {

// ---- the VALU kernels ----
// Phase A of the spin-0 kernels: no lane of the wave is live yet (scale 0 and |value| >= LEG_LIVE), so nothing is
// accumulated.  Four recurrence steps per iteration with the four coefficient rows fetched together;
// the rescale / activity test runs once per 4 steps (a chain grows by < 2^60 in 4 steps, far from
// overflow at 2^1024; what the late start drops: see LEG_LIVE).
#define S0_PHASE_A \
	while (k + 4 <= nk) { \
		bool act = false; \
		_Pragma("unroll") for (int s = 0; s < K; s++) act |= LEG_IS_LIVE(lam2[s], sc[s]); \
		if (__any(act)) break; \
		const double4_t q0 = LDC(coef, k), q1 = LDC(coef, k+1), q2 = LDC(coef, k+2), q3 = LDC(coef, k+3); \
		const double b0 = polar ? q0.c : q0.b, b1 = polar ? q1.c : q1.b, b2 = polar ? q2.c : q2.b, b3 = polar ? q3.c : q3.b; \
		_Pragma("unroll") for (int s = 0; s < K; s++) { \
			lam1[s] = fma(fma(q0.a, csq[s], b0), lam2[s], lam1[s]); \
			lam2[s] = fma(fma(q1.a, csq[s], b1), lam1[s], lam2[s]); \
			lam1[s] = fma(fma(q2.a, csq[s], b2), lam2[s], lam1[s]); \
			lam2[s] = fma(fma(q3.a, csq[s], b3), lam1[s], lam2[s]); \
			if (sc[s] < 0 && fabs(lam2[s]) > SC_BIG) { lam1[s] *= SC_SMALL; lam2[s] *= SC_SMALL; sc[s]++; } \
		} \
		k += 4; \
	}
// phase A with the recurrence seeds (legendre_dev.hpp, "Recurrence seeds"): mode 2 loads the state, the step reached and the start steps of the blocks (the seed
// tail, knext; legendre_dev.hpp, "Block starts"), mode 1 records them (the start steps as the blocks start: S0_BLOCK_BEGIN; LEG_NEVER until then)
#define S0_SEEDED_PHASE_A \
	if (a.seed_mode == 2) { \
		const double* sd = a.seed_d + ((long)m*a.nwave + wv)*(2*K*64); const int* si = a.seed_i + ((long)m*a.nwave + wv)*((K+1)*64); \
		k = PXS_UNIFORM_INT(si[K*64]); \
		_Pragma("unroll") for (int s = 0; s < K; s++) { lam1[s] = sd[s*64 + lane]; lam2[s] = sd[(K+s)*64 + lane]; sc[s] = si[s*64 + lane]; } \
	} else { \
		S0_PHASE_A \
		if (a.seed_mode == 1) { \
			double* sd = a.seed_d + ((long)m*a.nwave + wv)*(2*K*64); int* si = a.seed_i + ((long)m*a.nwave + wv)*((K+1)*64); \
			_Pragma("unroll") for (int s = 0; s < K; s++) { sd[s*64 + lane] = lam1[s]; sd[(K+s)*64 + lane] = lam2[s]; si[s*64 + lane] = sc[s]; } \
			if (lane == 0) si[K*64] = k; else if (lane <= K) si[K*64 + lane] = LEG_NEVER; \
		} \
	}
// does block c start at this 4-step test (one of its chains, or one of a more polar block, is live)?  Seeded launches read it off the seed tail.  Tests are
// at multiples of 4 steps (phase A ends at one): a phase B that ends on a lone pair leaves the last steps of the wave without a test
#define S0_BLOCK_STARTS(c) ((k & 3) == 0 && (a.seed_mode == 2 ? k >= knext : __any(leg_live_upto<c>(lam2, sc))))
// the seed tail of this (wave, m): [0] the step phase A reached, [1 + c] the start step of block c
#define S0_SEED_TAIL (a.seed_i + ((long)m*a.nwave + wv)*((K+1)*64) + K*64)
// block c starts at step k: counted from here on; recorded in the seed tail by the lane that wrote LEG_NEVER there.  NEXT_START(c): a seeded launch reads the start of block c
#define S0_BLOCK_BEGIN(c) { PXS_COUNT_BLOCK(DIR, (long)(nk - k)*4); if (a.seed_mode == 1 && lane == (c) + 1) S0_SEED_TAIL[(c) + 1] = k; }
#define S0_NEXT_START(c) if (a.seed_mode == 2) knext = PXS_UNIFORM_INT(S0_SEED_TAIL[(c) + 1]);

// two fast steps of the spin-0 synthesis (lam1/lam2 swap roles)
#define S0_SYN_PAIR(c0, c1, a0, a1) S0_SYN_PAIR_C(c0.a, polar ? c0.c : c0.b, c1.a, polar ? c1.c : c1.b, a0, a1)
// ... on the step coefficients themselves: (ca, cb) of a step = a and the additive constant
#define S0_SYN_PAIR_C(ca0, cb0, ca1, cb1, a0, a1) { \
	PXS_VCOPY(vb0, cb0); \
	PXS_VCOPY(vb1, cb1); \
	_Pragma("unroll") for (int s = 0; s < K; s++) { \
		p1r[s] = fma(lam2[s], a0.a, p1r[s]); p1i[s] = fma(lam2[s], a0.b, p1i[s]); \
		p2r[s] = fma(lam2[s], a0.c, p2r[s]); p2i[s] = fma(lam2[s], a0.d, p2i[s]); \
		lam1[s] = fma(fma(ca0, csq[s], vb0), lam2[s], lam1[s]); \
	} \
	_Pragma("unroll") for (int s = 0; s < K; s++) { \
		p1r[s] = fma(lam1[s], a1.a, p1r[s]); p1i[s] = fma(lam1[s], a1.b, p1i[s]); \
		p2r[s] = fma(lam1[s], a1.c, p2r[s]); p2i[s] = fma(lam1[s], a1.d, p2i[s]); \
		lam2[s] = fma(fma(ca1, csq[s], vb1), lam1[s], lam2[s]); \
	} }

// K = 4 is asked to fit 7 waves per SIMD (72 instead of 74 VGPRs, no spills): the synthesis kernels are short of waves, not of
// registers per wave (pinned to 2 / 3 / 4 waves per SIMD leg_syn_spin<3> takes 1.51 / 1.29 / 1.0 of its time): C4 leg_syn 126.3 -> 121.9 ms
template<int K> __global__ __launch_bounds__(64, (K == 4 ? 7 : 1)) void leg_syn_s0(const LegK a)
{
	const int lane = threadIdx.x; int wv, m, bb;
	if (!leg_block(a, wv, m, bb)) return;
	const long row0 = PXS_UNIFORM_LONG(a.row[m]);
	const int nk = (a.lmax - m)/2 + 1;
	const double4_t* __restrict__ coef = a.coef + row0;
	const double4_t* __restrict__ at = reinterpret_cast<const double4_t*>(a.almt + (long)bb*a.almt_bs) + row0;
	double x[K], csq[K], lam1[K], lam2[K], p1r[K], p1i[K], p2r[K], p2i[K];
	int sc[K], rn[K], rs[K];
	bool alive_any = false;
	const bool polar = leg_wave_polar(a, wv, K);
#pragma unroll
	for (int s = 0; s < K; s++) {
		const int p = leg_pair_u(a, wv, K, s, lane);
		const bool valid = leg_pair_valid(a, p);
		rn[s] = valid ? a.ring_n[p] : -1; rs[s] = valid ? a.ring_s[p] : -1;
		x[s] = valid ? a.cth[p] : 0.0;
		const double sth = valid ? a.sth[p] : 0.0;
		csq[s] = polar ? -sth*sth : x[s]*x[s];
		const bool alive = valid && ((double)m <= a.lmax*sth + a.ofs);
		lam1[s] = 0; lam2[s] = 0; sc[s] = 0;
		if (alive && a.seed_mode != 2) { double mt; int e; pow_scaled(sth, m, mt, e); to_scaled(mt, e, lam2[s], sc[s]); }
		p1r[s] = p1i[s] = p2r[s] = p2i[s] = 0;
		alive_any |= alive;
	}
	int k = 0;
	if (__any(alive_any)) {
		// phase A: nobody live yet (LEG_LIVE) -> recurrence only, 4 steps per check (S0_PHASE_A)
		S0_SEEDED_PHASE_A
		k = PXS_UNIFORM_INT(k); coef = (const double4_t*)PXS_UNIFORM_LONG((long)coef);
		PXS_COUNT(0, (long)(nk - k)*K*6 + (a.seed_mode != 2 ? (long)k*K*2 : 0L));
		// phase B: some lanes are still below scale 0.  The steps are the plain fast steps (no per-lane gating); every
		// 4 steps the lanes below scale 0 are rescaled.  Such a lane accumulates scaled-up garbage meanwhile; its sums are
		// reset when it reaches scale 0 (its true terms before that are < 2^-340 of the final value).  A lane at scale 0 accumulates
		// from the wave's start on, whatever its value.
		while (k + 1 < nk) {
			bool pend = false;
#pragma unroll
			for (int s = 0; s < K; s++) pend |= (sc[s] < 0);
			if (!__any(pend)) break;
			for (int it = 0; it < 2 && k + 1 < nk; it++, k += 2) {
				const double4_t c0 = LDC(coef, k), c1 = LDC(coef, k+1), a0 = LDC(at, k), a1 = LDC(at, k+1);
				S0_SYN_PAIR(c0, c1, a0, a1)
			}
#pragma unroll
			for (int s = 0; s < K; s++)
				if (sc[s] < 0 && fabs(lam2[s]) > SC_BIG) {
					lam1[s] *= SC_SMALL; lam2[s] *= SC_SMALL;
					if (++sc[s] == 0) p1r[s] = p1i[s] = p2r[s] = p2i[s] = 0;
				}
		}
#pragma unroll
		for (int s = 0; s < K; s++) if (sc[s] < 0) { p1r[s] = p1i[s] = p2r[s] = p2i[s] = 0; lam1[s] = lam2[s] = 0; }   // never reached scale 0
		// phase C: fast loop, two steps per pair (lam1/lam2 swap roles, no register moves), two pairs per trip on alternating row sets: the prefetched rows are consumed
		// where they landed (a single-pair loop rotated them with 8-16 s_mov_b64 per pair; SALU was 27-45 % of the VALU count, profiles/r04_leg_sq_counters_c3.txt).
		// The rows are the compact ones, (a, b') with b' = b or, in polar waves, a + b, read with one drain per step pair and the rows of the next pair (table and
		// pre-scaled alm) requested right behind it (legendre_dev.hpp, "Row prefetch")
		const double2* __restrict__ cf = (const double2*)PXS_UNIFORM_LONG((long)((polar ? a.coef2p : a.coef2) + row0));
		coef2x2_t f = LDC2(cf, k); double4_t a0 = LDC(at, k), a1 = LDC(at, k+1);
		while (k + 3 < nk) {
			PXS_ROWS_DRAIN();
			coef2x2_t n = LDC2(cf, k+2); double4_t m0 = LDC(at, k+2), m1 = LDC(at, k+3);
			PXS_ROWS_ISSUED();
			S0_SYN_PAIR_C(f.a0, f.b0, f.a1, f.b1, a0, a1)
			PXS_ROWS_DRAIN();
			f = LDC2(cf, k+4); a0 = LDC(at, k+4); a1 = LDC(at, k+5);
			PXS_ROWS_ISSUED();
			S0_SYN_PAIR_C(n.a0, n.b0, n.a1, n.b1, m0, m1)
			k += 4;
		}
		for (; k + 1 < nk; k += 2) {
			PXS_ROWS_DRAIN();
			const coef2x2_t n = LDC2(cf, k+2); const double4_t m0 = LDC(at, k+2), m1 = LDC(at, k+3);
			PXS_ROWS_ISSUED();
			S0_SYN_PAIR_C(f.a0, f.b0, f.a1, f.b1, a0, a1)
			f = n; a0 = m0; a1 = m1;
		}
		PXS_ROWS_DRAIN();
		if (k < nk) {
#pragma unroll
			for (int s = 0; s < K; s++) {
				p1r[s] = fma(lam2[s], a0.a, p1r[s]); p1i[s] = fma(lam2[s], a0.b, p1i[s]);
				p2r[s] = fma(lam2[s], a0.c, p2r[s]); p2i[s] = fma(lam2[s], a0.d, p2i[s]);
			}
		}
	}
	double2* __restrict__ out = a.leg + (long)bb*a.leg_bs + (long)m*a.ld;
#pragma unroll
	for (int s = 0; s < K; s++) {      // ring indices and cos(theta) are re-read here rather than kept in registers through the loops
		const int p = leg_pair_u(a, wv, K, s, lane);
		const bool valid = leg_pair_valid(a, p);
		const int rn_ = valid ? a.ring_n[p] : -1, rs_ = valid ? a.ring_s[p] : -1;
		const double x_ = valid ? a.cth[p] : 0.0;
		if (rn_ >= 0) out[rn_] = make_double2(p1r[s] + x_*p2r[s], p1i[s] + x_*p2i[s]);
		if (rs_ >= 0) out[rs_] = make_double2(p1r[s] - x_*p2r[s], p1i[s] - x_*p2i[s]);
	}
}

// two fast steps of the spin-0 analysis: 2 x 4 lane sums into the LDS reduction tile, flush every 4 steps.  Blocks SLO .. K - 1 have started and take part in the sums
#define S0_ANA_PAIR(c0, c1) { \
	PXS_VCOPY(vb0, polar ? c0.c : c0.b); \
	PXS_VCOPY(vb1, polar ? c1.c : c1.b); \
	double t0 = 0, t1 = 0, t2 = 0, t3 = 0, u0 = 0, u1 = 0, u2 = 0, u3 = 0; \
	_Pragma("unroll") for (int s = 0; s < K; s++) { \
		if (s >= SLO) { t0 = fma(lam2[s], d1r[s], t0); t1 = fma(lam2[s], d1i[s], t1); t2 = fma(lam2[s], d2r[s], t2); t3 = fma(lam2[s], d2i[s], t3); } \
		lam1[s] = fma(fma(c0.a, csq[s], vb0), lam2[s], lam1[s]); \
	} \
	_Pragma("unroll") for (int s = 0; s < K; s++) { \
		if (s >= SLO) { u0 = fma(lam1[s], d1r[s], u0); u1 = fma(lam1[s], d1i[s], u1); u2 = fma(lam1[s], d2r[s], u2); u3 = fma(lam1[s], d2i[s], u3); } \
		lam2[s] = fma(fma(c1.a, csq[s], vb1), lam1[s], lam2[s]); \
	} \
	/* steps come in aligned pairs (phase A advances by 4, phases B and C by 2): kk is even here */ \
	LEG_RED_PUT(kk, t0, t1, t2, t3) \
	LEG_RED_PUT(kk+1, u0, u1, u2, u3) \
	kk += 2; \
	if (kk == LEG_FSTEPS) { leg_flush(red, pout + 4*kbase, lane, LEG_FSTEPS, a.atomic); kk = 0; kbase = k+2; } }

// one step of the spin-0 analysis on the step coefficients themselves: the four lane sums of the step into T0..T3, LA the current values, LB the previous ones (-> the next)
#define S0_ANA_STEP_C(ca, cb, LA, LB, T0, T1, T2, T3) { \
	PXS_VCOPY(vb, cb); \
	_Pragma("unroll") for (int s = 0; s < K; s++) { \
		if (s >= SLO) { T0 = fma(LA[s], d1r[s], T0); T1 = fma(LA[s], d1i[s], T1); T2 = fma(LA[s], d2r[s], T2); T3 = fma(LA[s], d2i[s], T3); } \
		LB[s] = fma(fma(ca, csq[s], vb), LA[s], LB[s]); \
	} }
// two fast steps of phase C from step kfirst on: the drain of the scalar rows between the two, the flush of a full tile and the request of the next rows (NEXT) at it
#define S0_ANA_PAIR_D(ca0, cb0, ca1, cb1, kfirst, NEXT) { \
	double t0 = 0, t1 = 0, t2 = 0, t3 = 0, u0 = 0, u1 = 0, u2 = 0, u3 = 0; \
	S0_ANA_STEP_C(ca0, cb0, lam2, lam1, t0, t1, t2, t3) \
	_Pragma("unroll") for (int s = 0; s < K; s++) PXS_DONE(lam1[s]); \
	PXS_DONE(t0); PXS_DONE(t1); PXS_DONE(t2); PXS_DONE(t3); \
	PXS_ROWS_DRAIN(); \
	if (kk == LEG_FSTEPS) { leg_flush(red, pout + 4*kbase, lane, LEG_FSTEPS, a.atomic); kk = 0; kbase = (kfirst); } \
	NEXT; \
	PXS_ROWS_ISSUED(); \
	S0_ANA_STEP_C(ca1, cb1, lam1, lam2, u0, u1, u2, u3) \
	LEG_RED_PUT(kk, t0, t1, t2, t3) \
	LEG_RED_PUT(kk+1, u0, u1, u2, u3) \
	kk += 2; }

// Phases B and C of the spin-0 analysis with NB started blocks (SLO = K - NB: the first of them; legendre_dev.hpp, "Block starts").  A wave enters at nb = 1 and
// walks through the stages in order; `more`: block SLO - 1 starts at this 4-step test, on to the next stage.  inC: phase B is over (wave-wide, whatever the stage).
// A block fetches its ring data when it starts (the lanes of it at scale 0; the others when they get there), until then it takes no part in the lane sums.
// (The synthesis kernel keeps one loop for all blocks: with stages of the same kind it came out level, see legendre_dev.hpp.)
// phase B: plain fast steps; every 4 steps the lanes below scale 0 are rescaled, and a lane of a started block that reaches scale 0 fetches its ring data (its
// true terms before that are < 2^-340 of the result).
// phase C: every lane at scale 0 (or without data).  The one-drain loop of leg_syn_s0 on the compact rows (a, b'), with the drain BETWEEN the two steps of a pair -- the
// ds_writes of the reduction count on lgkmcnt too and are a step old there -- and the flush of a full tile at that drain.  A row set therefore spans the second step of
// a pair and the first step of the next one: it is requested at one drain, complete at the next and read from there to the one after (legendre_dev.hpp, "Row prefetch").
// At the top of a trip (n.a1, n.b1) is the row of step k and f the rows of steps k + 1, k + 2: a stage that ends there leaves them to the next.
#define S0_ANA_STAGE(NB) if constexpr ((NB) <= K) { if (nb == (NB)) { \
	constexpr int SLO = K - (NB); \
	bool more = false; \
	if (!inC) { \
	while (k + 1 < nk) { \
		if constexpr ((NB) < K) if (k < nk && S0_BLOCK_STARTS(SLO - 1)) { more = true; break; } \
		bool pend = false; \
		_Pragma("unroll") for (int s = 0; s < K; s++) pend |= (sc[s] < 0); \
		if (!__any(pend)) break; \
		for (int it = 0; it < 2 && k + 1 < nk; it++, k += 2) { \
			const double4_t c0 = LDC(coef, k), c1 = LDC(coef, k+1); \
			S0_ANA_PAIR(c0, c1) \
		} \
		_Pragma("unroll") for (int s = 0; s < K; s++) \
			if (sc[s] < 0 && fabs(lam2[s]) > SC_BIG) { \
				lam1[s] *= SC_SMALL; lam2[s] *= SC_SMALL; \
				if (++sc[s] == 0 && s >= SLO) load_data(s); \
			} \
	} \
	if (!more) { \
		n = LDC2(cf, k); f = LDC2(cf, k+1); \
		PXS_ROWS_DRAIN(); \
		n.a1 = n.a0; n.b1 = n.b0;      /* (n.a1, n.b1): the row of the first step of the next pair (the row of step k + 1 that came with it is dropped: one 16-byte row per wave and m) */ \
		inC = 1; \
	} } \
	if (!more) { \
		for (;;) {      /* (two pairs per iteration on alternating row sets, see leg_syn_s0) */ \
			if constexpr ((NB) < K) if (k < nk && S0_BLOCK_STARTS(SLO - 1)) { more = true; break; } \
			if (!(k + 3 < nk)) break; \
			S0_ANA_PAIR_D(n.a1, n.b1, f.a0, f.b0, k, n = LDC2(cf, k+3)) \
			S0_ANA_PAIR_D(f.a1, f.b1, n.a0, n.b0, k+2, f = LDC2(cf, k+5)) \
			k += 4; \
		} \
	} \
	if (!more) { \
		slo = SLO; \
		nb = K + 1; \
	} else if constexpr ((NB) < K) { S0_BLOCK_BEGIN(SLO - 1) if (sc[SLO - 1] == 0) load_data(SLO - 1); if constexpr ((NB) + 1 < K) { S0_NEXT_START(SLO - 2) } nb = (NB) + 1; } \
} }
// The last steps of a wave, fewer than four, with the blocks from `slo` on started, whichever stage ended: one copy, the started blocks tested at run time.  (A copy
// per stage cost registers, not time: the single-pair loop of every stage kept the chains in a register set of its own -- leg_ana_s0<8> 156 -> 176 VGPRs, a wave per SIMD.)
#define S0_ANA_TAIL { const int SLO = slo; \
		if (k + 1 < nk) { \
			S0_ANA_PAIR_D(n.a1, n.b1, f.a0, f.b0, k, (void)0) \
			k += 2; \
		} \
		PXS_ROWS_DRAIN(); \
		if (kk == LEG_FSTEPS) { leg_flush(red, pout + 4*kbase, lane, LEG_FSTEPS, a.atomic); kk = 0; kbase = k; } \
		if (k < nk) { \
			double t0 = 0, t1 = 0, t2 = 0, t3 = 0; \
			_Pragma("unroll") for (int s = 0; s < K; s++) if (s >= SLO) { t0 = fma(lam2[s], d1r[s], t0); t1 = fma(lam2[s], d1i[s], t1); t2 = fma(lam2[s], d2r[s], t2); t3 = fma(lam2[s], d2i[s], t3); } \
			LEG_RED_PUT(kk, t0, t1, t2, t3) \
			kk++; \
		} }


template<int K> __global__ __launch_bounds__(64) void leg_ana_s0(const LegK a)
{
	PXS_SHARED(double, red);
	const int lane = threadIdx.x; int wv, m, bb;
	if (!leg_block(a, wv, m, bb)) return;
	const long row0 = PXS_UNIFORM_LONG(a.row[m]);
	const int nk = (a.lmax - m)/2 + 1;
	const double4_t* __restrict__ coef = a.coef + row0;
	double* __restrict__ pout = a.part + (long)bb*a.mom_bs + ((long)wv*a.rows_chunk + (row0 - a.rowbase))*4;
	const double2* __restrict__ in = a.leg + (long)bb*a.leg_bs + (long)m*a.ld;
	double csq[K], lam1[K], lam2[K], d1r[K], d1i[K], d2r[K], d2i[K];
	int sc[K];
	bool alive_any = false;
	const bool polar = leg_wave_polar(a, wv, K);
	// ring data of slot s: sum and (difference x cos theta) of the north and south ring
	auto load_data = [&](int s) {
		const int p = leg_pair(a, wv, K, s, PXS_LATE_INT(lane));
		const bool valid = leg_pair_valid(a, p);
		const int rn = valid ? a.ring_n[p] : -1, rs = valid ? a.ring_s[p] : -1;
		const double x = valid ? a.cth[p] : 0.0;
		const double2 vn = rn >= 0 ? in[rn] : make_double2(0, 0);
		const double2 vs = rs >= 0 ? in[rs] : make_double2(0, 0);
		d1r[s] = vn.x + vs.x; d1i[s] = vn.y + vs.y;
		d2r[s] = (vn.x - vs.x)*x; d2i[s] = (vn.y - vs.y)*x;
	};
#pragma unroll
	for (int s = 0; s < K; s++) {
		const int p = leg_pair(a, wv, K, s, lane);
		const bool valid = leg_pair_valid(a, p);
		const double x = valid ? a.cth[p] : 0.0;
		const double sth = valid ? a.sth[p] : 0.0;
		csq[s] = polar ? -sth*sth : x*x;
		const bool alive = valid && ((double)m <= a.lmax*sth + a.ofs);
		lam1[s] = 0; lam2[s] = 0; sc[s] = 0;
		if (alive && a.seed_mode != 2) { double mt; int e; pow_scaled(sth, m, mt, e); to_scaled(mt, e, lam2[s], sc[s]); }
		// a lane below scale 0 keeps zero data until it gets there, so that it can run the ungated steps
		d1r[s] = d1i[s] = d2r[s] = d2i[s] = 0;
		alive_any |= alive;
	}
	if (!__any(alive_any)) return;      // partial buffer is pre-zeroed
	int k = 0;
	S0_SEEDED_PHASE_A
	k = PXS_UNIFORM_INT(k); coef = (const double4_t*)PXS_UNIFORM_LONG((long)coef);
	// executed work: the recurrence FMAs of every block from here on (and of phase A where it ran), the accumulation FMAs of block K - 1, which starts with the
	// wave; the other blocks add theirs as they start (S0_BLOCK_BEGIN)
	constexpr int DIR = 1;
	PXS_COUNT2(DIR, (long)(nk - k)*K*2 + (a.seed_mode != 2 ? (long)k*K*2 : 0L), (long)(nk - k)*4, K);
	int knext = LEG_NEVER;      // seeded launches: the start step of the next block to start (the seed tail)
	if constexpr (K > 1) { S0_NEXT_START(K - 2) }
	if (lane == 0 && !a.atomic) a.first[wv*a.nmc + (m - a.m0)] = k + 1;      // rows before k are not written (reduce_partials skips them)
	// ring data of block K - 1: the lanes that start at scale 0 or reached it during phase A (rings without signal have lam = 0)
	if (sc[K - 1] == 0) load_data(K - 1);
	int kk = 0, kbase = k;
	// phases B and C, by number of started blocks (S0_ANA_STAGE)
	const double2* __restrict__ cf = (const double2*)PXS_UNIFORM_LONG((long)((polar ? a.coef2p : a.coef2) + row0));
	coef2x2_t n, f;
	int nb = 1, inC = 0, slo = 0;
	S0_ANA_STAGE(1) S0_ANA_STAGE(2) S0_ANA_STAGE(3) S0_ANA_STAGE(4) S0_ANA_STAGE(5) S0_ANA_STAGE(6) S0_ANA_STAGE(7) S0_ANA_STAGE(8)
	static_assert(K <= 8, "leg_ana_s0: one S0_ANA_STAGE per block (K = 12 takes four more and was measured with them: profiles/README.md, \"Block starts\")");
	S0_ANA_TAIL
	if (kk > 0) leg_flush(red, pout + 4*kbase, lane, kk, a.atomic);
}


// ---- batched spin-0 analysis as an FP64-MFMA GEMM (round 5) -----------------------------------------------------------------------
// For the maps of a batched call the per-m problem is  mom[k][map, c] = sum_ring p_k(ring) D[ring][map, c]  with the SAME p_k(ring) for
// every map (c = the four real right-hand sides of leg_ana_s0: re / im of the ring-pair sum, re / im of the difference x cos theta):
// the ring axis is the K dimension of v_mfma_f64_16x16x4_f64, M = 16 consecutive recurrence steps, N = 16 = 4 maps x 4 sides.
// The reference loops over the maps, one ducc0 call each (pixell/curvedsky.py:1038-1046); here a wave runs ONE Ishioka recurrence per
// ring pair (lane = ring pair, phases A / B as in leg_ana_s0; a lane below scale 0 contributes p = 0), parks 16 steps of it in a
// [16][64] LDS tile and issues 16 MFMAs per tile and group of 4 maps against B operands (the ring data, 16 x 2 VGPRs per group) that
// stay in registers for the whole l loop.  What the VALU form pays per map -- the recurrence (2 of 6 FMAs), the 64-lane
// reduce-scatter (10 of ~58 VALU per step) and the three-VGPR-operand FMA rate -- is paid once per 4 NG maps or not at all.
//  * Workgroup = 8 waves over 512 consecutive ring pairs, wave w the pairs [64 w, 64 w + 64): polar waves join at the tile where their
//    first lane reaches scale 0.  Tiles are aligned to multiples of 16 steps of the m; every wave adds its 16 x 16 accumulators
//    into an LDS tile (ds_add_f64) and after ONE barrier per tile the waves share out the flush: one global_atomic_add_f64 per
//    (chunk of 512 pairs, row, map) -- the count of leg_ana_s0<8>.
//  * Recurrence lane L is MFMA slot (kk, q) = (L >> 4, L & 15): the P row is written as 64 consecutive doubles and lane (i, kk)
//    reads its 16 A operands P[i][16 kk + q] from rows of 65 doubles -- conflict-free for ds_read_b64 and ds_read2_b64 alike.
//  * The ring data reach the B registers through the LDS: the 512 threads read the rows leg[map][m][ring] of 4 maps coalesced (one
//    ring pair per thread), park (sum, difference x cos) as 16 doubles per pair (17-double entries: lane (j, kk) of MFMA q then reads
//    entry 64 w + 16 kk + q, double j, conflict-free), and every lane picks its 16 operands.  (First form: per-lane gathers straight
//    from global memory -- 16 % of the kernel's wave time.)
//  * Step coefficients come from a compact table (a, b) resp. (a, a + b) per step (LegTables::coef2), the 16 steps of the NEXT tile
//    requested with four s_load_dwordx16 before the MFMAs of the current one (first form: the 32-byte rows of the VALU kernels,
//    requested and awaited group by group -- four scalar-load round trips per tile, 38 % of the wave time).
// one Ishioka recurrence in extended-exponent form (the chain of the MFMA kernels, cf. SpinChain): p_{k+1} = (a x^2 + b) p_k + p_{k-1}, lam2 the current value
struct S0Chain {
	double csq, lam1, lam2; int sc;
	__device__ __forceinline__ double step(double ca, double cb) { const double p = lam2, nx = fma(mm_coef(ca, csq, cb), lam2, lam1); lam1 = p; lam2 = nx; return p; }
	__device__ __forceinline__ void rescale() { if (fabs(lam2) > SC_BIG) { lam1 *= SC_SMALL; lam2 *= SC_SMALL; sc++; } }
	__device__ __forceinline__ void park_sign(int, double*) const {}
};
// the spin-0 side of leg_ana_mm / leg_syn_mm (legendre_dev.hpp): one chain per lane, 64 ring pairs per wave
struct S0Mm {
	typedef S0Chain Chain;
	static constexpr int SLOTS = 64;
	static constexpr bool SIGNED = false;
	static constexpr bool BREG_SYNC = true;      // (the spin analysis has none: kept as it was, kernel by kernel)
	static __device__ __forceinline__ int steps(const LegK& a, int m, int& par) { par = 0; return (a.lmax - m)/2 + 1; }
	// start value of ring pair p at m; returns whether the pair carries signal at this m
	static __device__ __forceinline__ bool init(const LegK& a, int p, int m, int, bool polar, S0Chain& C) {
		const bool valid = p < a.npairs;
		const double x = valid ? a.cth[p] : 0.0, sth = valid ? a.sth[p] : 0.0;
		C.csq = polar ? -sth*sth : x*x;
		const bool alive = valid && ((double)m <= a.lmax*sth + a.ofs);
		C.lam1 = 0; C.lam2 = 0; C.sc = 0;
		if (alive) { double mt; int e; pow_scaled(sth, m, mt, e); to_scaled(mt, e, C.lam2, C.sc); }
		return alive;
	}
	// polar waves take the table (a, a + b)
	static __device__ __forceinline__ const double* table(const LegK& a, bool polar, long row0) { return reinterpret_cast<const double*>(polar ? a.coef2p : a.coef2) + 2*row0; }
	// phase A (S0_PHASE_A for one chain, on the 32-byte rows of the VALU kernels): recurrence only until the first lane of the wave is live (LEG_LIVE); returns the step reached
	static __device__ __forceinline__ int phase_a(const LegK& a, S0Chain& C, long row0, bool polar, int nk) {
		const double4_t* __restrict__ coef = a.coef + row0;
		int k = 0;
		while (k + 4 <= nk) {
			if (__any(LEG_IS_LIVE(C.lam2, C.sc))) break;
			const double4_t q0 = LDC(coef, k), q1 = LDC(coef, k+1), q2 = LDC(coef, k+2), q3 = LDC(coef, k+3);
			const double b0 = polar ? q0.c : q0.b, b1 = polar ? q1.c : q1.b, b2 = polar ? q2.c : q2.b, b3 = polar ? q3.c : q3.b;
			C.lam1 = fma(fma(q0.a, C.csq, b0), C.lam2, C.lam1);
			C.lam2 = fma(fma(q1.a, C.csq, b1), C.lam1, C.lam2);
			C.lam1 = fma(fma(q2.a, C.csq, b2), C.lam2, C.lam1);
			C.lam2 = fma(fma(q3.a, C.csq, b3), C.lam1, C.lam2);
			if (C.sc < 0) C.rescale();
			k += 4;
		}
		return k;
	}
	// analysis prologue: the north and south ring values of the slot's pair in the 4 maps from map0 on, parked as (sum re, im, difference x cos theta re, im) per map
	struct Data { double2 vn[4], vs[4]; };
	static __device__ __forceinline__ void load(const LegK& a, int m, int map0, int rn, int rs, Data& d) {
#pragma unroll
		for (int mm = 0; mm < 4; mm++) {
			const int map = map0 + mm;
			const double2* __restrict__ in = a.leg + (long)map*a.leg_bs + (long)m*a.ld;
			const bool okm = map < a.nmaps;
			d.vn[mm] = (okm && rn >= 0) ? in[rn] : make_double2(0, 0); d.vs[mm] = (okm && rs >= 0) ? in[rs] : make_double2(0, 0);
		}
	}
	static __device__ __forceinline__ void park(const Data& d, double x, int, double* __restrict__ ent) {
#pragma unroll
		for (int mm = 0; mm < 4; mm++) {
			ent[4*mm + 0] = d.vn[mm].x + d.vs[mm].x; ent[4*mm + 1] = d.vn[mm].y + d.vs[mm].y;
			ent[4*mm + 2] = (d.vn[mm].x - d.vs[mm].x)*x; ent[4*mm + 3] = (d.vn[mm].y - d.vs[mm].y)*x;
		}
	}
	// synthesis epilogue.  Register r of acc[g][rb] at lane (i4 = lane / 16, j = lane % 16): ring pair 16 rb + 4 r + i4, column j = 4 (map in the group) + c: a lane holds
	// one column of one ring pair, and the quad (even re, even im, odd re, odd im) is combined across lanes into the north and south ring values
	template<int NG> static __device__ __forceinline__ void store(const LegK& a, int m, int bb, int pbase, int lane, mm_acc (&acc)[NG][4]) {
		const int c = lane & 3;
#pragma unroll
		for (int g = 0; g < NG; g++) {
			const int map = (bb*NG + g)*4 + ((lane & 15) >> 2);
			double* __restrict__ out = reinterpret_cast<double*>(a.leg + (long)(map < a.nmaps ? map : 0)*a.leg_bs + (long)m*a.ld) + (c & 1);
#pragma unroll
			for (int rb = 0; rb < 4; rb++)
#pragma unroll
				for (int r = 0; r < 4; r++) {
					const int p = pbase + 16*rb + 4*r + (lane >> 4);
					const bool valid = p < a.npairs && map < a.nmaps;
					const double v = acc[g][rb][r], o = MMS_XOR2(v);
					const double x = valid ? a.cth[p] : 0.0;
					// c = 0, 1: north ring, even + x odd; c = 2, 3: south ring, even - x odd (this lane holds the odd part)
					const double val = c < 2 ? fma(x, o, v) : fma(-x, v, o);
					const int ring = valid ? (c < 2 ? a.ring_n[p] : a.ring_s[p]) : -1;
					if (ring >= 0) out[2*ring] = val;
				}
		}
	}
};
template<int NG, int W> __global__ __launch_bounds__(64*W, 4) void leg_ana_s0_mm(const LegK a) { leg_ana_mm<S0Mm, NG, W>(a); }


// ---- batched spin-0 synthesis as an FP64-MFMA GEMM (round 5) ----------------------------------------------------------------------
// The transpose of leg_ana_s0_mm: leg[ring][map, c] = sum_k p_k(ring) almt[k][map, c], c = the four real columns of alm_pre_s0 (even
// part re / im, odd part re / im).  M = 16 ring pairs, N = 16 = 4 maps x 4 columns, K = recurrence steps: the accumulators
// (64 ring pairs x 16 columns per group of 4 maps = 4 x 8 VGPRs) stay in registers for the whole l loop, one wave per workgroup
// and NO cross-wave step at all (every wave owns its rings).  A operands: lane (i, kk) of MFMA (rb, q) takes step q + 4 kk of ring
// pair 16 rb + i from the wave's [16][68] P tile (the same tile and recurrence as the analysis; rows of 68 doubles: the four steps of
// an MFMA lie 4 rows = 32 banks apart); B operands: the pre-scaled alm rows of the tile, one double per lane and MFMA step-quad,
// loaded a tile ahead (the 32 bytes per step and map the VALU kernel takes through the scalar cache).  At the end a lane holds one
// column of one ring pair: the quad (even re, even im, odd re, odd im) is combined across lanes into the north and south ring values.

template<int NG> __global__ __launch_bounds__(64, 4) void leg_syn_s0_mm(const LegK a) { leg_syn_mm<S0Mm, NG>(a); }

// ---- launches: the kernel of (direction, form, K or ng); the ring pairs per lane the host's rules select are 4 and 2 (synthesis), 8, 4 and 2 (analysis) ----
void launch_leg_s0(bool analysis, int ng, int K, dim3 grid, hipStream_t st, const LegK& a) {
	static const bool once = leg_mm_lds_optin({leg_ana_s0_mm<2, MM_WAVES>, leg_ana_s0_mm<1, MM_WAVES>}); (void)once;
	// (a K without a compiled kernel is an error, not another kernel: the grid, the seeds and the partial moments were laid out for the K asked for)
	const LegKernel k = analysis ? (ng == 2 ? leg_ana_s0_mm<2, MM_WAVES> : ng ? leg_ana_s0_mm<1, MM_WAVES> : K == 8 ? leg_ana_s0<8> : K == 4 ? leg_ana_s0<4> : K == 2 ? leg_ana_s0<2> : nullptr)
	                             : (ng == 2 ? leg_syn_s0_mm<2> : ng ? leg_syn_s0_mm<1> : K == 4 ? leg_syn_s0<4> : K == 2 ? leg_syn_s0<2> : nullptr);
	PXS_REQUIRE(k != nullptr, "internal: no spin-0 Legendre kernel compiled for this number of ring pairs per lane");
	leg_launch(k, analysis, ng, grid, st, a);
}

} // namespace pxs
