// Spin-s Legendre kernels for gfx950 (design notes: head of legendre.hip): leg_syn_spin / leg_ana_spin (one wave per workgroup, K ring pairs per lane) and the
// FP64-MFMA forms of batched calls, leg_syn_spin_mm / leg_ana_spin_mm.  Replaces ducc0's alm2leg / leg2alm for spin > 0 as reached from
// pixell/curvedsky.py:907-960, 1032-1084.
#include "legendre_dev.hpp"

namespace pxs {

// ---------------------------------------------------------------------------------
// spin-s kernels.  rows l = l0..lmax.  chains G+ (spin +s) and G- (spin -s) of the NORTH ring;
// south ring: F+_S = (-1)^(l+m) F-_N, F-_S = (-1)^(l+m) F+_N.
// G_{l+1} = (a x +- b) G_l - G_{l-1}; in polar waves x -> u = -2 sin^2(theta/2), +-b -> a +- b.
// ---------------------------------------------------------------------------------
template<int K> struct SpinState {
	double x[K], gp1[K], gp2[K], gm1[K], gm2[K];
	int scp[K], scm[K];
};

template<int K> __device__ __forceinline__ bool spin_init(const LegK& a, int wv, int lane, int m, SpinState<K>& S, int* rn, int* rs, bool polar) {
	const int s_ = a.spin;
	bool alive_any = false;
#pragma unroll
	for (int s = 0; s < K; s++) {
		const int p = leg_pair(a, wv, K, s, lane);
		const bool valid = leg_pair_valid(a, p);
		rn[s] = valid ? a.ring_n[p] : -1; rs[s] = valid ? a.ring_s[p] : -1;
		const double cth = valid ? a.cth[p] : 0.0;
		const double sth = valid ? a.sth[p] : 0.0;
		const double shh = valid ? a.sh2[p] : 0.0;
		S.x[s] = polar ? -2.0*shh*shh : cth;
		// libsharp's m-limit generalised to spin: rings with m beyond it carry nothing up to lmax
		const double t1 = a.lmax*sth + a.ofs;
		const double b = -2.0*s_*fabs(cth);
		const double c = (double)s_*s_ - t1*t1;
		const double discr = b*b - 4*c;
		const double mlim = discr <= 0 ? a.lmax : fmin((double)a.lmax, 0.5*(-b + sqrt(discr)));
		const bool alive = valid && ((double)m <= mlim + 0.5);
		S.gp1[s] = S.gm1[s] = 0; S.gp2[s] = S.gm2[s] = 0; S.scp[s] = S.scm[s] = 0;
		if (alive && a.seed_mode != 2) {
			const double sh = shh, ch = a.ch2[p];
			double m1, m2; int e1, e2;
			if (m >= s_) {
				pow_scaled(sh, m + s_, m1, e1); pow_scaled(ch, m - s_, m2, e2);
				double mt = m1*m2; int e = e1 + e2 + m; frexp_norm(mt, e); to_scaled(mt, e, S.gp2[s], S.scp[s]);
				pow_scaled(sh, m - s_, m1, e1); pow_scaled(ch, m + s_, m2, e2);
				mt = m1*m2; e = e1 + e2 + m; frexp_norm(mt, e); to_scaled(mt, e, S.gm2[s], S.scm[s]);
			} else {
				pow_scaled(sh, s_ + m, m1, e1); pow_scaled(ch, s_ - m, m2, e2);
				double mt = m1*m2; int e = e1 + e2; frexp_norm(mt, e); to_scaled(mt, e, S.gp2[s], S.scp[s]);
				pow_scaled(sh, s_ - m, m1, e1); pow_scaled(ch, s_ + m, m2, e2);
				mt = m1*m2; e = e1 + e2; frexp_norm(mt, e); to_scaled(mt, e, S.gm2[s], S.scm[s]);
				if ((s_ - m) & 1) S.gm2[s] = -S.gm2[s];
			}
		}
		alive_any |= alive;
	}
	return alive_any;
}

// The two VALU kernels below write the phase skeleton (seeds, phases A / B / C) out, with four macros, as leg_syn_s0 / leg_ana_s0 do (leg_s0.hip).  One driver
// with the chain state and the accumulators as policies was built for the four and taken out again.  The spin-0 synthesis on it lost its 52 bytes of scratch and was
// 7 % slower all the same (profiles/README.md).  These two
// on that driver fit the same registers (96 / 69 VGPRs synthesis, 152 / 124 / 96 analysis, no scratch) but computed the values of these kernels to rounding only: in
// phase A the compiler contracts a x + c into one FMA or leaves multiply and add apart depending on the basic block the addition ends up in, and for which slots
// it does so follows the code around the loop, not the expression (here: the G- chain of one slot unfused, on the driver of two).  Bit for bit is what a
// refactor owes, and no way of writing the expression pins the compiler's choice to the present one.  Change the two copies together.
// phase A of the spin kernels: 4 steps per rescale / activity test; sgn is unchanged by 4 steps
#define SPIN_PHASE_A \
	while (j + 4 <= nl) { \
		bool act = false; \
		_Pragma("unroll") for (int s = 0; s < K; s++) act |= LEG_IS_LIVE(S.gp2[s], S.scp[s]) || LEG_IS_LIVE(S.gm2[s], S.scm[s]); \
		if (__any(act)) break; \
		const double4_t q0 = LDC(coef, j), q1 = LDC(coef, j+1), q2 = LDC(coef, j+2), q3 = LDC(coef, j+3); \
		_Pragma("unroll") for (int s = 0; s < K; s++) { \
			double ax; \
			ax = q0.a*S.x[s]; S.gp1[s] = fma(ax + (polar ? q0.c : q0.b), S.gp2[s], -S.gp1[s]); S.gm1[s] = fma(ax + (polar ? q0.d : -q0.b), S.gm2[s], -S.gm1[s]); \
			ax = q1.a*S.x[s]; S.gp2[s] = fma(ax + (polar ? q1.c : q1.b), S.gp1[s], -S.gp2[s]); S.gm2[s] = fma(ax + (polar ? q1.d : -q1.b), S.gm1[s], -S.gm2[s]); \
			ax = q2.a*S.x[s]; S.gp1[s] = fma(ax + (polar ? q2.c : q2.b), S.gp2[s], -S.gp1[s]); S.gm1[s] = fma(ax + (polar ? q2.d : -q2.b), S.gm2[s], -S.gm1[s]); \
			ax = q3.a*S.x[s]; S.gp2[s] = fma(ax + (polar ? q3.c : q3.b), S.gp1[s], -S.gp2[s]); S.gm2[s] = fma(ax + (polar ? q3.d : -q3.b), S.gm1[s], -S.gm2[s]); \
			if (S.scp[s] < 0 && fabs(S.gp2[s]) > SC_BIG) { S.gp1[s] *= SC_SMALL; S.gp2[s] *= SC_SMALL; S.scp[s]++; } \
			if (S.scm[s] < 0 && fabs(S.gm2[s]) > SC_BIG) { S.gm1[s] *= SC_SMALL; S.gm2[s] *= SC_SMALL; S.scm[s]++; } \
		} \
		j += 4; \
	}

// phase A with the recurrence seeds (legendre_dev.hpp): mode 2 loads the state, the step reached and the start steps of the blocks (the seed tail, knext;
// legendre_dev.hpp, "Block starts"), mode 1 records them after running phase A (the start steps as the blocks start: SPIN_BLOCK_BEGIN; LEG_NEVER until then)
#define SPIN_SEEDED_PHASE_A \
	if (a.seed_mode == 2) { \
		const double* sd = a.seed_d + ((long)m*a.nwave + wv)*(4*K*64); const int* si = a.seed_i + ((long)m*a.nwave + wv)*((2*K+1)*64); \
		j = PXS_UNIFORM_INT(si[2*K*64]); \
		_Pragma("unroll") for (int s = 0; s < K; s++) { \
			S.gp1[s] = sd[s*64 + lane]; S.gp2[s] = sd[(K+s)*64 + lane]; S.gm1[s] = sd[(2*K+s)*64 + lane]; S.gm2[s] = sd[(3*K+s)*64 + lane]; \
			S.scp[s] = si[s*64 + lane]; S.scm[s] = si[(K+s)*64 + lane]; } \
	} else { \
		SPIN_PHASE_A \
		if (a.seed_mode == 1) { \
			double* sd = a.seed_d + ((long)m*a.nwave + wv)*(4*K*64); int* si = a.seed_i + ((long)m*a.nwave + wv)*((2*K+1)*64); \
			_Pragma("unroll") for (int s = 0; s < K; s++) { \
				sd[s*64 + lane] = S.gp1[s]; sd[(K+s)*64 + lane] = S.gp2[s]; sd[(2*K+s)*64 + lane] = S.gm1[s]; sd[(3*K+s)*64 + lane] = S.gm2[s]; \
				si[s*64 + lane] = S.scp[s]; si[(K+s)*64 + lane] = S.scm[s]; } \
			if (lane == 0) si[2*K*64] = j; else if (lane <= K) si[2*K*64 + lane] = LEG_NEVER; \
		} \
	}
// does block c start at this 4-step test (one of its chains, or one of a more polar block, is live)?  Seeded launches read it off the seed tail.  Tests are
// at multiples of 4 steps (phase A ends at one): a phase B that ends on a lone pair leaves the last steps of the wave without a test
#define SPIN_BLOCK_STARTS(c) ((j & 3) == 0 && (a.seed_mode == 2 ? j >= knext : __any(leg_live_upto<c>(S.gp2, S.scp) || leg_live_upto<c>(S.gm2, S.scm))))
// the seed tail of this (wave, m): [0] the step phase A reached, [1 + c] the start step of block c
#define SPIN_SEED_TAIL (a.seed_i + ((long)m*a.nwave + wv)*((2*K+1)*64) + 2*K*64)
// block c starts at step j: counted from here on; recorded in the seed tail by the lane that wrote LEG_NEVER there.  NEXT_START(c): a seeded launch reads the start of block c
#define SPIN_BLOCK_BEGIN(c) { PXS_COUNT_BLOCK(DIR, (long)(nl - j)*8); if (a.seed_mode == 1 && lane == (c) + 1) SPIN_SEED_TAIL[(c) + 1] = j; }
#define SPIN_NEXT_START(c) if (a.seed_mode == 2) knext = PXS_UNIFORM_INT(SPIN_SEED_TAIL[(c) + 1]);

// Row sets of the phase-C loops (legendre_dev.hpp, "Row prefetch"): the 32-byte rows of two consecutive steps, requested together.  SPIN_ROW0(r) / SPIN_ROW1(r):
// (ca, c1, c2) of the first / second step of set r, (a, b, -b) in plain waves and the columns (a, c, d) in polar ones -- written where the row is used, behind the
// drain: anything computed from a row at its request would make the compiler wait there.  (Plain waves on the compact rows (a, b), in a loop of their own next to the
// polar waves' loop, had every load at its distance too, but the kernels then held the chains and the sums of both loops in registers of their own:
// leg_syn_spin<3> 103 -> 168 VGPRs, leg_ana_spin<4> 152 -> 178, a wave per SIMD less each.)
struct spin_rows_t { double4_t r0, r1; };
__device__ __forceinline__ spin_rows_t spin_rows(const double4_t* coef, long i) { spin_rows_t r; r.r0 = LDC(coef, i); r.r1 = LDC(coef, i+1); return r; }
#define SPIN_ROW0(r) r.r0.a, polar ? r.r0.c : r.r0.b, polar ? r.r0.d : -r.r0.b
#define SPIN_ROW1(r) r.r1.a, polar ? r.r1.c : r.r1.b, polar ? r.r1.d : -r.r1.b

// (step coefficient a x +- b as one FMA with the additive constant copied to a VGPR once per step -- gfx950 allows one
// scalar source per VALU op -- instead of a multiply shared by two adds: 12 + 2/K instead of 13 VALU ops per ring pair and l)
// two fast steps of the spin synthesis (G1/G2 swap roles).  The south-ring sums take (-1)^(l+m) a: they are
// accumulated with sign +1 on even steps and -1 on odd steps and multiplied by the sign of the first step at the end.
#define SPIN_SYN_PAIR(f0, f1, a0, a1) SPIN_SYN_PAIR_C(f0.a, polar ? f0.c : f0.b, polar ? f0.d : -f0.b, f1.a, polar ? f1.c : f1.b, polar ? f1.d : -f1.b, a0, a1)
// ... on the step coefficients themselves: (ca, c1, c2) of a step = a and the additive constants of the G+ and the G- chain
#define SPIN_SYN_PAIR_C(ca0, c10, c20, ca1, c11, c21, a0, a1) { \
	{ \
		const double ca = ca0, c1 = c10, c2 = c20; \
		PXS_VCOPY(v1, c1); PXS_VCOPY(v2, c2); \
		_Pragma("unroll") for (int s = 0; s < K; s++) { \
			const double gp = S.gp2[s], gm = S.gm2[s]; \
			pnr[s] = fma(gp, a0.a, pnr[s]); pni[s] = fma(gp, a0.b, pni[s]); \
			mnr[s] = fma(gm, a0.c, mnr[s]); mni[s] = fma(gm, a0.d, mni[s]); \
			qsr[s] = fma(gm, a0.a, qsr[s]); qsi[s] = fma(gm, a0.b, qsi[s]); \
			nsr[s] = fma(gp, a0.c, nsr[s]); nsi[s] = fma(gp, a0.d, nsi[s]); \
			S.gp1[s] = fma(fma(ca, S.x[s], v1), gp, -S.gp1[s]); S.gm1[s] = fma(fma(ca, S.x[s], v2), gm, -S.gm1[s]); \
		} \
	} \
	{ \
		const double ca = ca1, c1 = c11, c2 = c21; \
		PXS_VCOPY(v1, c1); PXS_VCOPY(v2, c2); \
		_Pragma("unroll") for (int s = 0; s < K; s++) { \
			const double gp = S.gp1[s], gm = S.gm1[s]; \
			pnr[s] = fma(gp, a1.a, pnr[s]); pni[s] = fma(gp, a1.b, pni[s]); \
			mnr[s] = fma(gm, a1.c, mnr[s]); mni[s] = fma(gm, a1.d, mni[s]); \
			qsr[s] = fma(-gm, a1.a, qsr[s]); qsi[s] = fma(-gm, a1.b, qsi[s]); \
			nsr[s] = fma(-gp, a1.c, nsr[s]); nsi[s] = fma(-gp, a1.d, nsi[s]); \
			S.gp2[s] = fma(fma(ca, S.x[s], v1), gp, -S.gp2[s]); S.gm2[s] = fma(fma(ca, S.x[s], v2), gm, -S.gm2[s]); \
		} \
	} }

#define SPIN_SYN_PAIR_R(s0, s1, a0, a1) SPIN_SYN_PAIR_C(s0, s1, a0, a1)
// phase C of the spin synthesis (the row sets above; here a set is the two steps of a pair): one drain per step pair, the rows of the next pair
// (table and pre-scaled alm) requested right behind it, two pairs per trip on alternating row sets (leg_syn_s0)
#define SPIN_SYN_PHASE_C { \
	spin_rows_t f = spin_rows(coef, j); a0 = LDC(at, j); a1 = LDC(at, j+1); \
	while (j + 3 < nl) { \
		PXS_ROWS_DRAIN(); \
		spin_rows_t n = spin_rows(coef, j+2); double4_t m0 = LDC(at, j+2), m1 = LDC(at, j+3); \
		PXS_ROWS_ISSUED(); \
		SPIN_SYN_PAIR_R(SPIN_ROW0(f), SPIN_ROW1(f), a0, a1) \
		PXS_ROWS_DRAIN(); \
		f = spin_rows(coef, j+4); a0 = LDC(at, j+4); a1 = LDC(at, j+5); \
		PXS_ROWS_ISSUED(); \
		SPIN_SYN_PAIR_R(SPIN_ROW0(n), SPIN_ROW1(n), m0, m1) \
		j += 4; \
	} \
	for (; j + 1 < nl; j += 2) { \
		PXS_ROWS_DRAIN(); \
		const spin_rows_t n = spin_rows(coef, j+2); const double4_t m0 = LDC(at, j+2), m1 = LDC(at, j+3); \
		PXS_ROWS_ISSUED(); \
		SPIN_SYN_PAIR_R(SPIN_ROW0(f), SPIN_ROW1(f), a0, a1) \
		f = n; a0 = m0; a1 = m1; \
	} \
	PXS_ROWS_DRAIN(); }

// (leg_syn_spin<3> must stay below 128 VGPRs = 4 waves per SIMD; computing the lane as threadIdx.x & 63 for multi-wave
// workgroups once pushed it to 132 = 3 waves and leg_syn from 120 to 151 ms at config 3 -- keep an eye on that cliff.)
// (leg_syn_spin<3> held to 96 VGPRs = 5 waves per SIMD by __launch_bounds__: 20 bytes of spills, 102.0 -> 100.1 ms at C3: inside the noise, not kept)
template<int K> __global__ __launch_bounds__(64) void leg_syn_spin(const LegK a)
{
	const int lane = threadIdx.x; int wv, m, bb;
	if (!leg_block(a, wv, m, bb)) return;
	const int l0 = max(m, a.spin);
	const int nl = a.lmax - l0 + 1;
	double2* __restrict__ outq = a.leg + (long)bb*a.leg_bs + (long)m*a.ld;
	double2* __restrict__ outu = a.leg + (long)bb*a.leg_bs + ((long)a.nm + m)*a.ld;
	SpinState<K> S; int rn[K], rs[K];
	// north: P = sum G+ a+, M = sum G- a-;  south (before the sign): qs = sum +-G- a+, ns = sum +-G+ a-
	double pnr[K], pni[K], mnr[K], mni[K], qsr[K], qsi[K], nsr[K], nsi[K];
#pragma unroll
	for (int s = 0; s < K; s++) pnr[s] = pni[s] = mnr[s] = mni[s] = qsr[s] = qsi[s] = nsr[s] = nsi[s] = 0;
	const bool polar = leg_wave_polar(a, wv, K);
	const bool alive_any = spin_init<K>(a, wv, lane, m, S, rn, rs, polar);
	double sg0 = 1.0;
	if (nl > 0 && __any(alive_any)) {
		const long row0 = PXS_UNIFORM_LONG(a.row[m]);
		const double4_t* __restrict__ coef = a.coef + row0;
		const double4_t* __restrict__ at = reinterpret_cast<const double4_t*>(a.almt + (long)bb*a.almt_bs) + row0;
		int j = 0;
		SPIN_SEEDED_PHASE_A
		j = PXS_UNIFORM_INT(j); coef = (const double4_t*)PXS_UNIFORM_LONG((long)coef);
		PXS_COUNT(0, (long)(nl - j)*K*12 + (a.seed_mode != 2 ? (long)j*K*4 : 0L));
		sg0 = ((l0 + j + m) & 1) ? -1.0 : 1.0;      // (-1)^(l+m) of the first accumulated step; pairs of steps keep the parity
		// phase B: plain fast steps; every 4 steps the chains below scale 0 are rescaled.  A lane's sums hold scaled-up
		// garbage until both of its chains are at scale 0, when they are reset (true terms before that: < 2^-340 of the result)
		while (j + 1 < nl) {
			bool pend = false;
#pragma unroll
			for (int s = 0; s < K; s++) pend |= (S.scp[s] < 0) || (S.scm[s] < 0);
			if (!__any(pend)) break;
			for (int it = 0; it < 2 && j + 1 < nl; it++, j += 2) {
				const double4_t f0 = LDC(coef, j), f1 = LDC(coef, j+1), a0 = LDC(at, j), a1 = LDC(at, j+1);
				SPIN_SYN_PAIR(f0, f1, a0, a1)
			}
#pragma unroll
			for (int s = 0; s < K; s++) {
				const bool was = (S.scp[s] < 0) || (S.scm[s] < 0);
				if (S.scp[s] < 0 && fabs(S.gp2[s]) > SC_BIG) { S.gp1[s] *= SC_SMALL; S.gp2[s] *= SC_SMALL; S.scp[s]++; }
				if (S.scm[s] < 0 && fabs(S.gm2[s]) > SC_BIG) { S.gm1[s] *= SC_SMALL; S.gm2[s] *= SC_SMALL; S.scm[s]++; }
				if (was && S.scp[s] == 0 && S.scm[s] == 0) pnr[s] = pni[s] = mnr[s] = mni[s] = qsr[s] = qsi[s] = nsr[s] = nsi[s] = 0;
			}
		}
#pragma unroll
		for (int s = 0; s < K; s++)
			if (S.scp[s] < 0 || S.scm[s] < 0) {      // never reached scale 0
				pnr[s] = pni[s] = mnr[s] = mni[s] = qsr[s] = qsi[s] = nsr[s] = nsi[s] = 0;
				S.gp1[s] = S.gp2[s] = S.gm1[s] = S.gm2[s] = 0;
			}
		// phase C: fast loop, the one-drain loop of leg_syn_s0 on the 32-byte rows (legendre_dev.hpp, "Row prefetch")
		double4_t a0, a1;
		SPIN_SYN_PHASE_C
		if (j < nl) {
#pragma unroll
			for (int s = 0; s < K; s++) {
				const double gp = S.gp2[s], gm = S.gm2[s];
				pnr[s] = fma(gp, a0.a, pnr[s]); pni[s] = fma(gp, a0.b, pni[s]);
				mnr[s] = fma(gm, a0.c, mnr[s]); mni[s] = fma(gm, a0.d, mni[s]);
				qsr[s] = fma(gm, a0.a, qsr[s]); qsi[s] = fma(gm, a0.b, qsi[s]);
				nsr[s] = fma(gp, a0.c, nsr[s]); nsi[s] = fma(gp, a0.d, nsi[s]);
			}
		}
	}
	// Q = (P+M)/2, U = -i (P-M)/2.  The ring indices are re-read here rather than kept in registers through the loops.
#pragma unroll
	for (int s = 0; s < K; s++) {
		const int p = leg_pair(a, wv, K, s, lane);
		const bool valid = leg_pair_valid(a, p);
		const int rn_ = valid ? a.ring_n[p] : -1, rs_ = valid ? a.ring_s[p] : -1;
		if (rn_ >= 0) {
			outq[rn_] = make_double2(0.5*(pnr[s] + mnr[s]), 0.5*(pni[s] + mni[s]));
			outu[rn_] = make_double2(0.5*(pni[s] - mni[s]), -0.5*(pnr[s] - mnr[s]));
		}
		if (rs_ >= 0) {
			const double psr = sg0*qsr[s], psi = sg0*qsi[s], msr = sg0*nsr[s], msi = sg0*nsi[s];
			outq[rs_] = make_double2(0.5*(psr + msr), 0.5*(psi + msi));
			outu[rs_] = make_double2(0.5*(psi - msi), -0.5*(psr - msr));
		}
	}
}

// two fast steps of the spin analysis; mu+ = G+ T+_N + sgn G- T+_S, mu- = G- T-_N + sgn G+ T-_S with the sign of the
// first step already folded into the south-ring data (even steps +, odd steps -)
#define SPIN_ANA_PAIR(f0, f1) { \
	double t0 = 0, t1 = 0, t2 = 0, t3 = 0, u0 = 0, u1 = 0, u2 = 0, u3 = 0; \
	{ \
		const double ca = f0.a, c1 = polar ? f0.c : f0.b, c2 = polar ? f0.d : -f0.b; \
		PXS_VCOPY(v1, c1); PXS_VCOPY(v2, c2); \
		_Pragma("unroll") for (int s = 0; s < K; s++) { \
			const double gp = S.gp2[s], gm = S.gm2[s]; \
			if (s >= SLO) { \
				t0 = fma(gp, tpnr[s], t0); t0 = fma(gm, tpsr[s], t0); \
				t1 = fma(gp, tpni[s], t1); t1 = fma(gm, tpsi[s], t1); \
				t2 = fma(gm, tmnr[s], t2); t2 = fma(gp, tmsr[s], t2); \
				t3 = fma(gm, tmni[s], t3); t3 = fma(gp, tmsi[s], t3); \
			} \
			S.gp1[s] = fma(fma(ca, S.x[s], v1), gp, -S.gp1[s]); S.gm1[s] = fma(fma(ca, S.x[s], v2), gm, -S.gm1[s]); \
		} \
	} \
	{ \
		const double ca = f1.a, c1 = polar ? f1.c : f1.b, c2 = polar ? f1.d : -f1.b; \
		PXS_VCOPY(v1, c1); PXS_VCOPY(v2, c2); \
		_Pragma("unroll") for (int s = 0; s < K; s++) { \
			const double gp = S.gp1[s], gm = S.gm1[s]; \
			if (s >= SLO) { \
				u0 = fma(gp, tpnr[s], u0); u0 = fma(-gm, tpsr[s], u0); \
				u1 = fma(gp, tpni[s], u1); u1 = fma(-gm, tpsi[s], u1); \
				u2 = fma(gm, tmnr[s], u2); u2 = fma(-gp, tmsr[s], u2); \
				u3 = fma(gm, tmni[s], u3); u3 = fma(-gp, tmsi[s], u3); \
			} \
			S.gp2[s] = fma(fma(ca, S.x[s], v1), gp, -S.gp2[s]); S.gm2[s] = fma(fma(ca, S.x[s], v2), gm, -S.gm2[s]); \
		} \
	} \
	/* steps come in aligned pairs: kk is even here */ \
	LEG_RED_PUT(kk, t0, t1, t2, t3) \
	LEG_RED_PUT(kk+1, u0, u1, u2, u3) \
	kk += 2; \
	if (kk == LEG_FSTEPS) { leg_flush(red, pout + 4*jbase, lane, LEG_FSTEPS, a.atomic); kk = 0; jbase = j+2; } }

// the two steps of SPIN_ANA_PAIR on the step coefficients themselves, (ca, c1, c2) = a and the additive constants of the G+ and the G- chain: the first step of a
// pair (south-ring sign +, sums into t0..t3), the second (sign -, sums into u0..u3)
#define SPIN_ANA_STEP0_C(ca, c1, c2) { \
	PXS_VCOPY(v1, c1); PXS_VCOPY(v2, c2); \
	_Pragma("unroll") for (int s = 0; s < K; s++) { \
		const double gp = S.gp2[s], gm = S.gm2[s]; \
		if (s >= SLO) { \
			t0 = fma(gp, tpnr[s], t0); t0 = fma(gm, tpsr[s], t0); \
			t1 = fma(gp, tpni[s], t1); t1 = fma(gm, tpsi[s], t1); \
			t2 = fma(gm, tmnr[s], t2); t2 = fma(gp, tmsr[s], t2); \
			t3 = fma(gm, tmni[s], t3); t3 = fma(gp, tmsi[s], t3); \
		} \
		S.gp1[s] = fma(fma(ca, S.x[s], v1), gp, -S.gp1[s]); S.gm1[s] = fma(fma(ca, S.x[s], v2), gm, -S.gm1[s]); \
	} }
#define SPIN_ANA_STEP1_C(ca, c1, c2) { \
	PXS_VCOPY(v1, c1); PXS_VCOPY(v2, c2); \
	_Pragma("unroll") for (int s = 0; s < K; s++) { \
		const double gp = S.gp1[s], gm = S.gm1[s]; \
		if (s >= SLO) { \
			u0 = fma(gp, tpnr[s], u0); u0 = fma(-gm, tpsr[s], u0); \
			u1 = fma(gp, tpni[s], u1); u1 = fma(-gm, tpsi[s], u1); \
			u2 = fma(gm, tmnr[s], u2); u2 = fma(-gp, tmsr[s], u2); \
			u3 = fma(gm, tmni[s], u3); u3 = fma(-gp, tmsi[s], u3); \
		} \
		S.gp2[s] = fma(fma(ca, S.x[s], v1), gp, -S.gp2[s]); S.gm2[s] = fma(fma(ca, S.x[s], v2), gm, -S.gm2[s]); \
	} }
// two fast steps of phase C from step jfirst on: the drain of the scalar rows between the two, the flush of a full tile and the request of the next rows (NEXT) at it
// (leg_ana_s0, S0_ANA_PAIR_D)
#define SPIN_ANA_PAIR_D(ca0, c10, c20, ca1, c11, c21, jfirst, NEXT) { \
	double t0 = 0, t1 = 0, t2 = 0, t3 = 0, u0 = 0, u1 = 0, u2 = 0, u3 = 0; \
	SPIN_ANA_STEP0_C(ca0, c10, c20) \
	_Pragma("unroll") for (int s = 0; s < K; s++) { PXS_DONE(S.gp1[s]); PXS_DONE(S.gm1[s]); } \
	PXS_DONE(t0); PXS_DONE(t1); PXS_DONE(t2); PXS_DONE(t3); \
	PXS_ROWS_DRAIN(); \
	if (kk == LEG_FSTEPS) { leg_flush(red, pout + 4*jbase, lane, LEG_FSTEPS, a.atomic); kk = 0; jbase = (jfirst); } \
	NEXT; \
	PXS_ROWS_ISSUED(); \
	SPIN_ANA_STEP1_C(ca1, c11, c21) \
	LEG_RED_PUT(kk, t0, t1, t2, t3) \
	LEG_RED_PUT(kk+1, u0, u1, u2, u3) \
	kk += 2; }
// Phases B and C of the spin analysis with NB started blocks (SLO = K - NB; leg_s0.hip, S0_ANA_STAGE; the synthesis keeps one loop for all blocks).  A block fetches its ring data when it
// starts (the lanes of it with both chains at scale 0; the others when they get there), until then it takes no part in the lane sums.
// phase B: plain fast steps; every 4 steps the chains below scale 0 are rescaled, and a lane of a started block whose two chains have both reached scale 0
// fetches its ring data (true terms before that: < 2^-340 of the result).
// phase C: the one-drain loop of leg_syn_s0 with the drain between the two steps of a pair and the flush of a full tile at that drain, as in leg_ana_s0, on the
// 32-byte rows (legendre_dev.hpp, "Row prefetch").  A row set spans the second step of a pair and the first of the next one (leg_ana_s0): at the top of a trip
// n.r1 is the row of step j, f the rows of steps j + 1, j + 2; a stage that ends there leaves them to the next.
#define SPIN_ANA_STAGE(NB) if constexpr ((NB) <= K) { if (nb == (NB)) { \
	constexpr int SLO = K - (NB); \
	bool more = false; \
	if (!inC) { \
	while (j + 1 < nl) { \
		if constexpr ((NB) < K) if (j < nl && SPIN_BLOCK_STARTS(SLO - 1)) { more = true; break; } \
		bool pend = false; \
		_Pragma("unroll") for (int s = 0; s < K; s++) pend |= (S.scp[s] < 0) || (S.scm[s] < 0); \
		if (!__any(pend)) break; \
		for (int it = 0; it < 2 && j + 1 < nl; it++, j += 2) { \
			const double4_t f0 = LDC(coef, j), f1 = LDC(coef, j+1); \
			SPIN_ANA_PAIR(f0, f1) \
		} \
		_Pragma("unroll") for (int s = 0; s < K; s++) { \
			const bool was = (S.scp[s] < 0) || (S.scm[s] < 0); \
			if (S.scp[s] < 0 && fabs(S.gp2[s]) > SC_BIG) { S.gp1[s] *= SC_SMALL; S.gp2[s] *= SC_SMALL; S.scp[s]++; } \
			if (S.scm[s] < 0 && fabs(S.gm2[s]) > SC_BIG) { S.gm1[s] *= SC_SMALL; S.gm2[s] *= SC_SMALL; S.scm[s]++; } \
			if (s >= SLO && was && S.scp[s] == 0 && S.scm[s] == 0) load_data(s); \
		} \
	} \
	if (!more) { \
		n = spin_rows(coef, j); f = spin_rows(coef, j+1); \
		PXS_ROWS_DRAIN(); \
		n.r1 = n.r0; \
		inC = 1; \
	} } \
	if (!more) { \
		for (;;) {      /* (two pairs per iteration on alternating row sets, see leg_syn_s0) */ \
			if constexpr ((NB) < K) if (j < nl && SPIN_BLOCK_STARTS(SLO - 1)) { more = true; break; } \
			if (!(j + 3 < nl)) break; \
			SPIN_ANA_PAIR_R(SPIN_ROW1(n), SPIN_ROW0(f), j, n = spin_rows(coef, j+3)) \
			SPIN_ANA_PAIR_R(SPIN_ROW1(f), SPIN_ROW0(n), j+2, f = spin_rows(coef, j+5)) \
			j += 4; \
		} \
	} \
	if (!more) { \
		slo = SLO; \
		nb = K + 1; \
	} else if constexpr ((NB) < K) { SPIN_BLOCK_BEGIN(SLO - 1) if (S.scp[SLO - 1] == 0 && S.scm[SLO - 1] == 0) load_data(SLO - 1); if constexpr ((NB) + 1 < K) { SPIN_NEXT_START(SLO - 2) } nb = (NB) + 1; } \
} }
// (the last steps, fewer than four, with the blocks from `slo` on started: one copy for all stages, leg_s0.hip, S0_ANA_TAIL)
#define SPIN_ANA_TAIL { const int SLO = slo; \
		if (j + 1 < nl) { \
			SPIN_ANA_PAIR_R(SPIN_ROW1(n), SPIN_ROW0(f), j, (void)0) \
			j += 2; \
		} \
		PXS_ROWS_DRAIN(); \
		if (kk == LEG_FSTEPS) { leg_flush(red, pout + 4*jbase, lane, LEG_FSTEPS, a.atomic); kk = 0; jbase = j; } \
		if (j < nl) { \
			double t0 = 0, t1 = 0, t2 = 0, t3 = 0; \
			_Pragma("unroll") for (int s = 0; s < K; s++) if (s >= SLO) { \
				const double gp = S.gp2[s], gm = S.gm2[s]; \
				t0 = fma(gp, tpnr[s], t0); t0 = fma(gm, tpsr[s], t0); \
				t1 = fma(gp, tpni[s], t1); t1 = fma(gm, tpsi[s], t1); \
				t2 = fma(gm, tmnr[s], t2); t2 = fma(gp, tmsr[s], t2); \
				t3 = fma(gm, tmni[s], t3); t3 = fma(gp, tmsi[s], t3); \
			} \
			LEG_RED_PUT(kk, t0, t1, t2, t3) \
			kk++; \
		} }

#define SPIN_ANA_PAIR_R(s0, s1, jfirst, NEXT) SPIN_ANA_PAIR_D(s0, s1, jfirst, NEXT)

// (K = 2 is asked to keep its 5 waves per SIMD: 96 VGPRs; left alone the one-drain loop takes 98 = 4 waves.  No scratch either way)
template<int K> __global__ __launch_bounds__(64, (K == 2 ? 5 : 1)) void leg_ana_spin(const LegK a)
{
	PXS_SHARED(double, red);
	const int lane = threadIdx.x; int wv, m, bb;
	if (!leg_block(a, wv, m, bb)) return;
	const int l0 = max(m, a.spin);
	const int nl = a.lmax - l0 + 1;
	if (nl <= 0) return;
	const long row0 = PXS_UNIFORM_LONG(a.row[m]);
	const double4_t* __restrict__ coef = a.coef + row0;
	double* __restrict__ pout = a.part + (long)bb*a.mom_bs + ((long)wv*a.rows_chunk + (row0 - a.rowbase))*4;
	const double2* __restrict__ inq = a.leg + (long)bb*a.leg_bs + (long)m*a.ld;
	const double2* __restrict__ inu = a.leg + (long)bb*a.leg_bs + ((long)a.nm + m)*a.ld;
	SpinState<K> S; int rn[K], rs[K];
	const bool polar = leg_wave_polar(a, wv, K);
	const bool alive_any = spin_init<K>(a, wv, lane, m, S, rn, rs, polar);
	if (!__any(alive_any)) return;
	// T+ = Q + iU, T- = Q - iU for north and south rings; the south values carry (-1)^(l+m) of the first accumulated
	// step (phase A advances in multiples of 4, so that is the sign at l0).  A lane whose chains are still below scale 0
	// keeps zero data until both get there (phase B), so that it can run the ungated steps.
	const double sgn0 = ((l0 + m) & 1) ? -1.0 : 1.0;
	double tpnr[K], tpni[K], tmnr[K], tmni[K], tpsr[K], tpsi[K], tmsr[K], tmsi[K];
	auto load_data = [&](int s) {
		// ring indices are re-read here rather than kept in registers through the loops (the kernel sits at the 256-VGPR line)
		const int p = leg_pair(a, wv, K, s, PXS_LATE_INT(lane));
		const bool valid = leg_pair_valid(a, p);
		const int rn_ = valid ? a.ring_n[p] : -1, rs_ = valid ? a.ring_s[p] : -1;
		double2 q = rn_ >= 0 ? inq[rn_] : make_double2(0, 0), u = rn_ >= 0 ? inu[rn_] : make_double2(0, 0);
		tpnr[s] = q.x - u.y; tpni[s] = q.y + u.x; tmnr[s] = q.x + u.y; tmni[s] = q.y - u.x;
		q = rs_ >= 0 ? inq[rs_] : make_double2(0, 0); u = rs_ >= 0 ? inu[rs_] : make_double2(0, 0);
		tpsr[s] = sgn0*(q.x - u.y); tpsi[s] = sgn0*(q.y + u.x); tmsr[s] = sgn0*(q.x + u.y); tmsi[s] = sgn0*(q.y - u.x);
	};
#pragma unroll
	for (int s = 0; s < K; s++) tpnr[s] = tpni[s] = tmnr[s] = tmni[s] = tpsr[s] = tpsi[s] = tmsr[s] = tmsi[s] = 0;
	int j = 0;
	SPIN_SEEDED_PHASE_A
	j = PXS_UNIFORM_INT(j); coef = (const double4_t*)PXS_UNIFORM_LONG((long)coef);
	// executed work: the recurrence FMAs of every block from here on (and of phase A where it ran), the accumulation FMAs of block K - 1, which starts with the
	// wave; the other blocks add theirs as they start (SPIN_BLOCK_BEGIN)
	constexpr int DIR = 1;
	PXS_COUNT2(DIR, (long)(nl - j)*K*4 + (a.seed_mode != 2 ? (long)j*K*4 : 0L), (long)(nl - j)*8, K);
	int knext = LEG_NEVER;      // seeded launches: the start step of the next block to start (the seed tail)
	if constexpr (K > 1) { SPIN_NEXT_START(K - 2) }
	if (lane == 0 && !a.atomic) a.first[wv*a.nmc + (m - a.m0)] = j + 1;      // rows before j are not written (reduce_partials skips them)
	// ring data of block K - 1: the lanes whose chains start at scale 0 or both reached it during phase A
	if (S.scp[K - 1] == 0 && S.scm[K - 1] == 0) load_data(K - 1);
	int kk = 0, jbase = j;
	// phases B and C, by number of started blocks (SPIN_ANA_STAGE)
	spin_rows_t n, f;
	int nb = 1, inC = 0, slo = 0;
	SPIN_ANA_STAGE(1) SPIN_ANA_STAGE(2) SPIN_ANA_STAGE(3) SPIN_ANA_STAGE(4) SPIN_ANA_STAGE(5) SPIN_ANA_STAGE(6)
	static_assert(K <= 6, "leg_ana_spin: one SPIN_ANA_STAGE per block");
	SPIN_ANA_TAIL
	if (kk > 0) leg_flush(red, pout + 4*jbase, lane, kk, a.atomic);
}


// ---- batched spin-s analysis as an FP64-MFMA GEMM (round 5) -----------------------------------------------------------------------
// Stacks of T/Q/U maps (Monte-Carlo polarisation sims): the Q/U pairs of 4 or more maps in one call.  Per m
//   mu+[l][map] = sum_ring G+_l T+_N + sgn_l G-_l T+_S,   mu-[l][map] = sum_ring G-_l T-_N + sgn_l G+_l T-_S,   sgn_l = (-1)^(l + m)
// (leg_ana_spin) with the SAME G+ / G- for every map.  One chain per HALF-WAVE: lanes 0-31 of a wave run G+ of 32 ring pairs, lanes 32-63 G- of the
// same pairs, and the G- lanes park sgn_l G-.  With B = (T+_N re, im, T-_S re, im) on the G+ slots and (T+_S re, im, T-_N re, im) on the G- slots ONE
// GEMM over the 64 slots gives (mu+, sgn_l mu-): the sign of the last two columns is a function of the row and is applied at the flush.  That makes the
// kernel the shape of leg_ana_s0_mm -- one P tile per wave, 8 waves over 256 ring pairs, 8 maps per workgroup, four waves per SIMD.  (First form: both
// chains in every lane, two P tiles per wave, two accumulators: the LDS held two waves per SIMD and the f64 MFMA, which needs several issuing waves for
// its rate, ran the Q/U analysis of 16 maps in 111 ms against the VALU kernel's 123.)
// one chain of leg_ana_spin's pair of recurrences: G_{l+1} = (a x + c) G_l - G_{l-1}, c = +-b (polar waves: a +- b with x = -2 sin^2(theta / 2))
struct SpinChain {
	double x, g1, g2, sgl, pa; int sc, half, par;      // half: 0 the G+ chain, 1 the G- chain; par: l0 + m
	// coefficient of a step from the row (a, b): a x + (polar ? a : 0) +- b
	__device__ __forceinline__ double coef(double ca, double cb) const { return fma(ca, x, fma(sgl, cb, pa*ca)); }
	__device__ __forceinline__ double step(double ca, double cb) { const double p = g2, nx = fma(coef(ca, cb), g2, -g1); g1 = p; g2 = nx; return p; }
	__device__ __forceinline__ void rescale() { if (fabs(g2) > SC_BIG) { g1 *= SC_SMALL; g2 *= SC_SMALL; sc++; } }
	// the G- lanes park sgn_l G-: the sign of the first of the four rows from step kq on, alternating
	__device__ __forceinline__ void park_sign(int kq, double* p) const {
		const double se = (half && ((par + kq) & 1)) ? -1.0 : 1.0, so = half ? -se : 1.0;
		p[0] *= se; p[1] *= so; p[2] *= se; p[3] *= so;
	}
};
// the spin-s side of leg_ana_mm / leg_syn_mm (legendre_dev.hpp): one chain per half-wave, 32 ring pairs per wave; the polar form is folded into the chain (SpinChain::coef)
struct SpinMm {
	typedef SpinChain Chain;
	static constexpr int SLOTS = 32;
	static constexpr bool SIGNED = true;
	static constexpr bool BREG_SYNC = false;      // (the spin-0 analysis has one: kept as it was, kernel by kernel)
	static __device__ __forceinline__ int steps(const LegK& a, int m, int& par) { const int l0 = max(m, a.spin); par = l0 + m; return a.lmax - l0 + 1; }
	static __device__ __forceinline__ bool init(const LegK& a, int p, int m, int half, bool polar, SpinChain& C) {
		const int s_ = a.spin;
		const bool valid = p < a.npairs;
		const double cth = valid ? a.cth[p] : 0.0, sth = valid ? a.sth[p] : 0.0, shh = valid ? a.sh2[p] : 0.0;
		C.x = polar ? -2.0*shh*shh : cth; C.sgl = half ? -1.0 : 1.0; C.pa = polar ? 1.0 : 0.0; C.half = half; C.par = max(m, s_) + m;
		const double t1 = a.lmax*sth + a.ofs, b = -2.0*s_*fabs(cth), c = (double)s_*s_ - t1*t1, discr = b*b - 4*c;      // (libsharp's m-limit generalised to spin, as spin_init)
		const double mlim = discr <= 0 ? a.lmax : fmin((double)a.lmax, 0.5*(-b + sqrt(discr)));
		const bool alive = valid && ((double)m <= mlim + 0.5);
		C.g1 = 0; C.g2 = 0; C.sc = 0;
		if (alive) {
			const double sh = shh, ch = a.ch2[p];
			double m1, m2; int e1, e2;
			// exponents of sin(theta/2), cos(theta/2) of the start value: G+ (m + s, m - s) / G- (m - s, m + s) for m >= s, (s + m, s - m) / (s - m, s + m) below
			const int es = m >= s_ ? (half ? m - s_ : m + s_) : (half ? s_ - m : s_ + m), ec = m >= s_ ? (half ? m + s_ : m - s_) : (half ? s_ + m : s_ - m);
			pow_scaled(sh, es, m1, e1); pow_scaled(ch, ec, m2, e2);
			double mt = m1*m2; int e = e1 + e2 + (m >= s_ ? m : 0); frexp_norm(mt, e); to_scaled(mt, e, C.g2, C.sc);
			if (m < s_ && half && ((s_ - m) & 1)) C.g2 = -C.g2;
		}
		return alive;
	}
	static __device__ __forceinline__ const double* table(const LegK& a, bool, long row0) { return reinterpret_cast<const double*>(a.coef2) + 2*row0; }
	// phase A on the compact table: recurrence only until the first lane of the wave is live (LEG_LIVE); returns the step reached
	static __device__ __forceinline__ int phase_a(const LegK& a, SpinChain& C, long row0, bool polar, int n) {
		const double* __restrict__ tab = table(a, polar, row0);
		int k = 0;
		while (k + 4 <= n) {
			if (__any(LEG_IS_LIVE(C.g2, C.sc))) break;
			double cq[8];
#pragma unroll
			for (int i = 0; i < 8; i++) cq[i] = LDCD(tab, 2L*k + i);
#pragma unroll
			for (int i = 0; i < 4; i++) C.step(cq[2*i], cq[2*i + 1]);
			if (C.sc < 0) C.rescale();
			k += 4;
		}
		return k;
	}
	// analysis prologue: Q and U of the north and south rings of the slot's pair in the 4 maps from map0 on, parked per map as (T+_N re, im, T-_S re, im) on the G+
	// slots and (T+_S re, im, T-_N re, im) on the G- slots; T+ = Q + iU, T- = Q - iU
	struct Data { double2 qn[4], un[4], qs[4], us[4]; };
	static __device__ __forceinline__ void load(const LegK& a, int m, int map0, int rn, int rs, Data& d) {
#pragma unroll
		for (int mm = 0; mm < 4; mm++) {
			const int map = map0 + mm;
			const double2* __restrict__ inq = a.leg + (long)map*a.leg_bs + (long)m*a.ld;
			const double2* __restrict__ inu = a.leg + (long)map*a.leg_bs + ((long)a.nm + m)*a.ld;
			const bool okm = map < a.nmaps;
			d.qn[mm] = (okm && rn >= 0) ? inq[rn] : make_double2(0, 0); d.un[mm] = (okm && rn >= 0) ? inu[rn] : make_double2(0, 0);
			d.qs[mm] = (okm && rs >= 0) ? inq[rs] : make_double2(0, 0); d.us[mm] = (okm && rs >= 0) ? inu[rs] : make_double2(0, 0);
		}
	}
	static __device__ __forceinline__ void park(const Data& d, double, int half, double* __restrict__ ent) {
#pragma unroll
		for (int mm = 0; mm < 4; mm++) {
			const double tpn_r = d.qn[mm].x - d.un[mm].y, tpn_i = d.qn[mm].y + d.un[mm].x, tmn_r = d.qn[mm].x + d.un[mm].y, tmn_i = d.qn[mm].y - d.un[mm].x;
			const double tps_r = d.qs[mm].x - d.us[mm].y, tps_i = d.qs[mm].y + d.us[mm].x, tms_r = d.qs[mm].x + d.us[mm].y, tms_i = d.qs[mm].y - d.us[mm].x;
			ent[4*mm + 0] = half ? tps_r : tpn_r; ent[4*mm + 1] = half ? tps_i : tpn_i;
			ent[4*mm + 2] = half ? tmn_r : tms_r; ent[4*mm + 3] = half ? tmn_i : tms_i;
		}
	}
	// synthesis epilogue.  Register r of acc[g][rb] at lane (i4 = lane / 16, jc = lane % 16): slot 16 rb + 4 r + i4 (rb < 2: G+ of ring pair 16 rb + 4 r + i4, rb >= 2: G- of pair
	// 16 (rb - 2) + 4 r + i4), column 4 (map in the group) + c.  G+ rows: c = 0, 1: P re / im (north); 2, 3: M' re / im (south).  G- rows: c = 0, 1: P' re / im
	// (south); 2, 3: M re / im (north).  Q = (P + M) / 2, U = -i (P - M) / 2: lanes c < 2 write the north ring, lanes c >= 2 the south ring; even c the
	// real part of Q and the imaginary part of U, odd c the other two.
	template<int NG> static __device__ __forceinline__ void store(const LegK& a, int m, int bb, int pbase, int lane, mm_acc (&acc)[NG][4]) {
		const int c = lane & 3;
#pragma unroll
		for (int g = 0; g < NG; g++) {
			const int map = (bb*NG + g)*4 + ((lane & 15) >> 2);
			double* __restrict__ outq = reinterpret_cast<double*>(a.leg + (long)(map < a.nmaps ? map : 0)*a.leg_bs + (long)m*a.ld);
			double* __restrict__ outu = reinterpret_cast<double*>(a.leg + (long)(map < a.nmaps ? map : 0)*a.leg_bs + ((long)a.nm + m)*a.ld);
#pragma unroll
			for (int rb = 0; rb < 2; rb++)
#pragma unroll
				for (int r = 0; r < 4; r++) {
					const int p = pbase + 16*rb + 4*r + (lane >> 4);
					const bool valid = p < a.npairs && map < a.nmaps;
					const double own = acc[g][rb][r], oth = MMS_XOR2(acc[g][rb + 2][r]);
					const double P = c < 2 ? own : oth, M = c < 2 ? oth : own;
					const double sum = 0.5*(P + M), dif = 0.5*(P - M);
					const int ring = valid ? (c < 2 ? a.ring_n[p] : a.ring_s[p]) : -1;
					if (ring >= 0) {
						if (c & 1) { outq[2*ring + 1] = sum; outu[2*ring] = dif; }
						else       { outq[2*ring] = sum; outu[2*ring + 1] = -dif; }
					}
				}
		}
	}
};
template<int NG, int W> __global__ __launch_bounds__(64*W, 4) void leg_ana_spin_mm(const LegK a) { leg_ana_mm<SpinMm, NG, W>(a); }

// ---- batched spin-s synthesis as an FP64-MFMA GEMM (round 5) ----------------------------------------------------------------------
// The transpose of leg_ana_spin_mm (cf. leg_syn_spin): north  P = sum_l G+ a+, M = sum_l G- a-;  south  P' = sum_l sgn_l G- a+, M' = sum_l sgn_l G+ a-.
// One chain per half-wave as in the analysis: the 64 rows of a wave's accumulators are the G+ slots of 32 ring pairs (row blocks 0, 1) and their
// G- slots (row blocks 2, 3); the G- lanes park sgn_l G-, and with B = (a+, sgn_l a-) -- ONE B for all rows -- the G+ rows come out as (P, M') and the G-
// rows as (P', M).  The shape of leg_syn_s0_mm: one P tile, 4 x 8 accumulator VGPRs per group of 4 maps, one wave per workgroup, no cross-wave step.
template<int NG> __global__ __launch_bounds__(64, 4) void leg_syn_spin_mm(const LegK a) { leg_syn_mm<SpinMm, NG>(a); }

// ---- launches: the kernel of (direction, form, K or ng); the ring pairs per lane the host's rules select are 3 and 2 (synthesis), 6, 4, 3 and 2 (analysis) ----
void launch_leg_spin(bool analysis, int ng, int K, dim3 grid, hipStream_t st, const LegK& a) {
	static const bool once = leg_mm_lds_optin({leg_ana_spin_mm<2, MM_WAVES>, leg_ana_spin_mm<1, MM_WAVES>}); (void)once;
	// (a K without a compiled kernel is an error, not another kernel: the grid, the seeds and the partial moments were laid out for the K asked for)
	const LegKernel k = analysis ? (ng == 2 ? leg_ana_spin_mm<2, MM_WAVES> : ng ? leg_ana_spin_mm<1, MM_WAVES> : K == 6 ? leg_ana_spin<6> : K == 4 ? leg_ana_spin<4> : K == 3 ? leg_ana_spin<3> : K == 2 ? leg_ana_spin<2> : nullptr)
	                             : (ng == 2 ? leg_syn_spin_mm<2> : ng ? leg_syn_spin_mm<1> : K == 3 ? leg_syn_spin<3> : K == 2 ? leg_syn_spin<2> : nullptr);
	PXS_REQUIRE(k != nullptr, "internal: no spin-s Legendre kernel compiled for this number of ring pairs per lane");
	leg_launch(k, analysis, ng, grid, st, a);
}

} // namespace pxs
