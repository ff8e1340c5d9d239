// Compile-time-planned LDS sub-transforms of the chain kernels (fftchain.hip).
//
// lds_fft (fft_dev.hpp) interprets a pass table at run time: a switch on the radix per pass, two fdiv per butterfly, a run-time
// stride L (so no LDS access can carry an immediate offset) and run-time twiddle strides.  For the lengths a plan is known to use
// the whole plan is a type, StaticFft<N, R0, R1, ...>, in the manner of RfSeq in regfft_dev.hpp: radices, strides, twiddle steps
// and the digit-reversal permutation are constants, the loops have constant trip counts, and every LDS access of a butterfly is
// one per-thread base plus immediates.  The arithmetic of a butterfly is the same code as in the run-time passes (butterfly<R>,
// butterfly_comp<A, B>, cmul with the same W_n table), so the two paths agree to the compiler's reassociation.
//
// The radix sequence of a StaticFft must be the one FftContext::sub plans for (n, maxr) -- same radices, same order -- because
// the kernels share its W_n table and the host checks the two against each other (FftChain::static_check).
#pragma once
#include "fft_dev.hpp"

namespace pxs {

// x / D for 0 <= x < 4096 by one full-rate 24-bit multiply and a shift (the compiler's own constant division, and fdiv, take the
// quarter-rate v_mul_hi_u32).  M = floor(2^s / D) + 1 with s = 13 + ceil(log2 D): M D = 2^s + e, 0 < e <= D, so
// x M / 2^s = x/D + x e / (D 2^s) and x e <= 4096 D <= 2^(s-1) keeps the excess below 1/D: the floor is exact.  x M < 2^27.
static constexpr int SDIV_MAX = 4096;
constexpr int sdiv_shift(int D) { int s = 13; while ((1 << (s - 13)) < D) s++; return s; }
template<int D> __device__ __forceinline__ uint32_t sdiv(uint32_t x) {
	if constexpr (D <= 1) return x;
	else if constexpr ((D & (D - 1)) == 0) return x / (uint32_t)D;
	else {
		constexpr int s = sdiv_shift(D);
		constexpr uint32_t M = (1u << s)/D + 1;
#ifdef PXS_HOST_SIM
		return (x*M) >> s;
#else
		return __umul24(x, M) >> s;
#endif
	}
}

template<int N, int... Rs> struct StaticFft {
	static constexpr int n = N, ns = N | 1, nfac = (int)sizeof...(Rs);
	static_assert(N >= 2 && (Rs * ... * 1) == N, "StaticFft: the radices do not multiply to N");
	static constexpr int radix(int p) { constexpr int r[] = {Rs...}; return r[p]; }
	static constexpr int L(int p) { int l = 1; for (int i = 0; i < p; i++) l *= radix(i); return l; }      // butterfly stride of pass p
	static constexpr int tws(int p) { return N/(L(p)*radix(p)); }                                            // twiddle stride of pass p
	// slot of input j (digit reversal; the loop of FftContext::sub)
	static constexpr int perm_host(int j) {
		int t = j, pos = 0;
		for (int p = nfac - 1; p >= 0; p--) { const int i = t % radix(p); t /= radix(p); pos += i*L(p); }
		return pos;
	}
	template<int P = nfac - 1> static __device__ __forceinline__ uint32_t perm(uint32_t t) {
		if constexpr (P == 0) return t;
		else { const uint32_t q = sdiv<radix(P)>(t); return (t - q*radix(P))*L(P) + perm<P - 1>(q); }
	}
};
// the absent second transform of a one-transform stage
struct NoFft {
	static constexpr int n = 0, ns = 1, nfac = 0;
	static constexpr int radix(int) { return 1; }
	static constexpr int perm_host(int j) { return j; }
	template<int P = 0> static __device__ __forceinline__ uint32_t perm(uint32_t t) { return t; }
};

// one pass of F on T lines: butterfly b < T n/R is (line t, block blk, offset q), its points are buf[p0 + i L]
template<class F, int P, int NT, int T> __device__ __forceinline__ void static_pass(double2* buf, const double2* tw) {
	constexpr int R = F::radix(P), L = F::L(P), TWS = F::tws(P), nb = F::n/R, total = T*nb, iters = (total + NT - 1)/NT;
	static_assert(iters*NT <= SDIV_MAX, "static_pass: index range of sdiv");
	static_assert(R == 2 || R == 3 || R == 4 || R == 5 || R == 6 || R == 7 || R == 8 || R == 9, "static_pass: radix not compiled in");
#pragma unroll
	for (int it = 0; it < iters; it++) {
		const uint32_t b = threadIdx.x + it*NT;
		if (total % NT == 0 || b < (uint32_t)total) {
			const uint32_t t = sdiv<nb>(b), bb = b - t*nb, blk = sdiv<L>(bb), q = bb - blk*L;
			double2* p = buf + (t*F::ns + bb + blk*(L*(R - 1)));      // = t ns + blk L R + q
			double2 v[R];
#pragma unroll
			for (int i = 0; i < R; i++) v[i] = p[i*L];
			if constexpr (L > 1) {
				const uint32_t step = q*TWS;
#pragma unroll
				for (int i = 1; i < R; i++) v[i] = cmul(v[i], tw[i*step]);
			}
			if constexpr (R == 6 || R == 8 || R == 9) {
				constexpr int A = R == 8 ? 4 : 3, B = R == 9 ? 3 : 2;
				butterfly_comp<A, B>(v);
#pragma unroll
				for (int k = 0; k < R; k++) p[k*L] = v[B*(k % A) + k/A];
			} else {
				butterfly<R>(v);
#pragma unroll
				for (int i = 0; i < R; i++) p[i*L] = v[i];
			}
		}
	}
	PXS_LDS_BARRIER();
}

// all passes of F on T lines; ends with a barrier (as lds_fft does)
template<class F, int NT, int T, int P = 0> __device__ __forceinline__ void lds_fft_static(double2* buf, const double2* tw) {
	if constexpr (P < F::nfac) { static_pass<F, P, NT, T>(buf, tw); lds_fft_static<F, NT, T, P + 1>(buf, tw); }
}

} // namespace pxs
