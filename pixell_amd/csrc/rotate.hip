// Euler-angle rotation of alm on the GPU: curvedsky.rotate_alm (pixell/curvedsky.py:717-740 of the reference, which calls
// ducc0.sht.rotate_alm per component).  Active rotation f'(n) = f(R^-1 n), R = R_z(phi) R_y(theta) R_z(psi):
//
//     a'_lm = sum_m' e^{-im phi} d^l_mm'(theta) e^{-im' psi} a_lm',   d^l_mm'(theta) = i^{m-m'} sum_k D_km D_km' e^{-ik theta}
//
// with D = d^l(pi/2) (R_y(theta) = X^-1 R_z(theta) X, X = R_x(pi/2) = R_z(-pi/2) R_y(pi/2) R_z(pi/2)).  Written as two passes of one
// real contraction, out_m = Pout(m) sum_{k=-l..l} D_mk Pin(k) x_k, over alm of real fields (m >= 0 stored, x_{-k} = (-1)^k conj(x_k)):
//   pass 1: x = a, Pin(k) = e^{-ik psi} i^-k,                Pout(m) = i^m
//   pass 2: x = b, Pin(k) = e^{-ik theta} i^-k (-1)^k,       Pout(m) = e^{-im phi} i^m (-1)^m
// (D_km = (-1)^{m-k} D_mk folds the transpose of the second pass into its phases).  With D_{m,-k} = (-1)^{l+m} D_mk and
// Pin(-k) = conj(Pin(k)), the terms k and -k add to D_mk (y_k + (-1)^{l+m+k} conj(y_k)), y = Pin x: twice the real part of y_k where
// l+m+k is even, 2i times its imaginary part where it is odd.  So a row m needs ONE real FMA per column k and component: U_k = w_k Re y_k
// on the columns of its parity, V_k = w_k Im y_k on the others (w_0 = 1, w_k = 2).  Derivation and checks: DESIGN.md section 8.
//
// D rows are generated, never stored: one lane owns one row m of one l and walks the column k from l down to 0 with the three-term
// recurrence of d^l(pi/2) in its column index (Trapani & Navaza 2006)
//     D_{m,k-1} = -2m D_mk / sqrt((l+k)(l-k+1)) - sqrt((l-k)(l+k+1)/((l+k)(l-k+1))) D_{m,k+1},
// started from the closed form D_ml = 2^-l sqrt(C(2l, l+m)) (the square root of a binomial probability, evaluated without
// cancellation by Loader's saddle-point form) in an extended exponent (legendre_dev.hpp to_scaled).  A lane accumulates only once its
// scale is 0: before that its entries are below 2^-400 (the forbidden region k^2 + m^2 > l(l+1), where the recurrence grows).
//
// Layout of the work: the input is turned once into an l-major table x[l(l+1)/2 + k][c] of (U, V) with Pin and w applied, next to the
// recurrence coefficients coef[l(l+1)/2 + k] = (-2/sqrt((l+k)(l-k+1)), sqrt((l-k)(l+k+1)/((l+k)(l-k+1)))).  Both are the same for every
// lane of a wave (one l per wave) and are read through the constant address space (scalar loads), so a step costs a lane 3 + NC VALU
// operations and no LDS traffic.  A workgroup of 4 waves owns 256 consecutive rows of one l; waves 0/2 take the even rows, 1/3 the odd
// ones, so that which of U or V a column contributes is the same across a wave.  Workgroups are issued from the largest l down.
#include "../../include/pxsht.h"
#include "legendre_dev.hpp"

namespace pxs {

#ifdef PXS_HOST_SIM
#define RLD(p, i) ((p)[i])
#else
typedef double rot_d2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ double2 rot_ldc(const double2* p, long i) {
	const __attribute__((address_space(4))) rot_d2* c = (const __attribute__((address_space(4))) rot_d2*)(unsigned long long)p;
	const rot_d2 v = c[i]; return make_double2(v.x, v.y);
}
#define RLD(p, i) rot_ldc((p), (i))
#endif

static constexpr int ROT_ROWS = 256;      // rows of one l per workgroup (4 waves)

struct RotK {
	int lmax;
	const void* in; long in_cstride; int in_dtype;         // prep / phase kernels: user alm, triangular m-major
	void* out; long out_cstride; int out_dtype;
	const double2* coef;                                   // [nalm] (A, B)
	const double2* x;                                      // [nalm][NC] (U, V) of the pass
	double2* y;                                            // pass 1: [nalm][NC] (U, V) of pass 2
	double ang_in, ang_out;                                // angle of Pin / Pout of the kernel
};

__device__ __forceinline__ long rot_tri(int lmax, int l, int m) { return (long)m*(2*lmax + 1 - m)/2 + l; }
__device__ __forceinline__ long rot_lmaj(int l, int k) { return (long)l*(l + 1)/2 + k; }

// e^{-i n a}: n a is formed exactly as hi + lo (fma), so the phase keeps full precision for n up to lmax
__device__ __forceinline__ double2 rot_phase(int n, double a) {
	const double t = (double)n*a, e = fma((double)n, a, -t);
	double s, c; sincos(t, &s, &c);
	return make_double2(c - s*e, -(s + c*e));
}
__device__ __forceinline__ double2 cmul(double2 a, double2 b) { return make_double2(a.x*b.x - a.y*b.y, a.x*b.y + a.y*b.x); }
__device__ __forceinline__ double2 mul_ipow(double2 a, int n) {      // a * i^n
	switch (n & 3) { case 0: return a; case 1: return make_double2(-a.y, a.x); case 2: return make_double2(-a.x, -a.y); default: return make_double2(a.y, -a.x); }
}
__device__ __forceinline__ double2 rot_ld(const void* p, int dtype, long i) {
	if (dtype == PX_C64) { const float2 v = ((const float2*)p)[i]; return make_double2(v.x, v.y); }
	return ((const double2*)p)[i];
}
__device__ __forceinline__ void rot_st(void* p, int dtype, long i, double2 v) {
	if (dtype == PX_C64) ((float2*)p)[i] = make_float2((float)v.x, (float)v.y);
	else ((double2*)p)[i] = v;
}

// ln of the binomial probability C(n, x) 2^-n by Loader's saddle-point form (stirlerr, bd0): no cancellation between large logarithms,
// relative error of the probability ~1e-13 at n = 2 10^4 (against 3e-11 through lgamma differences)
__device__ __forceinline__ double rot_stirlerr(double n) {
	const double S0 = 1.0/12, S1 = 1.0/360, S2 = 1.0/1260, S3 = 1.0/1680, S4 = 1.0/1188;
	if (n <= 15) return lgamma(n + 1) - (n + 0.5)*log(n) + n - 0.918938533204672741780329736406;
	const double nn = n*n;
	if (n > 500) return (S0 - S1/nn)/n;
	if (n > 80) return (S0 - (S1 - S2/nn)/nn)/n;
	if (n > 35) return (S0 - (S1 - (S2 - S3/nn)/nn)/nn)/n;
	return (S0 - (S1 - (S2 - (S3 - S4/nn)/nn)/nn)/nn)/n;
}
__device__ __forceinline__ double rot_bd0(double x, double M) {      // x log(x/M) + M - x
	if (fabs(x - M) < 0.1*(x + M)) {
		double v = (x - M)/(x + M), s = (x - M)*v, ej = 2*x*v;
		v *= v;
		for (int j = 1; j < 200; j++) {
			ej *= v;
			const double s1 = s + ej/(2*j + 1);
			if (s1 == s) break;
			s = s1;
		}
		return s;
	}
	return x*log(x/M) + M - x;
}
// D^l_{m,l} = 2^-l sqrt(C(2l, l+m)) (0 <= m <= l) as v 2^(800 scale)
__device__ __forceinline__ void rot_start(int l, int m, double& v, int& scale) {
	if (m == l) { to_scaled(1.0, -l, v, scale); return; }
	const double n = 2.0*l, x = l + m, y = l - m;
	const double lp = rot_stirlerr(n) - rot_stirlerr(x) - rot_stirlerr(y) - rot_bd0(x, l) - rot_bd0(y, l) + 0.5*log(n/(6.283185307179586476925*x*y));
	const double h = 0.5*lp;                                     // ln D
	const double LN2_HI = 6.93147180369123816490e-01, LN2_LO = 1.90821492927058770002e-10;   // (LN2_HI has 32 significant bits)
	const int e = (int)floor(h*1.4426950408889634);
	const double r = (h - e*LN2_HI) - e*LN2_LO;                   // (e LN2_HI exact for |e| < 2^21)
	to_scaled(exp(r), e, v, scale);
}

// prep: user alm (m-major) -> x[l-major][c] = (U, V) of pass 1, and the coefficient table.  Threads run along l (coalesced reads).
template<int NC>
__global__ __launch_bounds__(256) void rot_prep_kernel(RotK p, double2* __restrict__ coef, double2* __restrict__ x)
{
	const int l = blockIdx.x*blockDim.x + threadIdx.x, k = blockIdx.y;
	if (l > p.lmax || l < k) return;
	const long j = rot_lmaj(l, k);
	const double2 ph = mul_ipow(rot_phase(k, p.ang_in), -k);
	const double w = k == 0 ? 1.0 : 2.0;
	for (int c = 0; c < NC; c++) {
		const double2 y = cmul(ph, rot_ld(p.in, p.in_dtype, c*p.in_cstride + rot_tri(p.lmax, l, k)));
		x[j*NC + c] = make_double2(w*y.x, w*y.y);
	}
	if (coef) {
		double A = 0, B = 0;
		if (k > 0) { A = -2/sqrt((double)(l + k)*(l - k + 1)); B = sqrt((double)(l - k)*(l + k + 1)/((double)(l + k)*(l - k + 1))); }
		coef[j] = make_double2(A, B);
	}
}

// workgroups per l (256 rows each) summed over l = 0..L
__device__ __forceinline__ long rot_nblk_upto(long L) {
	if (L < 0) return 0;
	const long q = L/ROT_ROWS, r = L%ROT_ROWS;
	return (L + 1) + ROT_ROWS*q*(q - 1)/2 + q*(r + 1);
}

template<int NC, int Q, bool RE, int MODE>      // MODE 0: recurrence only, 1: accumulate where the lane's scale is 0, 2: accumulate
__device__ __forceinline__ void rot_step(const double2* __restrict__ cf, const double2* __restrict__ xs, int k, double md, int sc,
		double& v0, double& v1, double* re, double* im)
{
	const double2 ab = RLD(cf, k);
	if (MODE > 0) {
		const double d = (MODE == 2 || sc == 0) ? v0 : 0.0;
		for (int c = 0; c < NC; c++) {
			const double2 u = RLD(xs, (long)k*NC + c);
			if (RE) re[c] = fma(d, u.x, re[c]); else im[c] = fma(d, u.y, im[c]);
		}
	}
	const double vn = fma(md*ab.x, v0, -(ab.y*v1));
	v1 = v0; v0 = vn;
}

// the rows of one wave: m = m0 + 2 lane (Q = parity of m0).  Column k contributes U to the real part where l - k is even (Q = 0) / odd
// (Q = 1), V to the imaginary part otherwise.
template<int NC, int Q>
__device__ __forceinline__ void rot_rows(int l, int m, bool act, const double2* __restrict__ cf, const double2* __restrict__ xs,
		double* re, double* im)
{
	const double md = act ? (double)m : 0.0;
	double v0 = 0, v1 = 0; int sc = 0;
	if (act) rot_start(l, m, v0, sc);
	for (int c = 0; c < NC; c++) { re[c] = 0; im[c] = 0; }
	int k = l;
	// phase A: some lane of the wave is still below scale 0; groups of 8 steps, then the rescale (a step grows a row by at most
	// sqrt(2l) < 2^8: 8 steps cannot carry |v| from 2^400 past the double range)
	while (k >= 0 && !__all(sc == 0)) {
		const bool any = __any(sc == 0);
		for (int s = 0; s < 8 && k >= 0; s++, k--) {
			const bool re_col = ((l - k + Q) & 1) == 0;
			if (any) {
				if (re_col) rot_step<NC, Q, true, 1>(cf, xs, k, md, sc, v0, v1, re, im);
				else rot_step<NC, Q, false, 1>(cf, xs, k, md, sc, v0, v1, re, im);
			} else rot_step<NC, Q, true, 0>(cf, xs, k, md, sc, v0, v1, re, im);
		}
		if (sc < 0 && fmax(fabs(v0), fabs(v1)) > SC_BIG) { v0 *= SC_SMALL; v1 *= SC_SMALL; sc++; }
	}
	// phase B: every lane at scale 0
	if (k >= 0 && ((l - k + Q) & 1)) { rot_step<NC, Q, false, 2>(cf, xs, k, md, sc, v0, v1, re, im); k--; }
	for (; k >= 1; k -= 2) {
		rot_step<NC, Q, true, 2>(cf, xs, k, md, sc, v0, v1, re, im);
		rot_step<NC, Q, false, 2>(cf, xs, k - 1, md, sc, v0, v1, re, im);
	}
	if (k == 0) rot_step<NC, Q, true, 2>(cf, xs, 0, md, sc, v0, v1, re, im);
}

// FINAL = 0 (pass 1): out_m = i^m (re + i im), stored l-major as the (U, V) of pass 2 (Pin = e^{-im theta} i^-m (-1)^m, w).
// FINAL = 1 (pass 2): out_m = e^{-im phi} i^m (-1)^m (re + i im), stored into the user's alm (m-major).
template<int NC, int FINAL>
__global__ __launch_bounds__(256) void rot_pass_kernel(RotK p, long nblk)
{
	const long b = blockIdx.x;
	const long total = rot_nblk_upto(p.lmax);
	// the l of this workgroup: blocks run from l = lmax down; blocks above l are total - rot_nblk_upto(l)
	int lo = 0, hi = p.lmax;
	while (lo < hi) { const int mid = (lo + hi)/2; if (total - rot_nblk_upto(mid) <= b) hi = mid; else lo = mid + 1; }
	const int l = lo;
	const int rb = (int)(b - (total - rot_nblk_upto(l)));
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const int q = wave & 1;
	const int m = rb*ROT_ROWS + 128*(wave >> 1) + 2*lane + q;
	if (rb*ROT_ROWS + 128*(wave >> 1) + q > l) return;           // the whole wave is past m = l
	const bool act = m <= l;
	const long base = rot_lmaj(l, 0);
	const double2* cf = p.coef + base;
	const double2* xs = p.x + base*NC;
	double re[NC], im[NC];
	if (q) rot_rows<NC, 1>(l, m, act, cf, xs, re, im);
	else rot_rows<NC, 0>(l, m, act, cf, xs, re, im);
	if (!act) return;
	if (!FINAL) {
		// i^m (re + i im) e^{-im theta} i^-m (-1)^m w
		const double2 ph = rot_phase(m, p.ang_out);
		const double w = (m == 0 ? 1.0 : 2.0)*((m & 1) ? -1.0 : 1.0);
		for (int c = 0; c < NC; c++) {
			const double2 y = cmul(ph, make_double2(re[c], im[c]));
			p.y[(base + m)*NC + c] = make_double2(w*y.x, w*y.y);
		}
	} else {
		const double2 ph = mul_ipow(rot_phase(m, p.ang_out), m);
		const double s = (m & 1) ? -1.0 : 1.0;
		const long i = rot_tri(p.lmax, l, m);
		for (int c = 0; c < NC; c++) {
			const double2 y = cmul(ph, make_double2(s*re[c], s*im[c]));
			rot_st(p.out, p.out_dtype, c*p.out_cstride + i, y);
		}
	}
}

// theta == 0: a'_lm = e^{-im psi} e^{-im phi} a_lm (elementwise, so out may alias in)
__global__ __launch_bounds__(256) void rot_phase_kernel(RotK p, int ncomp)
{
	const int l = blockIdx.x*blockDim.x + threadIdx.x, m = blockIdx.y;
	if (l > p.lmax || l < m) return;
	const double2 ph = cmul(rot_phase(m, p.ang_in), rot_phase(m, p.ang_out));
	const long i = rot_tri(p.lmax, l, m);
	for (int c = 0; c < ncomp; c++) rot_st(p.out, p.out_dtype, c*p.out_cstride + i, cmul(ph, rot_ld(p.in, p.in_dtype, c*p.in_cstride + i)));
}

template<int NC>
static void rot_group(RotK p, double2* coef, bool make_coef, double2* x1, double2* x2, double theta, double phi, hipStream_t st)
{
	const int L = p.lmax + 1;
	hipLaunchKernelGGL(rot_prep_kernel<NC>, dim3((L + 255)/256, L), dim3(256), 0, st, p, make_coef ? coef : (double2*)nullptr, x1);
	const long q = p.lmax/ROT_ROWS, r = p.lmax%ROT_ROWS;
	const long nblk = (p.lmax + 1) + ROT_ROWS*q*(q - 1)/2 + q*(r + 1);       // rot_nblk_upto(lmax)
	RotK p1 = p; p1.coef = coef; p1.x = x1; p1.y = x2; p1.ang_out = theta;
	hipLaunchKernelGGL((rot_pass_kernel<NC, 0>), dim3((unsigned)nblk), dim3(256), 0, st, p1, nblk);
	RotK p2 = p; p2.coef = coef; p2.x = x2; p2.y = nullptr; p2.ang_out = phi;
	hipLaunchKernelGGL((rot_pass_kernel<NC, 1>), dim3((unsigned)nblk), dim3(256), 0, st, p2, nblk);
}

} // namespace pxs

using namespace pxs;

extern "C" int pxa_rotate_alm(int lmax, int ncomp, const void* alm_in, int64_t in_cstride, void* alm_out, int64_t out_cstride, int alm_dtype,
                              double psi, double theta, double phi, int device, void* stream)
{
	PXS_TRY
	PXS_REQUIRE(lmax >= 0 && lmax <= 46340 && ncomp >= 1 && alm_in && alm_out, "pxa_rotate_alm: bad arguments");
	PXS_REQUIRE(alm_dtype == PX_C64 || alm_dtype == PX_C128, "pxa_rotate_alm: alm must be complex64 or complex128");
	const long nalm = (long)(lmax + 1)*(lmax + 2)/2;
	PXS_REQUIRE(ncomp == 1 || (std::abs(in_cstride) >= nalm && std::abs(out_cstride) >= nalm), "pxa_rotate_alm: component strides overlap");
	PXS_REQUIRE(std::isfinite(psi) && std::isfinite(theta) && std::isfinite(phi), "pxa_rotate_alm: angles must be finite");
	PXS_HIP(hipSetDevice(device));
	hipStream_t st = (hipStream_t)stream;
	RotK p{};
	p.lmax = lmax; p.in_dtype = alm_dtype; p.out_dtype = alm_dtype;
	if (theta == 0.0) {
		p.in = alm_in; p.in_cstride = in_cstride; p.out = alm_out; p.out_cstride = out_cstride; p.ang_in = psi; p.ang_out = phi;
		hipLaunchKernelGGL(rot_phase_kernel, dim3((lmax + 256)/256, lmax + 1), dim3(256), 0, st, p, ncomp);
		PXS_HIP(hipGetLastError());
		return 0;
	}
	// components in groups of at most 4 (the same coefficient table for all); the scratch is stream-ordered (allocated and freed on the
	// caller's stream: no host synchronisation, and no reuse while a kernel of this call may still read it)
	const int ngrp = (ncomp + 3)/4, gmax = (ncomp + ngrp - 1)/ngrp;
	const size_t bytes = sizeof(double2)*(size_t)nalm*(1 + 2*(size_t)gmax);
	void* scratch = nullptr;
	PXS_HIP(hipMallocAsync(&scratch, bytes, st));
	double2* coef = (double2*)scratch;
	double2* x1 = coef + nalm;
	double2* x2 = x1 + (size_t)nalm*gmax;
	for (int c0 = 0, g = 0; c0 < ncomp; g++) {
		const int nc = std::min(gmax, ncomp - c0);
		RotK q = p;
		q.in = (const char*)alm_in + (size_t)c0*in_cstride*dtype_bytes(alm_dtype); q.in_cstride = in_cstride;
		q.out = (char*)alm_out + (size_t)c0*out_cstride*dtype_bytes(alm_dtype); q.out_cstride = out_cstride;
		q.ang_in = psi;
		switch (nc) {
			case 1: rot_group<1>(q, coef, g == 0, x1, x2, theta, phi, st); break;
			case 2: rot_group<2>(q, coef, g == 0, x1, x2, theta, phi, st); break;
			case 3: rot_group<3>(q, coef, g == 0, x1, x2, theta, phi, st); break;
			default: rot_group<4>(q, coef, g == 0, x1, x2, theta, phi, st); break;
		}
		c0 += nc;
	}
	const hipError_t e = hipGetLastError();
	PXS_HIP(hipFreeAsync(scratch, st));
	PXS_HIP(e);
	PXS_CATCH
}
