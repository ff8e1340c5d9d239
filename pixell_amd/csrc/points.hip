// SHT synthesis and its adjoint at arbitrary positions (pxs_plan_points; ducc0.sht.experimental.synthesis_general /
// adjoint_synthesis_general as called at curvedsky.py:993-1016, 1088-1120).
//
//   forward   alm --CC synthesis (grid plan)--> f[c][Ntheta][Nphi] --mirror onto the doubled sphere--> g[2Ntheta-2][Nphi]
//             --2-D FFT--> deapodise by 1/(psi^(k1) psi^(k2)), zero-pad to the fine grid n1 x n2 (sigma = 2) --inverse 2-D FFT-->
//             interpolate W x W taps of the exponential-of-semicircle kernel per point
//   adjoint   the exact transpose of every step, in reverse order (spread, FFT, truncate + deapodise, inverse FFT, fold, adjoint
//             CC synthesis)
//
//   map pts   a pixel map instead of an alm (pxm_plan_map_points; aberration.interpol_map): map [ny][nx] --continued over the pole (ydouble)
//             or as it is--> g --2-D FFT--> the whole band, Nyquist terms split, deapodised and zero-padded --> the same last two steps
//
// g is exactly a 2-D trigonometric polynomial with |k_theta| <= lmax, |m| <= mmax: sLambda_lm(-theta) = (-1)^(m+s) sLambda_lm(theta),
// and (-theta, phi) is the point (theta, phi + pi), so the continuation of ring j past the pole is ring j shifted by half a turn
// times (-1)^s.  Two real fields travel in one complex grid (Q + iU, or two spin-0 maps).
//
// Points are binned by the fine-grid tile (T x T cells) of their first tap and sorted by tile with a stable LSD radix sort (block-local
// ranks, no atomics on the order), so every step is deterministic: the spreading keeps one padded (T+W-1)^2 tile per workgroup in LDS,
// lanes own rows of it (no two lanes touch one cell), the tiles go to a slab and a gather pass adds the (at most four) tiles that
// cover a cell in a fixed order.
#include "../../include/pxsht.h"
#include "common.hpp"
#include <cmath>
#include <vector>
#include <algorithm>
#include <memory>
#include <string>
#include <chrono>

namespace pxs {

static const int PT_T = 32;                  // tile edge (fine-grid cells)
static const int PT_WMAX = 16;               // largest kernel width
static const int RS_IPB = 1024, RS_THR = 256;   // radix sort: items and threads per block
enum { PT_ST_CC = 0, PT_ST_FFT = 1, PT_ST_GRID = 2, PT_ST_INTERP = 3, PT_ST_SPREAD = 4, PT_NSTAGE = 5 };
static const char* const PT_STAGE_NAMES[PT_NSTAGE] = {"cc_sht", "fft", "grid", "interp", "spread"};

__device__ __forceinline__ double es_kernel(double z, double beta) {
	const double t = 1.0 - z*z;
	return t > 0.0 ? exp(beta*(sqrt(t) - 1.0)) : 0.0;
}
// first tap of a fine coordinate x (wrapped into [0, n)), and the W kernel weights of taps first .. first + W - 1
__device__ __forceinline__ long pt_first(double x, long n, int W, double* s_out) {
	const double s = ceil(x - 0.5*W);
	*s_out = s;
	long i0 = (long)s % n; if (i0 < 0) i0 += n;
	return i0;
}
__device__ __forceinline__ long pt_taps(double x, long n, int W, double beta, double* w) {
	double s; const long i0 = pt_first(x, n, W, &s);
	const double inv = 2.0/W;
#pragma unroll
	for (int a = 0; a < PT_WMAX; a++) w[a] = a < W ? es_kernel((s + a - x)*inv, beta) : 0.0;
	return i0;
}
__device__ __forceinline__ double ld_real(const void* p, int dt, long i) {
	return dt == PX_F32 ? (double)((const float*)p)[i] : ((const double*)p)[i];
}
__device__ __forceinline__ void st_real(void* p, int dt, long i, double v) {
	if (dt == PX_F32) ((float*)p)[i] = (float)v; else ((double*)p)[i] = v;
}

// ---- binning and the stable sort by tile --------------------------------------------------------------------------------
__global__ void pt_bin(long npts, const double* loc, long n1, long n2, int W, int nt2, double2* xu, uint32_t* key, int* bad)
{
	const long i = (long)blockIdx.x*blockDim.x + threadIdx.x;
	if (i >= npts) return;
	double th = loc[2*i], ph = loc[2*i+1];
	if (!(th >= 0.0 && th <= PXS_PI) || !(ph == ph) || fabs(ph) > 1e300) { *bad = 1; th = 0.0; ph = 0.0; }
	double u = ph*(0.5/PXS_PI); u -= floor(u);
	const double x1 = th*(0.5/PXS_PI)*(double)n1, x2 = u*(double)n2;
	double s;
	const long i0 = pt_first(x1, n1, W, &s), j0 = pt_first(x2, n2, W, &s);
	xu[i] = make_double2(x1, x2);
	key[i] = (uint32_t)((i0/PT_T)*nt2 + j0/PT_T);
}

__global__ void rs_hist(long n, const uint32_t* key, int shift, long nblk, int64_t* H)
{
	PXS_SHARED(int, h);
	const int t = threadIdx.x;
	h[t] = 0;
	__syncthreads();
	const long base = (long)blockIdx.x*RS_IPB;
	for (int k = 0; k < RS_IPB/RS_THR; k++) { const long i = base + k*RS_THR + t; if (i < n) atomicAdd(&h[(key[i] >> shift) & 255], 1); }
	__syncthreads();
	H[(long)t*nblk + blockIdx.x] = h[t];
}

// exclusive scan of a[L] in chunks of 1024 (sums[chunk] = chunk total), the chunk totals in one workgroup, then the carry-in
__device__ void block_scan256(int64_t* s, int t) {
	for (int off = 1; off < 256; off <<= 1) {
		const int64_t x = t >= off ? s[t - off] : 0;
		__syncthreads(); s[t] += x; __syncthreads();
	}
}
__global__ void scan_chunks(long L, int64_t* a, int64_t* sums)
{
	PXS_SHARED(int64_t, s);
	const int t = threadIdx.x; const long base = (long)blockIdx.x*1024 + 4*t;
	int64_t v[4], tot = 0;
	for (int k = 0; k < 4; k++) { v[k] = base + k < L ? a[base + k] : 0; tot += v[k]; }
	s[t] = tot; __syncthreads();
	block_scan256(s, t);
	int64_t run = s[t] - tot;
	for (int k = 0; k < 4; k++) { if (base + k < L) a[base + k] = run; run += v[k]; }
	if (t == 255) sums[blockIdx.x] = s[255];
}
__global__ void scan_sums(long nc, int64_t* sums)
{
	PXS_SHARED(int64_t, s);
	const int t = threadIdx.x; int64_t carry = 0;
	for (long c0 = 0; c0 < nc; c0 += 256) {
		const long c = c0 + t; const int64_t v = c < nc ? sums[c] : 0;
		s[t] = v; __syncthreads();
		block_scan256(s, t);
		if (c < nc) sums[c] = carry + s[t] - v;
		carry += s[255];
		__syncthreads();
	}
}
__global__ void scan_add(long L, int64_t* a, const int64_t* sums)
{
	const long i = (long)blockIdx.x*blockDim.x + threadIdx.x;
	if (i < L) a[i] += sums[i/1024];
}

// stable scatter of one 8-bit digit: the rank of an item among the items of its block with the same digit is counted, in order
__global__ void rs_scatter(long n, const uint32_t* kin, const int64_t* vin, uint32_t* kout, int64_t* vout, int shift, long nblk, const int64_t* H)
{
	PXS_SHARED(unsigned char, dg);
	const int t = threadIdx.x; const long base = (long)blockIdx.x*RS_IPB;
	for (int k = 0; k < RS_IPB/RS_THR; k++) { const int j = k*RS_THR + t; const long i = base + j; dg[j] = i < n ? (unsigned char)((kin[i] >> shift) & 255) : 0; }
	__syncthreads();
	for (int k = 0; k < RS_IPB/RS_THR; k++) {
		const int j = k*RS_THR + t; const long i = base + j;
		if (i >= n) continue;
		const unsigned char d = dg[j];
		int r = 0;
		for (int q = 0; q < j; q++) r += dg[q] == d;
		const long pos = H[(long)d*nblk + blockIdx.x] + r;
		kout[pos] = kin[i]; vout[pos] = vin ? vin[i] : i;
	}
}

// tile offsets from the sorted keys: off[t] = first sorted position with key >= t (binary search, one lane per tile), off[ntiles] = n
__global__ void pt_offsets(long n, const uint32_t* ks, long ntiles, int64_t* off)
{
	const long t = (long)blockIdx.x*blockDim.x + threadIdx.x;
	if (t > ntiles) return;
	long lo = 0, hi = n;
	while (lo < hi) { const long mid = lo + (hi - lo)/2; if ((long)ks[mid] < t) lo = mid + 1; else hi = mid; }
	off[t] = lo;
}
__global__ void pt_gather_x(long n, const int64_t* perm, const double2* xu, double2* xs)
{
	const long s = (long)blockIdx.x*blockDim.x + threadIdx.x;
	if (s < n) xs[s] = xu[perm[s]];
}

// ---- grid stages (elementwise, HBM-bound) -------------------------------------------------------------------------------
__global__ void pt_double(int ntheta, int nphi, const double* fa, const double* fb, double sgn, double2* g)
{
	const long N1 = 2L*ntheta - 2, idx = (long)blockIdx.x*blockDim.x + threadIdx.x;
	if (idx >= N1*nphi) return;
	const long j = idx/nphi, k = idx - j*nphi;
	long src; double s = 1.0;
	if (j < ntheta) src = j*nphi + k;
	else { src = (N1 - j)*nphi + (k + nphi/2)%nphi; s = sgn; }
	g[idx] = make_double2(s*fa[src], fb ? s*fb[src] : 0.0);
}
__global__ void pt_fold(int ntheta, int nphi, const double2* g, double sgn, double* fa, double* fb)
{
	const long N1 = 2L*ntheta - 2, idx = (long)blockIdx.x*blockDim.x + threadIdx.x;
	if (idx >= (long)ntheta*nphi) return;
	const long j = idx/nphi, k = idx - j*nphi;
	double2 v = g[idx];
	if (j > 0 && j < ntheta - 1) { const double2 w = g[(N1 - j)*nphi + (k + nphi/2)%nphi]; v.x += sgn*w.x; v.y += sgn*w.y; }
	fa[idx] = v.x;
	if (fb) fb[idx] = v.y;
}
// coarse spectrum (N1 x N2) -> fine spectrum (n1 x n2), deapodised; everything outside |k1| <= lmax, |k2| <= mmax is zero
__global__ void pt_pad(long n1, long n2, long N1, long N2, int lmax, int mmax, const double2* c, const double* d1, const double* d2, double scale, double2* f)
{
	const long idx = (long)blockIdx.x*blockDim.x + threadIdx.x;
	if (idx >= n1*n2) return;
	const long r1 = idx/n2, r2 = idx - r1*n2;
	const long k1 = r1 <= n1/2 ? r1 : r1 - n1, k2 = r2 <= n2/2 ? r2 : r2 - n2;
	const long a1 = k1 < 0 ? -k1 : k1, a2 = k2 < 0 ? -k2 : k2;
	double2 v = make_double2(0.0, 0.0);
	if (a1 <= lmax && a2 <= mmax) {
		const double2 x = c[(k1 < 0 ? k1 + N1 : k1)*N2 + (k2 < 0 ? k2 + N2 : k2)];
		const double w = d1[a1]*d2[a2]*scale;
		v = make_double2(x.x*w, x.y*w);
	}
	f[idx] = v;
}
// its transpose: fine spectrum -> coarse spectrum
__global__ void pt_trunc(long n1, long n2, long N1, long N2, int lmax, int mmax, const double2* f, const double* d1, const double* d2, double scale, double2* c)
{
	const long idx = (long)blockIdx.x*blockDim.x + threadIdx.x;
	if (idx >= N1*N2) return;
	const long j1 = idx/N2, j2 = idx - j1*N2;
	const long k1 = j1 <= N1/2 ? j1 : j1 - N1, k2 = j2 <= N2/2 ? j2 : j2 - N2;
	const long a1 = k1 < 0 ? -k1 : k1, a2 = k2 < 0 ? -k2 : k2;
	double2 v = make_double2(0.0, 0.0);
	if (a1 <= lmax && a2 <= mmax) {
		const double2 x = f[(k1 < 0 ? k1 + n1 : k1)*n2 + (k2 < 0 ? k2 + n2 : k2)];
		const double w = d1[a1]*d2[a2]*scale;
		v = make_double2(x.x*w, x.y*w);
	}
	c[idx] = v;
}

// ---- pixel maps as the source (pxm_plan_map_points): the trigonometric interpolant of a map [ny][nx] at pixel coordinates ------------
// pix[{y, x}][npts] in pixels, any finite value: wrapped onto the periodic grid N1 x N2 before the tile key is formed
__global__ void mp_bin(long npts, const double* pix, long N1, long N2, long n1, long n2, int W, int nt2, double2* xu, uint32_t* key, int* bad)
{
	const long i = (long)blockIdx.x*blockDim.x + threadIdx.x;
	if (i >= npts) return;
	double y = pix[i], x = pix[npts + i];
	if (!(fabs(y) <= 1e300) || !(fabs(x) <= 1e300)) { *bad = 1; y = 0.0; x = 0.0; }
	y /= (double)N1; y -= floor(y);
	x /= (double)N2; x -= floor(x);
	const double x1 = y*(double)n1, x2 = x*(double)n2;
	double s;
	const long i0 = pt_first(x1, n1, W, &s), j0 = pt_first(x2, n2, W, &s);
	xu[i] = make_double2(x1, x2);
	key[i] = (uint32_t)((i0/PT_T)*nt2 + j0/PT_T);
}
// two real maps (fb may be null) -> one complex grid g[N1][nx]; ydouble: rows ny .. 2 ny - 1 are the rows ny - 1 .. 0 continued over the
// pole, g[ny + r][k] = f[ny - 1 - r][k - nx/2] (aberration.interpol_map)
__global__ void mp_pack(int ny, int nx, int ydouble, const void* fa, const void* fb, int dt, double2* g)
{
	const long N1 = ydouble ? 2L*ny : ny, idx = (long)blockIdx.x*blockDim.x + threadIdx.x;
	if (idx >= N1*nx) return;
	const long j = idx/nx, k = idx - j*nx;
	const long src = j < ny ? idx : (N1 - 1 - j)*nx + (k + nx - nx/2)%nx;
	g[idx] = make_double2(ld_real(fa, dt, src), fb ? ld_real(fb, dt, src) : 0.0);
}
// coarse spectrum (N1 x N2, the whole band) -> fine spectrum (n1 x n2), deapodised.  The Nyquist coefficient of an even axis goes half
// and half to +N/2 and -N/2: the operator stays real-to-real, so the two maps packed into one complex grid do not mix.  Where both axes
// are even the corner coefficient G[N1/2][N2/2] (real for a real map) stands for cos(pi (y + x)), the real part of its one-sided term:
// half each to (+N1/2, +N2/2) and (-N1/2, -N2/2), nothing to the other two corners.
__global__ void mp_pad(long n1, long n2, long N1, long N2, const double2* c, const double* d1, const double* d2, double scale, double2* f)
{
	const long idx = (long)blockIdx.x*blockDim.x + threadIdx.x;
	if (idx >= n1*n2) return;
	const long r1 = idx/n2, r2 = idx - r1*n2;
	const long k1 = r1 <= n1/2 ? r1 : r1 - n1, k2 = r2 <= n2/2 ? r2 : r2 - n2;
	const long a1 = k1 < 0 ? -k1 : k1, a2 = k2 < 0 ? -k2 : k2;
	double2 v = make_double2(0.0, 0.0);
	if (2*a1 <= N1 && 2*a2 <= N2) {
		const double2 x = c[(k1 < 0 ? k1 + N1 : k1)*N2 + (k2 < 0 ? k2 + N2 : k2)];
		const bool ny1 = 2*a1 == N1, ny2 = 2*a2 == N2;
		const double share = ny1 && ny2 ? ((k1 < 0) == (k2 < 0) ? 0.5 : 0.0) : (ny1 || ny2 ? 0.5 : 1.0);
		const double w = d1[a1]*d2[a2]*scale*share;
		v = make_double2(x.x*w, x.y*w);
	}
	f[idx] = v;
}

// ---- interpolation (forward) and spreading (adjoint) -----------------------------------------------------------------------
// one lane per point, in tile order (neighbouring lanes read neighbouring cells: the taps of a wave stay in L2), W x W taps straight
// from the fine grid; the result goes to the point's original index
__global__ __launch_bounds__(256) void pt_interp(long npts, const double2* xs, const int64_t* perm, const double2* f, long n1, long n2,
	int W, double beta, void* oa, void* ob, int dt)
{
	const long s = (long)blockIdx.x*blockDim.x + threadIdx.x;
	if (s >= npts) return;
	const double2 x = xs[s];
	double w1[PT_WMAX], w2[PT_WMAX];
	const long i0 = pt_taps(x.x, n1, W, beta, w1), j0 = pt_taps(x.y, n2, W, beta, w2);
	double re = 0.0, im = 0.0;
#pragma unroll
	for (int a = 0; a < PT_WMAX; a++) {
		if (a < W) {
			long r = i0 + a; if (r >= n1) r -= n1;
			const double2* row = f + r*n2;
			double sr = 0.0, si = 0.0;
#pragma unroll
			for (int b = 0; b < PT_WMAX; b++) {
				if (b < W) {
					long c = j0 + b; if (c >= n2) c -= n2;
					const double2 v = row[c];
					sr += w2[b]*v.x; si += w2[b]*v.y;
				}
			}
			re += w1[a]*sr; im += w1[a]*si;
		}
	}
	const long o = perm[s];
	st_real(oa, dt, o, re);
	if (ob) st_real(ob, dt, o, im);
}

// one wave per tile: its points, in sorted order, are staged 64 at a time (first taps, values, 2W weights); lane r owns row r of the
// padded tile in LDS, so the adds of a point never collide and the order of the sum is fixed.  Every tile is written (zeros if empty).
__global__ __launch_bounds__(64) void pt_spread(const int64_t* off, const double2* xs, const int64_t* perm, const void* ma, const void* mb, int dt,
	long n1, long n2, int nt2, int W, double beta, int P, double2* slab)
{
	PXS_SHARED(double, sh);
	double2* acc = reinterpret_cast<double2*>(sh);
	double* stg = sh + 2*P*P;
	const int t = threadIdx.x, stride = 2*W + 4;
	const long tile = blockIdx.x, q1 = tile/nt2, q2 = tile - q1*nt2;
	for (int c = t; c < P*P; c += 64) acc[c] = make_double2(0.0, 0.0);
	const long s0 = off[tile], s1 = off[tile+1];
	for (long c0 = s0; c0 < s1; c0 += 64) {
		__syncthreads();
		const long s = c0 + t;
		if (s < s1) {
			const double2 x = xs[s];
			double w1[PT_WMAX], w2[PT_WMAX];
			const long i0 = pt_taps(x.x, n1, W, beta, w1), j0 = pt_taps(x.y, n2, W, beta, w2);
			const long o = perm[s];
			double* g = stg + t*stride;
			g[0] = (double)(i0 - q1*PT_T); g[1] = (double)(j0 - q2*PT_T);
			g[2] = ld_real(ma, dt, o); g[3] = mb ? ld_real(mb, dt, o) : 0.0;
#pragma unroll
			for (int a = 0; a < PT_WMAX; a++) if (a < W) { g[4+a] = w1[a]; g[4+W+a] = w2[a]; }
		}
		__syncthreads();
		const int cnt = (int)min(64L, s1 - c0);
		for (int q = 0; q < cnt; q++) {
			const double* g = stg + q*stride;
			const int a = t - (int)g[0];
			if (a >= 0 && a < W) {
				const double wa = g[4+a], va = wa*g[2], vb = wa*g[3];
				double2* row = acc + t*P + (int)g[1];
				for (int b = 0; b < W; b++) { const double wb = g[4+W+b]; row[b].x += va*wb; row[b].y += vb*wb; }
			}
		}
	}
	__syncthreads();
	double2* out = slab + tile*(long)P*P;
	for (int c = t; c < P*P; c += 64) out[c] = acc[c];
}
// fine cell (c1, c2) = sum of the padded tiles that cover it (this tile and its predecessor along each axis), in a fixed order
__global__ void pt_gather(long n1, long n2, int nt1, int nt2, int P, const double2* slab, double2* f)
{
	const long idx = (long)blockIdx.x*blockDim.x + threadIdx.x;
	if (idx >= n1*n2) return;
	const long c1 = idx/n2, c2 = idx - c1*n2, qa = c1/PT_T, qb = c2/PT_T;
	double re = 0.0, im = 0.0;
	for (int u = 0; u < 2; u++) {
		const long q1 = u == 0 ? qa : (qa + nt1 - 1)%nt1;
		long d1 = c1 - q1*PT_T; if (d1 < 0) d1 += n1;
		if (d1 >= P) continue;
		for (int v = 0; v < 2; v++) {
			const long q2 = v == 0 ? qb : (qb + nt2 - 1)%nt2;
			long d2 = c2 - q2*PT_T; if (d2 < 0) d2 += n2;
			if (d2 >= P) continue;
			const double2 x = slab[((q1*nt2 + q2)*P + d1)*P + d2];
			re += x.x; im += x.y;
		}
	}
	f[idx] = make_double2(re, im);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
struct PointsState {
	int device = 0; long npts = 0; double eps = 0, beta = 0; int W = 0;
	int ntheta = 0, nphi = 0, lmax = 0, mmax = 0; long N1 = 0, n1 = 0, n2 = 0; int nt1 = 0, nt2 = 0;
	bool from_map = false, ydouble = false;      // a map points plan: the coarse grid is a pixel map [ntheta][nphi] (ydouble: continued over the pole), not a CC synthesis
	DevBuf xs, perm, off, d1, d2;       // point state: sorted fine coordinates, sorted -> original index, tile offsets, deapodisation
	DevBuf fbuf, cbuf, fine, slab;      // scratch of a call
	// stage timers (pxs_plan_option "profile"): device-event ms per stage, summed over the calls since enabled; plan_ms: host wall time
	// of points_create (kernels, host tables, allocation, the one synchronisation)
	bool prof = false; double stage_ms[PT_NSTAGE] = {}; double plan_ms = 0;
};

// Gauss-Legendre nodes and weights on [-1, 1]
static void gauss_legendre(int n, std::vector<double>& x, std::vector<double>& w) {
	x.resize(n); w.resize(n);
	for (int i = 0; i < n; i++) {
		long double z = cosl(3.141592653589793238462643383279502884L*(i + 0.75L)/(n + 0.5L)), dp = 0;
		for (int it = 0; it < 100; it++) {
			long double p0 = 1, p1 = z;
			for (int k = 2; k <= n; k++) { const long double p2 = ((2*k - 1)*z*p1 - (k - 1)*p0)/k; p0 = p1; p1 = p2; }
			dp = n*(z*p1 - p0)/(z*z - 1);
			const long double dz = p1/dp; z -= dz;
			if (fabsl(dz) < 1e-19L) break;
		}
		x[i] = (double)z; w[i] = (double)(2/((1 - z*z)*dp*dp));
	}
}
// 1 / psi^(k), k = 0..kmax, for the fine circle of n cells: psi^(k) = int psi(2u/W) e^{-2 pi i k u/n} du = W/2 int_{-1}^{1} psi(z) cos(pi k W z/n) dz
static std::vector<double> deapod_table(int kmax, long n, int W, double beta) {
	std::vector<double> x, w; gauss_legendre(200, x, w);
	std::vector<double> out(kmax + 1);
	std::vector<long double> acc(kmax + 1, 0.0L);
	for (size_t q = 0; q < x.size(); q++) {
		// the kernel value once per node; cos(k a) for every k by the Chebyshev recurrence c_{k+1} = 2 cos(a) c_k - c_{k-1}
		const long double t = 1 - (long double)x[q]*x[q];
		const long double psi = (long double)w[q]*expl(beta*(sqrtl(t) - 1));
		const long double c1 = cosl(3.141592653589793238462643383279502884L*W*(long double)x[q]/n);
		long double cm = 1.0L, c = c1;
		acc[0] += psi;
		for (int k = 1; k <= kmax; k++) { acc[k] += psi*c; const long double cn = 2*c1*c - cm; cm = c; c = cn; }
	}
	for (int k = 0; k <= kmax; k++) out[k] = (double)(1/(acc[k]*0.5L*W));
	return out;
}

static inline unsigned nblocks(long n, int b) { return (unsigned)((n + b - 1)/b); }

// kernel width and shape for a relative accuracy eps at oversampling 2
void points_kernel_params(double eps, int* W, double* beta) {
	int w = (int)std::ceil(std::log10(1.0/eps)) + 2;
	w = std::max(3, std::min(PT_WMAX, w));
	*W = w; *beta = 2.30*w;
}

static long fine_size(long n) {      // >= 2n (sigma = 2), a multiple of the tile, at least two tiles
	const long m = std::max<long>(2, (2*n + PT_T - 1)/PT_T);
	return PT_T*(long)pxf_fft_good_size(m);
}

// The point state of a plan whose fine grid (n1, n2, W) is set: bin(xu, key, bad) launches the kernel that writes every point's fine
// coordinates and tile key (and sets *bad for a point it refuses); the points are then sorted by tile into s->xs, s->perm, s->off.
// Synchronises the stream once; `refused`: the error of a refused point.
template<class Bin> static void sort_points(PointsState* s, Bin&& bin, const char* refused, hipStream_t st)
{
	const long npts = s->npts, ntiles = (long)s->nt1*s->nt2;
	s->off.alloc(sizeof(int64_t)*(ntiles + 1));
	if (npts == 0) { PXS_HIP(hipMemsetAsync(s->off.p, 0, s->off.bytes, st)); return; }
	DevBuf xu(sizeof(double2)*npts), k0(sizeof(uint32_t)*npts), k1(sizeof(uint32_t)*npts), v0(sizeof(int64_t)*npts), v1(sizeof(int64_t)*npts), bad(sizeof(int));
	PXS_HIP(hipMemsetAsync(bad.p, 0, sizeof(int), st));
	bin(xu.as<double2>(), k0.as<uint32_t>(), bad.as<int>());
	PXS_HIP(hipGetLastError());
	// LSD radix sort of (tile, index), 8 bits a pass
	int bits = 1; while ((1L << bits) < ntiles) bits++;
	const long nblk = (npts + RS_IPB - 1)/RS_IPB, L = 256*nblk, nch = (L + 1023)/1024;
	DevBuf H(sizeof(int64_t)*L), S(sizeof(int64_t)*nch);
	uint32_t* kin = k0.as<uint32_t>(); uint32_t* kout = k1.as<uint32_t>();
	int64_t* vin = nullptr; int64_t* vout = v0.as<int64_t>(); int64_t* vspare = v1.as<int64_t>();
	for (int shift = 0; shift < bits; shift += 8) {
		hipLaunchKernelGGL(rs_hist, dim3((unsigned)nblk), dim3(RS_THR), 256*sizeof(int), st, npts, kin, shift, nblk, H.as<int64_t>());
		hipLaunchKernelGGL(scan_chunks, dim3((unsigned)nch), dim3(256), 256*sizeof(int64_t), st, L, H.as<int64_t>(), S.as<int64_t>());
		hipLaunchKernelGGL(scan_sums, dim3(1), dim3(256), 256*sizeof(int64_t), st, nch, S.as<int64_t>());
		hipLaunchKernelGGL(scan_add, dim3(nblocks(L, 256)), dim3(256), 0, st, L, H.as<int64_t>(), S.as<int64_t>());
		hipLaunchKernelGGL(rs_scatter, dim3((unsigned)nblk), dim3(RS_THR), RS_IPB, st, npts, kin, vin, kout, vout, shift, nblk, H.as<int64_t>());
		PXS_HIP(hipGetLastError());
		std::swap(kin, kout);
		int64_t* nv = vin ? vin : vspare; vin = vout; vout = nv;
	}
	hipLaunchKernelGGL(pt_offsets, dim3(nblocks(ntiles + 1, 256)), dim3(256), 0, st, npts, kin, ntiles, s->off.as<int64_t>());
	s->xs.alloc(sizeof(double2)*npts); s->perm.alloc(sizeof(int64_t)*npts);
	PXS_HIP(hipMemcpyAsync(s->perm.p, vin, sizeof(int64_t)*npts, hipMemcpyDeviceToDevice, st));
	hipLaunchKernelGGL(pt_gather_x, dim3(nblocks(npts, 256)), dim3(256), 0, st, npts, s->perm.as<int64_t>(), xu.as<double2>(), s->xs.as<double2>());
	PXS_HIP(hipGetLastError());
	int hbad = 0;
	PXS_HIP(hipMemcpyAsync(&hbad, bad.p, sizeof(int), hipMemcpyDeviceToHost, st));
	PXS_HIP(hipStreamSynchronize(st));      // (the temporaries above are released on return)
	PXS_REQUIRE(!hbad, refused);
}

PointsState* points_create(int ntheta, int nphi, int lmax, int mmax, int device, long npts, const double* d_loc, double eps, hipStream_t st)
{
	const auto t0 = std::chrono::steady_clock::now();
	std::unique_ptr<PointsState> s(new PointsState());
	s->device = device; s->npts = npts; s->eps = eps; s->ntheta = ntheta; s->nphi = nphi; s->lmax = lmax; s->mmax = mmax;
	points_kernel_params(eps, &s->W, &s->beta);
	s->N1 = 2L*ntheta - 2;
	s->n1 = fine_size(s->N1); s->n2 = fine_size(nphi);
	s->nt1 = (int)(s->n1/PT_T); s->nt2 = (int)(s->n2/PT_T);
	PXS_REQUIRE((long)s->nt1*s->nt2 < (1L << 31), "pxs_plan_points: fine grid too large");
	s->d1 = upload(deapod_table(lmax, s->n1, s->W, s->beta));
	s->d2 = upload(deapod_table(mmax, s->n2, s->W, s->beta));
	PointsState* q = s.get();
	sort_points(q, [&](double2* xu, uint32_t* key, int* bad) {
		hipLaunchKernelGGL(pt_bin, dim3(nblocks(npts, 256)), dim3(256), 0, st, npts, d_loc, q->n1, q->n2, q->W, q->nt2, xu, key, bad); },
		"pxs_plan_points: theta outside [0, pi] or non-finite phi", st);
	s->plan_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	return s.release();
}

void points_free(PointsState* s) { delete s; }

// the stage timers of one call: run(stage, fn) puts fn between two events when the plan is profiled, collect() waits for them and adds
// the times to the plan's
struct StageTimer {
	PointsState* s; hipStream_t st;
	struct Ev { int stage; hipEvent_t a, b; };
	std::vector<Ev> evs;
	template<class F> void run(int stage, F&& fn) {
		if (!s->prof) { fn(); return; }
		Ev e{stage, nullptr, nullptr};
		PXS_HIP(hipEventCreate(&e.a)); PXS_HIP(hipEventCreate(&e.b));
		PXS_HIP(hipEventRecord(e.a, st)); fn(); PXS_HIP(hipEventRecord(e.b, st));
		evs.push_back(e);
	}
	void collect() {
		for (auto& e : evs) {
			float ms = 0; PXS_HIP(hipEventSynchronize(e.b)); PXS_HIP(hipEventElapsedTime(&ms, e.a, e.b));
			s->stage_ms[e.stage] += ms; (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b);
		}
		evs.clear();
	}
};

static void fft2(PointsState* s, hipStream_t st, long na, long nb, double2* data, bool forward) {
	const int64_t shape[2] = {na, nb}, strides[2] = {nb, 1};
	const int axes[2] = {0, 1};
	const int rc = pxf_fft_nd(2, shape, strides, strides, 2, axes, 0, forward ? 1 : 0, 1.0, PX_C128, PX_C128, data, data, s->device, st);
	if (rc != 0) throw Error(rc, std::string("points: 2-D FFT failed: ") + pxs_last_error());
}

// one call of pxs_synthesis on a points plan; grid: the CC plan it was made from
void points_run(PointsState* s, pxs_plan* grid, int spin, int mode, int adjoint, int nb, const AlmArg& alm, const MapArg& map, hipStream_t st)
{
	const int ncm = (spin == 0 && mode == PXS_MODE_STANDARD) ? 1 : 2;
	const long npix = (long)s->ntheta*s->nphi, nfield = (long)nb*ncm;
	const double sgn = (spin & 1) ? -1.0 : 1.0;
	const double scale = 1.0/((double)s->N1*s->nphi);
	const int P = PT_T + s->W - 1;
	const long ntiles = (long)s->nt1*s->nt2, nfine = s->n1*s->n2, ncoarse = s->N1*s->nphi;
	s->fbuf.ensure(sizeof(double)*nfield*npix);
	s->cbuf.ensure(sizeof(double2)*ncoarse);
	s->fine.ensure(sizeof(double2)*nfine);
	double* f = s->fbuf.as<double>();
	StageTimer timer{s, st};
	auto timed = [&](int stage, auto&& fn) { timer.run(stage, fn); };
	auto collect = [&]() { timer.collect(); };
	auto field = [&](long q) -> char* { const long b = q/ncm, c = q - b*ncm; return (char*)map.from(b).ptr + dtype_bytes(map.dtype)*c*map.cstride; };
	if (!adjoint) {
		timed(PT_ST_CC, [&] {
			const int rc = pxs_synthesis(grid, spin, mode, 0, nb, alm.ptr, alm.dtype, alm.cstride, alm.bstride, f, PX_F64, npix, ncm*npix, st);
			if (rc != 0) throw Error(rc, pxs_last_error()); });
		if (s->npts == 0) { collect(); return; }
		for (long q = 0; q < nfield; q += 2) {
			const bool two = q + 1 < nfield;
			timed(PT_ST_GRID, [&] { hipLaunchKernelGGL(pt_double, dim3(nblocks(ncoarse, 256)), dim3(256), 0, st, s->ntheta, s->nphi, f + q*npix, two ? f + (q+1)*npix : nullptr, sgn, s->cbuf.as<double2>()); });
			timed(PT_ST_FFT, [&] { fft2(s, st, s->N1, s->nphi, s->cbuf.as<double2>(), true); });
			timed(PT_ST_GRID, [&] { hipLaunchKernelGGL(pt_pad, dim3(nblocks(nfine, 256)), dim3(256), 0, st, s->n1, s->n2, s->N1, (long)s->nphi, s->lmax, s->mmax,
				s->cbuf.as<double2>(), s->d1.as<double>(), s->d2.as<double>(), scale, s->fine.as<double2>()); });
			timed(PT_ST_FFT, [&] { fft2(s, st, s->n1, s->n2, s->fine.as<double2>(), false); });
			timed(PT_ST_INTERP, [&] { hipLaunchKernelGGL(pt_interp, dim3(nblocks(s->npts, 256)), dim3(256), 0, st, s->npts, s->xs.as<double2>(), s->perm.as<int64_t>(),
				s->fine.as<double2>(), s->n1, s->n2, s->W, s->beta, (void*)field(q), two ? (void*)field(q+1) : nullptr, map.dtype); });
			PXS_HIP(hipGetLastError());
		}
	} else {
		s->slab.ensure(sizeof(double2)*(size_t)ntiles*P*P);
		for (long q = 0; q < nfield; q += 2) {
			const bool two = q + 1 < nfield;
			timed(PT_ST_SPREAD, [&] {
				if (s->npts > 0) {
					const size_t shm = sizeof(double)*(2*(size_t)P*P + 64*(2*s->W + 4));
					hipLaunchKernelGGL(pt_spread, dim3((unsigned)ntiles), dim3(64), shm, st, s->off.as<int64_t>(), s->xs.as<double2>(), s->perm.as<int64_t>(),
						(const void*)field(q), two ? (const void*)field(q+1) : nullptr, map.dtype, s->n1, s->n2, s->nt2, s->W, s->beta, P, s->slab.as<double2>());
					hipLaunchKernelGGL(pt_gather, dim3(nblocks(nfine, 256)), dim3(256), 0, st, s->n1, s->n2, s->nt1, s->nt2, P, s->slab.as<double2>(), s->fine.as<double2>());
				} else PXS_HIP(hipMemsetAsync(s->fine.p, 0, sizeof(double2)*nfine, st)); });
			timed(PT_ST_FFT, [&] { fft2(s, st, s->n1, s->n2, s->fine.as<double2>(), true); });
			timed(PT_ST_GRID, [&] { hipLaunchKernelGGL(pt_trunc, dim3(nblocks(ncoarse, 256)), dim3(256), 0, st, s->n1, s->n2, s->N1, (long)s->nphi, s->lmax, s->mmax,
				s->fine.as<double2>(), s->d1.as<double>(), s->d2.as<double>(), scale, s->cbuf.as<double2>()); });
			timed(PT_ST_FFT, [&] { fft2(s, st, s->N1, s->nphi, s->cbuf.as<double2>(), false); });
			timed(PT_ST_GRID, [&] { hipLaunchKernelGGL(pt_fold, dim3(nblocks(npix, 256)), dim3(256), 0, st, s->ntheta, s->nphi, s->cbuf.as<double2>(), sgn, f + q*npix, two ? f + (q+1)*npix : nullptr); });
			PXS_HIP(hipGetLastError());
		}
		timed(PT_ST_CC, [&] {
			const int rc = pxs_synthesis(grid, spin, mode, 1, nb, alm.ptr, alm.dtype, alm.cstride, alm.bstride, f, PX_F64, npix, ncm*npix, st);
			if (rc != 0) throw Error(rc, pxs_last_error()); });
	}
	collect();
}

// ---- map points plans (pxm_plan_map_points): the same point state, fine grid and interpolation; the coarse grid is a pixel map's -----
PointsState* mappoints_create(int ny, int nx, int ydouble, int device, long npts, const double* d_pix, double eps, hipStream_t st)
{
	const auto t0 = std::chrono::steady_clock::now();
	std::unique_ptr<PointsState> s(new PointsState());
	s->device = device; s->npts = npts; s->eps = eps; s->ntheta = ny; s->nphi = nx; s->from_map = true; s->ydouble = ydouble != 0;
	points_kernel_params(eps, &s->W, &s->beta);
	s->N1 = ydouble ? 2L*ny : ny;
	s->lmax = (int)(s->N1/2); s->mmax = nx/2;      // (the whole band: the tables reach the Nyquist frequency)
	s->n1 = fine_size(s->N1); s->n2 = fine_size(nx);
	s->nt1 = (int)(s->n1/PT_T); s->nt2 = (int)(s->n2/PT_T);
	PXS_REQUIRE((long)s->nt1*s->nt2 < (1L << 31), "pxm_plan_map_points: fine grid too large");
	s->d1 = upload(deapod_table(s->lmax, s->n1, s->W, s->beta));
	s->d2 = upload(deapod_table(s->mmax, s->n2, s->W, s->beta));
	PointsState* q = s.get();
	sort_points(q, [&](double2* xu, uint32_t* key, int* bad) {
		hipLaunchKernelGGL(mp_bin, dim3(nblocks(npts, 256)), dim3(256), 0, st, npts, d_pix, q->N1, (long)nx, q->n1, q->n2, q->W, q->nt2, xu, key, bad); },
		"pxm_plan_map_points: non-finite pixel coordinates", st);
	s->plan_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	return s.release();
}

bool points_from_map(const PointsState* s) { return s->from_map; }

// out[c][i] = the interpolant of map c at point i, for ncomp maps mstride elements apart (out: ostride), two maps per pass
void mappoints_run(PointsState* s, int ncomp, const void* maps, int mdt, long mstride, void* out, int odt, long ostride, hipStream_t st)
{
	const long npix = (long)s->ntheta*s->nphi;
	PXS_REQUIRE(ncomp <= 1 || ((mstride >= npix || mstride <= -npix) && (ostride >= s->npts || ostride <= -s->npts)), "pxm_map_points: the components overlap");
	if (s->npts == 0 || ncomp == 0) return;
	const long ncoarse = s->N1*s->nphi, nfine = s->n1*s->n2;
	const double scale = 1.0/((double)s->N1*s->nphi);
	try { s->cbuf.ensure(sizeof(double2)*ncoarse); s->fine.ensure(sizeof(double2)*nfine); }
	catch (const Error& e) {
		throw Error(e.code, "pxm_map_points: no memory for the grids of a pair of maps: coarse " + std::to_string(s->N1) + " x " + std::to_string(s->nphi) + " (" +
			std::to_string(sizeof(double2)*ncoarse) + " bytes), fine " + std::to_string(s->n1) + " x " + std::to_string(s->n2) + " (" + std::to_string(sizeof(double2)*nfine) + " bytes): " + e.what());
	}
	StageTimer timer{s, st};
	auto timed = [&](int stage, auto&& fn) { timer.run(stage, fn); };
	for (int c = 0; c < ncomp; c += 2) {
		const bool two = c + 1 < ncomp;
		const char* fa = (const char*)maps + dtype_bytes(mdt)*(size_t)c*mstride; const char* fb = two ? fa + dtype_bytes(mdt)*(size_t)mstride : nullptr;
		char* oa = (char*)out + dtype_bytes(odt)*(size_t)c*ostride; char* ob = two ? oa + dtype_bytes(odt)*(size_t)ostride : nullptr;
		timed(PT_ST_GRID, [&] { hipLaunchKernelGGL(mp_pack, dim3(nblocks(ncoarse, 256)), dim3(256), 0, st, s->ntheta, s->nphi, s->ydouble ? 1 : 0, (const void*)fa, (const void*)fb, mdt, s->cbuf.as<double2>()); });
		timed(PT_ST_FFT, [&] { fft2(s, st, s->N1, s->nphi, s->cbuf.as<double2>(), true); });
		timed(PT_ST_GRID, [&] { hipLaunchKernelGGL(mp_pad, dim3(nblocks(nfine, 256)), dim3(256), 0, st, s->n1, s->n2, s->N1, (long)s->nphi,
			s->cbuf.as<double2>(), s->d1.as<double>(), s->d2.as<double>(), scale, s->fine.as<double2>()); });
		timed(PT_ST_FFT, [&] { fft2(s, st, s->n1, s->n2, s->fine.as<double2>(), false); });
		timed(PT_ST_INTERP, [&] { hipLaunchKernelGGL(pt_interp, dim3(nblocks(s->npts, 256)), dim3(256), 0, st, s->npts, s->xs.as<double2>(), s->perm.as<int64_t>(),
			s->fine.as<double2>(), s->n1, s->n2, s->W, s->beta, (void*)oa, (void*)ob, odt); });
		PXS_HIP(hipGetLastError());
	}
	timer.collect();      // (profiling only: the one place a call waits for the device)
}

void points_profile(PointsState* s, bool on) { s->prof = on; for (int k = 0; k < PT_NSTAGE; k++) s->stage_ms[k] = 0; }

// per-point state and parameters (pxs_plan_query on a points plan)
int64_t points_query(const PointsState* s, const std::string& n) {
	if (n == "kernel_width") return s->W;
	if (n == "fine_ntheta") return s->n1;
	if (n == "fine_nphi") return s->n2;
	if (n == "npts") return s->npts;
	if (n == "plan_us") return (int64_t)std::llround(s->plan_ms*1e3);
	for (int k = 0; k < PT_NSTAGE; k++) if (n == std::string("stage_us_") + PT_STAGE_NAMES[k]) return (int64_t)std::llround(s->stage_ms[k]*1e3);
	throw Error(PXS_ERR_ARG, "pxs_plan_query: unknown name '" + n + "' for a points plan");
}

} // namespace pxs
