// SHT plans and pipelines (C-ABI pxs_* of include/pxsht.h) for gfx950.
//
//   synthesis        alm --Legendre--> leg[m][ring] --transpose*phase--> h[ring][m] --c2r ring FFT--> map
//   adjoint synth.   map --r2c ring FFT (pruned to m<=mmax)--> h[ring][m] --transpose*phase--> leg --Legendre^T--> alm
//   analysis_2d      map --ring FFT--> leg on the map's rings --theta resampling--> leg on a minimal
//                    Clenshaw-Curtis grid (lmax+2.. rings) incl. exact |sin| quadrature --Legendre^T--> alm
//   adj. analysis    the exact transpose of the above
//
// The theta resampling integrates the trigonometric interpolant exactly: mirror-extend each m
// column to the full circle with parity (-1)^(m+s), FFT, resize the spectrum onto a fine grid
// of M > N + 2 lmax points, multiply by the truncated Fourier series of |sin theta| there, FFT
// back, keep |k| <= lmax and evaluate on the CC grid.  All index remaps are fused into the FFT
// load/store functors (fft.hpp).
// flip_y / flip_x (curvedsky.map2buffer, curvedsky.py:1384-1411) are negative strides here.
#include "../../include/pxsht.h"
#include "fft.hpp"
#include "legendre.hpp"
#include "fftchain.hpp"
#include <map>
#include <memory>
#include <cmath>
#include <mutex>
#include <algorithm>

namespace pxs {

FftContext& fft_context(int device);
void fft_dense_lines(int device, hipStream_t st, long n, bool forward, long nlines, const double2* in, double2* out);   // api_fft.hip
void fft_release_stream(int device, hipStream_t st);                                                                  // api_fft.hip
const char* get_last_error();
// points plans (points.hip)
struct PointsState;
PointsState* points_create(int ntheta, int nphi, int lmax, int mmax, int device, long npts, const double* d_loc, double eps, hipStream_t st);
void points_free(PointsState* s);
void points_run(PointsState* s, pxs_plan* grid, int spin, int mode, int adjoint, int nb, const AlmArg& alm, const MapArg& map, hipStream_t st);
int64_t points_query(const PointsState* s, const std::string& name);
void points_profile(PointsState* s, bool on);

typedef long double LDb;
static const LDb PIl = 3.141592653589793238462643383279502884L;

struct GridInfo { long N; int c; bool ok; };
static GridInfo grid_info(const std::string& g, int n) {
	if (g == "CC")     return {2L*n-2, 0, true};
	if (g == "F1")     return {2L*n,   1, true};
	if (g == "MW")     return {2L*n-1, 1, true};
	if (g == "MWflip") return {2L*n-1, 0, true};
	// Driscoll-Healy (north pole + n-1 interior rings of spacing pi/n) and Fejer-2 (n interior rings of spacing pi/(n+1)): the
	// circle has sample points without a ring (a pole), so there is no interpolant to integrate: analysis on these grids is plain
	// quadrature with Fejer's second rule, exact up to get_ducc_maxlmax (curvedsky.py:1349-1353)
	if (g == "DH")     return {2L*n,   0, true};
	if (g == "F2")     return {2L*n+2, 2, true};
	return {0, 0, false};
}
static bool grid_weights_only(const std::string& g) { return g == "DH" || g == "F2"; }
// Fejer's second rule on K interior nodes theta_j = j pi/(K+1): w_j = 4 sin(theta_j)/(K+1) sum_{k=1}^{(K+1)/2} sin((2k-1) theta_j)/(2k-1)
// (ring weights, sum 2); the inner sum by the Chebyshev recurrence sin((2k+1)t) = 2 cos(2t) sin((2k-1)t) - sin((2k-3)t)
static std::vector<LDb> fejer2_weights(int K) {
	std::vector<LDb> w(K);
	for (int j = 1; j <= K; j++) {
		const LDb t = (LDb)j*PIl/(K+1), c2 = 2*cosl(2*t);
		LDb sm = -sinl(t), s0 = sinl(t), acc = 0;          // sin(-t), sin(t)
		for (int k = 1; k <= (K+1)/2; k++) { acc += s0/(2*k-1); const LDb sn = c2*s0 - sm; sm = s0; s0 = sn; }
		w[j-1] = 4*sinl(t)/(K+1)*acc;
	}
	return w;
}
static int grid_maxlmax(const std::string& g, int n) {
	if (g == "CC") return n-2;
	if (g == "DH") return (n-2)/2;
	if (g == "F2") return (n-1)/2;
	return n-1;
}
static std::vector<LDb> grid_theta(const std::string& g, int n) {
	GridInfo gi = grid_info(g, n);
	std::vector<LDb> th(n);
	for (int j = 0; j < n; j++) th[j] = (LDb)gi.c*PIl/gi.N + 2*PIl*j/gi.N;
	return th;
}
// Fourier coefficients of |sin|: s_q = -(2/pi)/(q^2-1) (q even), 0 (q odd)
static double abs_sin_coef(long q) { if (q & 1) return 0.0; LDb Q = q; return (double)(-(2/PIl)/(Q*Q-1)); }

// ---- glue kernels ----------------------------------------------------------------------
// out[b][c][r] = in[b][r][c] * tab[c] (optionally conj(tab)); 32x32 tiles through LDS
__global__ __launch_bounds__(256) void transpose_mul(const double2* __restrict__ in, double2* __restrict__ out,
		int nr, int nc, long in_bstride, long out_bstride, const double2* __restrict__ tab, int conj_tab, double scale)
{
	PXS_SHARED(double2, tile);   // [32][33]
	const int b = blockIdx.z;
	const int r0 = blockIdx.y*32, c0 = blockIdx.x*32;
	const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
	in += (long)b*in_bstride; out += (long)b*out_bstride;
	for (int j = ty; j < 32; j += 8) {
		const int r = r0 + j, c = c0 + tx;
		if (r < nr && c < nc) tile[j*33 + tx] = in[(long)r*nc + c];
	}
	__syncthreads();
	for (int j = ty; j < 32; j += 8) {
		const int c = c0 + j, r = r0 + tx;
		if (r < nr && c < nc) {
			double2 v = tile[tx*33 + j];
			if (tab) { double2 t = tab[c]; if (conj_tab) t.y = -t.y; v = make_double2(v.x*t.x - v.y*t.y, v.x*t.y + v.y*t.x); }
			v.x *= scale; v.y *= scale;
			out[(long)c*nr + r] = v;
		}
	}
}
// out[b][r][c] = in[b][c][r] * tab[c]: same kernel with roles swapped is enough (tab indexed by the OUTPUT column)
__global__ __launch_bounds__(256) void transpose_mul_outcol(const double2* __restrict__ in, double2* __restrict__ out,
		int nr, int nc, long in_bstride, long out_bstride, const double2* __restrict__ tab, int conj_tab, double scale, long ldin, long ldout)
{
	// in[b][c][r] (nc rows of length nr) -> out[b][r][c]
	PXS_SHARED(double2, tile);
	const int b = blockIdx.z;
	const int r0 = blockIdx.y*32, c0 = blockIdx.x*32;
	const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
	in += (long)b*in_bstride; out += (long)b*out_bstride;
	for (int j = ty; j < 32; j += 8) {
		const int c = c0 + j, r = r0 + tx;
		if (r < nr && c < nc) tile[j*33 + tx] = in[(long)c*ldin + r];
	}
	__syncthreads();
	for (int j = ty; j < 32; j += 8) {
		const int r = r0 + j, c = c0 + tx;
		if (r < nr && c < nc) {
			double2 v = tile[tx*33 + j];
			if (tab) { double2 t = tab[c]; if (conj_tab) t.y = -t.y; v = make_double2(v.x*t.x - v.y*t.y, v.x*t.y + v.y*t.x); }
			v.x *= scale; v.y *= scale;
			out[(long)r*ldout + c] = v;
		}
	}
}

// ring pairs were transformed as one complex line z = a + i b; rows hold Z[0..k] then Z[n-1..n-k] (k = mmax).
// X_a[m] = (Z[m] + conj(Z[n-m]))/2, X_b[m] = -i (Z[m] - conj(Z[n-m]))/2  ->  leg[b][m][2q], leg[b][m][2q+1], times tab[m]*scale.
__global__ __launch_bounds__(256) void unpack_pair_transpose(const double2* __restrict__ in, double2* __restrict__ out,
		int nr, int nm, long in_bstride, long out_bstride, const double2* __restrict__ tab, double scale)
{
	PXS_SHARED(double2, tile);   // two [32][33] tiles
	double2* tp = tile; double2* tm = tile + 32*33;
	const int b = blockIdx.z;
	const int q0 = blockIdx.y*32, m0 = blockIdx.x*32;
	const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
	const int npair = (nr + 1)/2, k = nm - 1, rowlen = 2*k + 1;
	in += (long)b*in_bstride; out += (long)b*out_bstride;
	for (int j = ty; j < 32; j += 8) {
		const int q = q0 + j, m = m0 + tx;
		if (q < npair && m < nm) {
			tp[j*33 + tx] = in[(long)q*rowlen + m];
			tm[j*33 + tx] = in[(long)q*rowlen + (m == 0 ? 0 : k + m)];
		}
	}
	__syncthreads();
	for (int j = ty; j < 32; j += 8) {
		const int m = m0 + j, q = q0 + tx;
		if (q < npair && m < nm) {
			const double2 zp = tp[tx*33 + j], zm = tm[tx*33 + j];
			// conj(zm) = (zm.x, -zm.y)
			double2 xa = make_double2(0.5*(zp.x + zm.x), 0.5*(zp.y - zm.y));
			double2 d  = make_double2(zp.x - zm.x, zp.y + zm.y);
			double2 xb = make_double2(0.5*d.y, -0.5*d.x);                 // -i d / 2
			const double2 t = tab[m];
			xa = make_double2((xa.x*t.x - xa.y*t.y)*scale, (xa.x*t.y + xa.y*t.x)*scale);
			xb = make_double2((xb.x*t.x - xb.y*t.y)*scale, (xb.x*t.y + xb.y*t.x)*scale);
			out[(long)m*nr + 2*q] = xa;
			if (2*q + 1 < nr) out[(long)m*nr + 2*q + 1] = xb;
		}
	}
}

// aliased rings (mmax >= nphi): leg[b][m][r] = h[b][r][m mod nphi] * tab[m]   (rare; simple gather)
__global__ __launch_bounds__(256) void gather_alias(const double2* __restrict__ in, double2* __restrict__ out,
		int nr, int nm, int ncin, int nphi, long in_bstride, long out_bstride, const double2* __restrict__ tab, double scale)
{
	const long idx = (long)blockIdx.x*blockDim.x + threadIdx.x;
	const int b = blockIdx.y;
	if (idx >= (long)nr*nm) return;
	const int m = (int)(idx / nr), r = (int)(idx - (long)m*nr);
	double2 v = in[(long)b*in_bstride + (long)r*ncin + (m % nphi)];
	const double2 t = tab[m];
	v = make_double2((v.x*t.x - v.y*t.y)*scale, (v.x*t.y + v.y*t.x)*scale);
	out[(long)b*out_bstride + idx] = v;
}

// ---- general ring sets (per-ring nphi, phi0, ringstart: healpix, profile rings; ducc's synthesis / adjoint_synthesis contract,
// curvedsky.py:328-349, 396-403, 537, 553, 936-960) ---------------------------------------------------------------------
// Rings are grouped by length; z holds one complex line per ring, group after group, so that every group is a dense
// [rings][n] block for one batched FFT.  A block of 256 threads works on 256 consecutive elements of one ring (blk_ring, blk_k0).
struct GenK {
	int nring, nm, nc; long ldleg, leg_cstride, zc, map_cstride, pix_stride;
	const int* blk_ring; const int* blk_k0; const int* nphi; const long* zoff; const long* rstart; const double* phi0;
	double scale;
};
// ring spectrum with aliasing: H[k] = sum_{m = k mod n, m <= mmax} f_m leg[m][r] e^{i m phi0_r}, f_0 = 1, f_m = 2: the real ring is
// Re of the backward DFT of H
__global__ __launch_bounds__(256) void gen_fold(const GenK g, const double2* __restrict__ leg, double2* __restrict__ z)
{
	const int r = g.blk_ring[blockIdx.x], k = g.blk_k0[blockIdx.x] + (int)threadIdx.x, c = blockIdx.y;
	const int n = g.nphi[r];
	if (k >= n) return;
	const double ph = g.phi0[r];
	const double2* col = leg + (long)c*g.leg_cstride + r;
	double ar = 0, ai = 0;
	for (int m = k; m < g.nm; m += n) {
		const double2 a = col[(long)m*g.ldleg];
		double sn, cs; sincos((double)m*ph, &sn, &cs);
		const double f = m ? 2.0 : 1.0;
		ar += f*(a.x*cs - a.y*sn); ai += f*(a.x*sn + a.y*cs);
	}
	z[(long)c*g.zc + g.zoff[r] + k] = make_double2(ar, ai);
}
template<class T> __global__ __launch_bounds__(256) void gen_scatter(const GenK g, const double2* __restrict__ z, T* __restrict__ map)
{
	const int r = g.blk_ring[blockIdx.x], j = g.blk_k0[blockIdx.x] + (int)threadIdx.x, c = blockIdx.y;
	if (j >= g.nphi[r]) return;
	map[(long)c*g.map_cstride + g.rstart[r] + (long)j*g.pix_stride] = (T)z[(long)c*g.zc + g.zoff[r] + j].x;
}
template<class T> __global__ __launch_bounds__(256) void gen_gather(const GenK g, const T* __restrict__ map, double2* __restrict__ z)
{
	const int r = g.blk_ring[blockIdx.x], j = g.blk_k0[blockIdx.x] + (int)threadIdx.x, c = blockIdx.y;
	if (j >= g.nphi[r]) return;
	z[(long)c*g.zc + g.zoff[r] + j] = make_double2((double)map[(long)c*g.map_cstride + g.rstart[r] + (long)j*g.pix_stride], 0.0);
}
// leg[m][r] = scale e^{-i m phi0_r} F_r[m mod n_r]
__global__ __launch_bounds__(256) void gen_unfold(const GenK g, const double2* __restrict__ z, double2* __restrict__ leg)
{
	const int r = blockIdx.x*256 + (int)threadIdx.x, c = blockIdx.z;
	if (r >= g.nring) return;
	const int n = g.nphi[r]; const double ph = g.phi0[r];
	const double2* line = z + (long)c*g.zc + g.zoff[r];
	for (int m = blockIdx.y; m < g.nm; m += gridDim.y) {
		const double2 a = line[m % n];
		double sn, cs; sincos((double)m*ph, &sn, &cs);
		leg[(long)c*g.leg_cstride + (long)m*g.ldleg + r] = make_double2(g.scale*(a.x*cs + a.y*sn), g.scale*(a.y*cs - a.x*sn));
	}
}

// leg[line][ring] *= w[ring] (DH / F2 analysis: plain quadrature weights)
__global__ __launch_bounds__(256) void scale_rings(double2* __restrict__ leg, long nlines, int nr, long ld, const double2* __restrict__ w)
{
	const long idx = (long)blockIdx.x*blockDim.x + threadIdx.x;
	if (idx >= nlines*nr) return;
	const long line = idx / nr; const int j = (int)(idx - line*nr);
	double2& v = leg[line*ld + j]; const double f = w[j].x;
	v.x *= f; v.y *= f;
}

// transpose of the parity mirror extension: out[line][j] = in[line][j] + sgn * in[line][mirror(j)], j < nr
// (self-mirrored samples -- pole rings -- are kept for even parity and dropped for odd parity)
__global__ __launch_bounds__(256) void fold_mirror(const double2* __restrict__ in, double2* __restrict__ out,
		int nr, long N, int c, long nlines, int par0)
{
	const long idx = (long)blockIdx.x*blockDim.x + threadIdx.x;
	if (idx >= nlines*nr) return;
	const long line = idx / nr; const int j = (int)(idx - line*nr);
	const bool odd = ((line + par0) & 1) != 0;
	long mj = N - j - c; if (mj >= N) mj -= N; if (mj < 0) mj += N;
	double2 v = in[line*N + j];
	if (mj == j) { if (odd) v = make_double2(0, 0); }
	else { const double2 w = in[line*N + mj]; if (odd) { v.x -= w.x; v.y -= w.y; } else { v.x += w.x; v.y += w.y; } }
	out[line*nr + j] = v;
}

// undo the pair packing of the theta-FFT chain: Z holds even(theta)+odd(theta) on the full circle of N points;
// out[line 2p + (even? ..)][j] = (Z[j] +- Z[mirror(j)])/2 * w[j] for the real rings j < nr.
__global__ __launch_bounds__(256) void split_pair(const double2* __restrict__ Z, double2* __restrict__ out,
		int nr, long N, int c, long npairs, long nlines, int par0, const double2* __restrict__ w, double scale)
{
	const long idx = (long)blockIdx.x*blockDim.x + threadIdx.x;
	if (idx >= npairs*nr) return;
	const long pr = idx / nr; const int j = (int)(idx - pr*nr);
	long mj = N - j - c; if (mj >= N) mj -= N; if (mj < 0) mj += N;
	const double2 z = Z[pr*N + j];
	double2 ev, od;
	if (mj == j) { ev = z; od = make_double2(0, 0); }
	else { const double2 y = Z[pr*N + mj]; ev = make_double2(0.5*(z.x + y.x), 0.5*(z.y + y.y)); od = make_double2(0.5*(z.x - y.x), 0.5*(z.y - y.y)); }
	const double f = scale*(w ? w[j].x : 1.0);
	ev.x *= f; ev.y *= f; od.x *= f; od.y *= f;
	const bool a_odd = (par0 & 1) != 0;
	const long la = 2*pr, lb = la + 1;
	out[la*nr + j] = a_odd ? od : ev;
	if (lb < nlines) out[lb*nr + j] = a_odd ? ev : od;
}

// split_pair fused with the transpose of leg2map (synthesis through the CC grid): Z[pair][N] -> h[ring][m] * conj(tab[m]) * scale,
// through a 32 (m) x 32 (ring) LDS tile; saves writing and re-reading leg[m][ring] (2 x 10 GB at config 3)
__global__ __launch_bounds__(256) void split_pair_transposed(const double2* __restrict__ Z, double2* __restrict__ out,
		int nr, int nm, long N, int c, int par0, const double2* __restrict__ tab, double scale)
{
	PXS_SHARED(double2, tile);                       // [32 m][33]
	const int r0 = blockIdx.y*32, m0 = blockIdx.x*32;
	const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // tx: ring within tile, ty: 0..7
	const bool a_odd = (par0 & 1) != 0;              // parity of column 0; m0 is even, so of every even column
	for (int pj = ty; pj < 16; pj += 8) {            // 16 pairs = 32 columns m0 + 2 pj, m0 + 2 pj + 1
		const long pr = (m0 >> 1) + pj; const int j = r0 + tx;
		double2 ev = make_double2(0, 0), od = make_double2(0, 0);
		if (j < nr && 2*pr < nm) {
			long mj = N - j - c; if (mj >= N) mj -= N; if (mj < 0) mj += N;
			const double2 z = Z[pr*N + j];
			if (mj == j) ev = z;
			else { const double2 y = Z[pr*N + mj]; ev = make_double2(0.5*(z.x + y.x), 0.5*(z.y + y.y)); od = make_double2(0.5*(z.x - y.x), 0.5*(z.y - y.y)); }
		}
		tile[(2*pj)*33 + tx] = a_odd ? od : ev;
		tile[(2*pj+1)*33 + tx] = a_odd ? ev : od;
	}
	__syncthreads();
	for (int j = ty; j < 32; j += 8) {
		const int r = r0 + j, m = m0 + tx;
		if (r < nr && m < nm) {
			const double2 v = tile[tx*33 + j];
			const double2 t = tab[m];
			out[(long)r*nm + m] = make_double2((v.x*t.x + v.y*t.y)*scale, (v.y*t.x - v.x*t.y)*scale);     // * conj(tab[m]) * scale
		}
	}
}

} // namespace pxs

using namespace pxs;

// How one pxs_synthesis / pxs_analysis call runs.  route_of() decides it ONCE per call, from the plan and the call's arguments; the
// scratch of the call (reserve_call), its batching, the stages it launches (run_core) and the queries all read this one object.
enum RouteKind {
	R_DIRECT,             // synthesis / its adjoint: Legendre stage on the map's own rings
	R_VIA_CC,             // ... on the minimal CC grid, fused theta chain between that grid and the map's rings (grids, bands of F1 grids)
	R_VIA_CC_UNFUSED,     // ... theta resampling through the generic FFT engine (no fused theta chain for this size), one map at a time
	R_VIA_CC_UNFUSED_H,   // ... whose last stage writes the ring-major h directly (plans without a ring chain)
	R_RING_WEIGHTS,       // analysis: quadrature weights on the map's rings + adjoint synthesis there (DH / F2; the weights form off the CC detour)
	R_CC_WEIGHTS,         // analysis: ring weights, transposed theta upsampling, Legendre stage on the CC grid (the weights form with fused chains)
	R_CHAIN,              // analysis: exact quadrature of the theta-interpolant through the fused chains (to_cc / to_cc_adjoint)
	R_UNFUSED };          // analysis: ... through the generic FFT engine on dense rows, one map at a time
static const char* const ROUTE_NAMES[] = {"direct", "via-cc", "via-cc-unfused", "via-cc-unfused-h", "ring-weights", "cc-weights", "chain", "unfused"};
// the theta operation of a route; the values are the `kind` of FftChain::theta_scratch
enum ThetaOp { TH_NONE = -1, TH_TO_CC = 0, TH_FROM_CC_ADJ = 1, TH_FROM_CC = 2, TH_TO_CC_ADJ = 3 };
struct Route {
	RouteKind kind = R_DIRECT;
	bool to_map = true;            // alm -> map (synthesis, adjoint analysis) or map -> alm
	bool batched = true;           // may take several maps per pass (batch_chunk); false: one map at a time
	int nc = 1, deriv1 = 0;        // map components per map
	const LegTables* tb = nullptr;       // (null in the routes the queries make: they size nothing)
	const RingSet* rs = nullptr;         // ring set of the Legendre stage: the plan's rs_map (buffer leg) or rs_cc (buffer leg2)
	// row strides of leg[c][m][ring], leg2[c][m][cc ring], h[c][ring][m] (padded to whole 128-byte lines on the fused routes, dense on
	// the unfused ones; 0: the route does not touch that buffer) and the rings of h per component
	long ld_leg = 0, ld_leg2 = 0, ld_h = 0; int nr_h = 0;
	long ld_leg_alloc = 0;         // leg is SIZED for rows of this stride: ld_leg but for the CC-grid synthesis, see route_of
	// theta operation between the map's grid (nr_th rings: the whole grid for a band) and the CC grid, with the tables of its form
	ThetaOp theta = TH_NONE; bool theta_fused = false, line = false;      // line: the single-kernel engine takes it (thetaline.hip; no intermediates)
	int nr_th = 0; const ThetaPlan* tp = nullptr; const double2 *sigma = nullptr, *wcc = nullptr, *whalf = nullptr; long M = 0; bool fine = false;
	bool reserve_chain = false;    // the call reserves the ping-pong scratch of the plan's FFT chains
	// bytes the call needs for nb maps per pass: the plan's leg / leg2 / hbuf, the Legendre work arrays, the chain's ping-pong scratch
	struct Scratch { size_t leg = 0, leg2 = 0, h = 0, almt = 0, mom = 0, c1 = 0, c2 = 0, r1 = 0; };
	Scratch scratch(const pxs_plan* p, int nb) const;
};

struct pxs_plan {
	// a plan serves one call at a time (it owns the scratch of the call, and the analysis option is read several times in a call):
	// the entry points that run or reconfigure it take this lock, so two host threads on one cached plan queue up instead of interleaving
	std::mutex call_mu;
	// ... on the device too: the calls are asynchronous, so the lock orders only their issue.  Every call records `used` on its stream
	// after its last launch, and a call that comes on another stream waits for it before its first (PlanUse below): calls on one plan
	// run in the order they were issued, whatever their streams.
	hipEvent_t used = nullptr; hipStream_t used_stream = nullptr; bool used_any = false;
	int device = 0;
	bool is_grid = false;
	std::string geometry;
	int nring = 0, nphi = 0;
	// rows of a larger F1 grid (declination bands through pxs_plan_rings): the grid has nfull rings, the map's first ring is its
	// ring row0.  Such plans share the CC-grid machinery of the grid plans for synthesis and its adjoint.  Grid plans: nfull = nring.
	int nfull = 0, row0 = 0; bool band = false;
	double phi0 = 0;
	long ring_off0 = 0, ring_stride = 0, pix_stride = 1;   // user-map offset of (ring r, pixel x) = ring_off0 + r*ring_stride + x*pix_stride
	int lmax = 0, mmax = 0; long lstride = 1;
	DevBuf d_mstart;
	RingSet rs_map, rs_cc;
	std::map<int, std::unique_ptr<LegTables>> tables;
	LegWork wk;
	DevBuf leg, leg2, hbuf, phase;
	// analysis resampling (grid plans)
	long N = 0; int mir_c = 0; long M = 0, Ncc = 0; int ncc = 0;
	DevBuf ph_shift, ph_up, sigma, wcc, wadj, whalf, b1, b2;
	// general ring sets (gen_* kernels): rings of equal length are one dense block of z
	struct GenGroup { long n, count, zoff; };
	bool general = false; std::vector<GenGroup> groups; long npixz = 0;
	DevBuf g_blk_ring, g_blk_k0, g_nphi, g_zoff, g_rstart, g_phi0, gz; long g_nblk = 0;
	std::vector<hipStream_t> gstreams; std::vector<hipEvent_t> gjoin; hipEvent_t gfork = nullptr;
	// points plans (pxs_plan_points): the CC grid plan they were made from (owned by the caller) and the per-point state
	pxs_plan* pgrid = nullptr; PointsState* pts = nullptr;
	~pxs_plan() {
		if (pts) points_free(pts);
		if (used) (void)hipEventDestroy(used);
		for (auto s_ : gstreams) { pxs::fft_release_stream(device, s_); (void)hipStreamDestroy(s_); }
		for (auto e : gjoin) (void)hipEventDestroy(e);
		if (gfork) (void)hipEventDestroy(gfork);
	}
	DevBuf wring;                // DH / F2 grids: per-ring quadrature weight / nphi (analysis = weighted adjoint synthesis)
	int ana_weights = 2;         // pxs_plan_option("analysis"): 2 = ducc0's route (default: the fine-CC form; ring weights on CC grids with ntheta >= 2 lmax + 2),
	                             // 0 = interpolant (|sin| series on the M circle), 1 = ring weights + adjoint synthesis where ntheta >= 2 lmax + 2;
	                             // PXS_ANALYSIS=ducc0|interpolant|weights presets it
	// the fine-CC form of the analysis (ducc0's resample_to_prepared_CC as published: the theta-interpolant, low-passed where the grid
	// has more than 2 N_cc circle samples, is evaluated on the CC grid of N_cc + 1 rings, multiplied by that grid's quadrature weights
	// and carried to the N_cc/2 + 1 rings of the Legendre stage by the transposed upsampling): the chain of the interpolant form with
	// M = 2 N_cc and the weights as the pointwise table
	ThetaPlan tpf; DevBuf sigma_f, wcc_f, whalf_f; long Mf = 0;      // tpf.ok: through the fused chains; Mf > 0: the tables exist (the unfused engine takes any plan)
	DevBuf wgrid, wgrid_ext, wunit_ext;     // ... its weights: get_gridweights / nphi per ring (built on first use); _ext: self-mirrored rings doubled (ring_weights_ext)
	bool syn_via_cc = false, syn_via_cc0 = false;      // synthesis through the CC grid: spin s / spin 0 (the recurrence of spin 0 is 4x cheaper per ring, the resampling is not)
	bool ring_pairs = true;      // transform two real rings per complex FFT (PXS_RING_PAIRS=0 disables)
	FftContext* fc = nullptr;
	// fused FFT chains (fftchain.hip).  chain_rings: ring FFTs through MA1/MA2, MS1/MS2; tp.ok: theta resampling through RA1-5 / RS1-3.
	// These say what the plan CAN do; which of it a call uses, and with which row strides (padded to whole 128-byte lines on the chain
	// routes, dense on the unfused ones kept for aliased rings and lengths without a usable factorisation), is the call's Route.
	std::unique_ptr<FftChain> chain; ThetaPlan tp; bool chain_rings = false;
	bool chain_theta() const { return chain_rings && tp.ok; }
	long ld_map() const { return chain_rings ? FftChain::pad8(nring) : nring; }
	long ld_cc()  const { return chain_theta() ? FftChain::pad8(ncc) : ncc; }
	long ld_h()   const { return chain_rings ? FftChain::pad8(mmax + 1) : mmax + 1; }
	FftChain::MapDesc map_desc(const MapArg& a, int ncb = 0) const {
		FftChain::MapDesc m; m.ptr = a.ptr; m.dtype = a.dtype; m.cstride = a.cstride; m.ring_off0 = ring_off0; m.ring_stride = ring_stride; m.pix_stride = pix_stride; m.nring = nring; m.nphi = nphi;
		m.bstride = a.bstride; m.ncb = ncb;
		return m; }
	LegProfile prof;
	size_t resample_chunk_bytes = size_t(1) << 40;    // per intermediate buffer of the theta-FFT chain (chunking to stay in the
	                                                  // Infinity Cache was measured slower: 22.4 -> 26.2 ms at config 2; PXS_RESAMPLE_MB re-enables it)

	LegTables& table(int spin) {
		auto& p = tables[spin];
		if (!p) { p.reset(new LegTables()); p->build(lmax, mmax, spin); }
		return *p;
	}
	// Legendre stage of a route for nb maps: alm -> the route's buffer on its ring set with its row stride (rs_map: leg, rs_cc: leg2) ...
	DevBuf& leg_buf(const Route& r) { return r.rs == &rs_cc ? leg2 : leg; }
	void leg_syn(hipStream_t st, const Route& r, const AlmArg& a, int nb) {
		const long ld = r.rs == &rs_cc ? r.ld_leg2 : r.ld_leg;
		leg_synthesis(st, *r.rs, *r.tb, wk, a.ptr, a.dtype, a.cstride, d_mstart.as<uint64_t>(), lstride, leg_buf(r).as<double2>(), r.deriv1, &prof, ld, nb, a.bstride, (long)r.nc*(mmax + 1)*ld);
	}
	// ... and its transpose
	void leg_ana(hipStream_t st, const Route& r, const AlmArg& a, int nb) {
		const long ld = r.rs == &rs_cc ? r.ld_leg2 : r.ld_leg;
		leg_analysis(st, *r.rs, *r.tb, wk, leg_buf(r).as<double2>(), a.ptr, a.dtype, a.cstride, d_mstart.as<uint64_t>(), lstride, r.deriv1, &prof, ld, nb, a.bstride, (long)r.nc*(mmax + 1)*ld);
	}
	// the fused theta operation of a route on nct components: leg <-> leg2 (analysis side), leg2 -> h (synthesis side); wring: optional weight per ring of the map
	void run_theta(hipStream_t st, const Route& r, int nct, int spin, const double2* wring) {
		const int nm = mmax + 1;
		double2 *l1 = leg.as<double2>(), *l2 = leg2.as<double2>(), *h = hbuf.as<double2>();
		prof.begin(st, PXS_STAGE_RESAMPLE);
		switch (r.theta) {
		case TH_TO_CC:       chain->to_cc(st, *r.tp, l1, r.ld_leg, r.nr_th, mir_c, l2, r.ld_leg2, ncc, nct, nm, spin, lmax, ph_shift.as<double2>(), r.sigma, r.wcc); break;
		case TH_FROM_CC_ADJ: chain->from_cc_adjoint(st, *r.tp, l1, r.ld_leg, r.nr_th, mir_c, l2, r.ld_leg2, ncc, nct, nm, spin, lmax, ph_shift.as<double2>(), wadj.as<double2>(), wring); break;
		case TH_FROM_CC:     chain->from_cc(st, *r.tp, l2, r.ld_leg2, ncc, h, r.ld_h, r.nr_h, mir_c, nct, nm, spin, lmax, ph_up.as<double2>(), phase.as<double2>(), 1.0/(double)Ncc, wring); break;
		case TH_TO_CC_ADJ:   chain->to_cc_adjoint(st, *r.tp, l2, r.ld_leg2, ncc, h, r.ld_h, r.nr_h, mir_c, nct, nm, spin, lmax, ph_shift.as<double2>(), r.sigma, r.whalf, phase.as<double2>(), 2.0); break;
		case TH_NONE: break;
		}
		prof.end(st, PXS_STAGE_RESAMPLE);
	}
};

Route::Scratch Route::scratch(const pxs_plan* p, int nb) const {
	Scratch s; const size_t nct = (size_t)nb*nc, nm = (size_t)p->mmax + 1, c16 = sizeof(double2);
	s.leg = c16*nct*nm*ld_leg_alloc; s.leg2 = c16*nct*nm*ld_leg2; s.h = c16*nct*nr_h*ld_h;
	if (to_map) s.almt = sizeof(double)*4*(tb->nrows + 4)*nb; else s.mom = sizeof(double)*4*std::max<long>(tb->nrows, 1)*nb;
	if (theta_fused && !line) FftChain::theta_scratch(*tp, (int)nm, (int)nct, theta, s.c1, s.c2);
	if (reserve_chain) p->chain->ring_scratch(p->nring, (int)nct, !to_map, s.r1, p->mmax);
	return s;
}

namespace {

// One call on a plan (call_mu held, the plan's device selected): waits, on the call's stream, for the plan's previous call where that
// ran on another stream, and records the plan's last use when the call has issued its launches (also when it ends in an exception:
// what it launched up to there uses the scratch all the same).
struct PlanUse {
	pxs_plan* p; hipStream_t st;
	PlanUse(pxs_plan* p_, hipStream_t st_) : p(p_), st(st_) {
		if (p->used_any && st != p->used_stream) PXS_HIP(hipStreamWaitEvent(st, p->used, 0));
	}
	~PlanUse() {
		if (!p->used && hipEventCreateWithFlags(&p->used, hipEventDisableTiming) != hipSuccess) p->used = nullptr;
		if (p->used && hipEventRecord(p->used, st) == hipSuccess) { p->used_stream = st; p->used_any = true; }
		else { (void)hipStreamSynchronize(st); p->used_any = false; }      // (no event: the call is complete before the next one starts)
	}
	PlanUse(const PlanUse&) = delete; PlanUse& operator=(const PlanUse&) = delete;
};

void plan_common(pxs_plan* p, int lmax, int mmax, const uint64_t* mstart, int64_t lstride, int device) {
	PXS_REQUIRE(lmax >= 0 && mmax >= 0 && mmax <= lmax, "need 0 <= mmax <= lmax");
	PXS_REQUIRE(mstart != nullptr, "mstart is required");
	PXS_HIP(hipSetDevice(device));
	p->device = device; p->lmax = lmax; p->mmax = mmax; p->lstride = lstride;
	std::vector<uint64_t> ms(mstart, mstart+mmax+1);
	p->d_mstart = upload(ms);
	p->fc = &fft_context(device);
	{ const char* e = getenv("PXS_FFT_TEMP_MB"); if (e) p->fc->temp_budget = (size_t)atol(e) << 20; }
	{ const char* e = lab_getenv("PXS_RING_PAIRS"); if (e) p->ring_pairs = atoi(e) != 0; }
	{	// scratch for the per-wave partial moments of the analysis: 16 GiB where the device has room (MI355X: 288 GB),
		// never more than 1/8 of what is free now.  Measured at config 3: 4 GiB 448.8, 8 GiB 442.7, 16 GiB 438.0, 24 GiB 437.7 ms.
		size_t fr = 0, tot = 0;
		if (hipMemGetInfo(&fr, &tot) == hipSuccess && fr > 0) p->wk.part_budget = std::min<size_t>(size_t(2) << 30, std::max<size_t>(fr/8, size_t(256) << 20));      // (ordered analysis only: <= 2 GB of partial moments, m in chunks)
		const char* e = getenv("PXS_PART_GB"); if (e) p->wk.part_budget = (size_t)atol(e) << 30;
		{ const char* d = getenv("PXS_DETERMINISTIC"); p->wk.deterministic = d && atoi(d) != 0; }      // default of pxs_plan_option("deterministic")
	}
	{ const char* e = getenv("PXS_RESAMPLE_MB"); if (e) p->resample_chunk_bytes = (size_t)atol(e) << 20; }
	{ const char* e = getenv("PXS_ANALYSIS"); if (e) { const std::string v(e); p->ana_weights = v == "weights" ? 1 : (v == "ducc0" ? 2 : (v == "interpolant" ? 0 : p->ana_weights)); } }
	if (p->general) return;      // per-ring lengths and phases: see setup_general
	std::string why;
	if (!FftContext::supported(p->nphi, &why)) throw Error(PXS_ERR_UNSUPPORTED, why);
	// e^{-i m phi0}
	std::vector<double2> ph(mmax+1);
	for (int m = 0; m <= mmax; m++) { LDb a = (LDb)m*(LDb)p->phi0; ph[m] = make_double2((double)cosl(a), (double)(-sinl(a))); }
	p->phase = upload(ph);
	{	static const bool use = [] { const char* e = lab_getenv("PXS_CHAIN"); return e ? atoi(e) != 0 : true; }();
		p->chain.reset(new FftChain(p->fc));
		p->chain_rings = use && p->ring_pairs && 2L*mmax < p->nphi && p->chain->plan_rings(p->nphi);
		if (getenv("PXS_CHAIN_VERBOSE")) fprintf(stderr, "[pxsht] ring chain nphi=%d mmax=%d: %s\n", p->nphi, mmax, p->chain_rings ? p->chain->describe().c_str() : "off");
	}
}

void setup_resampling(pxs_plan* p) {
	if (p->nfull == 0) p->nfull = p->nring;
	GridInfo gi = grid_info(p->geometry, p->nfull);
	p->N = gi.N; p->mir_c = gi.c;
	const int lmax = p->lmax;
	p->Ncc = FftContext::good_size(std::max<long>(2L*lmax + 2, 4));
	if (p->Ncc & 1) p->Ncc = FftContext::good_size(p->Ncc + 1);
	while (p->Ncc & 1) p->Ncc = FftContext::good_size(p->Ncc + 1);
	{	// ducc0's own N_cc = 2 good_size_complex(lmax + 1) where the FFT engine takes it and twice it (the fused chains decide for themselves below)
		static const bool ducc_size = [] { const char* e = lab_getenv("PXS_THETA_DUCC_NCC"); return e ? atoi(e) != 0 : true; }();
		const long nd = FftChain::ducc_ncc(lmax);
		if (ducc_size && nd >= 4 && FftContext::supported(nd) && FftContext::supported(2*nd)) p->Ncc = nd;
	}
	p->M = FftContext::good_size(p->N + 2L*lmax + 2);
	{ const char* e = lab_getenv("PXS_M_FINE"); if (e && atol(e) >= p->M && FftContext::supported(atol(e))) p->M = atol(e); }   // experiments: a larger fine grid with friendlier factors
	if (p->chain_rings) {	// the fused theta chains need N, M and Ncc to share a modulus: let their planner pick M and Ncc
		p->tp = FftChain::plan_theta(p->N, lmax);
		if (p->tp.ok) { p->Ncc = p->tp.Ncc; p->M = p->tp.M; }
		if (getenv("PXS_CHAIN_VERBOSE")) fprintf(stderr, "[pxsht] theta chain N=%ld lmax=%d: ok=%d g=%ld bN=%ld g2=%ld (M=%ld) ac=%ld (Ncc=%ld) | syn gs=%ld bs=%ld aNs=%ld\n",
			p->N, lmax, (int)p->tp.ok, p->tp.g, p->tp.bN, p->tp.g2, p->tp.M, p->tp.ac, p->tp.Ncc, p->tp.gs, p->tp.bs, p->tp.aNs);
	}
	p->ncc = (int)(p->Ncc/2 + 1);
	std::string why;
	if (!FftContext::supported(p->N, &why)) throw Error(PXS_ERR_UNSUPPORTED, why);
	// CC ring set
	std::vector<LDb> th(p->ncc);
	for (int j = 0; j < p->ncc; j++) th[j] = 2*PIl*j/p->Ncc;
	th[p->ncc-1] = PIl;
	p->rs_cc.build(th); p->rs_cc.upload_all();
	// shift phases e^{-i k theta0}, k = 0..N/2
	const LDb th0 = (LDb)gi.c*PIl/gi.N;
	std::vector<double2> ps(p->N/2 + 1);
	for (long k = 0; k <= p->N/2; k++) { LDb a = (LDb)k*th0; ps[k] = make_double2((double)cosl(a), (double)(-sinl(a))); }
	p->ph_shift = upload(ps);
	{ std::vector<double2> pu(ps.size()); for (size_t k = 0; k < ps.size(); k++) pu[k] = make_double2(ps[k].x, -ps[k].y); p->ph_up = upload(pu); }
	// synthesis: Legendre on the minimal CC grid + exact Fourier upsampling in theta pays once the map has clearly more rings
	// (measured: at nring / ncc = 1.33 -- C2, C4 -- the detour pays for spin 2 and costs 11 ms per 64 scalar maps at C4)
	// (a band: what counts is the ring-pair slots of its own rings, unpaired rings take a whole slot)
	{ const char* e = lab_getenv("PXS_SYN_VIA_CC"); const long rings = p->band ? 2L*p->rs_map.npairs : p->nring;
	  p->syn_via_cc = e ? atoi(e) != 0 : (rings > p->ncc + p->ncc/4);
	  p->syn_via_cc0 = e ? atoi(e) != 0 : (rings > p->ncc + p->ncc/2); }
	// sigma_i = sum_{|q|<=Ks} s_q e^{i q theta_i} on the M grid, via one device FFT
	const long Ks = lmax + p->N/2;
	PXS_REQUIRE(2*Ks < p->M, "internal: fine grid too small");
	std::vector<double2> spec(p->M, make_double2(0, 0));
	for (long q = 0; q <= Ks; q++) { double s = abs_sin_coef(q); spec[q].x = s; if (q > 0) spec[p->M - q].x = s; }
	DevBuf dspec = upload(spec);
	p->sigma.alloc(sizeof(double2)*p->M);
	FftDims d; d.n_i = 1; d.is_e = 1; d.os_e = 1;
	FftLoad ld; ld.ptr = dspec.p; FftStore st; st.ptr = p->sigma.p;
	p->fc->exec(nullptr, p->M, false, d, ld, st);
	PXS_HIP(hipStreamSynchronize(nullptr));
	// CC weights incl. all FFT normalisations: (pi/nphi)(2pi/Ncc) eps_j / (N M)
	std::vector<double2> w(p->ncc);
	for (int j = 0; j < p->ncc; j++) {
		LDb e = (j == 0 || j == p->ncc-1) ? 1 : 2;
		w[j] = make_double2((double)((PIl/p->nphi)*(2*PIl/p->Ncc)*e/((LDb)p->N*(LDb)p->M)), 0.0);
	}
	p->wcc = upload(w);
	{	// the same weights for the fused adjoint of the analysis (FftChain::to_cc_adjoint): halved off the two pole rings
		std::vector<double2> wh(w); for (int j = 1; j + 1 < p->ncc; j++) wh[j].x *= 0.5;
		p->whalf = upload(wh); }
	{	// weights of the transposed theta upsampling (FftChain::from_cc_adjoint): 1/N_cc, half at the two pole rings
		std::vector<double2> wa(p->ncc);
		for (int j = 0; j < p->ncc; j++) wa[j] = make_double2(((j == 0 || j == p->ncc-1) ? 0.5 : 1.0)/(double)p->Ncc, 0.0);
		p->wadj = upload(wa); }
	if (FftContext::supported(2*p->Ncc)) {	// the fine-CC form: M = 2 N_cc (through the fused chains: = g * (2 ac))
		if (p->tp.ok && FftChain::sub_ok_theta(2*p->tp.ac)) { p->tpf = p->tp; p->tpf.g2 = 2*p->tp.ac; p->tpf.M = 2*p->Ncc; } else p->tpf.ok = false;
		const long Mf = p->Mf = 2*p->Ncc; const int nf = (int)(Mf/2 + 1);
		std::vector<double> gw(nf);
		if (pxs_gridweights("CC", nf, gw.data()) != 0) throw Error(PXS_ERR_ARG, get_last_error());
		// table on the circle: (Mf / 2 pi) x the weight of the full-circle rule int g |sin| = sum_i t_i g(theta_i): ring weight
		// (sum over the rings = 2) at both images of a ring, twice that at the two poles, which the circle holds once
		std::vector<double2> sg(Mf);
		for (long i = 0; i < Mf; i++) {
			const long r = std::min(i, Mf - i);
			const LDb wr = (LDb)gw[r]/(2*PIl)*((r == 0 || r == Mf/2) ? 2 : 1);
			sg[i] = make_double2((double)(wr*(LDb)Mf/(2*PIl)), 0.0);
		}
		p->sigma_f = upload(sg);
		const double f = (double)p->M/(double)Mf;       // the FFT normalisation 1/(N M) of the weights, for this M
		std::vector<double2> wf(w), whf(w);
		for (int j = 0; j < p->ncc; j++) { wf[j].x *= f; whf[j].x *= (j == 0 || j == p->ncc-1) ? f : 0.5*f; }
		p->wcc_f = upload(wf); p->whalf_f = upload(whf);
	}
}

// tables of a general ring set: groups of equal length, z offsets, the block table of the gen_* kernels
void setup_general(pxs_plan* p, int nring, const uint64_t* nphi, const double* phi0, const uint64_t* ringstart) {
	std::vector<int> order(nring);
	for (int r = 0; r < nring; r++) { order[r] = r; PXS_REQUIRE(nphi[r] >= 1 && nphi[r] < (1ull << 31), "pxs_plan_rings: bad nphi"); }
	std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return nphi[a] < nphi[b]; });
	std::vector<int> np(nring), blk_ring, blk_k0; std::vector<long> zoff(nring), rstart(nring); std::vector<double> ph(phi0, phi0 + nring);
	long off = 0;
	p->groups.clear();
	for (int i = 0; i < nring; i++) {
		const int r = order[i];
		np[r] = (int)nphi[r]; rstart[r] = (long)ringstart[r]; zoff[r] = off;
		if (p->groups.empty() || p->groups.back().n != (long)nphi[r]) p->groups.push_back(pxs_plan::GenGroup{(long)nphi[r], 0, off});
		p->groups.back().count++;
		for (long k0 = 0; k0 < (long)nphi[r]; k0 += 256) { blk_ring.push_back(r); blk_k0.push_back((int)k0); }
		off += (long)nphi[r];
	}
	p->npixz = off; p->g_nblk = (long)blk_ring.size();
	p->g_blk_ring = upload(blk_ring); p->g_blk_k0 = upload(blk_k0); p->g_nphi = upload(np); p->g_zoff = upload(zoff);
	p->g_rstart = upload(rstart); p->g_phi0 = upload(ph);
	if (p->groups.size() >= 8) {
		static const int ns = [] { const char* e = lab_getenv("PXS_GEN_STREAMS"); return e ? std::max(0, atoi(e)) : 16; }();
		p->gstreams.resize(ns); p->gjoin.resize(ns);
		for (int i = 0; i < ns; i++) { PXS_HIP(hipStreamCreateWithFlags(&p->gstreams[i], hipStreamNonBlocking)); PXS_HIP(hipEventCreateWithFlags(&p->gjoin[i], hipEventDisableTiming)); }
		PXS_HIP(hipEventCreateWithFlags(&p->gfork, hipEventDisableTiming));
	}
}
static GenK gen_args(pxs_plan* p, int nc, long ldleg, long map_cstride, double scale) {
	GenK g; g.nring = p->nring; g.nm = p->mmax + 1; g.nc = nc; g.ldleg = ldleg; g.leg_cstride = (long)(p->mmax + 1)*ldleg; g.zc = p->npixz;
	g.map_cstride = map_cstride; g.pix_stride = p->pix_stride;
	g.blk_ring = p->g_blk_ring.as<int>(); g.blk_k0 = p->g_blk_k0.as<int>(); g.nphi = p->g_nphi.as<int>(); g.zoff = p->g_zoff.as<long>();
	g.rstart = p->g_rstart.as<long>(); g.phi0 = p->g_phi0.as<double>(); g.scale = scale;
	return g;
}
// one batched FFT per (component, length).  A healpix map has 2 nside lengths with two to four rings each: the launches are
// dealt round-robin to side streams that fork from / join the caller's stream, so that the many small transforms overlap
// (nside 2048, lmax 4096, 3 components: 282 ms on one stream, 94 ms on 16)
static void gen_ffts(pxs_plan* p, hipStream_t st, int nc, bool forward) {
	const size_t njobs = (size_t)nc*p->groups.size();
	const size_t ns = njobs >= 16 ? p->gstreams.size() : 0;
	if (ns) {
		PXS_HIP(hipEventRecord(p->gfork, st));
		for (size_t i = 0; i < ns; i++) PXS_HIP(hipStreamWaitEvent(p->gstreams[i], p->gfork, 0));
	}
	size_t job = 0;
	for (int c = 0; c < nc; c++)
		for (const auto& gr : p->groups) {
			double2* zl = p->gz.as<double2>() + (size_t)c*p->npixz + gr.zoff;
			fft_dense_lines(p->device, ns ? p->gstreams[job % ns] : st, gr.n, forward, gr.count, zl, zl);
			job++;
		}
	for (size_t i = 0; i < ns; i++) { PXS_HIP(hipEventRecord(p->gjoin[i], p->gstreams[i])); PXS_HIP(hipStreamWaitEvent(st, p->gjoin[i], 0)); }
}

int ncomp_of(int spin, int mode, bool alm_side) {
	if (mode == PXS_MODE_DERIV1) return alm_side ? 1 : 2;
	return spin == 0 ? 1 : 2;
}

// ring FFT of the nb maps of a pass: user map -> hbuf[c][ring][m] -> leg[c][m][ring] * e^{-i m phi0}
// (row stride of leg: the route's ld_leg; the unfused path below only writes dense rows, ld_leg == nring)
void map2leg(pxs_plan* p, hipStream_t st, const Route& r, const MapArg& m, int nb, double2* leg) {
	p->prof.begin(st, PXS_STAGE_RING_FFT);
	const int nm = p->mmax+1, nr = p->nring, nc = nb*r.nc, ncb = nb > 1 ? r.nc : 0;
	const long ldl = r.ld_leg;
	if (p->general) {
		PXS_REQUIRE(ncb == 0, "internal: general ring sets take one map per call");
		p->gz.ensure(sizeof(double2)*(size_t)nc*p->npixz);      // (general ring sets size their own z here)
		const GenK g = gen_args(p, nc, ldl, m.cstride, 1.0);
		const dim3 grid((unsigned)p->g_nblk, nc);
		if (m.dtype == PX_F32) hipLaunchKernelGGL(gen_gather<float>, grid, dim3(256), 0, st, g, (const float*)m.ptr, p->gz.as<double2>());
		else                     hipLaunchKernelGGL(gen_gather<double>, grid, dim3(256), 0, st, g, (const double*)m.ptr, p->gz.as<double2>());
		gen_ffts(p, st, nc, true);
		hipLaunchKernelGGL(gen_unfold, dim3((nr + 255)/256, std::min(nm, 4096), nc), dim3(256), 0, st, g, (const double2*)p->gz.p, leg);
		p->prof.end(st, PXS_STAGE_RING_FFT);
		PXS_HIP(hipGetLastError());
		return;
	}
	if (p->chain_rings) {
		p->chain->map2leg(st, p->map_desc(m, ncb), nc, p->mmax, leg, ldl, p->phase.as<double2>(), 1.0);
		p->prof.end(st, PXS_STAGE_RING_FFT);
		return;
	}
	PXS_REQUIRE(ldl == nr && ncb == 0, "internal: unfused ring FFT needs dense rows and single maps");
	auto esz = [](int dt) { return dt == PX_F32 ? 4 : 8; };
	// (the unfused ring FFT of a map sizes its own packed spectra in hbuf, here and below)
	if (2L*p->mmax < p->nphi && p->ring_pairs) {
		// two real rings per complex transform; the pruned two-sided spectrum (|k| <= mmax) is unpacked in the transpose
		const int npair = (nr + 1)/2; const long rowlen = 2L*p->mmax + 1;
		p->hbuf.ensure(sizeof(double2)*(size_t)nc*std::max<size_t>((size_t)npair*rowlen, (size_t)nr*nm));
		FftDims d; d.n_i = npair; d.is_i = p->ring_stride; d.os_i = rowlen; d.n_o1 = nc; d.is_o1 = m.cstride; d.os_o1 = (long)npair*rowlen;
		d.is_e = p->pix_stride; d.os_e = 1;
		FftLoad ld; ld.ptr = (const char*)m.ptr + esz(m.dtype)*p->ring_off0; ld.dtype = m.dtype; ld.mode = LD_REAL_PAIR; ld.pair_lines = nr;
		FftStore sf; sf.ptr = p->hbuf.p; sf.two_sided_k = p->mmax; sf.compact_two_sided = 1;
		p->fc->exec(st, p->nphi, true, d, ld, sf);
		dim3 grid((nm+31)/32, (npair+31)/32, nc);
		hipLaunchKernelGGL(unpack_pair_transpose, grid, dim3(256), sizeof(double2)*2*32*33, st, (const double2*)p->hbuf.p, leg, nr, nm,
			(long)npair*rowlen, (long)nr*nm, (const double2*)p->phase.p, 1.0);
		p->prof.end(st, PXS_STAGE_RING_FFT);
		PXS_HIP(hipGetLastError());
		return;
	}
	const int ncin = std::min(nm, p->nphi);           // distinct FFT bins needed (m >= nphi alias onto m mod nphi)
	p->hbuf.ensure(sizeof(double2)*(size_t)nc*nr*nm);
	FftDims d; d.n_i = nr; d.is_i = p->ring_stride; d.os_i = ncin; d.n_o1 = nc; d.is_o1 = m.cstride; d.os_o1 = (long)nr*ncin;
	d.is_e = p->pix_stride; d.os_e = 1;
	FftLoad ld; ld.ptr = (const char*)m.ptr + esz(m.dtype)*p->ring_off0; ld.dtype = m.dtype;
	FftStore sf; sf.ptr = p->hbuf.p; sf.ne = ncin;
	p->fc->exec(st, p->nphi, true, d, ld, sf);
	if (ncin == nm) {
		dim3 grid((nm+31)/32, (nr+31)/32, nc);
		hipLaunchKernelGGL(transpose_mul, grid, dim3(256), sizeof(double2)*32*33, st, (const double2*)p->hbuf.p, leg, nr, nm,
			(long)nr*nm, (long)nr*nm, (const double2*)p->phase.p, 0, 1.0);
	} else {
		dim3 grid((unsigned)(((long)nr*nm + 255)/256), nc);
		hipLaunchKernelGGL(gather_alias, grid, dim3(256), 0, st, (const double2*)p->hbuf.p, leg, nr, nm, ncin, p->nphi,
			(long)nr*ncin, (long)nr*nm, (const double2*)p->phase.p, 1.0);
	}
	p->prof.end(st, PXS_STAGE_RING_FFT);
	PXS_HIP(hipGetLastError());
}

// the nb maps of a pass: leg[c][m][ring] * e^{+i m phi0} -> hbuf[c][ring][m] -> c2r ring FFT -> user map
// (leg: rows of stride ldleg; null: the route's theta stage has written hbuf already.  hbuf: the route's ld_h and nr_h, sized by reserve_call)
void leg2map(pxs_plan* p, hipStream_t st, const Route& r, const double2* leg, long ldleg, const MapArg& m, int nb) {
	p->prof.begin(st, PXS_STAGE_RING_FFT);
	const int nm = p->mmax+1, nr = p->nring, nc = nb*r.nc, ncb = nb > 1 ? r.nc : 0;
	const bool have_h = leg == nullptr;
	if (p->general) {
		PXS_REQUIRE(ncb == 0 && !have_h, "internal: general ring sets take one map per call");
		p->gz.ensure(sizeof(double2)*(size_t)nc*p->npixz);      // (general ring sets size their own z here)
		const GenK g = gen_args(p, nc, ldleg, m.cstride, 1.0);
		const dim3 grid((unsigned)p->g_nblk, nc);
		hipLaunchKernelGGL(gen_fold, grid, dim3(256), 0, st, g, leg, p->gz.as<double2>());
		gen_ffts(p, st, nc, false);
		if (m.dtype == PX_F32) hipLaunchKernelGGL(gen_scatter<float>, grid, dim3(256), 0, st, g, (const double2*)p->gz.p, (float*)m.ptr);
		else                     hipLaunchKernelGGL(gen_scatter<double>, grid, dim3(256), 0, st, g, (const double2*)p->gz.p, (double*)m.ptr);
		p->prof.end(st, PXS_STAGE_RING_FFT);
		PXS_HIP(hipGetLastError());
		(void)nm;
		return;
	}
	const long ldh = r.ld_h;
	if (!have_h) {
		dim3 grid((nm+31)/32, (nr+31)/32, nc);
		hipLaunchKernelGGL(transpose_mul_outcol, grid, dim3(256), sizeof(double2)*32*33, st, leg, (double2*)p->hbuf.p, nr, nm,
			(long)nm*ldleg, (long)nr*ldh, (const double2*)p->phase.p, 1, 1.0, ldleg, ldh);
	}
	if (p->chain_rings) {
		// (the CC detour of a band plan: h holds all nfull rings of the grid, the map's rings start at row0)
		const bool full_h = r.nr_h > nr;
		p->chain->h2map(st, p->hbuf.as<double2>() + (full_h ? (size_t)p->row0*ldh : 0), ldh, p->map_desc(m, ncb), nc, p->mmax, full_h ? r.nr_h : 0);
		p->prof.end(st, PXS_STAGE_RING_FFT);
		return;
	}
	PXS_REQUIRE(ncb == 0, "internal: unfused ring FFT handles single maps");
	auto esz = [](int dt) { return dt == PX_F32 ? 4 : 8; };
	if (2L*p->mmax < p->nphi && p->ring_pairs) {
		// two rings per complex transform: Z = X_a + i X_b, real part -> ring 2q, imaginary part -> ring 2q+1
		FftDims d; d.n_i = (nr + 1)/2; d.is_i = nm; d.os_i = p->ring_stride; d.n_o1 = nc; d.is_o1 = (long)nr*nm; d.os_o1 = m.cstride;
		d.is_e = 1; d.os_e = p->pix_stride;
		FftLoad ld; ld.ptr = p->hbuf.p; ld.mode = LD_HERM_PAIR; ld.ne = nm; ld.pair_lines = nr;
		FftStore sf; sf.ptr = (char*)m.ptr + esz(m.dtype)*p->ring_off0; sf.dtype = m.dtype; sf.real_pair = 1; sf.pair_lines = nr;
		p->fc->exec(st, p->nphi, false, d, ld, sf);
	} else {
		FftDims d; d.n_i = nr; d.is_i = nm; d.os_i = p->ring_stride; d.n_o1 = nc; d.is_o1 = (long)nr*nm; d.os_o1 = m.cstride;
		d.is_e = 1; d.os_e = p->pix_stride;
		FftLoad ld; ld.ptr = p->hbuf.p; ld.mode = LD_HERM; ld.ne = nm; ld.herm_fold = 1;
		FftStore sf; sf.ptr = (char*)m.ptr + esz(m.dtype)*p->ring_off0; sf.dtype = m.dtype;
		p->fc->exec(st, p->nphi, false, d, ld, sf);
	}
	p->prof.end(st, PXS_STAGE_RING_FFT);
	PXS_HIP(hipGetLastError());
}

// leg on the map's rings [c][m][nring] -> weighted leg on the CC grid [c][m][ncc].
// Columns m and m+1 have opposite theta-parity, so their mirror extensions are the even and the odd part
// of ONE sequence: each pair shares the whole 4-FFT chain (every stage is linear and commutes with the
// reflection theta -> -theta) and is separated again at the end -- half the FFT work.
// (M, sigma, w: the fine circle, the pointwise table on it and the CC weights of the form of the analysis -- the |sin| series on
// M > N + 2 lmax points, or ducc0's route: the CC weights on M = 2 N_cc points, with the spectrum cut to |k| < M/2 when M <= N)
void resample_to_cc(pxs_plan* p, hipStream_t st, const double2* leg_in, double2* leg_cc, int nc, int spin, long M, const double2* sigma, const double2* wcc) {
	const int nm = p->mmax+1, nr = p->nring;
	const long npair_all = (nm + 1)/2;
	const long chunk = std::max<long>(32, std::min<long>(npair_all, (long)(p->resample_chunk_bytes/(sizeof(double2)*M))));
	p->b1.ensure(sizeof(double2)*(size_t)chunk*std::max(p->N, p->Ncc));
	p->b2.ensure(sizeof(double2)*(size_t)chunk*M);
	p->prof.begin(st, PXS_STAGE_RESAMPLE);
	for (int c = 0; c < nc; c++)
	for (long p0 = 0; p0 < npair_all; p0 += chunk) {
		const long np = std::min<long>(chunk, npair_all - p0);
		const long m0 = 2*p0, nlines = std::min<long>(2*np, nm - m0);
		{	// (a) packed mirror extension of lines (2i, 2i+1), forward FFT_N
			FftDims d; d.n_i = np; d.is_i = nr; d.os_i = p->N; d.is_e = 1; d.os_e = 1;
			FftLoad ld; ld.ptr = leg_in + ((size_t)c*nm + m0)*nr; ld.mode = LD_MIRROR_PAIR; ld.ne = nr; ld.mir_c = p->mir_c;
			ld.par0 = (spin + (int)m0) & 1; ld.pair_lines = nlines;
			FftStore sf; sf.ptr = p->b1.p;
			p->fc->exec(st, p->N, true, d, ld, sf);
		}
		{	// (b) shift to theta0 = 0, pad to M, backward FFT_M, multiply by the |sin| series
			FftDims d; d.n_i = np; d.is_i = p->N; d.os_i = M; d.is_e = 1; d.os_e = 1;
			FftLoad ld; ld.ptr = p->b1.p; ld.mode = LD_SPEC; ld.ne = p->N; ld.nyq_half = M > p->N ? 1 : 0; ld.kmax = M > p->N ? -1 : M/2 - 1; ld.mul = p->ph_shift.as<double2>();
			FftStore sf; sf.ptr = p->b2.p; sf.mul = sigma;
			p->fc->exec(st, M, false, d, ld, sf);
		}
		{	// (c) forward FFT_M in place; only |k| <= lmax are needed
			FftDims d; d.n_i = np; d.is_i = M; d.os_i = M; d.is_e = 1; d.os_e = 1;
			FftLoad ld; ld.ptr = p->b2.p;
			FftStore sf; sf.ptr = p->b2.p; sf.two_sided_k = p->lmax;
			p->fc->exec(st, M, true, d, ld, sf);
		}
		{	// (d) truncate to |k| <= lmax, backward FFT_Ncc onto the full CC circle
			FftDims d; d.n_i = np; d.is_i = M; d.os_i = p->Ncc; d.is_e = 1; d.os_e = 1;
			FftLoad ld; ld.ptr = p->b2.p; ld.mode = LD_SPEC; ld.ne = M; ld.kmax = p->lmax;
			FftStore sf; sf.ptr = p->b1.p;
			p->fc->exec(st, p->Ncc, false, d, ld, sf);
		}
		{	// (e) separate the pair by reflection symmetry, keep rings 0..ncc-1, apply the quadrature weights
			const long tot = np*p->ncc;
			hipLaunchKernelGGL(split_pair, dim3((unsigned)((tot+255)/256)), dim3(256), 0, st, (const double2*)p->b1.p,
				leg_cc + ((size_t)c*nm + m0)*p->ncc, p->ncc, p->Ncc, 0, np, nlines, (spin + (int)m0) & 1, wcc, 1.0);
		}
	}
	p->prof.end(st, PXS_STAGE_RESAMPLE);
	PXS_HIP(hipGetLastError());
}

// exact transpose of resample_to_cc: leg on the CC grid [c][m][ncc] -> leg on the map's rings [c][m][nring]
void resample_to_cc_adjoint(pxs_plan* p, hipStream_t st, const double2* leg_cc, double2* leg_out, int nc, int spin, long M, const double2* sigma, const double2* wcc) {
	const int nm = p->mmax+1, nr = p->nring;
	const long chunk = std::max<long>(32, std::min<long>(nm, (long)(p->resample_chunk_bytes/(sizeof(double2)*M))));
	p->b1.ensure(sizeof(double2)*(size_t)chunk*std::max(p->N, p->Ncc));
	p->b2.ensure(sizeof(double2)*(size_t)chunk*M);
	p->prof.begin(st, PXS_STAGE_RESAMPLE);
	for (int c = 0; c < nc; c++)
	for (long m0 = 0; m0 < nm; m0 += chunk) {
		const long nl = std::min<long>(chunk, nm - m0);
		{	// (d)^H: weights, zero-extend the rings to the Ncc circle, forward FFT_Ncc
			FftDims d; d.n_i = nl; d.is_i = p->ncc; d.os_i = p->Ncc; d.is_e = 1; d.os_e = 1;
			FftLoad ld; ld.ptr = leg_cc + ((size_t)c*nm + m0)*p->ncc; ld.ne = p->ncc; ld.mul = wcc;
			FftStore sf; sf.ptr = p->b1.p;
			p->fc->exec(st, p->Ncc, true, d, ld, sf);
		}
		{	// (c)^H: embed |k| <= lmax into the M spectrum, backward FFT_M, multiply by the |sin| series
			FftDims d; d.n_i = nl; d.is_i = p->Ncc; d.os_i = M; d.is_e = 1; d.os_e = 1;
			FftLoad ld; ld.ptr = p->b1.p; ld.mode = LD_SPEC; ld.ne = p->Ncc; ld.kmax = p->lmax;
			FftStore sf; sf.ptr = p->b2.p; sf.mul = sigma;
			p->fc->exec(st, M, false, d, ld, sf);
		}
		{	// (b)^H first half: forward FFT_M in place (only |k| <= N/2 needed)
			FftDims d; d.n_i = nl; d.is_i = M; d.os_i = M; d.is_e = 1; d.os_e = 1;
			FftLoad ld; ld.ptr = p->b2.p;
			FftStore sf; sf.ptr = p->b2.p; sf.two_sided_k = M > p->N ? p->N/2 : -1;
			p->fc->exec(st, M, true, d, ld, sf);
		}
		{	// (b)^H second half + (a)^H FFT: truncate M -> N with the Nyquist combination and conj phase, backward FFT_N
			// (M <= N: the transpose of the low pass, zero padding of |k| < M/2)
			FftDims d; d.n_i = nl; d.is_i = M; d.os_i = p->N; d.is_e = 1; d.os_e = 1;
			FftLoad ld; ld.ptr = p->b2.p; ld.mode = LD_SPEC_ADJ; ld.ne = M; ld.nyq_half = M > p->N ? 1 : 0; ld.kmax = M > p->N ? -1 : M/2 - 1; ld.mul = p->ph_shift.as<double2>();
			FftStore sf; sf.ptr = p->b1.p;
			p->fc->exec(st, p->N, false, d, ld, sf);
		}
		{	// (a)^H: fold the mirror images back onto the rings
			const long tot = nl*nr;
			hipLaunchKernelGGL(fold_mirror, dim3((unsigned)((tot+255)/256)), dim3(256), 0, st, (const double2*)p->b1.p,
				leg_out + ((size_t)c*nm + m0)*nr, nr, p->N, p->mir_c, nl, (spin + (int)m0) & 1);
		}
	}
	p->prof.end(st, PXS_STAGE_RESAMPLE);
	PXS_HIP(hipGetLastError());
}

// band-limited leg on the CC grid [c][m][ncc] -> leg on the map's rings [c][m][nring] (exact for degree <= lmax);
// columns (m, m+1) packed as in resample_to_cc
void resample_from_cc(pxs_plan* p, hipStream_t st, const double2* leg_cc, double2* leg_out, int nc, int spin, double2* h_out = nullptr) {
	const int nm = p->mmax+1, nr = p->nring;
	const long npair_all = (nm + 1)/2;
	const long chunk = std::max<long>(32, std::min<long>(npair_all, (long)(p->resample_chunk_bytes/(sizeof(double2)*p->N))));
	p->b1.ensure(sizeof(double2)*(size_t)chunk*std::max(p->N, p->Ncc));
	p->b2.ensure(sizeof(double2)*(size_t)chunk*p->N);
	p->prof.begin(st, PXS_STAGE_RESAMPLE);
	for (int c = 0; c < nc; c++)
	for (long p0 = 0; p0 < npair_all; p0 += chunk) {
		const long np = std::min<long>(chunk, npair_all - p0);
		const long m0 = 2*p0, nlines = std::min<long>(2*np, nm - m0);
		{	// packed mirror extension of the CC rings to the full circle, forward FFT_Ncc
			FftDims d; d.n_i = np; d.is_i = p->ncc; d.os_i = p->Ncc; d.is_e = 1; d.os_e = 1;
			FftLoad ld; ld.ptr = leg_cc + ((size_t)c*nm + m0)*p->ncc; ld.mode = LD_MIRROR_PAIR; ld.ne = p->ncc; ld.mir_c = 0;
			ld.par0 = (spin + (int)m0) & 1; ld.pair_lines = nlines;
			FftStore sf; sf.ptr = p->b1.p;
			p->fc->exec(st, p->Ncc, true, d, ld, sf);
		}
		{	// keep |k| <= lmax, shift to the target grid's theta0, backward FFT_N onto the full circle
			FftDims d; d.n_i = np; d.is_i = p->Ncc; d.os_i = p->N; d.is_e = 1; d.os_e = 1;
			FftLoad ld; ld.ptr = p->b1.p; ld.mode = LD_SPEC; ld.ne = p->Ncc; ld.kmax = p->lmax; ld.mul = p->ph_up.as<double2>();
			FftStore sf; sf.ptr = p->b2.p;
			p->fc->exec(st, p->N, false, d, ld, sf);
		}
		if (h_out && np == npair_all) {	// separate the pair straight into the ring-major layout of the ring FFT (times e^{+i m phi0})
			dim3 grid((nm+31)/32, (nr+31)/32);
			hipLaunchKernelGGL(split_pair_transposed, grid, dim3(256), sizeof(double2)*32*33, st, (const double2*)p->b2.p,
				h_out + (size_t)c*nr*nm, nr, nm, p->N, p->mir_c, spin & 1, (const double2*)p->phase.p, 1.0/(double)p->Ncc);
		} else {	// separate the pair, keep the real rings
			const long tot = np*nr;
			hipLaunchKernelGGL(split_pair, dim3((unsigned)((tot+255)/256)), dim3(256), 0, st, (const double2*)p->b2.p,
				leg_out + ((size_t)c*nm + m0)*nr, nr, p->N, p->mir_c, np, nlines, (spin + (int)m0) & 1, (const double2*)nullptr, 1.0/(double)p->Ncc);
		}
	}
	p->prof.end(st, PXS_STAGE_RESAMPLE);
	PXS_HIP(hipGetLastError());
}

} // namespace


extern "C" {

int pxs_grid_maxlmax(const char* geometry, int ntheta) { return grid_maxlmax(geometry ? geometry : "", ntheta); }

int pxs_gridweights(const char* geometry, int ntheta, double* out) {
	PXS_TRY
	PXS_REQUIRE(geometry && out && ntheta > 0, "pxs_gridweights: bad arguments");
	GridInfo gi = grid_info(geometry, ntheta);
	if (!gi.ok) throw Error(PXS_ERR_UNSUPPORTED, std::string("gridweights: unsupported geometry '") + geometry + "' (CC, F1, MW, MWflip, DH, F2)");
	if (grid_weights_only(geometry)) {
		const bool dh = std::string(geometry) == "DH";
		const std::vector<LDb> w = fejer2_weights(dh ? ntheta-1 : ntheta);
		if (dh) out[0] = 0;
		for (size_t j = 0; j < w.size(); j++) out[j + (dh ? 1 : 0)] = (double)(w[j]*2*PIl);
		return 0;
	}
	const long N = gi.N; const int n = ntheta;
	const LDb th0 = (LDb)gi.c*PIl/N;
	std::vector<LDb> v(N);
	const long K = (N-1)/2;
	if (N <= 4096) {
		for (long j = 0; j < N; j++) {
			LDb th = th0 + 2*PIl*j/N, s = (LDb)abs_sin_coef(0);
			for (long k = 2; k <= K; k += 2) s += 2*(-(2/PIl)/((LDb)k*k-1))*cosl(k*th);
			if (N % 2 == 0 && ((N/2) % 2) == 0) s += (-(2/PIl)/((LDb)(N/2)*(N/2)-1))*cosl((N/2)*(th-th0))*cosl((N/2)*th0);
			v[j] = s*PIl/N;
		}
	} else {
		// the same cosine series as one backward DFT of length N on the device (the direct sum is N^2/4 long-double cosines:
		// 60 s for the 21600-ring grid, paid by every map2alm of a declination band through quad_weights)
		std::vector<double2> c(N, make_double2(0, 0));
		c[0].x = (double)abs_sin_coef(0);
		for (long k = 2; k <= K; k += 2) {
			const LDb sk = -(2/PIl)/((LDb)k*k-1), a = (LDb)k*th0;
			c[k] = make_double2((double)(sk*cosl(a)), (double)(sk*sinl(a)));
			c[N-k] = make_double2(c[k].x, -c[k].y);
		}
		if (N % 2 == 0 && ((N/2) % 2) == 0) c[N/2] = make_double2((double)((-(2/PIl)/((LDb)(N/2)*(N/2)-1))*cosl((N/2)*th0)), 0.0);
		int dev = 0; PXS_HIP(hipGetDevice(&dev));
		DevBuf dc = upload(c);
		fft_dense_lines(dev, nullptr, N, false, 1, dc.as<double2>(), dc.as<double2>());
		PXS_HIP(hipStreamSynchronize(nullptr));
		PXS_HIP(hipMemcpy(c.data(), dc.p, sizeof(double2)*N, hipMemcpyDeviceToHost));
		for (long j = 0; j < N; j++) v[j] = (LDb)c[j].x*PIl/N;
	}
	for (int j = 0; j < n; j++) out[j] = 0;
	for (long jp = 0; jp < N; jp++) { long r = jp < n ? jp : ((-jp - gi.c) % N + N) % N; out[r] += (double)(v[jp]*2*PIl); }
	PXS_CATCH
}

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
		std::vector<double> w(ntheta);
		if (pxs_gridweights(geometry, ntheta, w.data()) != 0) throw Error(PXS_ERR_ARG, get_last_error());
		std::vector<double2> wd(ntheta);
		for (int j = 0; j < ntheta; j++) wd[j] = make_double2(w[j]/nphi, 0.0);
		p->wring = upload(wd);
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
	if (p->general) setup_general(p.get(), nring, nphi, phi0, ringstart);
	std::vector<LDb> th(nring);
	for (int r = 0; r < nring; r++) th[r] = theta[r];
	p->rs_map.build(th); p->rs_map.upload_all();
	// Rows of a Fejer-1 grid (a declination band of a CAR map, curvedsky.py:843-873): theta_r = (row0 + r + 1/2) pi / n.  Synthesis
	// and its adjoint can then run their Legendre stage on the ~lmax+2 CC rings of that grid instead of the band's own ring-pair
	// slots (an unpaired ring costs a whole slot); PXS_BAND_VIA_CC=0 turns it off.
	{	static const bool on = [] { const char* e = lab_getenv("PXS_BAND_VIA_CC"); return e ? atoi(e) != 0 : true; }();
		if (on && !p->general && p->chain_rings && nring >= 2) {
			const LDb d = th[1] - th[0];
			const long n = d > 0 ? (long)llroundl(PIl/d) : 0;
			const long k0 = n > 0 ? (long)llroundl(th[0]*n/PIl - 0.5L) : -1;
			bool ok = n > nring && k0 >= 0 && k0 + nring <= n && lmax <= n - 1 && n < (1L << 30) && FftContext::supported(2*n);
			for (int r = 0; ok && r < nring; r++) ok = fabsl(th[r] - ((LDb)(k0 + r) + 0.5L)*PIl/n) < 1e-11L;
			if (ok) {
				p->band = true; p->geometry = "F1"; p->nfull = (int)n; p->row0 = (int)k0;
				setup_resampling(p.get());
				if (!p->chain_theta()) { p->band = false; p->nfull = 0; p->row0 = 0; p->ncc = 0; }     // (no fused theta chain for this size: stay on the band's own rings)
			}
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
	} else throw Error(PXS_ERR_ARG, std::string("pxs_plan_option: unknown option '") + name + "'");
	PXS_CATCH
}

// tables of the interpolating forms of the analysis (fused chains or the unfused engine): the fine-CC form (the default; the weights option
// on a grid below 2 lmax + 2 rings takes it too), else the interpolant form
struct AnaSet { const ThetaPlan* tp; const double2* sigma; const double2* wcc; const double2* whalf; long M; bool fine; };
static AnaSet ana_set(const pxs_plan* p, bool allow_fine = true) {
	if (allow_fine && p->ana_weights != 0 && p->Mf > 0) return AnaSet{&p->tpf, p->sigma_f.as<double2>(), p->wcc_f.as<double2>(), p->whalf_f.as<double2>(), p->Mf, true};
	return AnaSet{&p->tp, p->sigma.as<double2>(), p->wcc.as<double2>(), p->whalf.as<double2>(), p->M, false};
}
static Route route_of(const pxs_plan* p, bool analysis, int spin, int mode, bool adjoint, const LegTables* tb);
static Route analysis_route_now(const pxs_plan* p) { return route_of(p, true, 0, PXS_MODE_STANDARD, false, nullptr); }      // pxs_analysis under the plan's current option
// The chain stage shapes of the plan's standard calls (analysis under its current option, synthesis of spin 0 and spin 2), each once:
// a dry run of the very calls (FftChain::dry_begin), so the list cannot drift from what they launch.
static std::vector<ChainShape> chain_shapes(const pxs_plan* cp) {
	pxs_plan* p = const_cast<pxs_plan*>(cp);
	std::vector<ChainShape> all, out;
	if (!p->chain || !p->chain_rings) return out;
	std::lock_guard<std::mutex> plan_lock(p->call_mu);
	const int nm = p->mmax + 1;
	FftChain::MapDesc md; memset(&md, 0, sizeof(md)); md.dtype = PX_F64; md.cstride = (long)p->nring*p->nphi; md.ring_stride = p->nphi; md.pix_stride = 1; md.nring = p->nring; md.nphi = p->nphi;
	p->chain->dry_begin(&all);
	try {
		for (int which = 0; which < 3; which++) {
			const bool ana = which == 0; const int spin = which == 2 ? 2 : 0;
			const Route r = route_of(p, ana, spin, PXS_MODE_STANDARD, false, nullptr);
			if (!r.reserve_chain) continue;
			if (ana) p->chain->map2leg(nullptr, md, r.nc, p->mmax, nullptr, r.ld_leg, nullptr, 1.0);
			else p->chain->h2map(nullptr, nullptr, r.ld_h, md, r.nc, p->mmax, 0);
			if (!r.theta_fused || r.line) continue;
			switch (r.theta) {
			case TH_TO_CC:       p->chain->to_cc(nullptr, *r.tp, nullptr, r.ld_leg, r.nr_th, p->mir_c, nullptr, r.ld_leg2, p->ncc, r.nc, nm, spin, p->lmax, nullptr, nullptr, nullptr); break;
			case TH_FROM_CC_ADJ: p->chain->from_cc_adjoint(nullptr, *r.tp, nullptr, r.ld_leg, r.nr_th, p->mir_c, nullptr, r.ld_leg2, p->ncc, r.nc, nm, spin, p->lmax, nullptr, nullptr, nullptr); break;
			case TH_FROM_CC:     p->chain->from_cc(nullptr, *r.tp, nullptr, r.ld_leg2, p->ncc, nullptr, r.ld_h, r.nr_h, p->mir_c, r.nc, nm, spin, p->lmax, nullptr, nullptr, 1.0, nullptr); break;
			case TH_TO_CC_ADJ:   p->chain->to_cc_adjoint(nullptr, *r.tp, nullptr, r.ld_leg2, p->ncc, nullptr, r.ld_h, r.nr_h, p->mir_c, r.nc, nm, spin, p->lmax, nullptr, nullptr, nullptr, nullptr, 2.0); break;
			case TH_NONE: break;
			}
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
	PXS_REQUIRE(p && name && value, "pxs_plan_query: null argument");
	const std::string n(name);
	if (p->pts) *value = points_query(p->pts, n);
	else if (n == "analysis_form") { const Route r = analysis_route_now(p); *value = (r.kind == R_RING_WEIGHTS || r.kind == R_CC_WEIGHTS) ? 1 : (r.fine ? 2 : 0); }
	else if (n == "ncc_circle") *value = p->ncc > 0 ? p->Ncc : 0;
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
	if (nana) *nana = p->ncc > 0 ? p->ncc : p->nring;      // (the CC grid where the plan has one, whatever the analysis option: what this has always reported)
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
 * kind 0: map2leg (MA1, MA2), 1: h2map (MS1, MS2), 2: to_cc (RA1-5), 3: from_cc (RS1-3), 4: from_cc_adjoint */
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
	auto run = [&]() {
		const FftChain::MapDesc md = p->map_desc(MapArg{dmap.p, PX_F64, (long)nr*p->nphi, 0});
		switch (kind) {
		case 0: p->chain->map2leg(st, md, nc, p->mmax, p->leg.as<double2>(), ldm, p->phase.as<double2>(), 1.0); break;
		case 1: p->chain->h2map(st, p->hbuf.as<double2>(), ldh, md, nc, p->mmax); break;
		case 2: { AnaSet as = ana_set(p); if (!as.tp->ok) as = ana_set(p, false);      // (the form the plan's analysis option selects, where the chains hold it)
			p->chain->to_cc(st, *as.tp, p->leg.as<double2>(), ldm, p->nring, p->mir_c, p->leg2.as<double2>(), ldc, p->ncc, nc, (int)nm, spin, p->lmax,
				p->ph_shift.as<double2>(), as.sigma, as.wcc); } break;
		case 3: p->chain->from_cc(st, p->tp, p->leg2.as<double2>(), ldc, p->ncc, p->hbuf.as<double2>(), ldh, p->nring, p->mir_c, nc, (int)nm, spin, p->lmax,
				p->ph_up.as<double2>(), p->phase.as<double2>(), 1.0/(double)p->Ncc); break;
		default: p->chain->from_cc_adjoint(st, p->tp, p->leg.as<double2>(), ldm, p->nring, p->mir_c, p->leg2.as<double2>(), ldc, p->ncc, nc, (int)nm, spin, p->lmax,
				p->ph_shift.as<double2>(), p->wadj.as<double2>()); break;
		}
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
	if (enable && !p->wk.count.p) { PXS_HIP(hipSetDevice(p->device)); p->wk.count.alloc(2*1024*sizeof(double)); PXS_HIP(hipMemset(p->wk.count.p, 0, p->wk.count.bytes)); }
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
	for (size_t i = 0; i + 1 < c.size(); i += 2) { flops[0] += c[i]*128.0; flops[1] += c[i+1]*128.0; }     // FMA instructions per lane x 64 lanes x 2 flops
	if (reset) PXS_HIP(hipMemset(p->wk.count.p, 0, p->wk.count.bytes));
	PXS_CATCH
}

int pxs_profile_read(pxs_plan* p, double* ms, int* counts, int reset) {
	PXS_TRY
	PXS_REQUIRE(p && ms && counts, "pxs_profile_read: null argument");
	p->prof.read(ms, counts, PXS_NSTAGE, reset != 0);
	PXS_CATCH
}

// THE route decision of a call: every test of what the plan can do and of the lab switches is here and nowhere else.
// analysis: pxs_analysis (else pxs_synthesis); tb: the recurrence tables of the spin (null: a query, which sizes nothing)
static Route route_of(const pxs_plan* p, bool analysis, int spin, int mode, bool adjoint, const LegTables* tb) {
	Route r;
	const int nr = p->nring;
	const bool th = p->chain_theta();
	const long ldm = p->ld_map(), ldc = p->ld_cc(), ldh = p->ld_h();
	r.to_map = analysis ? adjoint : !adjoint; r.tb = tb;
	r.nc = analysis ? (spin == 0 ? 1 : 2) : ncomp_of(spin, mode, false); r.deriv1 = mode == PXS_MODE_DERIV1;
	r.rs = &p->rs_map; r.nr_th = nr; r.tp = &p->tp;
	auto use_h = [&](int rows) { r.nr_h = rows; r.ld_h = ldh; };
	auto form = [&](const AnaSet& as) { r.tp = as.tp; r.sigma = as.sigma; r.wcc = as.wcc; r.whalf = as.whalf; r.M = as.M; r.fine = as.fine; };
	if (!analysis) {
		// Legendre stage on the minimal CC grid + exact Fourier resampling in theta where the map has clearly more rings (the thresholds of
		// setup_resampling): grids, and bands of F1 grids (their rows outside the band are zero)
		const bool cc = (p->is_grid || (p->band && th)) && (spin == 0 ? p->syn_via_cc0 : p->syn_via_cc) && p->ncc > 0;
		static const bool adj_cc = [] { const char* e = lab_getenv("PXS_ADJ_VIA_CC"); return e ? atoi(e) != 0 : true; }();
		static const bool fuse = [] { const char* e = lab_getenv("PXS_FUSE_SPLIT"); return e ? atoi(e) != 0 : true; }();
		r.ld_leg = r.ld_leg_alloc = ldm;
		if (!cc || (adjoint && !(th && adj_cc))) { r.kind = R_DIRECT; if (!adjoint && !p->general) use_h(nr); }
		else {
			r.rs = &p->rs_cc; r.ld_leg2 = ldc; r.nr_th = p->band ? p->nfull : nr;      // (a band: the theta stage works on every ring of its grid)
			if (adjoint) { r.kind = R_VIA_CC; r.theta = TH_FROM_CC_ADJ; r.ld_leg = r.ld_leg_alloc = p->band ? FftChain::pad8(p->nfull) : ldm; }
			else if (th) { r.kind = R_VIA_CC; r.theta = TH_FROM_CC; use_h(r.nr_th); r.ld_leg = 0; }      // (leg: unused, but sized as it always was -- a plan's scratch_bytes are part of what it reports)
			// (a grid whose ring FFTs are chained but whose theta resampling is not -- 2 ntheta with a prime factor >= 7 -- and one without any chain)
			else { r.kind = (fuse && !p->chain_rings) ? R_VIA_CC_UNFUSED_H : R_VIA_CC_UNFUSED; r.theta = TH_FROM_CC; use_h(nr); r.ld_leg = nr; }      // (the unfused split writes dense rows)
		}
	} else if (p->wring.p) { r.kind = R_RING_WEIGHTS; }
	// ring weights on the map's own rings: the weights option, and ducc0's route on CC grids with >= 2 lmax + 2 rings (its
	// resample_to_prepared_CC multiplies such a grid by its weights directly: need_first_resample is false for it)
	else if ((p->ana_weights == 1 || (p->ana_weights == 2 && p->geometry == "CC")) && (long)nr >= 2L*p->lmax + 2)
		r.kind = (th && p->ncc > 0) ? R_CC_WEIGHTS : R_RING_WEIGHTS;
	else {
		form(ana_set(p));
		// (the adjoint of the interpolant form: PXS_ADJ_ANA_FUSED=0 sends it through the unfused engine; read per call, the tests switch it.
		//  Unfused also: the fine-CC form on a plan whose chains cannot hold the circle of 2 N_cc points)
		auto adj_ana_fused = [] { const char* e = getenv("PXS_ADJ_ANA_FUSED"); return e ? atoi(e) != 0 : true; };
		r.kind = (th && (r.fine ? r.tp->ok : (!adjoint || adj_ana_fused()))) ? R_CHAIN : R_UNFUSED;
	}
	if (analysis) {      // buffers of the analysis routes: map -> leg [-> leg2] -> alm, or alm -> leg -> h -> map / alm -> leg2 -> h -> map
		if (r.kind == R_RING_WEIGHTS) { r.ld_leg = ldm; if (adjoint) use_h(nr); }
		else {
			r.rs = &p->rs_cc; r.ld_leg2 = r.kind == R_UNFUSED ? p->ncc : ldc;
			if (!adjoint || r.kind == R_UNFUSED) r.ld_leg = r.kind == R_UNFUSED ? nr : ldm;
			if (adjoint) use_h(nr);
			r.theta = r.kind == R_CC_WEIGHTS ? (adjoint ? TH_FROM_CC : TH_FROM_CC_ADJ) : (adjoint ? TH_TO_CC_ADJ : TH_TO_CC);
		}
		r.ld_leg_alloc = r.ld_leg;
	}
	const bool unfused = r.kind == R_VIA_CC_UNFUSED || r.kind == R_VIA_CC_UNFUSED_H || r.kind == R_UNFUSED;
	r.batched = !unfused;
	r.theta_fused = r.theta != TH_NONE && !unfused;
	r.line = r.theta_fused && r.theta <= TH_FROM_CC_ADJ && FftChain::line_takes(*r.tp, r.theta == TH_TO_CC);
	// the ring chain's scratch is reserved with the call (the unfused analysis leaves it to the chain's own launches, as it always did)
	r.reserve_chain = p->chain_rings && r.kind != R_UNFUSED;
	return r;
}

// per-ring weight / nphi of the ring-weights paths (DH / F2: fixed at plan time; the weights option: built on first use)
static const double2* ring_weights(pxs_plan* p) {
	if (p->wring.p) return p->wring.as<double2>();
	if (!p->wgrid.p) {
		std::vector<double> w(p->nring);
		if (pxs_gridweights(p->geometry.c_str(), p->nring, w.data()) != 0) throw Error(PXS_ERR_ARG, get_last_error());
		std::vector<double2> wd(p->nring);
		for (int j = 0; j < p->nring; j++) wd[j] = make_double2(w[j]/p->nphi, 0.0);
		p->wgrid = upload(wd);
	}
	return p->wgrid.as<double2>();
}
// ... for the transposed theta upsampling (FftChain::from_cc_adjoint): its first stage extends the weighted ring samples to the circle
// by reflection, which holds a self-mirrored ring (the pole rings of CC, one of MW / MWflip) once and every other ring twice -- the
// zero extension it stands for is half the sum of the symmetric and the antisymmetric one, so the self-mirrored rings count double
static const double2* ring_weights_ext(pxs_plan* p) {
	const double2* w = ring_weights(p);
	if (p->geometry == "F1") return w;
	if (!p->wgrid_ext.p) {
		std::vector<double2> wd(p->nring);
		PXS_HIP(hipMemcpy(wd.data(), w, sizeof(double2)*p->nring, hipMemcpyDeviceToHost));
		for (int r = 0; r < p->nring; r++) { const long t = 2L*r + p->mir_c; if (t == 0 || t == p->N || t == 2*p->N) wd[r].x *= 2; }
		p->wgrid_ext = upload(wd);
	}
	return p->wgrid_ext.as<double2>();
}

// unit weights for the transposed theta upsampling on grids with self-mirrored rings (see ring_weights_ext); null on F1 grids
static const double2* unit_weights_ext(pxs_plan* p) {
	if (p->geometry == "F1" || p->band) return nullptr;
	if (!p->wunit_ext.p) {
		std::vector<double2> wd(p->nring, make_double2(1, 0));
		for (int r = 0; r < p->nring; r++) { const long t = 2L*r + p->mir_c; if (t == 0 || t == p->N || t == 2*p->N) wd[r].x = 2; }
		p->wunit_ext = upload(wd);
	}
	return p->wunit_ext.as<double2>();
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
			resample_to_cc_adjoint(p, st, p->leg2.as<double2>(), leg, r.nc, spin, r.M, r.sigma, r.wcc);
			leg2map(p, st, r, leg, r.ld_leg, map, 1);
		} else {
			map2leg(p, st, r, map, 1, leg);
			resample_to_cc(p, st, leg, p->leg2.as<double2>(), r.nc, spin, r.M, r.sigma, r.wcc);
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
	auto weigh = [&] {
		if (!wleg) return;
		const long tot = (long)nct*nm*nr;
		hipLaunchKernelGGL(scale_rings, dim3((unsigned)((tot+255)/256)), dim3(256), 0, st, leg, (long)nct*nm, nr, r.ld_leg, wleg);
		PXS_HIP(hipGetLastError()); };
	if (r.to_map) {
		p->leg_syn(st, r, alm, nb);
		weigh();
		if (r.theta != TH_NONE) p->run_theta(st, r, nct, spin, wth);      // (writes h ring-major for the ring FFT)
		leg2map(p, st, r, r.theta != TH_NONE ? nullptr : leg, r.ld_leg, map, nb);
	} else {
		if (r.nr_th > nr) {      // a band through the CC grid: leg holds every ring of the grid, zero outside the band's rows
			PXS_HIP(hipMemsetAsync(p->leg.p, 0, sizeof(double2)*(size_t)nct*nm*r.ld_leg, st));
			leg += p->row0;
		}
		map2leg(p, st, r, map, nb, leg);
		weigh();
		if (r.theta != TH_NONE) p->run_theta(st, r, nct, spin, wth);
		p->leg_ana(st, r, alm, nb);
	}
}

// Scratch of a call is sized HERE and only here, from its route, before its first launch (a plan's buffers only grow, so this
// allocates on the first call of a kind and when a later call brings a larger batch).  What is sized elsewhere, at the point of use,
// belongs to the rarely taken paths: gz of the general ring sets and the packed spectra of the unfused ring FFT (map2leg, leg2map),
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
	const size_t per_map = sizeof(double2)*(size_t)ncm*((size_t)(p->mmax+1)*(p->nring + (p->ncc > 0 ? p->ncc : 0))*2 + (size_t)p->nring*p->nphi);
	// scratch budget of one pass: PXS_BATCH_GB, default 64 GB (MI355X: 288 GB; 8 maps of config 5 = 56 GB, so that the batched Legendre kernels get
	// their 8-map groups there; it was 32 in rounds 2-4), never more than 40 % of what is free on the device now beyond what the plan holds already
	static const size_t budget_env = [] { const char* e = getenv("PXS_BATCH_GB"); return (size_t)(e ? atol(e) : 0) << 30; }();
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
	for (int b0 = 0; b0 < nbatch; b0 += chunk) run_core(p, r, spin, std::min(chunk, nbatch - b0), alm.from(b0), map.from(b0), st);
}

int pxs_synthesis(pxs_plan* p, int spin, int mode, int adjoint, int nbatch,
                  void* alm, int alm_dtype, int64_t alm_cstride, int64_t alm_bstride,
                  void* map, int map_dtype, int64_t map_cstride, int64_t map_bstride, void* stream)
{
	PXS_TRY
	PXS_REQUIRE(p && alm && map, "pxs_synthesis: null argument");
	std::lock_guard<std::mutex> plan_lock(p->call_mu);
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
