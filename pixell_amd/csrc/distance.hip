// Distance transforms on separable cylindrical geometries: the distance of every pixel from the nearest of a set of points, the index of
// that point, and the edge pixels of a mask or a label map (enmap.distance_from / distance_transform / labeled_distance_transform of the
// reference, pixell/enmap.py:2127-2215, an OpenMP C extension there, cython/distances_core.c).  The semantics are this package's own
// (INTEGRATION.md E):
//   d(p)   = min_i r(p, i), r the great-circle distance, exact (the reference's default front propagation is not); FP64 throughout
//   dom(p) = the i that wins the comparison on h = sin^2(ddec/2) + cos dec_p cos dec_i sin^2(dra/2) (monotone in r), the lowest i among equal h
//   rmax > 0: d > rmax -> d = rmax, dom = -1;  skip[p] = 0 -> d = 0, dom = -1 without a search
// Pixel p = (y, x) sits at dec0 + y ddec, ra0 + x dra; points lie anywhere on the sphere, RA differences count modulo 2 pi.
//
// The search is a gather: one workgroup per 16 x 16 pixel tile, a lane per pixel.  Points are binned into the cells of the tile grid
// (off-map points into the nearest edge cell, with their true coordinates), each occupied cell gets a bounding cap (the cell's centre, the
// largest distance of a point in it) and a few jump-flooding passes give every cell some real point not far from it.  A tile first
// evaluates that point and the points of its own cell; the largest of its pixels' distances so far, U, bounds how far a winner can be,
// and the tile then visits the cells of the pixel window that U implies (all columns where the window holds a pole; the compact list of the
// occupied cells when the window is most of the map), skipping every cell whose cap is farther than U by the triangle inequality.  U
// tightens after every batch of cells.  Exactness does not depend on how good U is: it always comes from real points.
// Per chunk of NCH points the two separable terms of h are staged in LDS per (point, tile row) and (point, tile column): two sincos
// per point (of half the angle differences to the tile's first row and column: formed before the sine, so close points do not cancel)
// rotated to the other rows and columns by tables, so that a pixel-point pair costs one FMA and a compare.  Each pixel's winner is then
// evaluated once with Vincenty's atan2 form, accurate on [0, pi].  Nothing but atomic counts, maxima of non-negative numbers and fill
// cursors depends on the order lanes run in, and the results depend on none of them: the output is the same bit for bit from run to run.
#include "../../include/pxsht.h"
#include "common.hpp"
#include "scan_dev.hpp"
#include "pixgeo.hpp"
#include <limits>

namespace pxs {
namespace dst {

static constexpr int TILE = 16;           // a tile is TILE x TILE pixels: one lane of a 256-lane workgroup per pixel; the cells points are binned into are the tiles
static constexpr int NCH = 64;            // points staged in LDS per step
static constexpr int EDGE_PER = 4;        // pixels per lane of the edge finder

struct DGeo : PixGeo { int ncy, ncx; };      // the geometry and its ncy x ncx cells
struct Pts { long n; const double* dec; const double* ra; const long long* pix; };          // pix != null: point i is the centre of flat pixel pix[i]
struct Win { int ty1, nrow, nr, a0[3], w[3], W; };      // cell rows ty1 .. ty1 + nrow - 1, columns a0[j] .. a0[j] + w[j] - 1 for j < nr; W = sum w

__device__ __forceinline__ void pt_pos(const DGeo& g, const Pts& p, long i, double& dec, double& ra) {
	if (p.pix) {
		long long q = p.pix[i]; const long long npix = (long long)g.ny*g.nx;
		q = q < 0 ? 0 : (q >= npix ? npix - 1 : q);
		const int y = (int)(q/g.nx), x = (int)(q - (long long)y*g.nx);
		dec = pix_dec(g, y); ra = pix_ra(g, x);
	} else { dec = p.dec[i]; ra = p.ra[i]; }
}
__device__ __forceinline__ bool finite_pos(double dec, double ra) { return fabs(dec) <= 4.0 && fabs(ra) <= 1e6; }

// the distance of (dec1, ra1) from (dec2, ra2) in Vincenty's form, as distances_core.c:87-132 evaluates it (1: the pixel, 2: the point)
__device__ inline double vincenty(double dec1, double ra1, double dec2, double ra2) {
	double s1, c1, s2, c2, sr, cr;
	sincos(dec1, &s1, &c1); sincos(dec2, &s2, &c2); sincos(ra1 - ra2, &sr, &cr);
	const double y1 = c2*sr, y2 = c1*s2 - s1*c2*cr;
	return atan2(sqrt(y1*y1 + y2*y2), s1*s2 + c1*c2*cr);
}

// the cell of the pixel nearest to the point, clamped to the map (the copy of the point nearest to the middle of the map in x)
__device__ inline int cell_of(const DGeo& g, double dec, double ra) {
	if (!finite_pos(dec, ra)) return 0;
	double y = (dec - g.dec0)/g.ddec, x = (ra - g.ra0)/g.dra;
	x -= g.period*floor((x - 0.5*g.nx)/g.period + 0.5);
	y = rint(y); x = rint(x);
	const int iy = !(y > 0) ? 0 : (y > g.ny - 1 ? g.ny - 1 : (int)y), ix = !(x > 0) ? 0 : (x > g.nx - 1 ? g.nx - 1 : (int)x);
	return (iy/TILE)*g.ncx + ix/TILE;
}
// the middle of the cell's pixels
__device__ inline void cell_centre(const DGeo& g, int c, double& dec, double& ra) {
	const int cy = c/g.ncx, cx = c - cy*g.ncx;
	const int y0 = cy*TILE, x0 = cx*TILE;
	const int y1 = y0 + TILE - 1 < g.ny - 1 ? y0 + TILE - 1 : g.ny - 1, x1 = x0 + TILE - 1 < g.nx - 1 ? x0 + TILE - 1 : g.nx - 1;
	dec = g.dec0 + 0.5*(double)(y0 + y1)*g.ddec; ra = g.ra0 + 0.5*(double)(x0 + x1)*g.dra;
}
__device__ __forceinline__ double from_bits(unsigned long long u) { double d; memcpy(&d, &u, 8); return d; }
__device__ __forceinline__ unsigned long long to_bits(double d) { unsigned long long u; memcpy(&u, &d, 8); return u; }

__global__ __launch_bounds__(256) void pt_count_kernel(DGeo g, Pts pts, int* __restrict__ cnt)
{
	const long i = (long)blockIdx.x*blockDim.x + threadIdx.x;
	if (i >= pts.n) return;
	double dec, ra; pt_pos(g, pts, i, dec, ra);
	atomicAdd(&cnt[cell_of(g, dec, ra)], 1);
}

// the point into its cell's list (in the order the lanes arrive: nothing depends on it), the cell's cap radius (the order-preserving bit
// pattern of a non-negative double) and the cell's seed for the flooding: the highest point index + 1
__global__ __launch_bounds__(256) void pt_fill_kernel(DGeo g, Pts pts, const long long* __restrict__ off, int* __restrict__ cur, int* __restrict__ plist,
		unsigned long long* __restrict__ rad, int* __restrict__ seed)
{
	const long i = (long)blockIdx.x*blockDim.x + threadIdx.x;
	if (i >= pts.n) return;
	double dec, ra; pt_pos(g, pts, i, dec, ra);
	const int c = cell_of(g, dec, ra);
	plist[off[c] + atomicAdd(&cur[c], 1)] = (int)i;
	double cd, cr; cell_centre(g, c, cd, cr);
	const double r = finite_pos(dec, ra) ? vincenty(cd, cr, dec, ra) : PXS_PI;
	atomicMax(&rad[c], to_bits(r >= 0 ? r : PXS_PI));
	atomicMax(&seed[c], (int)i + 1);
}

// one jump-flooding pass: every cell takes, among its own seed and those of the 8 cells `step` away (x wraps when the map does), the
// point nearest to its centre.  seed: point index + 1, 0: none yet
__global__ __launch_bounds__(256) void flood_kernel(DGeo g, Pts pts, int step, const int* __restrict__ in, int* __restrict__ out)
{
	const long c = (long)blockIdx.x*blockDim.x + threadIdx.x;
	if (c >= (long)g.ncy*g.ncx) return;
	const int cy = (int)(c/g.ncx), cx = (int)(c - (long)cy*g.ncx);
	double cd, cr; cell_centre(g, (int)c, cd, cr);
	int best = 0; double bd = 0;
	for (int dy = -1; dy <= 1; dy++) for (int dx = -1; dx <= 1; dx++) {
		const int yy = cy + dy*step; int xx = cx + dx*step;
		if (yy < 0 || yy >= g.ncy) continue;
		if (xx < 0 || xx >= g.ncx) { if (!g.wrap) continue; xx %= g.ncx; if (xx < 0) xx += g.ncx; }
		const int s = in[(long)yy*g.ncx + xx];
		if (s <= 0 || s == best) continue;
		double pd, pr; pt_pos(g, pts, s - 1, pd, pr);
		const double d = finite_pos(pd, pr) ? vincenty(cd, cr, pd, pr) : 4.0;
		if (best == 0 || d < bd || (d == bd && s < best)) { best = s; bd = d; }
	}
	out[c] = best;
}

// the largest v of the workgroup's 256 lanes; red[256]: LDS
__device__ inline double block_max(double v, double* red) {
	const int t = threadIdx.x;
	__syncthreads();
	red[t] = v;
	__syncthreads();
	for (int d = 128; d > 0; d >>= 1) { if (t < d) red[t] = red[t] > red[t + d] ? red[t] : red[t + d]; __syncthreads(); }
	return red[0];
}
// inclusive sums of v over the 256 lanes, left in s[256] (LDS)
__device__ inline void block_scan_incl(int v, int* s) {
	const int t = threadIdx.x;
	__syncthreads();
	s[t] = v;
	__syncthreads();
	for (int d = 1; d < 256; d <<= 1) {
		const int a = t >= d ? s[t - d] : 0;
		__syncthreads();
		s[t] += a;
		__syncthreads();
	}
}

// the cells that can hold a point within `rad` of (cdec, cra), a pixel centre of the map: rows from the declination range, columns from
// the width of the small circle in RA (sin dRA = sin rad / cos dec) in every copy of the circle that reaches the map, clamped to the map as
// the points' cells are; all columns where the disc holds a pole
__device__ inline Win make_window(const DGeo& g, double cdec, double cra, double rad) {
	Win w; w.nr = 1; w.a0[0] = 0; w.w[0] = g.ncx; w.W = g.ncx; w.ty1 = 0; w.nrow = g.ncy;
	if (!(rad < PXS_PI)) return w;
	double ya = (cdec - rad - g.dec0)/g.ddec, yb = (cdec + rad - g.dec0)/g.ddec;
	if (ya > yb) { const double t = ya; ya = yb; yb = t; }
	ya = fmax(floor(ya) - 1, 0.0); yb = fmin(ceil(yb) + 1, (double)(g.ny - 1));
	if (!(yb >= ya)) { w.nrow = 0; return w; }
	w.ty1 = (int)ya/TILE; w.nrow = (int)yb/TILE - w.ty1 + 1;
	if (!(fabs(cdec) + rad < 0.5*PXS_PI)) return w;
	const double hw = (asin(fmin(1.0, sin(rad)/cos(cdec))) + 1e-9)/fabs(g.dra) + 1;
	if (!(2*hw + 2 < g.period)) return w;
	const double xc = (cra - g.ra0)/g.dra, lo = 0.5*g.nx - 0.5*g.period, hi = lo + g.period;
	w.nr = 0; w.W = 0;
	for (int k = -1; k <= 1; k++) {
		double xa = xc - hw + k*g.period, xb = xc + hw + k*g.period;
		if (xb < lo || xa > hi) continue;
		xa = fmin(fmax(floor(fmax(xa, lo)), 0.0), (double)(g.nx - 1)); xb = fmin(fmax(ceil(fmin(xb, hi)), 0.0), (double)(g.nx - 1));
		int a = (int)xa/TILE; const int b = (int)xb/TILE;
		if (w.nr > 0) {
			const int e = w.a0[w.nr-1] + w.w[w.nr-1] - 1;      // the ranges come in ascending order: join what overlaps
			if (a <= e + 1) { if (b > e) w.w[w.nr-1] = b - w.a0[w.nr-1] + 1; continue; }
		}
		w.a0[w.nr] = a; w.w[w.nr] = b - a + 1; w.nr++;
	}
	for (int j = 0; j < w.nr; j++) w.W += w.w[j];
	return w;
}
__device__ __forceinline__ int window_cell(const DGeo& g, const Win& w, int k) {
	const int row = k/w.W; int rem = k - row*w.W;
	int cx = 0;
	for (int j = 0; j < w.nr; j++) { if (rem < w.w[j]) { cx = w.a0[j] + rem; break; } rem -= w.w[j]; }
	return (w.ty1 + row)*g.ncx + cx;
}

template<class T> __global__ __launch_bounds__(256) void gather_kernel(DGeo g, Pts pts, double rmax, const int* __restrict__ cnt, const long long* __restrict__ off,
		const TileRec* __restrict__ act, const long long* __restrict__ tot, const int* __restrict__ plist, const unsigned long long* __restrict__ rad,
		const int* __restrict__ seed, const uint8_t* __restrict__ skip, T* __restrict__ omap, int* __restrict__ odom, int* __restrict__ visits)
{
	PXS_SHARED(double, sh);
	double* sy = sh; double* sx = sy + NCH*TILE;       // [point][tile row]: sin^2(ddec/2); [point][tile column]: cos dec_i sin^2(dra/2)
	double* rot = sx + NCH*TILE;                       // sin, cos of k ddec/2 and of k dra/2, k < TILE
	double* pst = rot + 4*TILE;                        // [point]: sin, cos of half the point's offset from the tile's first row, the same for the first column, cos dec_i
	double* red = pst + 5*NCH;
	int* sid = (int*)(red + 256);                      // the staged points' indices
	int* ssc = sid + NCH; int* qoff = ssc + 256; int* qn = qoff + 256;      // a batch of cells: inclusive sums of their point counts, where their lists start, the counts
	const int tid = threadIdx.x, py = tid/TILE, px = tid%TILE;
	const int tile = blockIdx.x, ty = tile/g.ncx, tx = tile - ty*g.ncx;
	const int y = ty*TILE + py, x = tx*TILE + px;
	const bool inside = y < g.ny && x < g.nx;
	const long p = (long)y*g.nx + x;
	const bool active = inside && (!skip || skip[p] != 0);
	if (!(block_max(active ? 1.0 : 0.0, red) > 0)) {      // nothing to search for in this tile
		if (inside) { omap[p] = T(0); if (odom) odom[p] = -1; }
		if (visits && tid == 0) visits[tile] = 0;
		return;
	}
	const double decp = pix_dec(g, y), rap = pix_ra(g, x), cp = cos(decp);
	const double dec_r0 = pix_dec(g, ty*TILE), ra_c0 = pix_ra(g, tx*TILE);
	double cdec, cra; cell_centre(g, tile, cdec, cra);
	if (tid < TILE) sincos(0.5*(double)tid*g.ddec, &rot[tid], &rot[TILE + tid]);
	else if (tid < 2*TILE) sincos(0.5*(double)(tid - TILE)*g.dra, &rot[2*TILE + tid - TILE], &rot[3*TILE + tid - TILE]);
	const double rt = block_max(active ? vincenty(cdec, cra, decp, rap) : 0.0, red);      // the tile's radius (and the tables are in place)
	double bh = 2.0; int bi = -1; long nvis = 0;

	// m <= NCH points, point j of them idx_of(j): staged, then every pixel against every one
	auto visit = [&](int m, auto idx_of) {
		__syncthreads();      // (the readers of the previous step are done)
		if (tid < m) {
			const int i = idx_of(tid);
			double pd, pr; pt_pos(g, pts, i, pd, pr);
			sid[tid] = i;
			sincos(0.5*(dec_r0 - pd), &pst[5*tid], &pst[5*tid + 1]); sincos(0.5*(ra_c0 - pr), &pst[5*tid + 2], &pst[5*tid + 3]);
			pst[5*tid + 4] = cos(pd);
		}
		__syncthreads();
		for (int t = tid; t < m*2*TILE; t += 256) {
			const int o = t/(2*TILE), k = t%(2*TILE);
			if (k < TILE) { const double s = pst[5*o]*rot[TILE + k] + pst[5*o + 1]*rot[k]; sy[o*TILE + k] = s*s; }
			else { const int kk = k - TILE; const double s = pst[5*o + 2]*rot[3*TILE + kk] + pst[5*o + 3]*rot[2*TILE + kk]; sx[o*TILE + kk] = pst[5*o + 4]*(s*s); }
		}
		__syncthreads();
		if (active) for (int o = 0; o < m; o++) {
			const double h = fma(cp, sx[o*TILE + px], sy[o*TILE + py]);
			const int i = sid[o];
			if (h < bh || (h == bh && i < bi)) { bh = h; bi = i; }
		}
		nvis += m;
	};
	// how far a winner can still be from its pixel: the largest distance found so far, a little more than that, and no further than rmax
	auto bound = [&]() {
		const double hm = block_max(active ? bh : 0.0, red);
		double u = hm >= 1.0 ? PXS_PI : 2.0*asin(sqrt(hm));
		u = u*(1 + 1e-9) + 1e-12;
		if (rmax > 0) u = fmin(u, rmax*(1 + 1e-9) + 1e-12);
		return u;
	};

	const int sd = seed[tile];
	if (sd > 0) visit(1, [&](int) { return sd - 1; });
	const int n0 = cnt[tile];
	if (n0 > 0) {
		const long long o0 = off[tile];
		for (int j0 = 0; j0 < n0; j0 += NCH) visit(n0 - j0 < NCH ? n0 - j0 : NCH, [&](int j) { return plist[o0 + j0 + j]; });
	}
	double U = bound();
	const Win win = make_window(g, cdec, cra, U + rt);
	const int nocc = (int)tot[1];
	const long kwin = (long)win.nrow*win.W;
	const bool walk = kwin >= nocc;      // the window is most of the map: the occupied cells themselves
	const int K = walk ? nocc : (int)kwin;
	for (int k0 = 0; k0 < K; k0 += 256) {
		const int k = k0 + tid;
		int n = 0; long long o = 0;
		if (k < K) {
			const int c = walk ? act[k].tile : window_cell(g, win, k);
			if (c != tile && (n = cnt[c]) > 0) {
				double ccd, ccr; cell_centre(g, c, ccd, ccr);
				const double rho = from_bits(rad[c]);
				if (vincenty(cdec, cra, ccd, ccr) - rt - rho*(1 + 1e-9) - 1e-12 > U) n = 0;      // no point of the cell can be nearer than U to a pixel of the tile
				else o = off[c];
			}
		}
		qn[tid] = n; qoff[tid] = (int)o;
		block_scan_incl(n, ssc);
		const int total = ssc[255];
		for (int b = 0; b < total; b += NCH) {
			visit(total - b < NCH ? total - b : NCH, [&](int j) {
				const int pos = b + j;
				int lo = 0, hi = 255;      // the first cell of the batch whose inclusive sum exceeds pos
				while (lo < hi) { const int mid = (lo + hi) >> 1; if (ssc[mid] > pos) hi = mid; else lo = mid + 1; }
				return plist[qoff[lo] + pos - (ssc[lo] - qn[lo])];
			});
		}
		if (total > 0 && k0 + 256 < K) U = bound();
		else __syncthreads();      // (the batch's tables are read before the next batch writes them)
	}
	if (inside) {
		double r = 0;
		if (!active) bi = -1;
		else if (bi < 0) r = rmax > 0 ? rmax : std::numeric_limits<double>::infinity();
		else {
			double pd, pr; pt_pos(g, pts, bi, pd, pr);
			r = vincenty(decp, rap, pd, pr);
			if (rmax > 0 && r > rmax) { r = rmax; bi = -1; }
		}
		omap[p] = (T)r; if (odom) odom[p] = bi;
	}
	if (visits && tid == 0) visits[tile] = (int)(nvis < 0x7fffffffl ? nvis : 0x7fffffffl);
}

// no points: rmax (infinity without one) where the search would have run
template<class T> __global__ __launch_bounds__(256) void nopoint_kernel(long npix, double v, const uint8_t* __restrict__ skip, T* __restrict__ omap, int* __restrict__ odom)
{
	const long p = (long)blockIdx.x*blockDim.x + threadIdx.x;
	if (p >= npix) return;
	omap[p] = (skip && skip[p] == 0) ? T(0) : (T)v;
	if (odom) odom[p] = -1;
}

// ---- the edge finder --------------------------------------------------------------------------------------------------------------
// LAB = 0: a pixel of value 0 on the border of the array or with a non-zero 4-neighbour (distances_core.c:1209-1231); LAB = 1: a non-zero
// pixel on the border or with a 4-neighbour of another value (:1233-1256)
template<class V, int LAB> __device__ __forceinline__ bool is_edge(const V* __restrict__ m, int ny, int nx, long p) {
	const V v = m[p];
	if (LAB ? v == 0 : v != 0) return false;
	const int y = (int)(p/nx), x = (int)(p - (long)y*nx);
	if (y == 0 || x == 0 || y == ny - 1 || x == nx - 1) return true;
	if (LAB) return m[p-1] != v || m[p+1] != v || m[p-nx] != v || m[p+nx] != v;
	return m[p-1] != 0 || m[p+1] != 0 || m[p-nx] != 0 || m[p+nx] != 0;
}
template<class V, int LAB> __global__ __launch_bounds__(256) void edge_count_kernel(int ny, int nx, const V* __restrict__ m, int* __restrict__ bcnt)
{
	PXS_SHARED(int, ssum);
	const long npix = (long)ny*nx, base = ((long)blockIdx.x*256 + threadIdx.x)*EDGE_PER;
	int n = 0;
	for (int k = 0; k < EDGE_PER; k++) if (base + k < npix) n += is_edge<V, LAB>(m, ny, nx, base + k);
	block_scan_incl(n, ssum);
	if (threadIdx.x == 255) bcnt[blockIdx.x] = ssum[255];
}
template<class V, int LAB> __global__ __launch_bounds__(256) void edge_fill_kernel(int ny, int nx, const V* __restrict__ m, const long long* __restrict__ off,
		long long* __restrict__ out, long long cap)
{
	PXS_SHARED(int, ssum);
	const long npix = (long)ny*nx, base = ((long)blockIdx.x*256 + threadIdx.x)*EDGE_PER;
	bool e[EDGE_PER]; int n = 0;
	for (int k = 0; k < EDGE_PER; k++) { e[k] = base + k < npix && is_edge<V, LAB>(m, ny, nx, base + k); n += e[k]; }
	block_scan_incl(n, ssum);
	long long pos = off[blockIdx.x] + ssum[threadIdx.x] - n;
	for (int k = 0; k < EDGE_PER; k++) if (e[k]) { if (pos < cap) out[pos] = base + k; pos++; }
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
namespace {
template<class V, int LAB> void run_edges(hipStream_t st, int ny, int nx, const void* map, int nblk, int* bcnt, long long* bsc, int* bsa, long long* tot,
		long long* off, TileRec* act, long long* out, long long cap)
{
	hipLaunchKernelGGL((edge_count_kernel<V, LAB>), dim3(nblk), dim3(256), 256*sizeof(int), st, ny, nx, (const V*)map, bcnt);
	scan_counts(st, nblk, bcnt, bsc, bsa, tot, off, act);
	if (out) hipLaunchKernelGGL((edge_fill_kernel<V, LAB>), dim3(nblk), dim3(256), 256*sizeof(int), st, ny, nx, (const V*)map, (const long long*)off, out, cap);
}
}

} // namespace dst
} // namespace pxs

using namespace pxs;
using namespace pxs::dst;

extern "C" {

int pxm_find_edges(int ny, int nx, const void* d_map, int labeled, int64_t* d_edges, int64_t cap, int64_t* count, int device, void* stream)
{
	PXS_TRY
	PXS_REQUIRE(ny >= 1 && nx >= 1 && d_map, "pxm_find_edges: bad arguments");
	PXS_REQUIRE(d_edges || count, "pxm_find_edges: nothing to return");
	PXS_REQUIRE(!d_edges || cap >= 0, "pxm_find_edges: bad capacity");
	const long npix = (long)ny*nx;
	const long nblk_l = (npix + 256*EDGE_PER - 1)/(256*EDGE_PER);
	PXS_REQUIRE(nblk_l < (1l << 31), "pxm_find_edges: the map is too large");
	const int nblk = (int)nblk_l, nsb = (nblk + 256*SCAN_PER - 1)/(256*SCAN_PER);
	PXS_HIP(hipSetDevice(device));
	hipStream_t st = (hipStream_t)stream;
	DevBuf& fixed = stream_scratch(SCR_DISTANCE, device, stream);
	Carve cv;
	const size_t o_cnt = cv.take(4*(size_t)nblk), o_off = cv.take(8*(size_t)nblk), o_act = cv.take(sizeof(TileRec)*(size_t)nblk);
	const size_t o_bsc = cv.take(8*(size_t)nsb), o_bsa = cv.take(4*(size_t)nsb), o_tot = cv.take(16);
	fixed.ensure(cv.at);
	char* base = fixed.as<char>();
	int* bcnt = (int*)(base + o_cnt); long long* off = (long long*)(base + o_off); TileRec* act = (TileRec*)(base + o_act);
	long long* bsc = (long long*)(base + o_bsc); int* bsa = (int*)(base + o_bsa); long long* tot = (long long*)(base + o_tot);
	if (labeled) run_edges<int32_t, 1>(st, ny, nx, d_map, nblk, bcnt, bsc, bsa, tot, off, act, (long long*)d_edges, (long long)cap);
	else run_edges<uint8_t, 0>(st, ny, nx, d_map, nblk, bcnt, bsc, bsa, tot, off, act, (long long*)d_edges, (long long)cap);
	PXS_HIP(hipGetLastError());
	if (count) {      // the one number the host needs: how many edge pixels there are
		long long htot[2] = {0, 0};
		PXS_HIP(hipMemcpyAsync(htot, tot, sizeof(htot), hipMemcpyDeviceToHost, st));
		PXS_HIP(hipStreamSynchronize(st));
		*count = htot[0];
	}
	PXS_CATCH
}

int pxm_distance_from(int ny, int nx, double dec0, double ddec, double ra0, double dra, int64_t npoint, const double* d_pt_dec, const double* d_pt_ra,
                      const int64_t* d_pt_pix, double rmax, const uint8_t* d_skip, void* d_omap, int map_dtype, int32_t* d_domains, int32_t* d_visits,
                      int device, void* stream)
{
	PXS_TRY
	PXS_REQUIRE(ny >= 1 && nx >= 1 && npoint >= 0 && npoint < (int64_t(1) << 31) - 1, "pxm_distance_from: bad sizes");
	const PixGeo pg = make_pixgeo("pxm_distance_from", ny, nx, dec0, ddec, ra0, dra);
	PXS_REQUIRE(map_dtype == PX_F32 || map_dtype == PX_F64, "pxm_distance_from: the map must be float32 or float64");
	PXS_REQUIRE(d_omap, "pxm_distance_from: null map");
	PXS_REQUIRE(npoint == 0 || d_pt_pix || (d_pt_dec && d_pt_ra), "pxm_distance_from: points need coordinates or pixel indices");
	PXS_REQUIRE(!(rmax != rmax), "pxm_distance_from: rmax is not a number");
	const long ncx = (nx + TILE - 1)/TILE, ncy = (ny + TILE - 1)/TILE, ncell = ncx*ncy, npix = (long)ny*nx;
	PXS_REQUIRE(ncell < (1l << 31), "pxm_distance_from: the map has too many tiles");
	PXS_HIP(hipSetDevice(device));
	hipStream_t st = (hipStream_t)stream;
	if (npoint == 0) {
		const double v = rmax > 0 ? rmax : std::numeric_limits<double>::infinity();
		if (map_dtype == PX_F32) hipLaunchKernelGGL((nopoint_kernel<float>), dim3(blocks_of(npix)), dim3(256), 0, st, npix, v, d_skip, (float*)d_omap, (int*)d_domains);
		else hipLaunchKernelGGL((nopoint_kernel<double>), dim3(blocks_of(npix)), dim3(256), 0, st, npix, v, d_skip, (double*)d_omap, (int*)d_domains);
		if (d_visits) PXS_HIP(hipMemsetAsync(d_visits, 0, 4*(size_t)ncell, st));
		PXS_HIP(hipGetLastError());
		return 0;
	}
	const DGeo g = {pg, (int)ncy, (int)ncx};
	const Pts pts = {(long)npoint, d_pt_dec, d_pt_ra, (const long long*)d_pt_pix};
	const int nsb = (int)((ncell + 256*SCAN_PER - 1)/(256*SCAN_PER));
	DevBuf& fixed = stream_scratch(SCR_DISTANCE, device, stream);
	Carve cv;
	const size_t o_cnt = cv.take(4*(size_t)ncell), o_cur = cv.take(4*(size_t)ncell), o_rad = cv.take(8*(size_t)ncell), o_sda = cv.take(4*(size_t)ncell);
	const size_t o_sdb = cv.take(4*(size_t)ncell), o_off = cv.take(8*(size_t)ncell), o_act = cv.take(sizeof(TileRec)*(size_t)ncell);
	const size_t o_bsc = cv.take(8*(size_t)nsb), o_bsa = cv.take(4*(size_t)nsb), o_tot = cv.take(16), o_pl = cv.take(4*(size_t)npoint);
	fixed.ensure(cv.at);
	char* base = fixed.as<char>();
	int* cnt = (int*)(base + o_cnt); int* cur = (int*)(base + o_cur); unsigned long long* rad = (unsigned long long*)(base + o_rad);
	int* sda = (int*)(base + o_sda); int* sdb = (int*)(base + o_sdb); long long* off = (long long*)(base + o_off); TileRec* act = (TileRec*)(base + o_act);
	long long* bsc = (long long*)(base + o_bsc); int* bsa = (int*)(base + o_bsa); long long* tot = (long long*)(base + o_tot); int* plist = (int*)(base + o_pl);
	PXS_HIP(hipMemsetAsync(cnt, 0, o_sdb - o_cnt, st));      // (the counts, the fill cursors, the cap radii and the seeds)
	hipLaunchKernelGGL(pt_count_kernel, dim3(blocks_of(npoint)), dim3(256), 0, st, g, pts, cnt);
	scan_counts(st, (int)ncell, cnt, bsc, bsa, tot, off, act);
	hipLaunchKernelGGL(pt_fill_kernel, dim3(blocks_of(npoint)), dim3(256), 0, st, g, pts, (const long long*)off, cur, plist, rad, sda);
	int s0 = 1;
	while (2*s0 < (ncx > ncy ? ncx : ncy)) s0 *= 2;
	for (int s = s0; s >= 1; s /= 2) {
		hipLaunchKernelGGL(flood_kernel, dim3(blocks_of(ncell)), dim3(256), 0, st, g, pts, s, (const int*)sda, sdb);
		int* t = sda; sda = sdb; sdb = t;
	}
	const size_t shmem = sizeof(double)*(2*NCH*TILE + 4*TILE + 5*NCH + 256) + sizeof(int)*(NCH + 3*256);
	if (map_dtype == PX_F32) hipLaunchKernelGGL((gather_kernel<float>), dim3((unsigned)ncell), dim3(256), shmem, st, g, pts, rmax, (const int*)cnt, (const long long*)off,
		(const TileRec*)act, (const long long*)tot, (const int*)plist, (const unsigned long long*)rad, (const int*)sda, d_skip, (float*)d_omap, (int*)d_domains, (int*)d_visits);
	else hipLaunchKernelGGL((gather_kernel<double>), dim3((unsigned)ncell), dim3(256), shmem, st, g, pts, rmax, (const int*)cnt, (const long long*)off,
		(const TileRec*)act, (const long long*)tot, (const int*)plist, (const unsigned long long*)rad, (const int*)sda, d_skip, (double*)d_omap, (int*)d_domains, (int*)d_visits);
	PXS_HIP(hipGetLastError());
	PXS_CATCH
}

} // extern "C"
