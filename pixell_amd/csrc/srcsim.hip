// Painting radially symmetric objects into a map and reading radial sums back out around a catalogue: pointsrcs.sim_objects /
// radial_sum of the reference (pixell/pointsrcs.py:35-210, an OpenMP C extension there, cython/srcsim_core.c), for separable
// cylindrical geometries.  The semantics are this package's own:
//   r(p, i)   = 2 asin(sqrt(min(h, 1))),  h = sin^2((dec_p - dec_i)/2) + cos dec_p cos dec_i sin^2((ra_p - ra_i)/2)       (no cancellation for close points)
//   P_i(r)    = the linear interpolation of the object's profile samples (rs, vs): vs[0] below rs[0], 0 from rs[n-1] on
//   rcut_i    = rs[min(k+1, n-1)], k the last sample with |vs[k]| >= vmin / max_c |amps[c,i]| (0 if none), capped by rmax > 0
//   forward   : map[c,p] = op(map[c,p], amps[c,i] P_i(r)) for every object with r <= rcut_i; for `add` the terms are summed in ascending i and the
//               sum is added to the map once, so what the map held is rounded against once, not once per object
//   transpose : amps[c,i] += sum_{p: r <= rcut_i} map[c,p] P_i(r)
//   radial sum: oprofs[i,c,k] += sum map[c,p] over bins[k] <= r < bins[k+1]
// Pixel p = (y, x) sits at float(dec0 + y ddec), float(ra0 + x dra), objects at float coordinates, as the reference takes them.
//
// The forward pass is a gather.  Every object gets a conservative pixel box (obj_prep_kernel); the 16 x 16 pixel tiles a box touches are
// counted, the counts scanned into list offsets and a list of the tiles that have objects, the lists filled and each one ordered by object
// index (so the result does not depend on the order the fill ran in); then one workgroup per listed tile, a lane per pixel, walks its
// list in steps of NCH objects.  A list entry is the object's whole record (ObjRec), a listed tile one TileRec.  Per step the two separable terms of h are taken once per (object, tile row) and (object, tile column)
// in FP64 and kept in LDS with the objects' records, so that a pixel-object pair costs one square root and one arc sine.  No atomics on
// the map, no tile without objects is visited, and a tile's list is as long as it needs to be.  The host reads one number back (the
// total list length, to size the lists).  The transpose and the radial sum run one workgroup per object over the object's own box.
#include "../../include/pxsht.h"
#include "common.hpp"
#include "scan_dev.hpp"
#include "pixgeo.hpp"

namespace pxs {

static constexpr int TILE = 16;           // a tile is TILE x TILE pixels: one lane of a 256-lane workgroup per pixel
static constexpr int NCH = 64;            // objects staged in LDS per step
static constexpr int NCC = 4;             // map components carried in registers per pass over a tile's list
static constexpr int PROF_LDS = 4096;     // profile samples (of all profiles together) up to which the tables are kept in LDS
static constexpr int SRC_MAXBLK = 2048;   // workgroups of the kernels that loop over the listed tiles

struct Box { int y1, nyb, x1, nxb; };     // rows y1 .. y1 + nyb - 1, columns (x1 + j) mod nx for j < nxb <= nx; nyb = 0: the disc misses the map
struct ObjRec { int idx; float dec, ra, cd, rc, hm; int po, pn; };      // a list entry: the object's index, position, cos dec, cut radius, a bound on h beyond which r > rc for certain, its profile (first sample, samples)
struct Prof { int nprof; const int* off; const float* rs; const float* vs; const float* vmax; int equi; };      // profile q: samples off[q] .. off[q+1]-1; vmax[k] = max_{j >= k} |vs[j]|

// the pixel coordinates rounded to float: the reference's float32 axes, bit for bit
__device__ __forceinline__ float pix_decf(const PixGeo& g, int y) { return (float)pix_dec(g, y); }
__device__ __forceinline__ float pix_raf(const PixGeo& g, int x) { return (float)pix_ra(g, x); }
__device__ __forceinline__ int prof_id(const Prof& pr, const int* pid, long i) { const int q = pid ? pid[i] : 0; return q < 0 ? 0 : (q >= pr.nprof ? pr.nprof - 1 : q); }

// The RA difference is brought into [-pi, pi] in double before it is rounded to float: across the seam of a map that covers the whole
// circle the two coordinates differ by 2 pi, and a float difference there is good to 2^-24 of 2 pi, not of the separation (paint_kernel takes
// its separable terms in double and has no such case).  Away from the seam nothing changes: the double difference rounds to the float one.
__device__ __forceinline__ float pair_dist(float pdec, float pra, float cp, float odec, float ora, float co) {
	const double dra = (double)pra - (double)ora;
	const float sd = sinf(0.5f*(pdec - odec)), sr = sinf((float)(0.5*(dra - 2*PXS_PI*rint(dra*(0.5/PXS_PI)))));
	const float h = sd*sd + cp*co*(sr*sr);
	return 2.0f*asinf(sqrtf(fminf(h, 1.0f)));
}

__device__ __forceinline__ float prof_eval(const float* rs, const float* vs, int n, int equi, float r) {
	if (r < rs[0]) return vs[0];
	if (!(r < rs[n-1])) return 0.0f;
	int i;
	if (equi) { i = (int)(r/rs[1]); i = i < 0 ? 0 : (i > n-2 ? n-2 : i); }
	else {
		int a = 0, b = n-1;
		while (b > a+1) { const int c = (a + b) >> 1; if (r < rs[c]) b = c; else a = c; }
		i = a;
	}
	const float x = (r - rs[i])/(rs[i+1] - rs[i]);
	return vs[i] + (vs[i+1] - vs[i])*x;
}

// every pixel whose centre can lie within rc of the object, and then some: the radius is widened by 1e-6 (relative and in radians, which
// covers the float rounding of the coordinates) and the box by up to a pixel on each side
__device__ inline Box bounding_box(const PixGeo& g, float odec, float ora, float rcf) {
	Box b = {0, 0, 0, 0};
	const double dec = odec, rc = (double)rcf*(1 + 1e-6) + 1e-6;
	if (!(rc >= 0) || !(fabs(dec) <= 4.0) || !(fabs((double)ora) <= 1e6)) return b;
	double ya = (dec - rc - g.dec0)/g.ddec, yb = (dec + rc - g.dec0)/g.ddec;
	if (ya > yb) { const double t = ya; ya = yb; yb = t; }
	ya = fmax(floor(ya), 0.0); yb = fmin(ceil(yb), (double)(g.ny - 1));
	if (!(yb >= ya)) return b;
	const double adra = fabs(g.dra), period = 2*PXS_PI/adra;
	const bool full = !(fabs(dec) + rc < 0.5*PXS_PI);      // the disc holds a pole: every column
	const double w = full ? period : (asin(fmin(1.0, sin(rc)/cos(dec))) + 1e-6)/adra;      // the half width of a small circle in RA: sin(dRA) = sin(rc)/cos(dec)
	double xc = ((double)ora - g.ra0)/g.dra;
	if (g.wrap) {
		if (full || 2*w + 2 >= g.nx) { b.x1 = 0; b.nxb = g.nx; }
		else {
			const double xa = floor(xc - w), xb = ceil(xc + w);
			const int n = (int)(xb - xa) + 1;
			b.x1 = (int)(xa - (double)g.nx*floor(xa/g.nx)); if (b.x1 >= g.nx || b.x1 < 0) b.x1 = 0;
			b.nxb = n < g.nx ? n : g.nx;
		}
	} else {
		xc -= period*floor((xc - 0.5*g.nx)/period + 0.5);      // the copy of the object nearest to the middle of the map
		const double xa = full ? 0.0 : fmax(floor(xc - w), 0.0), xb = full ? (double)(g.nx - 1) : fmin(ceil(xc + w), (double)(g.nx - 1));
		if (!(xb >= xa)) return b;
		b.x1 = (int)xa; b.nxb = (int)(xb - xa) + 1;
	}
	b.y1 = (int)ya; b.nyb = (int)(yb - ya) + 1;
	return b;
}

// f(tile) once for every tile the box touches
template<class F> __device__ inline void for_each_tile(const PixGeo& g, const Box& b, int ntx, F f) {
	if (b.nyb <= 0) return;
	const int ty1 = b.y1/TILE, ty2 = (b.y1 + b.nyb - 1)/TILE;
	const int xe = b.x1 + b.nxb - 1;
	const int ta1 = b.x1/TILE, ta2 = (xe < g.nx ? xe : g.nx - 1)/TILE;
	int tb2 = -1;      // the part that wrapped round holds columns 0 .. xe - nx: its tiles, short of the one the first part starts in
	if (xe >= g.nx) { tb2 = (xe - g.nx)/TILE; if (tb2 > ta1 - 1) tb2 = ta1 - 1; }
	for (int ty = ty1; ty <= ty2; ty++) {
		for (int tx = ta1; tx <= ta2; tx++) f(ty*ntx + tx);
		for (int tx = 0; tx <= tb2; tx++) f(ty*ntx + tx);
	}
}

// fixed_rcut >= 0: every object has that cut radius (radial sums); otherwise it follows from the amplitudes and the profile
__global__ __launch_bounds__(256) void obj_prep_kernel(PixGeo g, long nobj, const float* __restrict__ odec, const float* __restrict__ ora,
		const float* __restrict__ amps, int ncomp, long astride, const int* __restrict__ pid, Prof pr, float vmin, float rmax, float fixed_rcut,
		float* __restrict__ rcut, Box* __restrict__ box)
{
	const long i = (long)blockIdx.x*blockDim.x + threadIdx.x;
	if (i >= nobj) return;
	float rc = fixed_rcut;
	if (!(fixed_rcut >= 0)) {
		float amax = 0;
		for (int c = 0; c < ncomp; c++) amax = fmaxf(amax, fabsf(amps[c*astride + i]));
		const int q = prof_id(pr, pid, i), o = pr.off[q], n = pr.off[q+1] - o;
		const float vrel = vmin/amax;
		int lo = 0, hi = n;      // vmax does not increase: the samples with vmax >= vrel are the first `lo`, and the last of them is the last one with |vs| >= vrel
		while (lo < hi) { const int mid = (lo + hi) >> 1; if (pr.vmax[o + mid] >= vrel) lo = mid + 1; else hi = mid; }
		const int k = lo > 0 ? lo - 1 : 0;
		rc = pr.rs[o + (k + 1 < n ? k + 1 : n - 1)];
		if (rmax > 0) rc = fminf(rc, rmax);
	}
	rcut[i] = rc;
	box[i] = bounding_box(g, odec[i], ora[i], rc);
}

__global__ __launch_bounds__(256) void tile_count_kernel(PixGeo g, int ntx, long nobj, const Box* __restrict__ box, int* __restrict__ cnt)
{
	const long i = (long)blockIdx.x*blockDim.x + threadIdx.x;
	if (i >= nobj) return;
	for_each_tile(g, box[i], ntx, [&](int t) { atomicAdd(&cnt[t], 1); });
}

// the object's record into the list of every tile its box touches, in the order the lanes arrive (tile_sort_kernel orders the lists)
__global__ __launch_bounds__(256) void tile_fill_kernel(PixGeo g, int ntx, long nobj, const Box* __restrict__ box, const float* __restrict__ odec,
		const float* __restrict__ ora, const int* __restrict__ pid, Prof pr, const float* __restrict__ rcut, const long long* __restrict__ off,
		int* __restrict__ cur, ObjRec* __restrict__ raw)
{
	const long i = (long)blockIdx.x*blockDim.x + threadIdx.x;
	if (i >= nobj) return;
	const Box b = box[i];
	if (b.nyb <= 0) return;
	const int q = prof_id(pr, pid, i);
	ObjRec r;
	r.idx = (int)i; r.dec = odec[i]; r.ra = ora[i]; r.cd = (float)cos((double)r.dec); r.rc = rcut[i];
	const float s = sinf(0.5f*fminf(r.rc, (float)PXS_PI));
	r.hm = s*s*1.0001f + 1e-30f;
	r.po = pr.off[q]; r.pn = pr.off[q+1] - r.po;
	for_each_tile(g, b, ntx, [&](int t) { raw[off[t] + atomicAdd(&cur[t], 1)] = r; });
}

// list[off .. off + n) = raw[off .. off + n) in ascending order, tile by tile.  An object is in a tile's list once, so an entry's place is
// the number of smaller ones; counted against LDS copies of 256 entries at a time (n^2/256 steps per lane: lists are tens of entries long)
// The workgroups of this kernel and of paint_kernel take every gridDim.x-th listed tile and fetch the next tile's record before they work on
// the current one, so that a tile costs one round trip to memory (its list), not one per level of indirection.
__global__ __launch_bounds__(256) void tile_sort_kernel(const TileRec* __restrict__ act, const long long* __restrict__ tot,
		const ObjRec* __restrict__ raw, ObjRec* __restrict__ list)
{
	PXS_SHARED(int, sv);
	const int tid = threadIdx.x, nact = (int)tot[1];
	int a = blockIdx.x;
	TileRec next = act[a < nact ? a : 0];
	for (; a < nact; a += gridDim.x) {
		const TileRec t = next;
		if (a + (int)gridDim.x < nact) next = act[a + gridDim.x];
		const int n = t.n;
		const long long o0 = t.off;
		if (n == 1) { if (tid == 0) list[o0] = raw[o0]; continue; }
		for (int e0 = 0; e0 < n; e0 += 256) {
			const bool mine = e0 + tid < n;
			ObjRec v; v.idx = 0;
			if (mine) v = raw[o0 + e0 + tid];
			int rank = 0;
			for (int c0 = 0; c0 < n; c0 += 256) {
				__syncthreads();
				if (c0 + tid < n) sv[tid] = raw[o0 + c0 + tid].idx;
				__syncthreads();
				const int m = n - c0 < 256 ? n - c0 : 256;
				if (mine) for (int k = 0; k < m; k++) rank += sv[k] < v.idx;
			}
			if (mine) list[o0 + rank] = v;
		}
	}
}

// OP: 0 add, 1 max, 2 min.  nprofl: the profile samples staged in LDS (all of them, or 0: read from global memory)
template<class T, int OP> __global__ __launch_bounds__(256) void paint_kernel(PixGeo g, int ntx, T* __restrict__ map, int ncomp, long cstride,
		const float* __restrict__ amps, long astride, Prof pr, int nprofl, const TileRec* __restrict__ act, const long long* __restrict__ tot,
		const ObjRec* __restrict__ list)
{
	PXS_SHARED(float, sh);
	float* prs = sh; float* pvs = prs + nprofl;
	float* sy = pvs + nprofl; float* sx = sy + NCH*TILE;      // [object][tile row]: sin^2(ddec/2); [object][tile column]: cos dec_i sin^2(dra/2)
	float* src = sx + NCH*TILE; float* shm = src + NCH;        // cut radius, and the bound on h
	int* spo = (int*)(shm + NCH); int* spn = spo + NCH; int* sid = spn + NCH;      // the object's profile (first sample, samples) and its index
	const int tid = threadIdx.x, py = tid/TILE, px = tid%TILE;
	for (int k = tid; k < nprofl; k += 256) { prs[k] = pr.rs[k]; pvs[k] = pr.vs[k]; }
	const float* rs = nprofl ? prs : pr.rs; const float* vs = nprofl ? pvs : pr.vs;
	const int nact = (int)tot[1];
	int a = blockIdx.x;
	TileRec next = act[a < nact ? a : 0];
	for (; a < nact; a += gridDim.x) {
		const TileRec tr = next;
		if (a + (int)gridDim.x < nact) next = act[a + gridDim.x];
		const int ty = tr.tile/ntx, tx = tr.tile - ty*ntx;
		const int y = ty*TILE + py, x = tx*TILE + px;
		const bool inside = y < g.ny && x < g.nx;
		const long p = (long)y*g.nx + x;
		const float cp = cosf(pix_decf(g, y));
		const long long o0 = tr.off;
		const int n = tr.n;
		for (int c0 = 0; c0 < ncomp; c0 += NCC) {
			const int nc = ncomp - c0 < NCC ? ncomp - c0 : NCC;
			T acc[NCC];
			for (int c = 0; c < NCC; c++) acc[c] = (OP != 0 && inside && c < nc) ? map[(c0 + c)*cstride + p] : T(0);      // add: the objects' sum starts from zero and meets the map once, at the end
			for (int j0 = 0; j0 < n; j0 += NCH) {
				const int m = n - j0 < NCH ? n - j0 : NCH;
				__syncthreads();      // (the readers of the previous step are done)
				if (tid < m) {
					const ObjRec r = list[o0 + j0 + tid];
					sid[tid] = r.idx; src[tid] = r.rc; shm[tid] = r.hm; spo[tid] = r.po; spn[tid] = r.pn;
				}
				for (int t = tid; t < m*2*TILE; t += 256) {
					const int o = t/(2*TILE), k = t%(2*TILE);
					const ObjRec* r = list + (o0 + j0 + o);
					if (k < TILE) { const double s = sin(0.5*((double)pix_decf(g, ty*TILE + k) - (double)r->dec)); sy[o*TILE + k] = (float)(s*s); }
					else { const double s = sin(0.5*((double)pix_raf(g, tx*TILE + k - TILE) - (double)r->ra)); sx[o*TILE + k - TILE] = (float)((double)r->cd*s*s); }
				}
				__syncthreads();
				if (inside) for (int o = 0; o < m; o++) {
					const float h = sy[o*TILE + py] + cp*sx[o*TILE + px];
					if (h > shm[o]) continue;
					const float r = 2.0f*asinf(sqrtf(fminf(h, 1.0f)));
					if (!(r <= src[o])) continue;
					const float P = prof_eval(rs + spo[o], vs + spo[o], spn[o], pr.equi, r);
					const int i = sid[o];
					for (int c = 0; c < NCC; c++) if (c < nc) {
						const T v = (T)(amps[(c0 + c)*astride + i]*P);
						if (OP == 0) acc[c] += v; else if (OP == 1) acc[c] = v > acc[c] ? v : acc[c]; else acc[c] = v < acc[c] ? v : acc[c];
					}
				}
			}
			if (inside) for (int c = 0; c < nc; c++) { T& mv = map[(c0 + c)*cstride + p]; mv = OP == 0 ? mv + acc[c] : acc[c]; }
		}
	}
}

// one workgroup per object over the pixels of its box; the 256 partial sums are added up as a tree in LDS (a fixed order)
template<class T> __global__ __launch_bounds__(256) void transpose_kernel(PixGeo g, const T* __restrict__ map, int ncomp, long cstride,
		const float* __restrict__ odec, const float* __restrict__ ora, float* __restrict__ amps, long astride, const int* __restrict__ pid,
		Prof pr, const float* __restrict__ rcut, const Box* __restrict__ box)
{
	PXS_SHARED(float, red);
	const long i = blockIdx.x;
	const int tid = threadIdx.x;
	const Box b = box[i];
	if (b.nyb <= 0) return;
	const int q = prof_id(pr, pid, i), po = pr.off[q], pn = pr.off[q+1] - po;
	const float od = odec[i], orr = ora[i], co = cosf(od), rc = rcut[i];
	const long npx = (long)b.nyb*b.nxb;
	for (int c0 = 0; c0 < ncomp; c0 += NCC) {
		const int nc = ncomp - c0 < NCC ? ncomp - c0 : NCC;
		float acc[NCC];
		for (int c = 0; c < NCC; c++) acc[c] = 0;
		for (long j = tid; j < npx; j += 256) {
			const int jy = (int)(j/b.nxb), y = b.y1 + jy;
			int x = b.x1 + (int)(j - (long)jy*b.nxb); if (x >= g.nx) x -= g.nx;
			const float pd = pix_decf(g, y);
			const float r = pair_dist(pd, pix_raf(g, x), cosf(pd), od, orr, co);
			if (!(r <= rc)) continue;
			const float P = prof_eval(pr.rs + po, pr.vs + po, pn, pr.equi, r);
			for (int c = 0; c < NCC; c++) if (c < nc) acc[c] += (float)map[(c0 + c)*cstride + (long)y*g.nx + x]*P;
		}
		for (int c = 0; c < nc; c++) {
			__syncthreads();
			red[tid] = acc[c];
			__syncthreads();
			for (int d = 128; d > 0; d >>= 1) { if (tid < d) red[tid] += red[tid + d]; __syncthreads(); }
			if (tid == 0) amps[(c0 + c)*astride + i] += red[0];
		}
	}
}

// one workgroup per object; the bins of all components are summed in LDS
template<class T> __global__ __launch_bounds__(256) void radial_sum_kernel(PixGeo g, const T* __restrict__ map, int ncomp, long cstride,
		const float* __restrict__ odec, const float* __restrict__ ora, int nbin, const float* __restrict__ bins, int equi,
		const Box* __restrict__ box, float* __restrict__ oprofs)
{
	PXS_SHARED(float, acc);
	const long i = blockIdx.x;
	const int tid = threadIdx.x;
	const Box b = box[i];
	if (b.nyb <= 0) return;
	for (int t = tid; t < ncomp*nbin; t += 256) acc[t] = 0;
	__syncthreads();
	const float od = odec[i], orr = ora[i], co = cosf(od), r0 = bins[0], r1 = bins[nbin];
	const long npx = (long)b.nyb*b.nxb;
	for (long j = tid; j < npx; j += 256) {
		const int jy = (int)(j/b.nxb), y = b.y1 + jy;
		int x = b.x1 + (int)(j - (long)jy*b.nxb); if (x >= g.nx) x -= g.nx;
		const float pd = pix_decf(g, y);
		const float r = pair_dist(pd, pix_raf(g, x), cosf(pd), od, orr, co);
		if (!(r >= r0 && r < r1)) continue;
		int k;
		if (equi) {      // a guess, put right against the edges themselves
			k = (int)(r/bins[1]); k = k < 0 ? 0 : (k > nbin-1 ? nbin-1 : k);
			while (k > 0 && r < bins[k]) k--;
			while (k < nbin-1 && r >= bins[k+1]) k++;
		} else {
			int lo = 0, hi = nbin;
			while (hi > lo+1) { const int c = (lo + hi) >> 1; if (r < bins[c]) hi = c; else lo = c; }
			k = lo;
		}
		for (int c = 0; c < ncomp; c++) atomicAdd(&acc[c*nbin + k], (float)map[c*cstride + (long)y*g.nx + x]);
	}
	__syncthreads();
	for (int t = tid; t < ncomp*nbin; t += 256) oprofs[i*ncomp*nbin + t] += acc[t];
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
namespace {
template<class T> void launch_paint(int op, dim3 grid, size_t shmem, hipStream_t st, PixGeo g, int ntx, void* map, int ncomp, long cstride,
		const float* amps, long astride, Prof pr, int nprofl, const TileRec* act, const long long* tot, const ObjRec* list)
{
	if (op == 0) hipLaunchKernelGGL((paint_kernel<T, 0>), grid, dim3(256), shmem, st, g, ntx, (T*)map, ncomp, cstride, amps, astride, pr, nprofl, act, tot, list);
	else if (op == 1) hipLaunchKernelGGL((paint_kernel<T, 1>), grid, dim3(256), shmem, st, g, ntx, (T*)map, ncomp, cstride, amps, astride, pr, nprofl, act, tot, list);
	else hipLaunchKernelGGL((paint_kernel<T, 2>), grid, dim3(256), shmem, st, g, ntx, (T*)map, ncomp, cstride, amps, astride, pr, nprofl, act, tot, list);
}
}

} // namespace pxs

using namespace pxs;

extern "C" {

int pxm_sim_objects(int ny, int nx, double dec0, double ddec, double ra0, double dra, void* d_map, int map_dtype, int ncomp, int64_t map_cstride,
                    int64_t nobj, const float* d_obj_dec, const float* d_obj_ra, float* d_amps, int64_t amp_cstride, const int32_t* d_prof_ids,
                    int nprof, const int32_t* d_prof_off, int64_t nsamp, const float* d_prof_rs, const float* d_prof_vs, const float* d_prof_vmax,
                    int prof_equi, double vmin, double rmax, int op, int transpose, int device, void* stream)
{
	PXS_TRY
	PXS_REQUIRE(ny >= 1 && nx >= 1 && ncomp >= 0 && nobj >= 0 && nobj < (int64_t(1) << 31), "pxm_sim_objects: bad sizes");
	const PixGeo g = make_pixgeo("pxm_sim_objects", ny, nx, dec0, ddec, ra0, dra);
	PXS_REQUIRE(map_dtype == PX_F32 || map_dtype == PX_F64, "pxm_sim_objects: the map must be float32 or float64");
	PXS_REQUIRE(op >= 0 && op <= 2, "pxm_sim_objects: op must be 0 (add), 1 (max) or 2 (min)");
	PXS_REQUIRE(!(transpose && op != 0), "pxm_sim_objects: the transpose is that of op = add");
	PXS_REQUIRE(vmin >= 0 && rmax >= 0, "pxm_sim_objects: vmin and rmax must not be negative");
	if (nobj == 0 || ncomp == 0) return 0;
	PXS_REQUIRE(d_map && d_obj_dec && d_obj_ra && d_amps, "pxm_sim_objects: null array");
	PXS_REQUIRE(ncomp == 1 || (map_cstride >= (int64_t)ny*nx && amp_cstride >= nobj), "pxm_sim_objects: the components overlap");
	PXS_REQUIRE(nprof >= 1 && d_prof_off && d_prof_rs && d_prof_vs && d_prof_vmax && nsamp >= nprof && nsamp < (int64_t(1) << 31), "pxm_sim_objects: bad profile tables");
	const long ntx = (nx + TILE - 1)/TILE, nty = (ny + TILE - 1)/TILE, ntiles = ntx*nty;
	PXS_REQUIRE(ntiles < (1l << 31), "pxm_sim_objects: the map has too many tiles");
	PXS_HIP(hipSetDevice(device));
	hipStream_t st = (hipStream_t)stream;
	const Prof pr = {nprof, d_prof_off, d_prof_rs, d_prof_vs, d_prof_vmax, prof_equi ? 1 : 0};
	const int nblk = (int)((ntiles + 256*SCAN_PER - 1)/(256*SCAN_PER));
	DevBuf& fixed = stream_scratch(SCR_SRC_FIXED, device, stream);
	Carve cv;
	const size_t o_rcut = cv.take(4*(size_t)nobj), o_box = cv.take(sizeof(Box)*(size_t)nobj);
	const size_t o_cnt = cv.take(4*(size_t)ntiles), o_cur = cv.take(4*(size_t)ntiles), o_off = cv.take(8*(size_t)ntiles), o_act = cv.take(sizeof(TileRec)*(size_t)ntiles);
	const size_t o_bsc = cv.take(8*(size_t)nblk), o_bsa = cv.take(4*(size_t)nblk), o_tot = cv.take(16);
	fixed.ensure(cv.at);
	char* base = fixed.as<char>();
	float* rcut = (float*)(base + o_rcut); Box* box = (Box*)(base + o_box);
	hipLaunchKernelGGL(obj_prep_kernel, dim3(blocks_of(nobj)), dim3(256), 0, st, g, (long)nobj, d_obj_dec, d_obj_ra, (const float*)d_amps, ncomp, (long)amp_cstride,
		d_prof_ids, pr, (float)vmin, (float)rmax, -1.0f, rcut, box);
	if (transpose) {
		if (map_dtype == PX_F32) hipLaunchKernelGGL((transpose_kernel<float>), dim3((unsigned)nobj), dim3(256), 256*sizeof(float), st, g, (const float*)d_map, ncomp, (long)map_cstride, d_obj_dec, d_obj_ra, d_amps, (long)amp_cstride, d_prof_ids, pr, (const float*)rcut, (const Box*)box);
		else hipLaunchKernelGGL((transpose_kernel<double>), dim3((unsigned)nobj), dim3(256), 256*sizeof(float), st, g, (const double*)d_map, ncomp, (long)map_cstride, d_obj_dec, d_obj_ra, d_amps, (long)amp_cstride, d_prof_ids, pr, (const float*)rcut, (const Box*)box);
		PXS_HIP(hipGetLastError());
		return 0;
	}
	int* cnt = (int*)(base + o_cnt); int* cur = (int*)(base + o_cur); long long* off = (long long*)(base + o_off); TileRec* act = (TileRec*)(base + o_act);
	long long* bsc = (long long*)(base + o_bsc); int* bsa = (int*)(base + o_bsa); long long* tot = (long long*)(base + o_tot);
	PXS_HIP(hipMemsetAsync(cnt, 0, o_off - o_cnt, st));      // (the counts and the fill cursors)
	hipLaunchKernelGGL(tile_count_kernel, dim3(blocks_of(nobj)), dim3(256), 0, st, g, (int)ntx, (long)nobj, (const Box*)box, cnt);
	scan_counts(st, (int)ntiles, cnt, bsc, bsa, tot, off, act);
	PXS_HIP(hipGetLastError());
	long long htot[2] = {0, 0};      // the one number the host needs: how long the lists are together
	PXS_HIP(hipMemcpyAsync(htot, tot, sizeof(htot), hipMemcpyDeviceToHost, st));
	PXS_HIP(hipStreamSynchronize(st));
	if (htot[0] <= 0) return 0;
	DevBuf& pairs = stream_scratch(SCR_SRC_PAIRS, device, stream); pairs.ensure(2*sizeof(ObjRec)*(size_t)htot[0]);
	ObjRec* raw = pairs.as<ObjRec>(); ObjRec* list = raw + htot[0];
	const unsigned nwg = (unsigned)(htot[1] < SRC_MAXBLK ? htot[1] : SRC_MAXBLK);
	hipLaunchKernelGGL(tile_fill_kernel, dim3(blocks_of(nobj)), dim3(256), 0, st, g, (int)ntx, (long)nobj, (const Box*)box, d_obj_dec, d_obj_ra, d_prof_ids, pr, (const float*)rcut, (const long long*)off, cur, raw);
	hipLaunchKernelGGL(tile_sort_kernel, dim3(nwg), dim3(256), 256*sizeof(int), st, (const TileRec*)act, (const long long*)tot, (const ObjRec*)raw, list);
	const int nprofl = nsamp <= PROF_LDS ? (int)nsamp : 0;
	const size_t shmem = sizeof(float)*((size_t)2*nprofl + 2*NCH*TILE + 5*NCH);
	if (map_dtype == PX_F32) launch_paint<float>(op, dim3(nwg), shmem, st, g, (int)ntx, d_map, ncomp, (long)map_cstride, d_amps, (long)amp_cstride, pr, nprofl, act, tot, list);
	else launch_paint<double>(op, dim3(nwg), shmem, st, g, (int)ntx, d_map, ncomp, (long)map_cstride, d_amps, (long)amp_cstride, pr, nprofl, act, tot, list);
	PXS_HIP(hipGetLastError());
	PXS_CATCH
}

int pxm_radial_sum(int ny, int nx, double dec0, double ddec, double ra0, double dra, const void* d_map, int map_dtype, int ncomp, int64_t map_cstride,
                   int64_t nobj, const float* d_obj_dec, const float* d_obj_ra, int nbin, const float* d_bins, double rlast, int equi, float* d_oprofs,
                   int device, void* stream)
{
	PXS_TRY
	PXS_REQUIRE(ny >= 1 && nx >= 1 && ncomp >= 0 && nobj >= 0 && nobj < (int64_t(1) << 31) && nbin >= 0, "pxm_radial_sum: bad sizes");
	const PixGeo g = make_pixgeo("pxm_radial_sum", ny, nx, dec0, ddec, ra0, dra);
	PXS_REQUIRE(map_dtype == PX_F32 || map_dtype == PX_F64, "pxm_radial_sum: the map must be float32 or float64");
	if (nobj == 0 || ncomp == 0 || nbin == 0) return 0;
	PXS_REQUIRE(d_map && d_obj_dec && d_obj_ra && d_bins && d_oprofs && rlast >= 0, "pxm_radial_sum: bad arguments");
	PXS_REQUIRE(ncomp == 1 || map_cstride >= (int64_t)ny*nx, "pxm_radial_sum: the components overlap");
	PXS_REQUIRE((size_t)ncomp*nbin*sizeof(float) <= 48*1024, "pxm_radial_sum: components x bins must not exceed 12288");
	PXS_HIP(hipSetDevice(device));
	hipStream_t st = (hipStream_t)stream;
	DevBuf& fixed = stream_scratch(SCR_SRC_FIXED, device, stream);
	Carve cv;
	const size_t o_rcut = cv.take(4*(size_t)nobj), o_box = cv.take(sizeof(Box)*(size_t)nobj);
	fixed.ensure(cv.at);
	char* base = fixed.as<char>();
	float* rcut = (float*)(base + o_rcut); Box* box = (Box*)(base + o_box);
	const Prof none = {0, nullptr, nullptr, nullptr, nullptr, 0};
	hipLaunchKernelGGL(obj_prep_kernel, dim3(blocks_of(nobj)), dim3(256), 0, st, g, (long)nobj, d_obj_dec, d_obj_ra, (const float*)nullptr, 0, 0l,
		(const int*)nullptr, none, 0.0f, 0.0f, (float)rlast, rcut, box);
	const size_t shmem = sizeof(float)*(size_t)ncomp*nbin;
	if (map_dtype == PX_F32) hipLaunchKernelGGL((radial_sum_kernel<float>), dim3((unsigned)nobj), dim3(256), shmem, st, g, (const float*)d_map, ncomp, (long)map_cstride, d_obj_dec, d_obj_ra, nbin, d_bins, equi ? 1 : 0, (const Box*)box, d_oprofs);
	else hipLaunchKernelGGL((radial_sum_kernel<double>), dim3((unsigned)nobj), dim3(256), shmem, st, g, (const double*)d_map, ncomp, (long)map_cstride, d_obj_dec, d_obj_ra, nbin, d_bins, equi ? 1 : 0, (const Box*)box, d_oprofs);
	PXS_HIP(hipGetLastError());
	PXS_CATCH
}

} // extern "C"
