// The scan of per-tile counts into list offsets and a compact list of the tiles that have a count, shared by the kernels that build
// per-tile lists (srcsim.hip: objects per tile; distance.hip: points per cell, edge pixels per block of pixels).  Kernels are static:
// every translation unit that includes this header gets its own copies.
#pragma once
#include "common.hpp"

namespace pxs {

static constexpr int SCAN_PER = 4;        // tiles per lane of the scan
struct TileRec { long long off; int tile, n; };      // a tile with a count: its list is entries off .. off + n - 1

// exclusive sums over the 256 lanes of a workgroup of a 64-bit and a 32-bit number at once; sc[256], sa[256]: LDS
__device__ static inline void block_scan2(long long lc, int la, long long* sc, int* sa, long long& ex_c, int& ex_a, long long& tot_c, int& tot_a) {
	const int t = threadIdx.x;
	sc[t] = lc; sa[t] = la;
	__syncthreads();
	for (int d = 1; d < 256; d <<= 1) {
		const long long a = t >= d ? sc[t-d] : 0; const int b = t >= d ? sa[t-d] : 0;
		__syncthreads();
		sc[t] += a; sa[t] += b;
		__syncthreads();
	}
	ex_c = sc[t] - lc; ex_a = sa[t] - la; tot_c = sc[255]; tot_a = sa[255];
	__syncthreads();
}

// the scan of the tile counts in three steps: sums per workgroup of 256*SCAN_PER tiles; their exclusive sums and the totals (one workgroup);
// off[tile] and the list `act` of the tiles with a count.  tot[0]: pairs of (tile, object), tot[1]: tiles with objects
static __global__ __launch_bounds__(256) void scan_part_kernel(int ntiles, const int* __restrict__ cnt, long long* __restrict__ bs_c, int* __restrict__ bs_a)
{
	PXS_SHARED(long long, ssh); long long* sc = ssh; int* sa = (int*)(ssh + 256);
	const long base = ((long)blockIdx.x*256 + threadIdx.x)*SCAN_PER;
	long long lc = 0; int la = 0;
	for (int k = 0; k < SCAN_PER; k++) if (base + k < ntiles) { const int v = cnt[base + k]; lc += v; la += v > 0; }
	long long ec, tc; int ea, ta;
	block_scan2(lc, la, sc, sa, ec, ea, tc, ta);
	if (threadIdx.x == 0) { bs_c[blockIdx.x] = tc; bs_a[blockIdx.x] = ta; }
}
static __global__ __launch_bounds__(256) void scan_top_kernel(int nblk, long long* __restrict__ bs_c, int* __restrict__ bs_a, long long* __restrict__ tot)
{
	PXS_SHARED(long long, ssh); long long* sc = ssh; int* sa = (int*)(ssh + 256);
	long long run_c = 0; int run_a = 0;
	for (int b0 = 0; b0 < nblk; b0 += 256) {
		const int b = b0 + threadIdx.x;
		const long long lc = b < nblk ? bs_c[b] : 0; const int la = b < nblk ? bs_a[b] : 0;
		long long ec, tc; int ea, ta;
		block_scan2(lc, la, sc, sa, ec, ea, tc, ta);
		if (b < nblk) { bs_c[b] = run_c + ec; bs_a[b] = run_a + ea; }
		run_c += tc; run_a += ta;
	}
	if (threadIdx.x == 0) { tot[0] = run_c; tot[1] = run_a; }
}
static __global__ __launch_bounds__(256) void scan_apply_kernel(int ntiles, const int* __restrict__ cnt, const long long* __restrict__ bs_c, const int* __restrict__ bs_a,
		long long* __restrict__ off, TileRec* __restrict__ act)
{
	PXS_SHARED(long long, ssh); long long* sc = ssh; int* sa = (int*)(ssh + 256);
	const long base = ((long)blockIdx.x*256 + threadIdx.x)*SCAN_PER;
	int v[SCAN_PER]; long long lc = 0; int la = 0;
	for (int k = 0; k < SCAN_PER; k++) { v[k] = base + k < ntiles ? cnt[base + k] : 0; lc += v[k]; la += v[k] > 0; }
	long long ec, tc; int ea, ta;
	block_scan2(lc, la, sc, sa, ec, ea, tc, ta);
	ec += bs_c[blockIdx.x]; ea += bs_a[blockIdx.x];
	for (int k = 0; k < SCAN_PER; k++) if (base + k < ntiles) {
		off[base + k] = ec;
		if (v[k] > 0) { TileRec t; t.off = ec; t.tile = (int)(base + k); t.n = v[k]; act[ea++] = t; }
		ec += v[k];
	}
}


// cnt[n] -> off[n], act, tot; bsc, bsa: one entry per workgroup of the scan, (n + 256*SCAN_PER - 1)/(256*SCAN_PER) of them
static const size_t SCAN_LDS = 256*sizeof(long long) + 256*sizeof(int);
static inline void scan_counts(hipStream_t st, int n, const int* cnt, long long* bsc, int* bsa, long long* tot, long long* off, TileRec* act) {
	const int nblk = (n + 256*SCAN_PER - 1)/(256*SCAN_PER);
	hipLaunchKernelGGL(scan_part_kernel, dim3(nblk), dim3(256), SCAN_LDS, st, n, cnt, bsc, bsa);
	hipLaunchKernelGGL(scan_top_kernel, dim3(1), dim3(256), SCAN_LDS, st, nblk, bsc, bsa, tot);
	hipLaunchKernelGGL(scan_apply_kernel, dim3(nblk), dim3(256), SCAN_LDS, st, n, cnt, (const long long*)bsc, (const int*)bsa, off, act);
}

} // namespace pxs
