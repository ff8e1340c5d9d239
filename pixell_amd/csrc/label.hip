// Connected-component labelling of a mask, per-label reductions over a label map, and the per-pixel small solve of a map of linear
// systems: what the reference's analysis.py asks of scipy.ndimage (label, center_of_mass, maximum, ...) and of np.linalg.solve
// (analysis.py:553-564, 1052-1060), on maps that stay on the device.
//
// pxm_label.  Union-find with parent <= self over flat pixel indices, so the root of a component is its lowest pixel; the label array is
// the parent array: a foreground pixel holds parent + 1, background holds 0.  Launches, in stream order, none of which waits for another
// workgroup:
//   (a) tile_kernel      one workgroup labels a TILE x TILE tile in LDS and writes the tile-local roots as global indices; a tile without
//                        foreground costs its read of the mask and a store of zeros
//   (b) merge_*_kernel   the pixels of the first row / column of every tile unite with their neighbours in the tile above / to the left
//                        (and column 0 with column nx-1 when the map wraps): atomicMin on the larger root, nothing else
//   (c) flatten_kernel   every pixel gets its root; roots (parent == self) are counted per block of 256*PER pixels
//   (d) scan_counts, rank_kernel (the k-th root in index order becomes -(k+1)), final_kernel (every pixel takes |word of its root|)
// Every find loop follows strictly decreasing parents and every union retries on a strictly smaller pair, so all loops end.  From (b) on
// a parent word only changes through atomicMin, and the finds of (b) read with relaxed agent-scope atomic loads: the L2s of the XCDs are not
// coherent for plain loads within a kernel, and a stale parent is harmless only because it is still an ancestor.
// The numbering is that of a raster-order flood fill (scipy.ndimage.label): a pure function of the mask.
//
// pxm_label_stats.  One pass over the label map: the lanes of a wave that hold the same label combine with wave shuffles (the first two
// distinct labels of a wave; what is left goes lane by lane) before one lane touches memory.  count, box, max, min are integer or
// ordered-key atomics and the arg indices an atomicMin over the pixels that hold the extreme value, all independent of the order of
// arrival; the four sums are float64 atomicAdds in arrival order.
//
// pxm_solve_mapsys.  One lane per pixel, the n x n system in registers, in-place Gauss-Jordan elimination with partial (row) pivoting in
// FP64; the loops are unrolled and rows swap through compile-time indices so that nothing is indexed at run time.
#include "common.hpp"
#include "scan_dev.hpp"
#include <cmath>
#include <climits>

namespace pxs {
namespace lab {

static constexpr int TILE = 16;      // a tile is TILE x TILE pixels: one lane of a 256-lane workgroup per pixel
static constexpr int PER = 4;        // consecutive pixels per lane of the flat passes: one 16-byte access
static constexpr int ROWS = 4;       // rows per workgroup of the reductions (more where the grid would not fit)

struct alignas(16) Quad { int v[PER]; };

#define PXS_LD_WG(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
#define PXS_LD_AGENT(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

// ---- (a) tiles ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int lds_find(int* s, int i) {
	int v = PXS_LD_WG(s + i);
	while (v != i) { i = v; v = PXS_LD_WG(s + i); }      // v < i: ends
	return i;
}
__device__ __forceinline__ void lds_unite(int* s, int a, int b) {
	for (;;) {
		a = lds_find(s, a); b = lds_find(s, b);
		if (a == b) return;
		if (a < b) { const int t = a; a = b; b = t; }
		const int old = atomicMin(&s[a], b);
		if (old == a) return;
		a = old;      // somebody linked a below itself first: old < a, unite that with b
	}
}
template<int CONN> __global__ __launch_bounds__(256) void tile_kernel(int ny, int nx, int ntx, const uint8_t* __restrict__ mask, int* __restrict__ L)
{
	PXS_SHARED(int, sl);      // 256 parents (-1: background) and one flag
	const int t = threadIdx.x, ly = t >> 4, lx = t & (TILE - 1);
	const int ty = (int)(blockIdx.x/ntx), tx = (int)(blockIdx.x - (unsigned)ty*ntx);
	const int y = ty*TILE + ly, x = tx*TILE + lx;
	const bool in = y < ny && x < nx;
	const long p = (long)y*nx + x;
	const bool fg = in && mask[p] != 0;
	if (t == 0) sl[256] = 0;
	sl[t] = fg ? t : -1;
	__syncthreads();
	if (fg) sl[256] = 1;
	__syncthreads();
	if (!sl[256]) { if (in) L[p] = 0; return; }
	if (fg) {
		if (lx > 0 && sl[t-1] >= 0) lds_unite(sl, t, t - 1);
		if (ly > 0) {
			if (sl[t-TILE] >= 0) lds_unite(sl, t, t - TILE);
			if (CONN == 2) {
				if (lx > 0 && sl[t-TILE-1] >= 0) lds_unite(sl, t, t - TILE - 1);
				if (lx < TILE - 1 && sl[t-TILE+1] >= 0) lds_unite(sl, t, t - TILE + 1);
			}
		}
	}
	__syncthreads();
	if (!in) return;
	int out = 0;
	if (fg) { const int r = lds_find(sl, t); out = (ty*TILE + (r >> 4))*nx + tx*TILE + (r & (TILE - 1)) + 1; }
	L[p] = out;
}

// ---- (b) across the borders of the tiles ----------------------------------------------------------------------------------------
__device__ __forceinline__ int glob_find(int* L, int i) {
	int v = PXS_LD_AGENT(L + i) - 1;
	while (v != i) { i = v; v = PXS_LD_AGENT(L + i) - 1; }      // v < i: ends
	return i;
}
__device__ __forceinline__ void glob_unite(int* L, int a, int b) {
	for (;;) {
		a = glob_find(L, a); b = glob_find(L, b);
		if (a == b) return;
		if (a < b) { const int t = a; a = b; b = t; }
		const int old = atomicMin(&L[a], b + 1) - 1;
		if (old == a) return;
		a = old;
	}
}
// the first row of every tile row but the first, with the row above it
template<int CONN> __global__ __launch_bounds__(256) void merge_rows_kernel(int ny, int nx, int wrap, int* L)
{
	const long i = (long)blockIdx.x*256 + threadIdx.x;
	const int nrb = (ny - 1)/TILE;
	if (i >= (long)nrb*nx) return;
	const int k = (int)(i/nx), x = (int)(i - (long)k*nx), y = (k + 1)*TILE;
	const int p = y*nx + x, q0 = p - nx - x;
	if (L[p] == 0) return;
	if (L[q0+x] != 0) glob_unite(L, p, q0 + x);
	if (CONN == 2) {
		const int xl = x > 0 ? x - 1 : (wrap ? nx - 1 : -1), xr = x < nx - 1 ? x + 1 : (wrap ? 0 : -1);
		if (xl >= 0 && L[q0+xl] != 0) glob_unite(L, p, q0 + xl);
		if (xr >= 0 && L[q0+xr] != 0) glob_unite(L, p, q0 + xr);
	}
}
// the first column of every tile column but the first, with the column to its left; with wrap, column 0 with column nx-1
template<int CONN> __global__ __launch_bounds__(256) void merge_cols_kernel(int ny, int nx, int wrap, int* L)
{
	const long i = (long)blockIdx.x*256 + threadIdx.x;
	const int ncb = (nx - 1)/TILE + (wrap ? 1 : 0);
	if (i >= (long)ncb*ny) return;
	const int y = (int)(i/ncb), j = (int)(i - (long)y*ncb);
	const int x = (j + (wrap ? 0 : 1))*TILE, xl = x > 0 ? x - 1 : nx - 1;
	const int p = y*nx + x;
	if (L[p] == 0) return;
	if (L[p-x+xl] != 0) glob_unite(L, p, p - x + xl);
	if (CONN == 2) {
		if (y > 0 && L[p-nx-x+xl] != 0) glob_unite(L, p, p - nx - x + xl);
		if (y < ny - 1 && L[p+nx-x+xl] != 0) glob_unite(L, p, p + nx - x + xl);
	}
}

// ---- (c), (d) roots, ranks, labels ----------------------------------------------------------------------------------------------
__device__ __forceinline__ Quad load_quad(const int* L, long base, long npix) {
	Quad q;
	if (base + PER <= npix) q = *reinterpret_cast<const Quad*>(L + base);
	else for (int k = 0; k < PER; k++) q.v[k] = base + k < npix ? L[base+k] : 0;
	return q;
}
__device__ __forceinline__ void store_quad(int* L, long base, long npix, const Quad& q) {
	if (base + PER <= npix) *reinterpret_cast<Quad*>(L + base) = q;
	else for (int k = 0; k < PER; k++) if (base + k < npix) L[base+k] = q.v[k];
}
__global__ __launch_bounds__(256) void flatten_kernel(long npix, int* L, int* __restrict__ bcnt)
{
	PXS_SHARED(int, sn);
	if (threadIdx.x == 0) sn[0] = 0;
	__syncthreads();
	const long base = ((long)blockIdx.x*256 + threadIdx.x)*PER;
	Quad q = load_quad(L, base, npix);
	int n = 0; bool changed = false;
	for (int k = 0; k < PER; k++) if (q.v[k] != 0) {
		if (q.v[k] - 1 == base + k) n++;
		else { const int r = glob_find(L, q.v[k] - 1) + 1; if (r != q.v[k]) { q.v[k] = r; changed = true; } }
	}
	if (changed) store_quad(L, base, npix, q);      // (words of this lane alone; what others read of them on their way down is an ancestor either way)
	if (n) atomicAdd(&sn[0], n);
	__syncthreads();
	if (threadIdx.x == 0) bcnt[blockIdx.x] = sn[0];
}
__global__ __launch_bounds__(256) void rank_kernel(long npix, int* L, const int* __restrict__ bcnt, const long long* __restrict__ off)
{
	PXS_SHARED(long long, ssh); long long* sc = ssh; int* sa = (int*)(ssh + 256);
	if (bcnt[blockIdx.x] == 0) return;      // (the whole workgroup)
	const long base = ((long)blockIdx.x*256 + threadIdx.x)*PER;
	const Quad q = load_quad(L, base, npix);
	int n = 0;
	for (int k = 0; k < PER; k++) n += q.v[k] != 0 && q.v[k] - 1 == base + k;
	long long ec, tc; int ea, ta;
	block_scan2(n, 0, sc, sa, ec, ea, tc, ta);
	long long rank = off[blockIdx.x] + ec;
	for (int k = 0; k < PER; k++) if (q.v[k] != 0 && q.v[k] - 1 == base + k) L[base+k] = -(int)(++rank);
}
// the word of a root is -label before its own lane has been here and +label after: both say the same
__global__ __launch_bounds__(256) void final_kernel(long npix, int* L)
{
	const long base = ((long)blockIdx.x*256 + threadIdx.x)*PER;
	Quad q = load_quad(L, base, npix);
	bool any = false;
	for (int k = 0; k < PER; k++) if (q.v[k] != 0) {
		const int r = q.v[k] < 0 ? q.v[k] : PXS_LD_AGENT(L + q.v[k] - 1);
		q.v[k] = r < 0 ? -r : r; any = true;
	}
	if (any) store_quad(L, base, npix, q);
}

// ---- per-label reductions -------------------------------------------------------------------------------------------------------
// doubles as unsigned keys of the same order (-0 counts as +0)
__device__ __forceinline__ unsigned long long to_key(double v) {
	v += 0.0;
	unsigned long long b; memcpy(&b, &v, 8);
	return (b >> 63) ? ~b : (b | (1ull << 63));
}
__device__ __forceinline__ double from_key(unsigned long long k) {
	const unsigned long long b = (k >> 63) ? (k & ~(1ull << 63)) : ~k;
	double v; memcpy(&v, &b, 8); return v;
}
__device__ __forceinline__ double load_real(const void* p, int dt, long i) {
	return dt == PX_F64 ? ((const double*)p)[i] : (double)((const float*)p)[i];
}
#ifdef PXS_HOST_SIM
#define PXS_FIRST_LANE(m) __builtin_ctzll(m)
#else
#define PXS_FIRST_LANE(m) (__ffsll((long long)(m)) - 1)
#endif

struct StatOut {
	unsigned long long* count; int* box; double* sums; unsigned long long* kmax; unsigned long long* kmin;
	unsigned long long* amax; unsigned long long* amin;
};

__global__ __launch_bounds__(256) void stats_init_kernel(int nlabel, int ny, int nx, StatOut o)
{
	const long i = (long)blockIdx.x*256 + threadIdx.x;
	if (i >= nlabel) return;
	o.count[i] = 0;
	o.box[i] = ny; o.box[(long)nlabel+i] = -1; o.box[2l*nlabel+i] = nx; o.box[3l*nlabel+i] = -1;
	for (int k = 0; k < 4; k++) o.sums[(long)k*nlabel+i] = 0.0;
	o.kmax[i] = 0; o.kmin[i] = ~0ull; o.amax[i] = ~0ull; o.amin[i] = ~0ull;
}

__global__ __launch_bounds__(256) void stats_kernel(int ny, int nx, int rows, int nlabel, const int* __restrict__ lab, const void* __restrict__ V, int vdt,
		const void* __restrict__ W, int wdt, StatOut o, int* __restrict__ err)
{
	const int x = blockIdx.x*256 + threadIdx.x, lane = threadIdx.x & 63;
	const long nl = nlabel;
	for (int r = 0; r < rows; r++) {
		const int y = blockIdx.y*rows + r;      // (the same for the whole workgroup)
		if (y >= ny) break;
		const long p = (long)y*nx + x;
		int l = x < nx ? lab[p] : 0;
		if (l < 0 || l > nlabel) { atomicMax(err, 1); l = 0; }
		bool act = l > 0;
		double w = 1.0, v = 0.0;
		if (act) { if (W) w = load_real(W, wdt, p); if (V) v = load_real(V, vdt, p); }
		const unsigned long long key = to_key(v);
		for (int it = 0; it < 2; it++) {
			const unsigned long long m = __ballot(act);
			if (!m) break;
			const int leader = PXS_FIRST_LANE(m);
			const int l0 = __shfl(l, leader);
			const bool mine = act && l == l0;
			int c = mine, x0 = mine ? x : INT_MAX, x1 = mine ? x : -1;
			double sw = mine ? w : 0.0, swx = mine ? w*x : 0.0, sv = mine ? v : 0.0;
			long long k1 = (long long)(mine ? key : 0ull), k0 = (long long)(mine ? key : ~0ull);
			for (int d = 1; d < 64; d <<= 1) {
				c += __shfl_xor(c, d);
				const int a0 = __shfl_xor(x0, d), a1 = __shfl_xor(x1, d);
				x0 = a0 < x0 ? a0 : x0; x1 = a1 > x1 ? a1 : x1;
				sw += __shfl_xor(sw, d); swx += __shfl_xor(swx, d); sv += __shfl_xor(sv, d);
				const unsigned long long b1 = (unsigned long long)__shfl_xor(k1, d), b0 = (unsigned long long)__shfl_xor(k0, d);
				if (b1 > (unsigned long long)k1) k1 = (long long)b1;
				if (b0 < (unsigned long long)k0) k0 = (long long)b0;
			}
			if (lane == leader) {
				const long s = l0 - 1;
				atomicAdd(&o.count[s], (unsigned long long)c);
				atomicMin(&o.box[s], y); atomicMax(&o.box[nl+s], y); atomicMin(&o.box[2*nl+s], x0); atomicMax(&o.box[3*nl+s], x1);
				atomicAdd(&o.sums[s], sw); atomicAdd(&o.sums[nl+s], sw*y); atomicAdd(&o.sums[2*nl+s], swx);
				if (V) { atomicAdd(&o.sums[3*nl+s], sv); atomicMax(&o.kmax[s], (unsigned long long)k1); atomicMin(&o.kmin[s], (unsigned long long)k0); }
			}
			if (mine) act = false;
		}
		if (act) {      // a wave of many labels: what the two rounds left
			const long s = l - 1;
			atomicAdd(&o.count[s], 1ull);
			atomicMin(&o.box[s], y); atomicMax(&o.box[nl+s], y); atomicMin(&o.box[2*nl+s], x); atomicMax(&o.box[3*nl+s], x);
			atomicAdd(&o.sums[s], w); atomicAdd(&o.sums[nl+s], w*y); atomicAdd(&o.sums[2*nl+s], w*x);
			if (V) { atomicAdd(&o.sums[3*nl+s], v); atomicMax(&o.kmax[s], key); atomicMin(&o.kmin[s], key); }
		}
	}
}
// the lowest pixel that holds the extreme value of its label
__global__ __launch_bounds__(256) void stats_arg_kernel(int ny, int nx, int rows, int nlabel, const int* __restrict__ lab, const void* __restrict__ V, int vdt, StatOut o)
{
	const int x = blockIdx.x*256 + threadIdx.x;
	if (x >= nx) return;
	for (int r = 0; r < rows; r++) {
		const int y = blockIdx.y*rows + r;
		if (y >= ny) break;
		const long p = (long)y*nx + x;
		const int l = lab[p];
		if (l <= 0 || l > nlabel) continue;
		const unsigned long long key = to_key(load_real(V, vdt, p));
		if (key == o.kmax[l-1]) atomicMin(&o.amax[l-1], (unsigned long long)p);
		if (key == o.kmin[l-1]) atomicMin(&o.amin[l-1], (unsigned long long)p);
	}
}
__global__ __launch_bounds__(256) void stats_final_kernel(int nlabel, int have_v, StatOut o)
{
	const long i = (long)blockIdx.x*256 + threadIdx.x;
	if (i >= nlabel) return;
	const bool have = have_v && o.count[i] > 0;
	const double vmax = have ? from_key(o.kmax[i]) : NAN, vmin = have ? from_key(o.kmin[i]) : NAN;
	((double*)o.kmax)[i] = vmax; ((double*)o.kmin)[i] = vmin;
}

// ---- the per-pixel solve --------------------------------------------------------------------------------------------------------
template<int N, class T> __global__ __launch_bounds__(256) void solve_kernel(long npix, const T* __restrict__ K, const T* __restrict__ R, T* __restrict__ F, T* __restrict__ D)
{
	const long p = (long)blockIdx.x*256 + threadIdx.x;
	if (p >= npix) return;
	double A[N][N], b[N]; int perm[N];
	#pragma unroll
	for (int i = 0; i < N; i++) {
		#pragma unroll
		for (int j = 0; j < N; j++) A[i][j] = (double)K[(long)(i*N+j)*npix + p];
		b[i] = (double)R[(long)i*npix + p]; perm[i] = i;
	}
	bool singular = false;
	#pragma unroll
	for (int k = 0; k < N; k++) {
		int piv = k; double big = fabs(A[k][k]);
		#pragma unroll
		for (int r = k + 1; r < N; r++) { const double a = fabs(A[r][k]); if (a > big) { big = a; piv = r; } }
		if (!(big > 0)) singular = true;      // (a zero or a NaN column)
		#pragma unroll
		for (int r = k + 1; r < N; r++) if (r == piv) {
			#pragma unroll
			for (int j = 0; j < N; j++) { const double t = A[k][j]; A[k][j] = A[r][j]; A[r][j] = t; }
			const double t = b[k]; b[k] = b[r]; b[r] = t;
			const int u = perm[k]; perm[k] = perm[r]; perm[r] = u;
		}
		// column k of the matrix makes way for column k of the inverse of the row-permuted matrix
		const double d = A[k][k];
		A[k][k] = 1.0;
		#pragma unroll
		for (int j = 0; j < N; j++) A[k][j] /= d;
		b[k] /= d;
		#pragma unroll
		for (int i = 0; i < N; i++) if (i != k) {
			const double f = A[i][k];
			A[i][k] = 0.0;
			#pragma unroll
			for (int j = 0; j < N; j++) A[i][j] -= f*A[k][j];
			b[i] -= f*b[k];
		}
	}
	// A holds inv(P K), P the row swaps: inv(K)[a][a] = A[a][j] for the j with perm[j] == a
	#pragma unroll
	for (int a = 0; a < N; a++) {
		double dg = 0.0;
		#pragma unroll
		for (int j = 0; j < N; j++) if (perm[j] == a) dg = A[a][j];
		F[(long)a*npix + p] = singular ? (T)NAN : (T)b[a];
		D[(long)a*npix + p] = singular ? (T)NAN : (T)sqrt(dg);
	}
}
template<int N> void run_solve(hipStream_t st, long npix, const void* K, const void* R, void* F, void* D, int dtype)
{
	if (dtype == PX_F64) hipLaunchKernelGGL((solve_kernel<N, double>), dim3(blocks_of(npix)), dim3(256), 0, st, npix, (const double*)K, (const double*)R, (double*)F, (double*)D);
	else hipLaunchKernelGGL((solve_kernel<N, float>), dim3(blocks_of(npix)), dim3(256), 0, st, npix, (const float*)K, (const float*)R, (float*)F, (float*)D);
}

template<int CONN> void run_label(hipStream_t st, int ny, int nx, int wrap, const uint8_t* mask, int* L)
{
	const int ntx = (nx + TILE - 1)/TILE, nty = (ny + TILE - 1)/TILE;
	hipLaunchKernelGGL((tile_kernel<CONN>), dim3((unsigned)((long)ntx*nty)), dim3(256), 257*sizeof(int), st, ny, nx, ntx, mask, L);
	const long nrow = (long)((ny - 1)/TILE)*nx, ncol = (long)((nx - 1)/TILE + (wrap ? 1 : 0))*ny;
	if (nrow > 0) hipLaunchKernelGGL((merge_rows_kernel<CONN>), dim3(blocks_of(nrow)), dim3(256), 0, st, ny, nx, wrap, L);
	if (ncol > 0) hipLaunchKernelGGL((merge_cols_kernel<CONN>), dim3(blocks_of(ncol)), dim3(256), 0, st, ny, nx, wrap, L);
}

} // namespace lab
} // namespace pxs

using namespace pxs;
using namespace pxs::lab;

extern "C" {

int pxm_label(int ny, int nx, const void* d_mask, int connectivity, int wrap_x, int32_t* d_labels, int64_t* count, int device, void* stream)
{
	PXS_TRY
	PXS_REQUIRE(ny >= 1 && nx >= 1 && d_mask && d_labels, "pxm_label: bad arguments");
	PXS_REQUIRE(connectivity == 1 || connectivity == 2, "pxm_label: connectivity must be 1 or 2");
	PXS_REQUIRE(wrap_x == 0 || wrap_x == 1, "pxm_label: wrap_x must be 0 or 1");
	const long npix = (long)ny*nx;
	PXS_REQUIRE(npix < (1l << 31), "pxm_label: the map must have fewer than 2^31 pixels");
	PXS_REQUIRE(((uintptr_t)d_labels & 15) == 0, "pxm_label: the labels must be 16-byte aligned");
	const int nblk = (int)((npix + 256*PER - 1)/(256*PER)), nsb = (nblk + 256*SCAN_PER - 1)/(256*SCAN_PER);
	PXS_HIP(hipSetDevice(device));
	hipStream_t st = (hipStream_t)stream;
	DevBuf& fixed = stream_scratch(SCR_LABEL, device, stream);
	Carve cv;
	const size_t o_cnt = cv.take(4*(size_t)nblk), o_off = cv.take(8*(size_t)nblk), o_act = cv.take(sizeof(TileRec)*(size_t)nblk);
	const size_t o_bsc = cv.take(8*(size_t)nsb), o_bsa = cv.take(4*(size_t)nsb), o_tot = cv.take(16);
	fixed.ensure(cv.at);
	char* base = fixed.as<char>();
	int* bcnt = (int*)(base + o_cnt); long long* off = (long long*)(base + o_off); TileRec* act = (TileRec*)(base + o_act);
	long long* bsc = (long long*)(base + o_bsc); int* bsa = (int*)(base + o_bsa); long long* tot = (long long*)(base + o_tot);
	if (connectivity == 1) run_label<1>(st, ny, nx, wrap_x, (const uint8_t*)d_mask, d_labels);
	else run_label<2>(st, ny, nx, wrap_x, (const uint8_t*)d_mask, d_labels);
	hipLaunchKernelGGL(flatten_kernel, dim3(nblk), dim3(256), sizeof(int), st, npix, d_labels, bcnt);
	scan_counts(st, nblk, bcnt, bsc, bsa, tot, off, act);
	hipLaunchKernelGGL(rank_kernel, dim3(nblk), dim3(256), SCAN_LDS, st, npix, d_labels, (const int*)bcnt, (const long long*)off);
	hipLaunchKernelGGL(final_kernel, dim3(nblk), dim3(256), 0, st, npix, d_labels);
	PXS_HIP(hipGetLastError());
	if (count) {      // the one number the host needs: how many components there are
		long long htot[2] = {0, 0};
		PXS_HIP(hipMemcpyAsync(htot, tot, sizeof(htot), hipMemcpyDeviceToHost, st));
		PXS_HIP(hipStreamSynchronize(st));
		*count = htot[0];
	}
	PXS_CATCH
}

int pxm_label_stats(int ny, int nx, const int32_t* d_labels, int64_t nlabel, const void* d_v, int v_dtype, const void* d_w, int w_dtype,
		int64_t* d_count, int32_t* d_box, double* d_sums, double* d_vmax, double* d_vmin, int64_t* d_argmax, int64_t* d_argmin, int device, void* stream)
{
	PXS_TRY
	PXS_REQUIRE(ny >= 1 && nx >= 1 && d_labels && nlabel >= 0 && nlabel < (int64_t(1) << 31) - 1, "pxm_label_stats: bad arguments");
	PXS_REQUIRE(!d_v || v_dtype == PX_F32 || v_dtype == PX_F64, "pxm_label_stats: the values must be float32 or float64");
	PXS_REQUIRE(!d_w || w_dtype == PX_F32 || w_dtype == PX_F64, "pxm_label_stats: the weights must be float32 or float64");
	PXS_REQUIRE(nlabel == 0 || (d_count && d_box && d_sums && d_vmax && d_vmin && d_argmax && d_argmin), "pxm_label_stats: null output");
	PXS_HIP(hipSetDevice(device));
	hipStream_t st = (hipStream_t)stream;
	DevBuf& fixed = stream_scratch(SCR_LABEL, device, stream);
	fixed.ensure(16);
	int* err = fixed.as<int>();
	PXS_HIP(hipMemsetAsync(err, 0, sizeof(int), st));
	StatOut o{(unsigned long long*)d_count, d_box, d_sums, (unsigned long long*)d_vmax, (unsigned long long*)d_vmin, (unsigned long long*)d_argmax, (unsigned long long*)d_argmin};
	const int nl = (int)nlabel;
	if (nl > 0) hipLaunchKernelGGL(stats_init_kernel, dim3(blocks_of(nl)), dim3(256), 0, st, nl, ny, nx, o);
	const int rows = std::max(ROWS, (ny + 65534)/65535);
	const dim3 grid((nx + 255)/256, (ny + rows - 1)/rows);
	hipLaunchKernelGGL(stats_kernel, grid, dim3(256), 0, st, ny, nx, rows, nl, (const int*)d_labels, d_v, v_dtype, d_w, w_dtype, o, err);
	if (nl > 0 && d_v) hipLaunchKernelGGL(stats_arg_kernel, grid, dim3(256), 0, st, ny, nx, rows, nl, (const int*)d_labels, d_v, v_dtype, o);
	if (nl > 0) hipLaunchKernelGGL(stats_final_kernel, dim3(blocks_of(nl)), dim3(256), 0, st, nl, d_v ? 1 : 0, o);
	PXS_HIP(hipGetLastError());
	int herr = 0;
	PXS_HIP(hipMemcpyAsync(&herr, err, sizeof(int), hipMemcpyDeviceToHost, st));
	PXS_HIP(hipStreamSynchronize(st));
	PXS_REQUIRE(herr == 0, "pxm_label_stats: a label lies outside 0..nlabel");
	PXS_CATCH
}

int pxm_solve_mapsys(int n, int64_t npix, const void* d_kappa, const void* d_rho, void* d_flux, void* d_dflux, int dtype, int device, void* stream)
{
	PXS_TRY
	PXS_REQUIRE(npix >= 0 && (npix == 0 || (d_kappa && d_rho && d_flux && d_dflux)), "pxm_solve_mapsys: bad arguments");
	PXS_REQUIRE(dtype == PX_F32 || dtype == PX_F64, "pxm_solve_mapsys: the maps must be float32 or float64");
	if (n < 2 || n > 8) throw Error(PXS_ERR_UNSUPPORTED, "pxm_solve_mapsys: systems of 2 to 8 components only");
	if (npix == 0) return 0;
	PXS_HIP(hipSetDevice(device));
	hipStream_t st = (hipStream_t)stream;
	switch (n) {
		case 2: run_solve<2>(st, npix, d_kappa, d_rho, d_flux, d_dflux, dtype); break;
		case 3: run_solve<3>(st, npix, d_kappa, d_rho, d_flux, d_dflux, dtype); break;
		case 4: run_solve<4>(st, npix, d_kappa, d_rho, d_flux, d_dflux, dtype); break;
		case 5: run_solve<5>(st, npix, d_kappa, d_rho, d_flux, d_dflux, dtype); break;
		case 6: run_solve<6>(st, npix, d_kappa, d_rho, d_flux, d_dflux, dtype); break;
		case 7: run_solve<7>(st, npix, d_kappa, d_rho, d_flux, d_dflux, dtype); break;
		default: run_solve<8>(st, npix, d_kappa, d_rho, d_flux, d_dflux, dtype); break;
	}
	PXS_HIP(hipGetLastError());
	PXS_CATCH
}

} // extern "C"
