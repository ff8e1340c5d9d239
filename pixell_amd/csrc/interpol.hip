// Spline interpolation of maps [ny][nx] at arbitrary positions: what the reference's utils.interpol / SplineInterpolator (pixell/utils.py:630-783:
// scipy.ndimage.spline_filter followed by map_coordinates(prefilter=False)) gives enmap.at and enmap.project.  Two steps:
//
// pxm_spline_filter(_axes)   the cubic B-spline coefficients c of the samples f: along each axis B c = f, B the (1/6, 4/6, 1/6) collocation matrix under the
//   axis' extension rule (whole-sample mirror, half-sample reflect or periodic; _axes: one rule per axis, as a full-sky map wants them).  With z = sqrt(3) - 2 the solution is the two-sided sum
//   c[k] = G sum_j z^|j| f[k - j], G = -6z/(1 - z^2), over the extended samples, which the usual pair of recursions evaluates:
//       C+[k] = f[k] + z C+[k-1]             (causal)            c[k1] = G (C+[k1] + z C-[k1+1])      C-[k] = f[k] + z C-[k+1]
//       c[k]  = z (c[k+1] - 6 C+[k])         (anticausal)
//   |z|^k < 2^-53 from k = 28, so a line is cut into chunks of CHUNK samples and every chunk starts its recursions from nothing HALO = 32 samples
//   before its first and after its last sample, on its neighbours' samples or on the extension of the line: the result is the whole-line
//   recursion's to rounding, there is no start value to derive per rule, and a line of any length (1, 2, 3, ...) is a case of the same code.
//   y pass: a lane per column walks the rows of its chunk (the loads of a wave are a contiguous piece of a row).  x pass: a wave takes 64 rows
//   and walks its chunk in tiles of 64 rows x XT columns that go through LDS, so that global memory sees pieces of rows while every lane recurses
//   along its own row.  Each pass reads its input once (and the halos), writes C+, reads it back and writes c; a pass cannot work in place
//   (its halos are its neighbours' samples), so the y pass writes a caller-owned scratch map and the x pass reads it.  FP64 throughout.
//
// pxm_interpol   a lane per point: pixel coordinates by a per-axis affine map of the point's coordinates or of its index in an output grid, the
//   optional rewind of enmap.sky2pix(safe=True), the border rule, then tap indices and weights once and one sum per map.  No position map is
//   read that the caller did not have already.  Every tap index goes through the border's index rule, whatever the coordinate was.
#include "../../include/pxsht.h"
#include "common.hpp"
#include "interpol_dev.hpp"

namespace pxs {
namespace ipl {

static constexpr int CHUNK = 256;      // samples of a line per workgroup and pass (interpol.CHUNK in Python: the tests size their cases from it)
static constexpr int HALO = 32;        // samples a recursion runs before its results count
static constexpr int XT = 32;          // columns of an LDS tile of the x pass; CHUNK and HALO are multiples of it
static constexpr int XROWS = 64;       // rows of a tile: one per lane of the wave
static constexpr int XLD = XT + 1;     // row pitch of the tile in LDS (odd: the lanes of a wave, one row each, hit different banks)
static_assert(CHUNK % XT == 0 && HALO % XT == 0, "the tiles of the x pass must tile the chunk and its halos");

static constexpr double POLE = -0.26794919243112270647;      // sqrt(3) - 2
static constexpr double GAIN = -6.0*POLE/(1.0 - POLE*POLE);

// the y pass: in [nmap][ny][nx] of T, maps in_ms apart -> out [nmap][ny][nx] f64.  grid (ceil(nx/256), chunks of rows, nmap)
template<class T> __global__ __launch_bounds__(256) void filter_y_kernel(int ny, int nx, int ext, const T* __restrict__ in, long in_ms, double* out)
{
	const int x = blockIdx.x*256 + threadIdx.x;
	if (x >= nx) return;
	const T* f = in + (long)blockIdx.z*in_ms + x;
	double* o = out + (long)blockIdx.z*ny*nx + x;
	const int k0 = blockIdx.y*CHUNK, k1 = (k0 + CHUNK < ny ? k0 + CHUNK : ny) - 1;
	if (ny == 1) { o[0] = (double)f[0]; return; }
	double cp = 0.0;
	for (int k = k0 - HALO; k < k0; k++) cp = fma(POLE, cp, (double)f[(long)ext_index(ext, k, ny)*nx]);
	for (int k = k0; k <= k1; k++) { cp = fma(POLE, cp, (double)f[(long)k*nx]); o[(long)k*nx] = cp; }
	double cm = 0.0;
	for (int k = k1 + HALO; k > k1; k--) cm = fma(POLE, cm, (double)f[(long)ext_index(ext, k, ny)*nx]);
	double c = GAIN*fma(POLE, cm, cp);
	o[(long)k1*nx] = c;
	for (int k = k1 - 1; k >= k0; k--) { c = POLE*(c - 6.0*o[(long)k*nx]); o[(long)k*nx] = c; }
}

// the x pass: src -> dst, both [nmap][ny][nx] f64 and not the same.  grid (chunks of columns, ceil(ny/64), nmap), 64 lanes: lane r recurses
// along row blockIdx.y*64 + r, and the tile's loads and stores take two rows of XT columns per step
__global__ __launch_bounds__(64) void filter_x_kernel(int ny, int nx, int ext, const double* __restrict__ src, double* dst)
{
	PXS_SHARED(double, sh);
	const int lane = threadIdx.x, tc = lane % XT, tr = lane / XT;      // where this lane loads and stores within a step: column tc of row 2 step + tr
	const int y0 = blockIdx.y*XROWS;
	const long base = (long)blockIdx.z*ny*nx;
	const int k0 = blockIdx.x*CHUNK, k1 = (k0 + CHUNK < nx ? k0 + CHUNK : nx) - 1;
	if (nx == 1) { if (y0 + lane < ny) dst[base + y0 + lane] = src[base + y0 + lane]; return; }
	// the tile of columns c0 .. c0 + XT - 1 (extended) of p into LDS, or the columns <= k1 of it from LDS to dst
	auto load = [&](const double* p, int c0) {
		__syncthreads();
		const int col = ext_index(ext, (long)c0 + tc, nx);
		for (int s = 0; s < XROWS/2; s++) { const int r = 2*s + tr; if (y0 + r < ny) sh[r*XLD + tc] = p[base + (long)(y0 + r)*nx + col]; }
		__syncthreads();
	};
	auto store = [&](int c0) {
		__syncthreads();
		if (c0 + tc <= k1) for (int s = 0; s < XROWS/2; s++) { const int r = 2*s + tr; if (y0 + r < ny) dst[base + (long)(y0 + r)*nx + c0 + tc] = sh[r*XLD + tc]; }
	};
	double* row = sh + lane*XLD;
	double cp = 0.0;
	for (int c0 = k0 - HALO; c0 < k0; c0 += XT) { load(src, c0); for (int j = 0; j < XT; j++) cp = fma(POLE, cp, row[j]); }
	for (int c0 = k0; c0 <= k1; c0 += XT) {
		load(src, c0);
		const int m = k1 - c0 + 1 < XT ? k1 - c0 + 1 : XT;
		for (int j = 0; j < m; j++) { cp = fma(POLE, cp, row[j]); row[j] = cp; }
		store(c0);
	}
	double cm = 0.0;
	for (int c0 = k1 + 1 + HALO - XT; c0 > k1; c0 -= XT) { load(src, c0); for (int j = XT - 1; j >= 0; j--) cm = fma(POLE, cm, row[j]); }
	double c = GAIN*fma(POLE, cm, cp);
	const int last = k0 + (k1 - k0)/XT*XT;      // the tile that holds k1
	for (int c0 = last; c0 >= k0; c0 -= XT) {
		load(dst, c0);      // C+, as this workgroup stored it
		const int m = k1 - c0 + 1 < XT ? k1 - c0 + 1 : XT;
		for (int j = m - 1; j >= 0; j--) { if (c0 + j < k1) c = POLE*(c - 6.0*row[j]); row[j] = c; }
		store(c0);
	}
}

// ---- the gather ---------------------------------------------------------------------------------------------------------------------
struct Gather { Axis y, x; long npts; int onx; int order, border; };

// maps [nmap][ny][nx] of T, mstride apart -> out [nmap][npts] of T.  pts: f64 [2][npts], or null: point i is (i / onx, i % onx)
template<class T> __global__ __launch_bounds__(256) void gather_kernel(Gather g, int nmap, const T* __restrict__ maps, long mstride, const double* __restrict__ pts,
		T cval, T* __restrict__ out)
{
	const long i = (long)blockIdx.x*blockDim.x + threadIdx.x;
	if (i >= g.npts) return;
	double py, px;
	if (pts) { py = pts[i]; px = pts[g.npts + i]; }
	else { const long oy = i/g.onx; py = (double)oy; px = (double)(i - oy*g.onx); }
	double y, x;
	const bool in = axis_coord(g.y, py, g.order, g.border, y) & axis_coord(g.x, px, g.order, g.border, x);
	if (!in) { for (int m = 0; m < nmap; m++) out[(long)m*g.npts + i] = cval; return; }
	int iy[4], ix[4]; double wy[4], wx[4];
	axis_taps(g.y.n, y, g.order, g.border, iy, wy); axis_taps(g.x.n, x, g.order, g.border, ix, wx);
	if (g.order == 0) {      // a copy: exact in every dtype
		const long q = (long)iy[0]*g.x.n + ix[0];
		for (int m = 0; m < nmap; m++) out[(long)m*g.npts + i] = maps[(long)m*mstride + q];
		return;
	}
	const int nt = g.order + 1;
	for (int m = 0; m < nmap; m++) {
		const T* mp = maps + (long)m*mstride;
		double acc = 0.0;
		for (int a = 0; a < nt; a++) {
			const T* rp = mp + (long)iy[a]*g.x.n;
			double s = 0.0;
			for (int b = 0; b < nt; b++) s = fma(wx[b], (double)rp[ix[b]], s);
			acc = fma(wy[a], s, acc);
		}
		out[(long)m*g.npts + i] = (T)acc;
	}
}

template<class T> static void launch_gather(hipStream_t st, const Gather& g, int nmap, const void* maps, long mstride, const double* pts, double cval, void* out) {
	hipLaunchKernelGGL((gather_kernel<T>), dim3(blocks_of(g.npts)), dim3(256), 0, st, g, nmap, (const T*)maps, mstride, pts, (T)cval, (T*)out);
}

} // namespace ipl
} // namespace pxs

using namespace pxs;
using namespace pxs::ipl;

extern "C" {

int pxm_spline_filter_axes(int nmap, int ny, int nx, const void* d_in, int in_dtype, int64_t in_mstride, double* d_tmp, double* d_out,
                           int extension_y, int extension_x, int device, void* stream)
{
	PXS_TRY
	PXS_REQUIRE(nmap >= 0 && ny >= 1 && nx >= 1, "pxm_spline_filter: bad sizes");
	PXS_REQUIRE(in_dtype == PX_F32 || in_dtype == PX_F64, "pxm_spline_filter: the maps must be float32 or float64");
	for (int extension : {extension_y, extension_x})
		PXS_REQUIRE(extension == EXT_MIRROR || extension == EXT_REFLECT || extension == EXT_PERIODIC, "pxm_spline_filter: unknown extension rule");
	PXS_REQUIRE(nmap == 0 || (d_in && d_tmp && d_out && d_tmp != d_out && (const void*)d_tmp != d_in), "pxm_spline_filter: the input, the scratch and the output are three arrays");
	PXS_REQUIRE(nmap <= 1 || in_mstride >= (int64_t)ny*nx, "pxm_spline_filter: the maps overlap");
	const long ncy = (ny + CHUNK - 1)/CHUNK, ncx = (nx + CHUNK - 1)/CHUNK, nry = (ny + XROWS - 1)/XROWS;
	PXS_REQUIRE(ncy <= 65535 && nry <= 65535 && nmap <= 65535, "pxm_spline_filter: too many rows or maps for one launch");
	PXS_HIP(hipSetDevice(device));
	if (nmap == 0) return 0;
	hipStream_t st = (hipStream_t)stream;
	const dim3 gy(blocks_of(nx), (unsigned)ncy, (unsigned)nmap), gx((unsigned)ncx, (unsigned)nry, (unsigned)nmap);
	if (in_dtype == PX_F32) hipLaunchKernelGGL((filter_y_kernel<float>), gy, dim3(256), 0, st, ny, nx, extension_y, (const float*)d_in, (long)in_mstride, d_tmp);
	else hipLaunchKernelGGL((filter_y_kernel<double>), gy, dim3(256), 0, st, ny, nx, extension_y, (const double*)d_in, (long)in_mstride, d_tmp);
	hipLaunchKernelGGL(filter_x_kernel, gx, dim3(XROWS), sizeof(double)*XROWS*XLD, st, ny, nx, extension_x, (const double*)d_tmp, d_out);
	PXS_HIP(hipGetLastError());
	PXS_CATCH
}

int pxm_spline_filter(int nmap, int ny, int nx, const void* d_in, int in_dtype, int64_t in_mstride, double* d_tmp, double* d_out, int extension,
                      int device, void* stream)
{
	return pxm_spline_filter_axes(nmap, ny, nx, d_in, in_dtype, in_mstride, d_tmp, d_out, extension, extension, device, stream);
}

int pxm_interpol(int nmap, int ny, int nx, const void* d_maps, int map_dtype, int64_t mstride, int64_t npts, const double* d_pts, int ony, int onx,
                 double yoff, double yscale, double xoff, double xscale, double yref, double yper, double xref, double xper,
                 int order, int border, double cval, void* d_out, int device, void* stream)
{
	PXS_TRY
	PXS_REQUIRE(nmap >= 0 && ny >= 1 && nx >= 1 && npts >= 0, "pxm_interpol: bad sizes");
	PXS_REQUIRE(order == 0 || order == 1 || order == 3, "pxm_interpol: the order must be 0, 1 or 3");
	PXS_REQUIRE(border >= B_NEAREST && border <= B_GRIDWRAP, "pxm_interpol: unknown border rule");
	PXS_REQUIRE(map_dtype == PX_F32 || map_dtype == PX_F64 || (order == 0 && (map_dtype == PX_U8 || map_dtype == PX_I32)), "pxm_interpol: float32 or float64 maps (order 0: uint8 and int32 as well)");
	PXS_REQUIRE(order != 3 || map_dtype == PX_F64, "pxm_interpol: order 3 reads float64 coefficients");
	PXS_REQUIRE(nmap <= 1 || mstride >= (int64_t)ny*nx, "pxm_interpol: the maps overlap");
	PXS_REQUIRE(d_pts || (ony >= 0 && onx >= 1 && (int64_t)ony*onx == npts), "pxm_interpol: without points, ony*onx must equal npts");
	PXS_REQUIRE(yoff == yoff && yscale == yscale && xoff == xoff && xscale == xscale, "pxm_interpol: the affine map is not a number");
	PXS_REQUIRE((npts + 255)/256 < (int64_t(1) << 31), "pxm_interpol: too many points for one launch");
	PXS_HIP(hipSetDevice(device));
	if (nmap == 0 || npts == 0) return 0;
	PXS_REQUIRE(d_maps && d_out, "pxm_interpol: null arrays");
	const Gather g = {{ny, yoff, yscale, yref, yper}, {nx, xoff, xscale, xref, xper}, (long)npts, d_pts ? 1 : onx, order, border};
	hipStream_t st = (hipStream_t)stream;
	switch (map_dtype) {
		case PX_F32: launch_gather<float>(st, g, nmap, d_maps, (long)mstride, d_pts, cval, d_out); break;
		case PX_F64: launch_gather<double>(st, g, nmap, d_maps, (long)mstride, d_pts, cval, d_out); break;
		case PX_U8: launch_gather<uint8_t>(st, g, nmap, d_maps, (long)mstride, d_pts, cval, d_out); break;
		default: launch_gather<int32_t>(st, g, nmap, d_maps, (long)mstride, d_pts, cval, d_out); break;
	}
	PXS_HIP(hipGetLastError());
	PXS_CATCH
}

} // extern "C"
