// Curved-sky lensing between the two transforms of lensing.lens_map_curved (pixell/lensing.py:367-503): the observed pixel positions
// (enmap.posmap), their geodesic offset by the gradient of the lensing potential (lensing.offset_by_grad, :552-589; pole_wrap :623-632)
// and the polarisation rotation the parallel transport induces (enmap.rotate_pol, enmap.py:1402-1416).  Both kernels are one streaming
// pass over the pixels: HBM-bound, no LDS, a grid-stride loop over at most DEFLECT_MAXBLK blocks.
//
// The offset is taken in vector form, which has no special case at the poles.  With n the unit vector of the point, (e_theta, e_phi)
// the local basis there, d = |grad| and t = u_theta e_theta + u_phi e_phi the unit tangent along the gradient (zenith coordinates:
// u_theta = -grad_dec/d, u_phi = grad_ra/d):
//   n' = cos d n + sin d t                     the new point:  theta' = atan2(hypot(n'_x, n'_y), n'_z), phi' = atan2(n'_y, n'_x)
//   t' = -sin d n + cos d t                    the direction of travel, parallel-transported along the geodesic
//   psi = -2 (a' - a)                          a, a': the angle of t in (e_theta, e_phi) and of t' in (e_theta', e_phi')
// a' - a comes out of one atan2 of the cross and dot products of the two direction pairs, so that a small rotation keeps its relative accuracy.
#include "../../include/pxsht.h"
#include "common.hpp"

namespace pxs {

static constexpr int DEFLECT_MAXBLK = 2048;      // 256 CUs x 8 blocks of 256 threads: the rest of the pixels by the grid-stride loop

__device__ __forceinline__ double ld_real(const void* p, int dtype, long i) {
	return dtype == PX_F32 ? (double)((const float*)p)[i] : ((const double*)p)[i];
}

// ra into [0, 2 pi) (the form pxs_plan_points documents; it accepts any finite value, so the rounding case 2 pi is harmless)
__device__ __forceinline__ double wrap_2pi(double a) {
	if (a < 0 || a >= 2*PXS_PI) a -= 2*PXS_PI*floor(a/(2*PXS_PI));
	return a;
}

// pos == nullptr: pixel i of the separable CAR band [ny][nx] sits at dec0 + (i / nx) ddec, ra0 + (i % nx) dra; otherwise pos[{dec, ra}(, psi0)][npts]
__global__ __launch_bounds__(256) void deflect_kernel(long npts, int nx, double dec0, double ddec, double ra0, double dra,
		const double* __restrict__ pos, int pos_ncomp, const void* __restrict__ grad, int gdtype, long gstride, int geodesic,
		double2* __restrict__ loc, double* __restrict__ psi)
{
	const long step = (long)gridDim.x*blockDim.x;
	for (long i = (long)blockIdx.x*blockDim.x + threadIdx.x; i < npts; i += step) {
		double dec, ra, p0 = 0.0;
		if (pos) { dec = pos[i]; ra = pos[npts + i]; if (pos_ncomp > 2) p0 = pos[2*npts + i]; }
		else { const long y = i/nx; dec = dec0 + (double)y*ddec; ra = ra0 + (double)(i - y*nx)*dra; }
		const double g0 = ld_real(grad, gdtype, i), g1 = ld_real(grad, gdtype, gstride + i);
		double theta, phi, rot = p0;
		if (geodesic) {
			const double d = hypot(g0, g1);
			if (d > 0.0) {
				double sd, cd, sr, cr, sD, cD;
				sincos(dec, &sd, &cd); sincos(ra, &sr, &cr); sincos(d, &sD, &cD);
				const double ut = -g0/d, up = g1/d;
				// n = (cd cr, cd sr, sd), e_theta = (sd cr, sd sr, -cd), e_phi = (-sr, cr, 0)
				const double tx = ut*sd*cr - up*sr, ty = ut*sd*sr + up*cr, tz = -ut*cd;
				const double nx_ = cD*cd*cr + sD*tx, ny_ = cD*cd*sr + sD*ty, nz_ = cD*sd + sD*tz;
				const double r = hypot(nx_, ny_);
				theta = atan2(r, nz_); phi = atan2(ny_, nx_);
				if (psi) {
					const double qx = -sD*cd*cr + cD*tx, qy = -sD*cd*sr + cD*ty, qz = -sD*sd + cD*tz;      // t'
					const double cp = r > 0.0 ? nx_/r : 1.0, sp = r > 0.0 ? ny_/r : 0.0;
					const double x2 = (qx*cp + qy*sp)*nz_ - qz*r, y2 = qy*cp - qx*sp;                    // t' in (e_theta', e_phi')
					rot = p0 - 2.0*atan2(y2*ut - x2*up, x2*ut + y2*up);
				}
			} else { theta = 0.5*PXS_PI - dec; phi = ra; rot = p0; }
		} else {
			double d2 = dec + g0; phi = ra + g1/cos(dec);
			if (d2 > 0.5*PXS_PI) { d2 = PXS_PI - d2; phi += PXS_PI; }
			else if (d2 < -0.5*PXS_PI) { d2 = -PXS_PI - d2; phi += PXS_PI; }
			theta = 0.5*PXS_PI - d2; rot = 0.0;
		}
		theta = fmin(fmax(theta, 0.0), PXS_PI);      // (rounding of pi/2 - dec at the poles; NaN passes through and is refused by the point plan)
		loc[i] = make_double2(theta, wrap_2pi(phi));
		if (psi) psi[i] = rot;
	}
}

// (a, b) <- (c a - s b, s a + c b), c + i s = e^{i spin psi}, for npair pairs that share psi.  V pixels per thread and step: T2 is the
// 2-vector of T.  The angle's sine and cosine are taken once per pixel, whatever the number of pairs.
template<class T, class T2> __global__ __launch_bounds__(256) void rotate_pol_vec_kernel(long nvec, int npair, T2* __restrict__ a, T2* __restrict__ b,
		long pstride2, const double2* __restrict__ psi, double spin)
{
	const long step = (long)gridDim.x*blockDim.x;
	for (long i = (long)blockIdx.x*blockDim.x + threadIdx.x; i < nvec; i += step) {
		const double2 ang = psi[i];
		double s0, c0, s1, c1;
		sincos(spin*ang.x, &s0, &c0); sincos(spin*ang.y, &s1, &c1);
		for (int p = 0; p < npair; p++) {
			const long k = p*pstride2 + i;
			const T2 va = a[k], vb = b[k];
			T2 ra, rb;
			ra.x = (T)(c0*(double)va.x - s0*(double)vb.x); rb.x = (T)(s0*(double)va.x + c0*(double)vb.x);
			ra.y = (T)(c1*(double)va.y - s1*(double)vb.y); rb.y = (T)(s1*(double)va.y + c1*(double)vb.y);
			a[k] = ra; b[k] = rb;
		}
	}
}
template<class T> __global__ __launch_bounds__(256) void rotate_pol_kernel(long i0, long npts, int npair, T* __restrict__ a, T* __restrict__ b,
		long pstride, const double* __restrict__ psi, double spin)
{
	const long step = (long)gridDim.x*blockDim.x;
	for (long i = i0 + (long)blockIdx.x*blockDim.x + threadIdx.x; i < npts; i += step) {
		double s, c; sincos(spin*psi[i], &s, &c);
		for (int p = 0; p < npair; p++) {
			const long k = p*pstride + i;
			const double va = (double)a[k], vb = (double)b[k];
			a[k] = (T)(c*va - s*vb); b[k] = (T)(s*va + c*vb);
		}
	}
}

static inline unsigned stream_blocks(long n) {
	const long nb = (n + 255)/256;
	return (unsigned)(nb < 1 ? 1 : (nb > DEFLECT_MAXBLK ? DEFLECT_MAXBLK : nb));
}

template<class T, class T2> static void launch_rotate(long npts, int npair, void* a, void* b, long pstride, const double* psi, int spin, hipStream_t st)
{
	// two pixels per lane (16-byte accesses for float64) when every pair starts on a 2-vector boundary; the odd last pixel, or everything otherwise, one by one
	const bool vec = ((uintptr_t)a % sizeof(T2) == 0) && ((uintptr_t)b % sizeof(T2) == 0) && ((uintptr_t)psi % sizeof(double2) == 0) && (npair == 1 || pstride % 2 == 0);
	const long nvec = vec ? npts/2 : 0;
	if (nvec > 0) hipLaunchKernelGGL((rotate_pol_vec_kernel<T, T2>), dim3(stream_blocks(nvec)), dim3(256), 0, st, nvec, npair, (T2*)a, (T2*)b, pstride/2, (const double2*)psi, (double)spin);
	if (2*nvec < npts) hipLaunchKernelGGL((rotate_pol_kernel<T>), dim3(stream_blocks(npts - 2*nvec)), dim3(256), 0, st, 2*nvec, npts, npair, (T*)a, (T*)b, pstride, psi, (double)spin);
}

} // namespace pxs

using namespace pxs;

extern "C" {

int pxm_deflect(int64_t npts, int ny, int nx, double dec0, double ddec, double ra0, double dra, const double* d_pos, int pos_ncomp,
                const void* d_grad, int grad_dtype, int64_t grad_cstride, int geodesic, double* d_loc, double* d_psi, int device, void* stream)
{
	PXS_TRY
	PXS_REQUIRE(npts >= 0 && (npts == 0 || (d_grad && d_loc)), "pxm_deflect: bad arguments");
	PXS_REQUIRE(grad_dtype == PX_F32 || grad_dtype == PX_F64, "pxm_deflect: the gradient must be float32 or float64");
	PXS_REQUIRE(npts == 0 || grad_cstride >= npts || grad_cstride <= -npts, "pxm_deflect: the gradient's components overlap");
	if (d_pos) PXS_REQUIRE(pos_ncomp == 2 || pos_ncomp == 3, "pxm_deflect: positions are [{dec,ra}(,psi0)][npts]");
	else PXS_REQUIRE(ny >= 0 && nx >= 0 && (int64_t)ny*nx == npts, "pxm_deflect: ny*nx must equal npts when no positions are given");
	PXS_REQUIRE((uintptr_t)d_loc % 16 == 0, "pxm_deflect: loc must be 16-byte aligned");
	PXS_HIP(hipSetDevice(device));
	if (npts > 0) hipLaunchKernelGGL(deflect_kernel, dim3(stream_blocks(npts)), dim3(256), 0, (hipStream_t)stream, (long)npts, nx > 0 ? nx : 1, dec0, ddec, ra0, dra,
		d_pos, pos_ncomp, d_grad, grad_dtype, (long)grad_cstride, geodesic ? 1 : 0, (double2*)d_loc, d_psi);
	PXS_HIP(hipGetLastError());
	PXS_CATCH
}

int pxm_rotate_pol(int64_t npts, int npair, void* a, void* b, int64_t pair_stride, int dtype, const double* d_psi, int spin, int device, void* stream)
{
	PXS_TRY
	PXS_REQUIRE(npts >= 0 && npair >= 0 && (npts == 0 || npair == 0 || (a && b && d_psi)), "pxm_rotate_pol: bad arguments");
	PXS_REQUIRE(dtype == PX_F32 || dtype == PX_F64, "pxm_rotate_pol: maps must be float32 or float64");
	PXS_REQUIRE(npair <= 1 || pair_stride >= npts || pair_stride <= -npts, "pxm_rotate_pol: the pairs overlap");
	PXS_HIP(hipSetDevice(device));
	if (npts > 0 && npair > 0 && spin != 0) {
		if (dtype == PX_F32) launch_rotate<float, float2>((long)npts, npair, a, b, (long)pair_stride, d_psi, spin, (hipStream_t)stream);
		else launch_rotate<double, double2>((long)npts, npair, a, b, (long)pair_stride, d_psi, spin, (hipStream_t)stream);
	}
	PXS_HIP(hipGetLastError());
	PXS_CATCH
}

} // extern "C"
