// The modulation half of the Doppler boost (aberration.apply_modulation, aberration.py:285-354, over utils.planck, dplanck, iplanck_T,
// utils.py:2537-2561): one streaming pass over the pixels, in place, every component of a pixel under one load of the modulation A.
//
// With P(T) = V / expm1(x_f / T), x_f = h f / k, V = 2 h f^3 / c^2, and the linearised unit lin = P / P'(T0), V / P'(T0) =
// T0 expm1(x0)^2 / (x0 e^{x0}), x0 = x_f / T0: the results depend on the frequency through x_f alone.  Both conversions are differences
// of nearly equal numbers (micro-kelvins on 2.7 K), which the reference forms as such and loses six digits to; here they are taken in closed form:
//   T -> lin   P(T1) - P(T2) = V e^{x1} expm1(x2 - x1) / (expm1(x1) expm1(x2)),  x2 - x1 = x_f (T1 - T2) / (T1 T2)
//   lin -> T   I = P(Tb) (1 + r), r = lin expm1(xb) P'(T0) / V:  x_f / T = log1p(V / I) = xb + e,  e = log1p(r e^{-xb}) - log1p(r),
//              T - Tb = -Tb e / (xb + e)
// All arithmetic is FP64 whatever the map's type.
#include "../../include/pxsht.h"
#include "common.hpp"

namespace pxs {

static constexpr int MOD_MAXBLK = 2048;
static constexpr double MOD_H = 6.62606957e-34, MOD_K = 1.3806488e-23, MOD_TCMB = 2.72548;      // utils.h, utils.k, utils.T_cmb

struct ModPar { int mode, dipole; double xf, T0, unit, vs, dip_add; };      // vs = V / P'(T0) in K; dip_add = T0 / unit

// true temperature fluctuation (K, about T0) -> linearised (K), under the modulation a; mono: the monopole's own boost stays in (dipole)
__device__ __forceinline__ double mod_T2lin(double dT, double a, bool mono, const ModPar& p) {
	const double T1 = a*(dT + p.T0), T2 = mono ? p.T0 : a*p.T0;
	const double diff = mono ? a*dT + (a - 1.0)*p.T0 : a*dT;
	const double x1 = p.xf/T1, x2 = p.xf/T2, dx = p.xf*diff/(T1*T2);
	return p.vs*exp(x1)*expm1(dx)/(expm1(x1)*expm1(x2));
}
// its inverse.  (T_cmb, not T0, is taken off at the end, as the reference does)
__device__ __forceinline__ double mod_lin2T(double lin, double a, bool mono, const ModPar& p) {
	const double Tb = mono ? p.T0 : p.T0/a, aTb = mono ? a*p.T0 : p.T0;
	const double xb = p.xf/Tb, r = lin/p.vs*expm1(xb);
	const double e = log1p(r*exp(-xb)) - log1p(r);
	return (aTb - MOD_TCMB) - a*Tb*e/(xb + e);
}

template<class T> __global__ __launch_bounds__(256) void modulate_kernel(long npix, int ncomp, T* __restrict__ map, long cstride, const T* __restrict__ A,
		unsigned long long spin0, ModPar p)
{
	const long step = (long)gridDim.x*blockDim.x;
	for (long i = (long)blockIdx.x*blockDim.x + threadIdx.x; i < npix; i += step) {
		const double a = (double)A[i];
		for (int c = 0; c < ncomp; c++) {
			const long k = c*cstride + i;
			const double v = (double)map[k];
			const bool mono = p.dipole && ((spin0 >> c) & 1);
			double o;
			if (p.mode == PXM_MOD_T2T) o = v*a + (p.dipole && c == 0 ? (a - 1.0)*p.dip_add : 0.0);
			else if (p.mode == PXM_MOD_T2LIN) o = mod_T2lin(v*p.unit, a, mono, p)/p.unit;
			else if (p.mode == PXM_MOD_LIN2T) o = mod_lin2T(v*p.unit, a, mono, p)/p.unit;
			else o = mod_T2lin(mod_lin2T(v*p.unit, 1.0, mono, p), a, mono, p)/p.unit;
			map[k] = (T)o;
		}
	}
}

} // namespace pxs

using namespace pxs;

extern "C" int pxm_modulate(int64_t npix, int ncomp, void* d_map, int dtype, int64_t map_cstride, const void* d_A, uint64_t spin0_mask,
                            int mode, int dipole, double T0, double freq, double map_unit, int device, void* stream)
{
	PXS_TRY
	PXS_REQUIRE(npix >= 0 && ncomp >= 0 && ncomp <= 64 && (npix == 0 || ncomp == 0 || (d_map && d_A)), "pxm_modulate: bad arguments (at most 64 components a call)");
	PXS_REQUIRE(dtype == PX_F32 || dtype == PX_F64, "pxm_modulate: maps must be float32 or float64");
	PXS_REQUIRE(mode >= PXM_MOD_NONE && mode <= PXM_MOD_LIN2LIN, "pxm_modulate: unknown mode");
	PXS_REQUIRE(ncomp <= 1 || map_cstride >= npix || map_cstride <= -npix, "pxm_modulate: the components overlap");
	PXS_REQUIRE(mode == PXM_MOD_NONE || (T0 > 0 && freq > 0 && map_unit > 0), "pxm_modulate: T0, freq and map_unit must be positive");
	PXS_HIP(hipSetDevice(device));
	if (mode == PXM_MOD_NONE || npix == 0 || ncomp == 0) return 0;
	ModPar p; p.mode = mode; p.dipole = dipole ? 1 : 0; p.xf = MOD_H*freq/MOD_K; p.T0 = T0; p.unit = map_unit; p.dip_add = T0/map_unit;
	const double x0 = p.xf/T0, em = expm1(x0);
	p.vs = T0*em*em/(x0*exp(x0));
	const long nb = (npix + 255)/256;
	const dim3 grid((unsigned)(nb > MOD_MAXBLK ? MOD_MAXBLK : nb));
	if (dtype == PX_F32) hipLaunchKernelGGL((modulate_kernel<float>), grid, dim3(256), 0, (hipStream_t)stream, (long)npix, ncomp, (float*)d_map, (long)map_cstride, (const float*)d_A, (unsigned long long)spin0_mask, p);
	else hipLaunchKernelGGL((modulate_kernel<double>), grid, dim3(256), 0, (hipStream_t)stream, (long)npix, ncomp, (double*)d_map, (long)map_cstride, (const double*)d_A, (unsigned long long)spin0_mask, p);
	PXS_HIP(hipGetLastError());
	PXS_CATCH
}
