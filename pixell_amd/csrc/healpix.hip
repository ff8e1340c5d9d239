// Healpix pixel arithmetic in the RING scheme (Gorski et al. 2005) and the two fused reprojection kernels of pixell_amd.reproject:
// what the reference's reproject.map2healpix / healpix2map (pixell/reproject.py:118-361, method="spline") walk in host batches through
// healpy.pix2ang / ang2pix / get_interp_val, coordinates.transform_euler, enmap.at and enmap.rotate_pol.  nside is any integer >= 1;
// pixel indices and everything formed from them are 64-bit.
//
//   ring r = 1 .. 4 nside - 1 from the north, j = min(r, 4 nside - r) its distance from the nearer pole (geometry.healpix_rings):
//     cap  (j < nside)  4 j pixels, first pixel 2 j (j - 1) (north), sin(theta/2) = j/(sqrt(6) nside), phi0 = pi/(4 j)
//     belt              4 nside pixels, first pixel 2 nside (nside - 1) + (r - nside) 4 nside, cos theta = (2 nside - j) 2/(3 nside) (north),
//                       phi0 = pi/(4 nside) where j - nside is even, 0 otherwise
//     the south mirrors the north: theta -> pi - theta, first pixel npix - 2 j (j + 1)
//   centre of pixel p      its ring by an integer square root in the caps (ring_of), then (theta_r, phi0_r + 2 pi k/n_r)
//   pixel of (theta, phi)  ang2pix below: the face coordinates jp, jm of the published pixelisation; 1 - |z| = 2 sin^2 of the half angle
//                          from the nearer pole in the caps, never a difference of cosines
//   ring-bilinear value    interp_weights below (the HEALPix C++ get_interpol): the ring above the point and the one below, two pixels on
//                          each by linear interpolation in phi, the two rings by linear interpolation in theta; beyond the first or the
//                          last ring the four pixels of that ring share the polar part equally.  Weights are >= 0 and sum to 1.
//
// Rotation (both fused kernels): the direction n of an OUTPUT pixel becomes n' = M n, M the nine doubles the host forms from the Euler
// angles, and the input is read at n'.  The angle of polarisation is that of M e_ra(n) in the (east, north) frame at n',
// psi = atan2(M e_ra . e_dec(n'), M e_ra . e_ra(n')), which the reference takes by finite differences (coordinates.transform_meta); a
// spin-s pair (a, b) becomes rotate_pol(., -psi, spin=s): a' = cos(s psi) a + sin(s psi) b, b' = -sin(s psi) a + cos(s psi) b.
//
// One lane per OUTPUT pixel (grid-stride), which does its index and weight arithmetic once and loops over the components: stores are
// contiguous along the lane index, the reads are gathers that neighbouring lanes share.  No atomics, no LDS.  FP64 arithmetic.
#include "../../include/pxsht.h"
#include "common.hpp"
#include "interpol_dev.hpp"
#include <cmath>

namespace pxs {
namespace hpx {
using namespace ipl;

static constexpr double TWOPI = 2.0*PXS_PI, HALFPI = 0.5*PXS_PI;
enum : int { MAXCOMP = 32 };
enum : int { MODE_PIX2ANG = 0, MODE_ANG2PIX = 1, MODE_WEIGHTS = 2 };

struct Ring { double theta, phi0; long start, n; };

__device__ __forceinline__ long isqrt64(long v) {
	long s = (long)sqrt((double)v);
	while (s*s > v) s--;
	while ((s + 1)*(s + 1) <= v) s++;
	return s;
}

// ring r in [1, 4 nside - 1]
__device__ __forceinline__ Ring ring_info(long nside, long r) {
	const long nl4 = 4*nside, npix = 12*nside*nside;
	const bool south = r > 2*nside;
	const long j = south ? nl4 - r : r;
	Ring g;
	if (j < nside) {
		g.theta = 2.0*asin((double)j/(sqrt(6.0)*(double)nside));
		g.n = 4*j; g.phi0 = PXS_PI/(double)(4*j);
		g.start = south ? npix - 2*j*(j + 1) : 2*j*(j - 1);
	} else {
		double c = (double)(2*nside - j)*(2.0/(double)(3*nside));
		c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
		g.theta = acos(c);
		g.n = nl4; g.phi0 = ((j - nside) & 1) == 0 ? PXS_PI/(double)nl4 : 0.0;
		g.start = 2*nside*(nside - 1) + (r - nside)*nl4;
	}
	if (south) g.theta = PXS_PI - g.theta;
	return g;
}

// the ring of pixel p in [0, npix) and its place k on it
__device__ __forceinline__ long ring_of(long nside, long p, long& k) {
	const long ncap = 2*nside*(nside - 1), npix = 12*nside*nside;
	if (p < ncap) {
		const long r = (1 + isqrt64(1 + 2*p)) >> 1;
		k = p - 2*r*(r - 1);
		return r;
	}
	if (p < npix - ncap) {
		const long q = p - ncap, r = q/(4*nside);
		k = q - r*4*nside;
		return r + nside;
	}
	const long q = npix - 1 - p, j = (1 + isqrt64(1 + 2*q)) >> 1;
	k = 4*j - 1 - (q - 2*j*(j - 1));
	return 4*nside - j;
}

__device__ __forceinline__ void pix2ang(long nside, long p, double& theta, double& phi) {
	long k;
	const Ring g = ring_info(nside, ring_of(nside, p, k));
	theta = g.theta;
	phi = g.phi0 + TWOPI*(double)k/(double)g.n;
}

// 1 - |cos theta| in the caps
__device__ __forceinline__ double one_minus_za(double theta, bool north) {
	const double s = sin(0.5*(north ? theta : PXS_PI - theta));
	return 2.0*s*s;
}

__device__ __forceinline__ long imod(long a, long n) { long m = a % n; return m < 0 ? m + n : m; }

// the pixel that holds (theta, phi); -1: not a direction
__device__ __forceinline__ long ang2pix(long nside, double theta, double phi) {
	if (!(fabs(theta) < 1e15) || !(fabs(phi) < 1e15)) return -1;
	const long nl4 = 4*nside, npix = 12*nside*nside;
	const double z = cos(theta), za = fabs(z);
	double tt = fmod(phi, TWOPI);
	if (tt < 0) tt += TWOPI;
	tt /= HALFPI;
	if (tt >= 4.0) tt -= 4.0;
	long pix;
	if (za <= 2.0/3.0) {
		const double t1 = (double)nside*(0.5 + tt), t2 = (double)nside*z*0.75;
		const long jp = (long)floor(t1 - t2), jm = (long)floor(t1 + t2);
		const long ir = nside + 1 + jp - jm, kshift = 1 - (ir & 1);
		const long ip = imod((jp + jm - nside + kshift + 1) >> 1, nl4);
		pix = 2*nside*(nside - 1) + (ir - 1)*nl4 + ip;
	} else {
		const double tp = tt - floor(tt), tmp = (double)nside*sqrt(3.0*one_minus_za(theta, z > 0));
		const long jp = (long)floor(tp*tmp), jm = (long)floor((1.0 - tp)*tmp);
		const long ir = jp + jm + 1;
		const long ip = imod((long)floor(tt*(double)ir), 4*ir);
		pix = z > 0 ? 2*ir*(ir - 1) + ip : npix - 2*ir*(ir + 1) + ip;
	}
	return pix >= 0 && pix < npix ? pix : -1;
}

// the two pixels of a ring around phi and the weight of the second
__device__ __forceinline__ void ring_pair(const Ring& g, double phi, long& p1, long& p2, double& w) {
	const double t = (phi - g.phi0)/(TWOPI/(double)g.n), fl = floor(t);
	w = t - fl;
	const long i1 = imod((long)fl, g.n);
	p1 = g.start + i1;
	p2 = g.start + (i1 + 1 == g.n ? 0 : i1 + 1);
}

// the four pixels and weights of the ring-bilinear value at (theta, phi); false: not a direction
__device__ __forceinline__ bool interp_weights(long nside, double theta, double phi, long* pix, double* w) {
	if (!(fabs(theta) < 1e15) || !(fabs(phi) < 1e15)) return false;
	const long nl4 = 4*nside, npix = 12*nside*nside;
	const double z = cos(theta), za = fabs(z);
	long ir1;
	if (za <= 2.0/3.0) ir1 = (long)floor((double)nside*(2.0 - 1.5*z));
	else {
		const long i = (long)floor((double)nside*sqrt(3.0*one_minus_za(theta, z > 0)));
		ir1 = z > 0 ? i : nl4 - i - 1;
	}
	ir1 = ir1 < 0 ? 0 : (ir1 > nl4 - 1 ? nl4 - 1 : ir1);
	const long ir2 = ir1 + 1;
	double theta1 = 0.0, theta2 = 0.0, wp;
	if (ir1 > 0) {
		const Ring g = ring_info(nside, ir1);
		ring_pair(g, phi, pix[0], pix[1], wp);
		w[0] = 1.0 - wp; w[1] = wp; theta1 = g.theta;
	}
	if (ir2 < nl4) {
		const Ring g = ring_info(nside, ir2);
		ring_pair(g, phi, pix[2], pix[3], wp);
		w[2] = 1.0 - wp; w[3] = wp; theta2 = g.theta;
	}
	if (ir1 == 0) {
		double wt = theta/theta2;
		wt = wt < 0.0 ? 0.0 : (wt > 1.0 ? 1.0 : wt);
		const double fac = (1.0 - wt)*0.25;
		w[0] = fac; w[1] = fac; w[2] = w[2]*wt + fac; w[3] = w[3]*wt + fac;
		pix[0] = (pix[2] + 2) & 3; pix[1] = (pix[3] + 2) & 3;
	} else if (ir2 == nl4) {
		double wt = (theta - theta1)/(PXS_PI - theta1);
		wt = wt < 0.0 ? 0.0 : (wt > 1.0 ? 1.0 : wt);
		const double fac = wt*0.25;
		w[0] = w[0]*(1.0 - wt) + fac; w[1] = w[1]*(1.0 - wt) + fac; w[2] = fac; w[3] = fac;
		pix[2] = npix - 4 + ((pix[0] - (npix - 4) + 2) & 3); pix[3] = npix - 4 + ((pix[1] - (npix - 4) + 2) & 3);
	} else {
		double wt = (theta - theta1)/(theta2 - theta1);
		wt = wt < 0.0 ? 0.0 : (wt > 1.0 ? 1.0 : wt);
		w[0] *= 1.0 - wt; w[1] *= 1.0 - wt; w[2] *= wt; w[3] *= wt;
	}
	return true;
}

struct Rot { int on; double m[9]; };
struct Spins { int ncomp; signed char s[MAXCOMP]; };      // s[c] != 0: components c, c + 1 are a pair of that spin

// n = direction of (dec, ra) -> (dec', ra') of M n, and the angle psi of M e_ra(n) in the (east, north) frame at M n
__device__ __forceinline__ void rotate_dir(const Rot& R, double dec, double ra, double& odec, double& ora, double& psi) {
	double sd, cd, sr, cr;
	sincos(dec, &sd, &cd); sincos(ra, &sr, &cr);
	const double n[3] = {cd*cr, cd*sr, sd}, e[3] = {-sr, cr, 0.0};
	const double* m = R.m;
	const double Vx = m[0]*n[0] + m[1]*n[1] + m[2]*n[2], Vy = m[3]*n[0] + m[4]*n[1] + m[5]*n[2], Vz = m[6]*n[0] + m[7]*n[1] + m[8]*n[2];
	const double Ex = m[0]*e[0] + m[1]*e[1], Ey = m[3]*e[0] + m[4]*e[1], Ez = m[6]*e[0] + m[7]*e[1];
	odec = atan2(Vz, hypot(Vx, Vy)); ora = atan2(Vy, Vx);
	const double ce = Vx*Ey - Vy*Ex, cn = (Vx*Vx + Vy*Vy)*Ez - Vz*(Vx*Ex + Vy*Ey);
	psi = ce == 0.0 && cn == 0.0 ? 0.0 : atan2(cn, ce);      // (on a pole of the input's system there is no north: no rotation)
}

// the store of component m's value v: spin-0 components at once, a pair once its second component is known
template<class T> struct PairStore {
	const Spins& sp; double psi, scale; bool rot; T* op; long stride;
	double held; int spin;
	__device__ __forceinline__ PairStore(const Spins& s, double psi_, double scale_, bool rot_, T* op_, long stride_) : sp(s), psi(psi_), scale(scale_), rot(rot_), op(op_), stride(stride_), held(0.0), spin(0) {}
	__device__ __forceinline__ void put(int m, double v) {
		if (spin != 0) {
			double s, c;
			sincos((double)spin*psi, &s, &c);
			op[(long)(m - 1)*stride] = (T)(scale*(c*held + s*v));
			op[(long)m*stride] = (T)(scale*(c*v - s*held));
			spin = 0;
		} else if (rot && sp.s[m] != 0 && m + 1 < sp.ncomp) { held = v; spin = sp.s[m]; }
		else op[(long)m*stride] = (T)(scale*v);
	}
};

// ---- index arithmetic on arrays ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void index_kernel(int mode, long nside, long n, const int64_t* __restrict__ pin, const double* __restrict__ theta, const double* __restrict__ phi,
		int64_t* __restrict__ pout, double* __restrict__ out)
{
	const long npix = 12*nside*nside;
	for (long i = (long)blockIdx.x*256 + threadIdx.x; i < n; i += (long)gridDim.x*256) {
		if (mode == MODE_PIX2ANG) {
			const long p = pin[i];
			double t = NAN, f = NAN;
			if (p >= 0 && p < npix) pix2ang(nside, p, t, f);
			out[i] = t; out[n + i] = f;
		} else if (mode == MODE_ANG2PIX) pout[i] = ang2pix(nside, theta[i], phi[i]);
		else {
			long pix[4] = {-1, -1, -1, -1}; double w[4] = {NAN, NAN, NAN, NAN};
			interp_weights(nside, theta[i], phi[i], pix, w);
			for (int k = 0; k < 4; k++) { pout[(long)k*n + i] = pix[k]; out[(long)k*n + i] = w[k]; }
		}
	}
}

// the value of map mp at the direction whose pixel / weights a lane holds
template<class T> __device__ __forceinline__ double heal_value(const T* __restrict__ mp, int order, long p0, const long* pix, const double* w) {
	if (order == 0) return (double)mp[p0];
	double acc = 0.0;
	for (int k = 0; k < 4; k++) acc = fma(w[k], (double)mp[pix[k]], acc);
	return acc;
}

// maps [ncomp][npix] of T, mstride apart, at n points -> out [ncomp][n]
template<class T> __global__ __launch_bounds__(256) void interp_kernel(long nside, int ncomp, const T* __restrict__ maps, long mstride, long n, const double* __restrict__ theta,
		const double* __restrict__ phi, int order, T* __restrict__ out)
{
	for (long i = (long)blockIdx.x*256 + threadIdx.x; i < n; i += (long)gridDim.x*256) {
		long pix[4], p0 = -1; double w[4];
		bool ok;
		if (order == 0) { p0 = ang2pix(nside, theta[i], phi[i]); ok = p0 >= 0; }
		else ok = interp_weights(nside, theta[i], phi[i], pix, w);
		for (int m = 0; m < ncomp; m++) out[(long)m*n + i] = ok ? (T)heal_value(maps + (long)m*mstride, order, p0, pix, w) : (T)NAN;
	}
}

// ---- CAR -> healpix ---------------------------------------------------------------------------------------------------------------
struct ToHeal { Axis y, x; int order, border_y, border_x; long nside, first, n; double scale, cval; };

// maps [ncomp][ny][nx] of TI, mstride apart -> out [ncomp][n] of TO (ostride apart): healpix pixels first .. first + n - 1
template<class TI, class TO> __global__ __launch_bounds__(256) void map2healpix_kernel(ToHeal g, Rot R, Spins sp, const TI* __restrict__ maps, long mstride, TO* __restrict__ out, long ostride)
{
	for (long i = (long)blockIdx.x*256 + threadIdx.x; i < g.n; i += (long)gridDim.x*256) {
		double theta, phi, psi = 0.0;
		pix2ang(g.nside, g.first + i, theta, phi);
		double dec = HALFPI - theta, ra = phi;
		if (R.on) rotate_dir(R, dec, ra, dec, ra, psi);
		TO* op = out + i;
		double y, x;
		const bool in = axis_coord(g.y, dec, g.order, g.border_y, y) & axis_coord(g.x, ra, g.order, g.border_x, x);
		if (!in) { for (int m = 0; m < sp.ncomp; m++) op[(long)m*ostride] = (TO)(g.scale*g.cval); continue; }
		int iy[4], ix[4]; double wy[4], wx[4];
		axis_taps(g.y.n, y, g.order, g.border_y, iy, wy); axis_taps(g.x.n, x, g.order, g.border_x, ix, wx);
		const int nt = g.order + 1;
		PairStore<TO> st(sp, psi, g.scale, R.on != 0, op, ostride);
		for (int m = 0; m < sp.ncomp; m++) {
			const TI* mp = maps + (long)m*mstride;
			double acc = 0.0;
			for (int a = 0; a < nt; a++) {
				const TI* rp = mp + (long)iy[a]*g.x.n;
				double s = 0.0;
				for (int b = 0; b < nt; b++) s = fma(wx[b], (double)rp[ix[b]], s);
				acc = fma(wy[a], s, acc);
			}
			st.put(m, acc);
		}
	}
}

// ---- healpix -> CAR ---------------------------------------------------------------------------------------------------------------
struct ToMap { int ny, nx; double dec0, ddec, ra0, dra; long nside; int order; };

// maps [ncomp][npix] of T, mstride apart -> out [ncomp][ny][nx] of T; rowfac f64 [ny] or null
template<class T> __global__ __launch_bounds__(256) void healpix2map_kernel(ToMap g, Rot R, Spins sp, const T* __restrict__ maps, long mstride, const double* __restrict__ rowfac, T* __restrict__ out)
{
	const long npts = (long)g.ny*g.nx;
	for (long i = (long)blockIdx.x*256 + threadIdx.x; i < npts; i += (long)gridDim.x*256) {
		const long yy = i/g.nx, xx = i - yy*g.nx;
		double dec = g.dec0 + (double)yy*g.ddec, ra = g.ra0 + (double)xx*g.dra, psi = 0.0;
		if (R.on) rotate_dir(R, dec, ra, dec, ra, psi);
		const double theta = HALFPI - dec;
		long pix[4], p0 = -1; double w[4];
		bool ok;
		if (g.order == 0) { p0 = ang2pix(g.nside, theta, ra); ok = p0 >= 0; }
		else ok = interp_weights(g.nside, theta, ra, pix, w);
		T* op = out + i;
		if (!ok) { for (int m = 0; m < sp.ncomp; m++) op[(long)m*npts] = (T)NAN; continue; }
		PairStore<T> st(sp, psi, rowfac ? rowfac[yy] : 1.0, R.on != 0, op, npts);
		for (int m = 0; m < sp.ncomp; m++) st.put(m, heal_value(maps + (long)m*mstride, g.order, p0, pix, w));
	}
}

static unsigned grid_of(long n) { const long b = (n + 255)/256; return (unsigned)(b < 1 ? 1 : (b > 65536 ? 65536 : b)); }

static Rot rot_of(const double* rot) {
	Rot R; R.on = rot != nullptr;
	for (int k = 0; k < 9; k++) { R.m[k] = rot ? rot[k] : (k % 4 == 0 ? 1.0 : 0.0); PXS_REQUIRE(R.m[k] == R.m[k], "the rotation matrix is not a number"); }
	return R;
}
static Spins spins_of(int ncomp, int npair, const int* pairs, const char* who) {
	PXS_REQUIRE(ncomp >= 0 && ncomp <= MAXCOMP, std::string(who) + ": at most 32 components per call");
	PXS_REQUIRE(npair >= 0 && (npair == 0 || pairs), std::string(who) + ": bad pair list");
	Spins sp; sp.ncomp = ncomp;
	for (int c = 0; c < MAXCOMP; c++) sp.s[c] = 0;
	for (int k = 0; k < npair; k++) {
		const int c = pairs[2*k], s = pairs[2*k + 1];
		PXS_REQUIRE(c >= 0 && c + 1 < ncomp && s >= -127 && s <= 127, std::string(who) + ": a pair is (first component, spin), both components in range");
		PXS_REQUIRE(sp.s[c] == 0 && (c == 0 || sp.s[c - 1] == 0) && sp.s[c + 1] == 0, std::string(who) + ": the pairs overlap");
		sp.s[c] = (signed char)s;
	}
	return sp;
}

} // namespace hpx
} // namespace pxs

using namespace pxs;
using namespace pxs::hpx;

extern "C" {

int pxm_healpix_index(int mode, int64_t nside, int64_t n, const int64_t* d_pix_in, const double* d_theta, const double* d_phi, int64_t* d_pix_out, double* d_out,
                      int device, void* stream)
{
	PXS_TRY
	PXS_REQUIRE(mode >= MODE_PIX2ANG && mode <= MODE_WEIGHTS, "pxm_healpix_index: the mode is 0 (pix2ang), 1 (ang2pix) or 2 (weights)");
	PXS_REQUIRE(nside >= 1 && nside <= (int64_t(1) << 29) && n >= 0, "pxm_healpix_index: bad sizes");
	PXS_HIP(hipSetDevice(device));
	if (n == 0) return 0;
	if (mode == MODE_PIX2ANG) PXS_REQUIRE(d_pix_in && d_out, "pxm_healpix_index: null arrays");
	else PXS_REQUIRE(d_theta && d_phi && d_pix_out && (mode == MODE_ANG2PIX || d_out), "pxm_healpix_index: null arrays");
	hipLaunchKernelGGL(index_kernel, dim3(grid_of(n)), dim3(256), 0, (hipStream_t)stream, mode, (long)nside, (long)n, d_pix_in, d_theta, d_phi, d_pix_out, d_out);
	PXS_HIP(hipGetLastError());
	PXS_CATCH
}

int pxm_healpix_interp(int64_t nside, int ncomp, const void* d_maps, int map_dtype, int64_t mstride, int64_t n, const double* d_theta, const double* d_phi,
                       int order, void* d_out, int device, void* stream)
{
	PXS_TRY
	PXS_REQUIRE(nside >= 1 && nside <= (int64_t(1) << 29) && ncomp >= 0 && n >= 0, "pxm_healpix_interp: bad sizes");
	PXS_REQUIRE(order == 0 || order == 1, "pxm_healpix_interp: the order must be 0 or 1");
	PXS_REQUIRE(map_dtype == PX_F32 || map_dtype == PX_F64, "pxm_healpix_interp: float32 or float64 maps");
	PXS_REQUIRE(ncomp <= 1 || mstride >= 12*nside*nside, "pxm_healpix_interp: the maps overlap");
	PXS_HIP(hipSetDevice(device));
	if (n == 0 || ncomp == 0) return 0;
	PXS_REQUIRE(d_maps && d_theta && d_phi && d_out, "pxm_healpix_interp: null arrays");
	hipStream_t st = (hipStream_t)stream;
	if (map_dtype == PX_F32) hipLaunchKernelGGL((interp_kernel<float>), dim3(grid_of(n)), dim3(256), 0, st, (long)nside, ncomp, (const float*)d_maps, (long)mstride, (long)n, d_theta, d_phi, order, (float*)d_out);
	else hipLaunchKernelGGL((interp_kernel<double>), dim3(grid_of(n)), dim3(256), 0, st, (long)nside, ncomp, (const double*)d_maps, (long)mstride, (long)n, d_theta, d_phi, order, (double*)d_out);
	PXS_HIP(hipGetLastError());
	PXS_CATCH
}

int pxm_map2healpix(int ncomp, int ny, int nx, const void* d_maps, int map_dtype, int64_t mstride,
                    double yoff, double yscale, double xoff, double xscale, double yref, double yper, double xref, double xper,
                    int order, int border_y, int border_x, double cval, int64_t nside, int64_t first, int64_t n, const double* rot,
                    int npair, const int* pairs, double scale, void* d_out, int out_dtype, int64_t ostride, int device, void* stream)
{
	PXS_TRY
	PXS_REQUIRE(ny >= 1 && nx >= 1 && nside >= 1 && nside <= (int64_t(1) << 29), "pxm_map2healpix: bad sizes");
	PXS_REQUIRE(first >= 0 && n >= 0 && first + n <= 12*nside*nside, "pxm_map2healpix: the pixel range leaves the healpix map");
	PXS_REQUIRE(order == 0 || order == 1 || order == 3, "pxm_map2healpix: the order must be 0, 1 or 3");
	PXS_REQUIRE(border_y >= B_NEAREST && border_y <= B_GRIDWRAP && border_x >= B_NEAREST && border_x <= B_GRIDWRAP, "pxm_map2healpix: unknown border rule");
	PXS_REQUIRE((map_dtype == PX_F32 || map_dtype == PX_F64) && (out_dtype == PX_F32 || out_dtype == PX_F64), "pxm_map2healpix: float32 or float64 maps");
	PXS_REQUIRE(order != 3 || map_dtype == PX_F64, "pxm_map2healpix: order 3 reads float64 coefficients");
	PXS_REQUIRE(map_dtype == out_dtype || (map_dtype == PX_F64 && out_dtype == PX_F32), "pxm_map2healpix: the output has the maps' dtype, or is float32 from float64");
	PXS_REQUIRE(ncomp <= 1 || (mstride >= (int64_t)ny*nx && ostride >= n), "pxm_map2healpix: the maps overlap");
	PXS_REQUIRE(yoff == yoff && yscale == yscale && xoff == xoff && xscale == xscale && scale == scale, "pxm_map2healpix: the affine map is not a number");
	const Rot R = rot_of(rot);
	const Spins sp = spins_of(ncomp, npair, pairs, "pxm_map2healpix");
	PXS_HIP(hipSetDevice(device));
	if (ncomp == 0 || n == 0) return 0;
	PXS_REQUIRE(d_maps && d_out, "pxm_map2healpix: null arrays");
	const ToHeal g = {{ny, yoff, yscale, yref, yper}, {nx, xoff, xscale, xref, xper}, order, border_y, border_x, (long)nside, (long)first, (long)n, scale, cval};
	hipStream_t st = (hipStream_t)stream;
	const dim3 grid(grid_of(n));
	if (map_dtype == PX_F32) hipLaunchKernelGGL((map2healpix_kernel<float, float>), grid, dim3(256), 0, st, g, R, sp, (const float*)d_maps, (long)mstride, (float*)d_out, (long)ostride);
	else if (out_dtype == PX_F64) hipLaunchKernelGGL((map2healpix_kernel<double, double>), grid, dim3(256), 0, st, g, R, sp, (const double*)d_maps, (long)mstride, (double*)d_out, (long)ostride);
	else hipLaunchKernelGGL((map2healpix_kernel<double, float>), grid, dim3(256), 0, st, g, R, sp, (const double*)d_maps, (long)mstride, (float*)d_out, (long)ostride);
	PXS_HIP(hipGetLastError());
	PXS_CATCH
}

int pxm_healpix2map(int ncomp, int64_t nside, const void* d_maps, int map_dtype, int64_t mstride, int ny, int nx, double dec0, double ddec, double ra0, double dra,
                    int order, const double* rot, int npair, const int* pairs, const double* d_rowfac, void* d_out, int device, void* stream)
{
	PXS_TRY
	PXS_REQUIRE(ny >= 0 && nx >= 0 && nside >= 1 && nside <= (int64_t(1) << 29), "pxm_healpix2map: bad sizes");
	PXS_REQUIRE(order == 0 || order == 1, "pxm_healpix2map: the order must be 0 or 1");
	PXS_REQUIRE(map_dtype == PX_F32 || map_dtype == PX_F64, "pxm_healpix2map: float32 or float64 maps");
	PXS_REQUIRE(ncomp <= 1 || mstride >= 12*nside*nside, "pxm_healpix2map: the maps overlap");
	PXS_REQUIRE(dec0 == dec0 && ddec == ddec && ra0 == ra0 && dra == dra, "pxm_healpix2map: the geometry is not a number");
	const Rot R = rot_of(rot);
	const Spins sp = spins_of(ncomp, npair, pairs, "pxm_healpix2map");
	PXS_HIP(hipSetDevice(device));
	if (ncomp == 0 || ny == 0 || nx == 0) return 0;
	PXS_REQUIRE(d_maps && d_out, "pxm_healpix2map: null arrays");
	const ToMap g = {ny, nx, dec0, ddec, ra0, dra, (long)nside, order};
	hipStream_t st = (hipStream_t)stream;
	const dim3 grid(grid_of((long)ny*nx));
	if (map_dtype == PX_F32) hipLaunchKernelGGL((healpix2map_kernel<float>), grid, dim3(256), 0, st, g, R, sp, (const float*)d_maps, (long)mstride, d_rowfac, (float*)d_out);
	else hipLaunchKernelGGL((healpix2map_kernel<double>), grid, dim3(256), 0, st, g, R, sp, (const double*)d_maps, (long)mstride, d_rowfac, (double*)d_out);
	PXS_HIP(hipGetLastError());
	PXS_CATCH
}

} // extern "C"
