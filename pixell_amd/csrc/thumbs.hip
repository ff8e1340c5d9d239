// Catalogue cut-outs ("thumbnails") of maps [ny][nx]: what the reference's reproject.thumbnails (pixell/reproject.py:10-105) makes in a Python
// loop over objects, as one launch.  Every object of a catalogue gets a small map [oy][ox] on a geometry centred on (0, 0) (CAR or gnomonic),
// with the object moved to that centre and Q/U rotated to the local north there.  For every (object, thumbnail pixel):
//
//   v, e     the unit vector of the thumbnail pixel and the unit vector towards east there, in the thumbnail's own system.  They are the same
//            for every object, so a setup kernel writes them once per call into a table [oy ox][6] (directions_kernel):
//              CAR   x = (i + 1 - crpix_x) cdelt_x, y = (j + 1 - crpix_y) cdelt_y in degrees are (ra, dec): v = (cos y cos x, cos y sin x, sin y)
//              TAN   the same x, y in radians are the standard coordinates (xi, eta) about (0, 0): v = (1, xi, eta)/|.|
//              e = (-v_y, v_x, 0)/|.| in both (CAR: (-sin x, cos x, 0), which also holds on the poles)
//   V = R v  R = Rz(ra_o) Ry(-dec_o): what coordinates.recenter(., [0, 0, ra_o, dec_o]) does (coordinates.py:289-305): the thumbnail's (0, 0)
//            lands on the object, and north at the centre stays north.  dec = atan2(V_z, hypot(V_x, V_y)), ra = atan2(V_y, V_x)
//   gather   the input pixel by the per-axis affine map and rewind of pxm_interpol, then the taps of interpol_dev.hpp with a border rule
//            PER AXIS (RA of a map that goes round the sky: grid-wrap; dec: constant), one sum per map
//   psi      the angle of R e in the (east, north) frame E, N of the sky position: atan2(Re . N, Re . E), which is what the reference takes
//            by finite differences (coordinates.transform_meta).  Q, U become rotate_pol(., -psi): Q' = cos 2psi Q + sin 2psi U,
//            U' = -sin 2psi Q + cos 2psi U.  With n = Re . N and e = Re . E up to a common positive factor, cos 2psi = (e^2 - n^2)/(e^2 + n^2)
//            and sin 2psi = 2 e n/(e^2 + n^2): no angle is formed.
//
// A workgroup belongs to one object (its R is uniform: the object's position is a scalar load), a lane to one thumbnail pixel for all maps.
// Objects and the pixel chunks of a thumbnail go over one flattened block index (gridDim.y would stop at 65 535 objects).  Workgroups are
// 64 lanes for thumbnails of up to 64 pixels, 256 otherwise.  The taps are direct gathers: neighbouring lanes are neighbouring thumbnail
// pixels, which read neighbouring input pixels, and a thumbnail's footprint is a few kB per map.  FP64 arithmetic.
#include "../../include/pxsht.h"
#include "common.hpp"
#include "interpol_dev.hpp"

namespace pxs {
namespace thb {
using namespace ipl;

enum : int { PROJ_CAR = 0, PROJ_TAN = 1 };
static constexpr double DEG = PXS_PI/180.0;

struct Thumb { Axis y, x; int npix, bpo; int order, border_y, border_x; int pol, qc, uc; };      // bpo: workgroups per object

// tab [oy ox][6]: v and e of thumbnail pixel (j, i)
__global__ __launch_bounds__(256) void directions_kernel(int oy, int ox, int proj, double cdelt_y, double crpix_y, double cdelt_x, double crpix_x, double* __restrict__ tab)
{
	const int p = blockIdx.x*256 + threadIdx.x;
	if (p >= oy*ox) return;
	const int j = p/ox, i = p - j*ox;
	const double x = ((double)(i + 1) - crpix_x)*cdelt_x*DEG, y = ((double)(j + 1) - crpix_y)*cdelt_y*DEG;
	double* t = tab + 6l*p;
	if (proj == PROJ_CAR) {
		double sx, cx, sy, cy;
		sincos(x, &sx, &cx); sincos(y, &sy, &cy);
		t[0] = cy*cx; t[1] = cy*sx; t[2] = sy;
		t[3] = -sx; t[4] = cx;
	} else {
		const double rv = 1.0/sqrt(1.0 + x*x + y*y), re = 1.0/sqrt(1.0 + x*x);
		t[0] = rv; t[1] = x*rv; t[2] = y*rv;
		t[3] = -x*re; t[4] = re;
	}
	t[5] = 0.0;
}

// maps [nmap][ny][nx] of T, mstride apart; obj f64 [nobj][2] = (dec, ra) -> out [nobj][nmap][npix] of T.  grid (nobj bpo), up to 256 lanes
template<class T> __global__ __launch_bounds__(256) void thumbs_kernel(Thumb g, int nmap, const T* __restrict__ maps, long mstride, const double* __restrict__ obj,
		const double* __restrict__ tab, T cval, T* __restrict__ out)
{
	const long o = blockIdx.x/(unsigned)g.bpo;
	const int p = (int)(blockIdx.x - o*g.bpo)*blockDim.x + threadIdx.x;
	if (p >= g.npix) return;
	double sd, cd, sr, cr;
	sincos(obj[2*o], &sd, &cd); sincos(obj[2*o + 1], &sr, &cr);
	const double* t = tab + 6l*p;
	// R = Rz(ra) Ry(-dec): (x, y, z) -> (cd x - sd z, y, sd x + cd z) -> (cr x' - sr y', sr x' + cr y', z')
	const double vx = cd*t[0] - sd*t[2], Vz = sd*t[0] + cd*t[2];
	const double Vx = cr*vx - sr*t[1], Vy = sr*vx + cr*t[1];
	T* op = out + o*nmap*g.npix + p;
	double y, x;
	const bool in = axis_coord(g.y, atan2(Vz, hypot(Vx, Vy)), g.order, g.border_y, y) & axis_coord(g.x, atan2(Vy, Vx), g.order, g.border_x, x);
	if (!in) { for (int m = 0; m < nmap; m++) op[(long)m*g.npix] = cval; return; }
	int iy[4], ix[4]; double wy[4], wx[4];
	axis_taps(g.y.n, y, g.order, g.border_y, iy, wy); axis_taps(g.x.n, x, g.order, g.border_x, ix, wx);
	const int nt = g.order + 1;
	double q = 0.0, u = 0.0;
	for (int m = 0; m < nmap; m++) {
		const T* mp = maps + (long)m*mstride;
		double acc = 0.0;      // (order 0: one tap of weight 1, exact in every dtype)
		for (int a = 0; a < nt; a++) {
			const T* rp = mp + (long)iy[a]*g.x.n;
			double s = 0.0;
			for (int b = 0; b < nt; b++) s = fma(wx[b], (double)rp[ix[b]], s);
			acc = fma(wy[a], s, acc);
		}
		if (g.pol && m == g.qc) q = acc;
		else if (g.pol && m == g.uc) u = acc;
		else op[(long)m*g.npix] = (T)acc;
	}
	if (!g.pol) return;
	// R e, and its components along east and north at V, both times hypot(Vx, Vy)
	const double ex = cd*t[3], Ez = sd*t[3];      // (e_z = 0)
	const double Ex = cr*ex - sr*t[4], Ey = sr*ex + cr*t[4];
	const double ce = Vx*Ey - Vy*Ex, cn = (Vx*Vx + Vy*Vy)*Ez - Vz*(Vx*Ex + Vy*Ey);
	const double h2 = ce*ce + cn*cn;
	double c2 = 1.0, s2 = 0.0;
	if (h2 > 0) { c2 = (ce*ce - cn*cn)/h2; s2 = 2.0*ce*cn/h2; }      // (on a pole of the sky there is no north: no rotation)
	op[(long)g.qc*g.npix] = (T)(c2*q + s2*u);
	op[(long)g.uc*g.npix] = (T)(c2*u - s2*q);
}

template<class T> static void launch_thumbs(hipStream_t st, const Thumb& g, long nobj, int bs, int nmap, const void* maps, long mstride, const double* obj, const double* tab,
		double cval, void* out) {
	hipLaunchKernelGGL((thumbs_kernel<T>), dim3((unsigned)(nobj*g.bpo)), dim3(bs), 0, st, g, nmap, (const T*)maps, mstride, obj, tab, (T)cval, (T*)out);
}

} // namespace thb
} // namespace pxs

using namespace pxs;
using namespace pxs::thb;

extern "C" {

int pxm_thumbnails(int nmap, int ny, int nx, const void* d_maps, int map_dtype, int64_t mstride,
                   double yoff, double yscale, double xoff, double xscale, double yref, double yper, double xref, double xper,
                   int64_t nobj, const double* d_obj, int oy, int ox, int proj, double cdelt_y, double crpix_y, double cdelt_x, double crpix_x,
                   int order, int border_y, int border_x, double cval, int pol, int qcomp, int ucomp, void* d_out, int device, void* stream)
{
	PXS_TRY
	PXS_REQUIRE(nmap >= 0 && ny >= 1 && nx >= 1 && nobj >= 0 && oy >= 0 && ox >= 0, "pxm_thumbnails: bad sizes");
	PXS_REQUIRE((int64_t)oy*ox < (int64_t(1) << 24), "pxm_thumbnails: a thumbnail has fewer than 2^24 pixels");
	PXS_REQUIRE(order == 0 || order == 1 || order == 3, "pxm_thumbnails: the order must be 0, 1 or 3");
	PXS_REQUIRE(border_y >= B_NEAREST && border_y <= B_GRIDWRAP && border_x >= B_NEAREST && border_x <= B_GRIDWRAP, "pxm_thumbnails: unknown border rule");
	PXS_REQUIRE(proj == PROJ_CAR || proj == PROJ_TAN, "pxm_thumbnails: the projection is 0 (CAR) or 1 (TAN)");
	PXS_REQUIRE(map_dtype == PX_F32 || map_dtype == PX_F64 || (order == 0 && (map_dtype == PX_U8 || map_dtype == PX_I32)), "pxm_thumbnails: float32 or float64 maps (order 0: uint8 and int32 as well)");
	PXS_REQUIRE(order != 3 || map_dtype == PX_F64, "pxm_thumbnails: order 3 reads float64 coefficients");
	PXS_REQUIRE(nmap <= 1 || mstride >= (int64_t)ny*nx, "pxm_thumbnails: the maps overlap");
	PXS_REQUIRE(!pol || ((map_dtype == PX_F32 || map_dtype == PX_F64) && qcomp >= 0 && qcomp < nmap && ucomp >= 0 && ucomp < nmap && qcomp != ucomp),
		"pxm_thumbnails: the rotation needs two different components of float32 or float64 maps");
	PXS_REQUIRE(yoff == yoff && yscale == yscale && xoff == xoff && xscale == xscale, "pxm_thumbnails: the affine map is not a number");
	PXS_REQUIRE(cdelt_y == cdelt_y && crpix_y == crpix_y && cdelt_x == cdelt_x && crpix_x == crpix_x, "pxm_thumbnails: the thumbnail geometry is not a number");
	const int npix = oy*ox, bs = npix <= 64 ? 64 : 256, bpo = (npix + bs - 1)/bs;
	PXS_REQUIRE(nobj*(int64_t)(bpo > 0 ? bpo : 1) < (int64_t(1) << 31), "pxm_thumbnails: too many objects for one launch");
	PXS_HIP(hipSetDevice(device));
	if (nmap == 0 || nobj == 0 || npix == 0) return 0;
	PXS_REQUIRE(d_maps && d_obj && d_out, "pxm_thumbnails: null arrays");
	hipStream_t st = (hipStream_t)stream;
	DevBuf& tab = stream_scratch(SCR_THUMBS, device, stream);
	tab.ensure(sizeof(double)*6*(size_t)npix);
	hipLaunchKernelGGL(directions_kernel, dim3(blocks_of(npix)), dim3(256), 0, st, oy, ox, proj, cdelt_y, crpix_y, cdelt_x, crpix_x, tab.as<double>());
	const Thumb g = {{ny, yoff, yscale, yref, yper}, {nx, xoff, xscale, xref, xper}, npix, bpo, order, border_y, border_x, pol != 0, qcomp, ucomp};
	switch (map_dtype) {
		case PX_F32: launch_thumbs<float>(st, g, (long)nobj, bs, nmap, d_maps, (long)mstride, d_obj, tab.as<double>(), cval, d_out); break;
		case PX_F64: launch_thumbs<double>(st, g, (long)nobj, bs, nmap, d_maps, (long)mstride, d_obj, tab.as<double>(), cval, d_out); break;
		case PX_U8: launch_thumbs<uint8_t>(st, g, (long)nobj, bs, nmap, d_maps, (long)mstride, d_obj, tab.as<double>(), cval, d_out); break;
		default: launch_thumbs<int32_t>(st, g, (long)nobj, bs, nmap, d_maps, (long)mstride, d_obj, tab.as<double>(), cval, d_out); break;
	}
	PXS_HIP(hipGetLastError());
	PXS_CATCH
}

} // extern "C"
