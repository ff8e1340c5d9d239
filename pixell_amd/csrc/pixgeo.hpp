// The separable cylindrical geometry the pixel operators (srcsim.hip, distance.hip) compute their coordinates from: pixel (y, x) lies at
// dec0 + y ddec, ra0 + x dra (radians).  What pixell_amd/wcs.py separable_geometry() hands over.
#pragma once
#include "common.hpp"
#include <cmath>

namespace pxs {

struct PixGeo { int ny, nx; double dec0, ddec, ra0, dra; int wrap; double period; };      // wrap: the columns cover the whole circle; period: the pixels that 2 pi of RA are

// `who`: the entry point, for the message
inline PixGeo make_pixgeo(const char* who, int ny, int nx, double dec0, double ddec, double ra0, double dra) {
	PXS_REQUIRE(ddec != 0 && dra != 0 && (double)nx*std::fabs(dra) <= 2*PXS_PI + 1e-6, std::string(who) + ": bad geometry (the columns may cover the circle at most once)");
	PixGeo g; g.ny = ny; g.nx = nx; g.dec0 = dec0; g.ddec = ddec; g.ra0 = ra0; g.dra = dra;
	g.wrap = std::fabs((double)nx*std::fabs(dra) - 2*PXS_PI) < 1e-6 ? 1 : 0;
	g.period = 2*PXS_PI/std::fabs(dra);
	return g;
}

__device__ __forceinline__ double pix_dec(const PixGeo& g, int y) { return g.dec0 + (double)y*g.ddec; }
__device__ __forceinline__ double pix_ra(const PixGeo& g, int x) { return g.ra0 + (double)x*g.dra; }

} // namespace pxs
