// The tap and border rules of the spline gathers, shared by pxm_interpol (interpol.hip) and pxm_thumbnails (thumbs.hip): how a line is
// extended, how a coordinate becomes a pixel coordinate on one axis under that axis' border rule, and the tap indices and weights there.
// Everything is per axis, so a kernel may give its two axes different rules.
#pragma once
#include "common.hpp"

namespace pxs {
namespace ipl {

enum : int { EXT_MIRROR = 0, EXT_REFLECT = 1, EXT_PERIODIC = 2, EXT_CLAMP = 3 };
enum : int { B_NEAREST = 0, B_MIRROR = 1, B_CONSTANT = 2, B_WRAP = 3, B_GRIDWRAP = 4 };

// sample i of a line of n under the extension rule: always in [0, n)
__device__ __forceinline__ int ext_index(int ext, long i, int n) {
	if (i >= 0 && i < n) return (int)i;
	if (n == 1) return 0;
	if (ext == EXT_CLAMP) return i < 0 ? 0 : n - 1;
	const long P = ext == EXT_MIRROR ? 2l*(n - 1) : (ext == EXT_REFLECT ? 2l*n : (long)n);
	long m = i % P; if (m < 0) m += P;
	if (m < n) return (int)m;
	return (int)(ext == EXT_MIRROR ? P - m : P - 1 - m);
}

struct Axis { int n; double off, scale, ref, per; };

// the pixel coordinate of p on an axis under the border rule; false: the point takes cval
__device__ __forceinline__ bool axis_coord(const Axis& a, double p, int order, int border, double& xo) {
	double x = fma(a.scale, p, a.off);
	if (a.per > 0) {
		double m = fmod(x - a.ref + 0.5*a.per, a.per);
		if (m < 0) m += a.per;
		x = a.ref + m - 0.5*a.per;
	}
	if (!(fabs(x) < 1e15)) return false;      // (not a number, or no pixel at all)
	const double L = (double)(a.n - 1);
	if (border == B_CONSTANT) { if (x < 0 || x > L) return false; }
	else if (border == B_WRAP) {
		if (a.n == 1) x = 0;
		else if (x < 0) x += L*(double)((long)(-x/L) + 1);
		else if (x > L) x -= L*(double)(long)(x/L);
	} else if (border == B_MIRROR && order == 0) {
		if (a.n == 1) x = 0;
		else { x = fabs(x); x -= 2*L*floor(x/(2*L)); if (x > L) x = 2*L - x; }
	}
	xo = x;
	return true;
}
// the order + 1 taps of an axis at x: indices under the border's index rule, weights
__device__ __forceinline__ void axis_taps(int n, double x, int order, int border, int* idx, double* w) {
	const int ext = border == B_NEAREST ? EXT_CLAMP : (border == B_GRIDWRAP ? EXT_PERIODIC : EXT_MIRROR);
	if (order == 0) { idx[0] = ext_index(ext, (long)floor(x + 0.5), n); w[0] = 1.0; return; }
	const double fl = floor(x), t = x - fl;
	const long i0 = (long)fl;
	if (order == 1) {
		idx[0] = ext_index(ext, i0, n); idx[1] = ext_index(ext, i0 + 1, n);
		w[0] = 1.0 - t; w[1] = t;
		return;
	}
	for (int k = 0; k < 4; k++) idx[k] = ext_index(ext, i0 - 1 + k, n);
	const double u = 1.0 - t;
	w[0] = u*u*u*(1.0/6.0); w[3] = t*t*t*(1.0/6.0);
	w[1] = (4.0 - 6.0*t*t + 3.0*t*t*t)*(1.0/6.0); w[2] = (4.0 - 6.0*u*u + 3.0*u*u*u)*(1.0/6.0);
}

} // namespace ipl
} // namespace pxs
