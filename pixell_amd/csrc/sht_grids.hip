// Grid arithmetic of the SHT plans (host only): the circle of a 2-D geometry, its ring colatitudes, the largest lmax its analysis is
// exact for, and the quadrature weights (pxs_gridweights, pxs_grid_maxlmax of include/pxsht.h).
#include "sht_plan.hpp"
#include <cmath>

namespace pxs {

GridInfo grid_info(const std::string& g, int n) {
	if (g == "CC")     return {2L*n-2, 0, true};
	if (g == "F1")     return {2L*n,   1, true};
	if (g == "MW")     return {2L*n-1, 1, true};
	if (g == "MWflip") return {2L*n-1, 0, true};
	// Driscoll-Healy (north pole + n-1 interior rings of spacing pi/n) and Fejer-2 (n interior rings of spacing pi/(n+1)): the
	// circle has sample points without a ring (a pole), so there is no interpolant to integrate: analysis on these grids is plain
	// quadrature with Fejer's second rule, exact up to get_ducc_maxlmax (curvedsky.py:1349-1353)
	if (g == "DH")     return {2L*n,   0, true};
	if (g == "F2")     return {2L*n+2, 2, true};
	return {0, 0, false};
}
bool grid_weights_only(const std::string& g) { return g == "DH" || g == "F2"; }
// Fejer's second rule on K interior nodes theta_j = j pi/(K+1): w_j = 4 sin(theta_j)/(K+1) sum_{k=1}^{(K+1)/2} sin((2k-1) theta_j)/(2k-1)
// (ring weights, sum 2); the inner sum by the Chebyshev recurrence sin((2k+1)t) = 2 cos(2t) sin((2k-1)t) - sin((2k-3)t)
static std::vector<LDb> fejer2_weights(int K) {
	std::vector<LDb> w(K);
	for (int j = 1; j <= K; j++) {
		const LDb t = (LDb)j*PIl/(K+1), c2 = 2*cosl(2*t);
		LDb sm = -sinl(t), s0 = sinl(t), acc = 0;          // sin(-t), sin(t)
		for (int k = 1; k <= (K+1)/2; k++) { acc += s0/(2*k-1); const LDb sn = c2*s0 - sm; sm = s0; s0 = sn; }
		w[j-1] = 4*sinl(t)/(K+1)*acc;
	}
	return w;
}
int grid_maxlmax(const std::string& g, int n) {
	if (g == "CC") return n-2;
	if (g == "DH") return (n-2)/2;
	if (g == "F2") return (n-1)/2;
	return n-1;
}
std::vector<LDb> grid_theta(const std::string& g, int n) {
	GridInfo gi = grid_info(g, n);
	std::vector<LDb> th(n);
	for (int j = 0; j < n; j++) th[j] = (LDb)gi.c*PIl/gi.N + 2*PIl*j/gi.N;
	return th;
}
// Fourier coefficients of |sin|: s_q = -(2/pi)/(q^2-1) (q even), 0 (q odd)
double abs_sin_coef(long q) { if (q & 1) return 0.0; LDb Q = q; return (double)(-(2/PIl)/(Q*Q-1)); }

std::vector<double> grid_weights(const std::string& g, int n) {
	std::vector<double> w(n); if (pxs_gridweights(g.c_str(), n, w.data()) != 0) throw Error(PXS_ERR_ARG, get_last_error());
	return w; }
DevBuf ring_weight_table(const std::string& g, int n, int nphi) {
	const std::vector<double> w = grid_weights(g, n); std::vector<double2> wd(n);
	for (int j = 0; j < n; j++) wd[j] = make_double2(w[j]/nphi, 0.0);
	return upload(wd);
}

} // namespace pxs

extern "C" {

int pxs_grid_maxlmax(const char* geometry, int ntheta) { return grid_maxlmax(geometry ? geometry : "", ntheta); }

int pxs_gridweights(const char* geometry, int ntheta, double* out) {
	PXS_TRY
	PXS_REQUIRE(geometry && out && ntheta > 0, "pxs_gridweights: bad arguments");
	GridInfo gi = grid_info(geometry, ntheta);
	if (!gi.ok) throw Error(PXS_ERR_UNSUPPORTED, std::string("gridweights: unsupported geometry '") + geometry + "' (CC, F1, MW, MWflip, DH, F2)");
	if (grid_weights_only(geometry)) {
		const bool dh = std::string(geometry) == "DH";
		const std::vector<LDb> w = fejer2_weights(dh ? ntheta-1 : ntheta);
		if (dh) out[0] = 0;
		for (size_t j = 0; j < w.size(); j++) out[j + (dh ? 1 : 0)] = (double)(w[j]*2*PIl);
		return 0;
	}
	const long N = gi.N; const int n = ntheta;
	const LDb th0 = (LDb)gi.c*PIl/N;
	std::vector<LDb> v(N);
	const long K = (N-1)/2;
	if (N <= 4096) {
		for (long j = 0; j < N; j++) {
			LDb th = th0 + 2*PIl*j/N, s = (LDb)abs_sin_coef(0);
			for (long k = 2; k <= K; k += 2) s += 2*(-(2/PIl)/((LDb)k*k-1))*cosl(k*th);
			if (N % 2 == 0 && ((N/2) % 2) == 0) s += (-(2/PIl)/((LDb)(N/2)*(N/2)-1))*cosl((N/2)*(th-th0))*cosl((N/2)*th0);
			v[j] = s*PIl/N;
		}
	} else {
		// the same cosine series as one backward DFT of length N on the device (the direct sum is N^2/4 long-double cosines:
		// 60 s for the 21600-ring grid, paid by every map2alm of a declination band through quad_weights)
		std::vector<double2> c(N, make_double2(0, 0));
		c[0].x = (double)abs_sin_coef(0);
		for (long k = 2; k <= K; k += 2) {
			const LDb sk = -(2/PIl)/((LDb)k*k-1), a = (LDb)k*th0;
			c[k] = make_double2((double)(sk*cosl(a)), (double)(sk*sinl(a)));
			c[N-k] = make_double2(c[k].x, -c[k].y);
		}
		if (N % 2 == 0 && ((N/2) % 2) == 0) c[N/2] = make_double2((double)((-(2/PIl)/((LDb)(N/2)*(N/2)-1))*cosl((N/2)*th0)), 0.0);
		int dev = 0; PXS_HIP(hipGetDevice(&dev));
		DevBuf dc = upload(c);
		fft_dense_lines(dev, nullptr, N, false, 1, dc.as<double2>(), dc.as<double2>());
		PXS_HIP(hipStreamSynchronize(nullptr));
		PXS_HIP(hipMemcpy(c.data(), dc.p, sizeof(double2)*N, hipMemcpyDeviceToHost));
		for (long j = 0; j < N; j++) v[j] = (LDb)c[j].x*PIl/N;
	}
	for (int j = 0; j < n; j++) out[j] = 0;
	for (long jp = 0; jp < N; jp++) { long r = jp < n ? jp : ((-jp - gi.c) % N + N) % N; out[r] += (double)(v[jp]*2*PIl); }
	PXS_CATCH
}

} // extern "C"
