// CPU model of where the waves of the VALU Legendre kernels leave phase A, for a range of live thresholds (LEG_LIVE, legendre_dev.hpp):
// the accumulating wave-steps and FMA counts of leg_syn_s0<4>, leg_ana_s0<8>, leg_syn_spin<3>, leg_ana_spin<4> on a CC ring set, with the
// library's own tables (LegTables::build_host), start values (pow_scaled / to_scaled, spin_init), m-limit and 4-step test, and the largest
// term a threshold drops.  Plain (non-polar) form of the recurrences throughout: the polar form is the same algebra.
//   g++ -O2 -fopenmp -o leg_live_count tools/leg_live_count.cpp && ./leg_live_count [lmax 10000] [Ncc 20160] [m stride 1] [K of leg_ana_s0] [K of leg_ana_spin]
//                                                                                  [K of leg_syn_s0 4] [K of leg_syn_spin 3] [first pair 0]
// The analysis K default to what the host picks for the ring set (leg_ana_k, legendre.hip: 8 for spin 0; 6 for spin 2 where 4 gives at least 8 waves per m, else 4; k_small_grid's
// rules for small ring sets are not modelled: give the K), so that the counts are those of the kernels as built and can be set against PXS_COUNT.
// first pair: the ring set is the band of the CC rings from that pair to the equator (a declination cut: no polar cap).
// Prints, per kernel and threshold, sum over (m, wave) of (steps - start step) x K x FMAs per step (what PXS_COUNT adds up in a
// seeded launch) and its ratio to the scale-0 rule, then log2 of the largest |lambda| (chain value x alpha) any chain has at a step
// before it is live itself -- an upper bound of what its wave drops, since a wave starts no later than any of its lanes.
// Then, at LEG_LIVE = 2^-140, three ways of dealing ring pairs to waves and blocks: (a) 64 K consecutive pairs per wave with the padding behind the last pair
// (the partition until leg_pair_of existed), (b) the padding in front of pair 0, in wave 0 (leg_pair_of: what the kernels do and PXS_COUNT adds up), (c) = (b) and
// a block of 64 pairs accumulates only from the first 4-step test at which one of its chains, or of a more polar block of the wave, is live: the recurrence FMAs
// (2 of 6, 4 of 12) from the wave's start, the accumulation FMAs from the block's.  (c) is what the kernels do (legendre_dev.hpp, "Block starts") and what PXS_COUNT adds up
// in a seeded launch; the last lines print (b) and (c) as exact integers (FMAs per lane; x 128 = pxs_profile_flops), for tests/test_leg_block_starts.py.
// Last, per kernel, the share of the accumulating wave-steps that lie in phase B (some lane of the wave still below scale 0: the steps with the rescale sweep).
// Runtime on 16 cores: lmax 10^4 at stride 1 about 10 minutes, at stride 7 a minute and a half (the ratios agree to four digits); lmax 4000 (C2: Ncc 8064) at stride 1 a minute.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <algorithm>
#include <climits>
typedef long double LDb;
static const double SC_BIG = 0x1p+400, SC_SMALL = 0x1p-800;
static const int SC_STEP = 800;
static void frexp_norm(double& m, int& e) { int d; m = frexp(m, &d); e += d; }
static void pow_scaled(double x, int n, double& mant, int& e) {
	double rm = 0.5; int re = 1; int be = 0; double bm = frexp(x, &be);
	while (n) { if (n & 1) { rm *= bm; re += be; frexp_norm(rm, re); } bm *= bm; be *= 2; frexp_norm(bm, be); n >>= 1; }
	mant = rm; e = re;
}
static void to_scaled(double mant, int e, double& v, int& scale) {
	if (mant == 0.0) { v = 0.0; scale = 0; return; }
	int s = (e >= 0) ? (e + SC_STEP/2)/SC_STEP : -((-e + SC_STEP/2)/SC_STEP);
	if (s > 0) s = 0;
	v = ldexp(mant, e - SC_STEP*s); scale = s;
}
static const int NT = 8;
static const double THR[NT] = {0.0, 0x1p-340, 0x1p-200, 0x1p-160, 0x1p-140, 0x1p-130, 0x1p-120, 0x1p-90};
static const char* THRN[NT] = {"scale 0", "2^-340", "2^-200", "2^-160", "2^-140", "2^-130", "2^-120", "2^-90"};
static bool live(double v, int sc, int t) { return sc == 0 && (t == 0 ? v != 0.0 : fabs(v) >= THR[t]); }
static double lg(double v, int sc, double alpha) { return (v == 0.0 || alpha == 0.0) ? -1e9 : log2(fabs(v)) + 800.0*sc + log2(fabs(alpha)); }

static const int TLIVE = 4;      // index of LEG_LIVE = 2^-140 in THR
static void run(const int lmax, const long Ncc, const int mstride, int kana0, int kanas, int ksyn0, int ksyns, const int pair0) {
	const LDb PIl = 3.141592653589793238462643383279502884L;
	const int ncc = (int)(Ncc/2 + 1), npairs = (ncc + 1)/2 - pair0;
	if (npairs <= 0) { fprintf(stderr, "no ring pair left\n"); exit(1); }
	std::vector<double> cth(npairs), sth(npairs), sh2(npairs), ch2(npairs);
	for (int p = 0; p < npairs; p++) { const LDb th = 2*PIl*(p + pair0)/Ncc; cth[p] = (double)cosl(th); sth[p] = (double)sinl(th); sh2[p] = (double)sinl(th/2); ch2[p] = (double)cosl(th/2); }
	const double ofs = std::max(100.0, 0.01*lmax);
	if (kana0 <= 0) kana0 = 8;
	if (kanas <= 0) kanas = (npairs + 64*4 - 1)/(64*4) >= 8 ? 6 : 4;
	const int KMAX = 16;      // (blocks per wave the model takes; the kernels compile K up to 8 / 6)
	if (ksyn0 <= 0) ksyn0 = 4;
	if (ksyns <= 0) ksyns = 3;
	if (kana0 > KMAX || kanas > KMAX || ksyn0 > KMAX || ksyns > KMAX) { fprintf(stderr, "K up to %d\n", KMAX); exit(1); }
	const int KS[2][2] = {{ksyn0, kana0}, {ksyns, kanas}};      // [spin 0 / spin 2][synthesis / analysis]
	char kn[4][32]; snprintf(kn[0], 32, "leg_ana_s0<%d>", kana0); snprintf(kn[1], 32, "leg_ana_spin<%d>", kanas); snprintf(kn[2], 32, "leg_syn_s0<%d>", ksyn0); snprintf(kn[3], 32, "leg_syn_spin<%d>", ksyns);
	const char* KN[2][2] = {{kn[2], kn[0]}, {kn[3], kn[1]}};
	double fma_sum[2][2][NT] = {}, steps_sum[2][2][NT] = {}, part_sum[2][2][3] = {}, phb_sum[2][2][2] = {}; double dropmax[2][NT]; double grow4[2] = {0, 0};
	for (int i = 0; i < 2; i++) for (int t = 0; t < NT; t++) dropmax[i][t] = -1e9;
	// sectoral normalisations (build_host)
	std::vector<LDb> cms(lmax + 1), nrm(lmax + 1);
	{ LDb cm = 1/sqrtl(4*PIl); for (int m = 0; m <= lmax; m++) { if (m > 0) cm = -cm*sqrtl((LDb)(2*m+1)/(LDb)(2*m)); cms[m] = cm; } }
	{ const int s = 2; LDb h = 2*s+1; for (int i = 1; i <= s; i++) h = h*(LDb)(s+i)/(LDb)i;
	  for (int m = 0; m < s; m++) { if (m > 0) h = h*(LDb)(s-m+1)/(LDb)(s+m); nrm[m] = sqrtl(h/(4*PIl)); }
	  LDb c2 = (LDb)(2*s+1)/(4*PIl*powl(4.0L, s)); nrm[s] = sqrtl(c2);
	  for (int m = s+1; m <= lmax; m++) { c2 = c2*(LDb)(2*m+1)*(LDb)(2*m)/(4*(LDb)(m+s)*(LDb)(m-s)); nrm[m] = sqrtl(c2); } }
#pragma omp parallel for schedule(dynamic, 1)
	for (int m = 0; m <= lmax; m += mstride) {
		for (int sp = 0; sp < 2; sp++) {
			const int s = sp ? 2 : 0, l0 = std::max(m, s);
			const int n = sp ? lmax - l0 + 1 : (lmax - m)/2 + 1;      // steps of this m
			if (n <= 0) continue;
			std::vector<double> ca(n + 4, 0.0), cb(n + 4, 0.0), al(n + 4, 0.0);
			if (!sp) {
				auto eps = [&](int l) -> LDb { if (l <= m) return 0; LDb L = l, M = m; return sqrtl((L*L-M*M)/(4*L*L-1)); };
				LDb a_prev = 0, a_cur = sqrtl((LDb)(2*m+3))*cms[m];
				for (int k = 0; k < n; k++) {
					const int lp = m + 2*k + 1;
					const LDb e2 = eps(lp+1)*eps(lp+1) + eps(lp)*eps(lp), f = eps(lp)*eps(lp-1), d = eps(lp+1)*eps(lp+2);
					const LDb a_next = (k == 0) ? a_cur/d : -f*a_prev/d;
					const LDb ak = a_cur/(a_next*d);
					ca[k] = (double)ak; cb[k] = (double)(-ak*e2); al[k] = (double)a_cur;
					a_prev = a_cur; a_cur = a_next;
				}
			} else {
				auto Sf = [&](int l) -> LDb { LDb L = l, M = m, Sp = s; return sqrtl((L*L-M*M)*(L*L-Sp*Sp)); };
				LDb b_prev = 0, b_cur = ((m & 1) ? -1 : 1)*nrm[m];
				for (int l = l0; l <= lmax; l++) {
					const LDb L = l, q = sqrtl((2*L+3)/(2*L+1))*(2*L+1);
					const LDb A = q*(L+1)/Sf(l+1), B = q*(LDb)m*(LDb)s/(L*Sf(l+1));
					const LDb C = (l > l0) ? sqrtl((2*L+3)/(2*L-1))*(L+1)*Sf(l)/(L*Sf(l+1)) : 0;
					const LDb b_next = (l == l0) ? A*b_cur : C*b_prev;
					ca[l-l0] = (double)(A*b_cur/b_next); cb[l-l0] = (double)(B*b_cur/b_next); al[l-l0] = (double)b_cur;
					b_prev = b_cur; b_cur = b_next;
				}
			}
			const int kend = 4*(n/4);      // where phase A stops whatever the chains do
			std::vector<int> klive(NT*(size_t)npairs), ktrue(npairs, INT_MAX), kzero(npairs, 0); std::vector<char> alive(npairs);      // kzero: the 4-step test at which every chain of the pair is at scale 0 (n: never);      // ktrue: the test at which the chain IS live at LEG_LIVE (klive: or phase A ran out of steps)
			double dm[NT]; for (int t = 0; t < NT; t++) dm[t] = -1e9; double g4 = 0;
			for (int p = 0; p < npairs; p++) {
				// nc chains: spin 0 one (v2 current, v1 previous), spin 2 two
				double v1[2] = {0, 0}, v2[2] = {0, 0}; int sc[2] = {0, 0}; const int nc = sp ? 2 : 1;
				if (!sp) {
					alive[p] = (double)m <= lmax*sth[p] + ofs;
					if (alive[p]) { double mt; int e; pow_scaled(sth[p], m, mt, e); to_scaled(mt, e, v2[0], sc[0]); }
				} else {
					const double t1 = lmax*sth[p] + ofs, b = -2.0*s*fabs(cth[p]), c = (double)s*s - t1*t1, discr = b*b - 4*c;
					const double mlim = discr <= 0 ? lmax : fmin((double)lmax, 0.5*(-b + sqrt(discr)));
					alive[p] = (double)m <= mlim + 0.5;
					if (alive[p]) for (int h = 0; h < 2; h++) {
						const int es = m >= s ? (h ? m - s : m + s) : (h ? s - m : s + m), ec = m >= s ? (h ? m + s : m - s) : (h ? s + m : s - m);
						double m1, m2; int e1, e2; pow_scaled(sh2[p], es, m1, e1); pow_scaled(ch2[p], ec, m2, e2);
						double mt = m1*m2; int e = e1 + e2 + (m >= s ? m : 0); frexp_norm(mt, e); to_scaled(mt, e, v2[h], sc[h]);
						if (m < s && h && ((s - m) & 1)) v2[h] = -v2[h];
					}
				}
				int* kl = &klive[NT*(size_t)p]; for (int t = 0; t < NT; t++) kl[t] = -1;
				const double x = sp ? cth[p] : cth[p]*cth[p];
				int k = 0, found = 0; kzero[p] = n;
				if (!alive[p]) { for (int t = 0; t < NT; t++) kl[t] = kend; continue; }
				while (true) {
					for (int t = 0; t < NT; t++) if (kl[t] < 0) { bool lv = false; for (int h = 0; h < nc; h++) lv |= live(v2[h], sc[h], t); if (lv || k + 4 > n) { kl[t] = k; found++; if (lv && t == TLIVE) ktrue[p] = k; } }
					bool below = false; for (int h = 0; h < nc; h++) below |= sc[h] < 0;
					if (!below) kzero[p] = std::min(kzero[p], k);
					if (found == NT && (!below || k + 4 > n)) break;
					double before = 0; for (int h = 0; h < nc; h++) if (sc[h] == 0) before = fmax(before, fabs(v2[h]));
					// four steps; the values of these steps are dropped by every threshold not yet reached
					for (int i = 0; i < 4; i++) {
						for (int h = 0; h < nc; h++) {
							const double val = lg(v2[h], sc[h], al[k + i]);
							for (int t = 0; t < NT; t++) if (kl[t] < 0) dm[t] = fmax(dm[t], val);
							const double cf = sp ? ca[k+i]*x + (h ? -cb[k+i] : cb[k+i]) : ca[k+i]*x + cb[k+i];
							const double nx = sp ? fma(cf, v2[h], -v1[h]) : fma(cf, v2[h], v1[h]);
							v1[h] = v2[h]; v2[h] = nx;
						}
					}
					for (int h = 0; h < nc; h++) {
						if (found < NT && sc[h] == 0 && before > 0 && before < 0x1p-90) g4 = fmax(g4, fabs(v2[h])/before);
						if (sc[h] < 0 && fabs(v2[h]) > SC_BIG) { v1[h] *= SC_SMALL; v2[h] *= SC_SMALL; sc[h]++; }
					}
					k += 4;
				}
			}
			double fs[2][NT], ss[2][NT];
			for (int d = 0; d < 2; d++) {
				const int K = KS[sp][d], per = 64*K;
				for (int t = 0; t < NT; t++) { fs[d][t] = 0; ss[d][t] = 0; }
				for (int w0 = 0; w0 < npairs; w0 += per) {
					bool any = false; int ks[NT]; for (int t = 0; t < NT; t++) ks[t] = kend;
					for (int p = w0; p < std::min(npairs, w0 + per); p++) if (alive[p]) { any = true; for (int t = 0; t < NT; t++) ks[t] = std::min(ks[t], klive[NT*(size_t)p + t]); }
					if (!any) continue;
					for (int t = 0; t < NT; t++) { ss[d][t] += n - ks[t]; fs[d][t] += (double)(n - ks[t])*K*(sp ? 12 : 6); }
				}
			}
			// the partitions at LEG_LIVE: pt = 0 padding behind the last pair, 1 in front of pair 0, 2 the same and blocks from their own step
			double ps[2][3] = {}, pb[2][2] = {};
			for (int d = 0; d < 2; d++) {
				const int K = KS[sp][d], per = 64*K, nwave = (npairs + per - 1)/per, frec = sp ? 4 : 2, facc = sp ? 8 : 4;
				for (int pt = 0; pt < 3; pt++) {
					const int pad = pt ? nwave*per - npairs : 0;
					for (int w = 0; w < nwave; w++) {
						bool any = false; int k0 = kend, kz = 0; int bs[KMAX];
						for (int b = 0; b < K; b++) {
							bs[b] = INT_MAX;
							for (int p = std::max(0, w*per + 64*b - pad); p < std::min(npairs, w*per + 64*b + 64 - pad); p++)
								if (alive[p]) { any = true; bs[b] = std::min(bs[b], ktrue[p]); kz = std::max(kz, kzero[p]); }
							k0 = std::min(k0, bs[b]);
						}
						if (!any) continue;
						if (pt == 1) { pb[d][0] += std::max(0, std::min(kz, n) - k0); pb[d][1] += n - k0; }
						if (pt < 2) { ps[d][pt] += (double)(n - k0)*K*(frec + facc); continue; }
						double f = (double)(n - k0)*K*frec; int eff = INT_MAX;
						for (int b = 0; b < K; b++) {
							eff = std::min(eff, bs[b]);
							const int start = b == K - 1 ? k0 : eff;      // (the last block starts with the wave)
							if (start < n) f += (double)(n - start)*facc;
						}
						ps[d][pt] += f;
					}
				}
			}
#pragma omp critical
			{
				for (int d = 0; d < 2; d++) for (int pt = 0; pt < 3; pt++) part_sum[sp][d][pt] += ps[d][pt];
				for (int d = 0; d < 2; d++) for (int i = 0; i < 2; i++) phb_sum[sp][d][i] += pb[d][i];
				for (int d = 0; d < 2; d++) for (int t = 0; t < NT; t++) { fma_sum[sp][d][t] += fs[d][t]; steps_sum[sp][d][t] += ss[d][t]; }
				for (int t = 0; t < NT; t++) dropmax[sp][t] = fmax(dropmax[sp][t], dm[t]);
				grow4[sp] = fmax(grow4[sp], g4);
			}
		}
	}
	printf("lmax %d, Ncc %ld: %d ring pairs from pair %d on, every %d-th m (sums x %d)\n", lmax, Ncc, npairs, pair0, mstride, mstride);
	for (int sp = 0; sp < 2; sp++) for (int d = 0; d < 2; d++) {
		printf("%s  (x 128 = FP64 flops; the T/Q/U round trip runs it once)\n", KN[sp][d]);
		for (int t = 0; t < NT; t++) printf("  live at %-8s wave-steps %.6e  FMA per lane %.6e  ratio %.4f\n", THRN[t], steps_sum[sp][d][t]*mstride, fma_sum[sp][d][t]*mstride, fma_sum[sp][d][t]/fma_sum[sp][d][0]);
	}
	for (int dir = 0; dir < 2; dir++) {
		printf("%s, spin 0 + spin 2 kernels:\n", dir ? "analysis" : "synthesis");
		for (int t = 0; t < NT; t++) { const double a = fma_sum[0][dir][t] + fma_sum[1][dir][t], b = fma_sum[0][dir][0] + fma_sum[1][dir][0];
			printf("  live at %-8s flops %.4e  ratio %.4f\n", THRN[t], a*128*mstride, a/b); }
	}
	printf("at LEG_LIVE = %s, FP64 flops (FMA per lane x 128): padding behind the last pair | in wave 0 | in wave 0 and blocks from their own step (ratios to the first)\n", THRN[TLIVE]);
	for (int sp = 0; sp < 2; sp++) for (int d = 0; d < 2; d++) { const double* q = part_sum[sp][d];
		printf("  %-16s %.5e | %.5e | %.5e   (%.4f, %.4f)\n", KN[sp][d], q[0]*128*mstride, q[1]*128*mstride, q[2]*128*mstride, q[1]/q[0], q[2]/q[0]); }
	for (int d = 0; d < 2; d++) { double q[3]; for (int pt = 0; pt < 3; pt++) q[pt] = part_sum[0][d][pt] + part_sum[1][d][pt];
		printf("  %-16s %.5e | %.5e | %.5e   (%.4f, %.4f)\n", d ? "analysis, both" : "synthesis, both", q[0]*128*mstride, q[1]*128*mstride, q[2]*128*mstride, q[1]/q[0], q[2]/q[0]); }
	printf("FMAs per lane of a seeded launch, exact: all blocks from the wave's start (b) | blocks from their own step (c)\n");
	for (int sp = 0; sp < 2; sp++) for (int d = 0; d < 2; d++) printf("  %-16s %.0f | %.0f\n", KN[sp][d], part_sum[sp][d][1]*mstride, part_sum[sp][d][2]*mstride);
	printf("phase B share of the accumulating wave-steps (padding in wave 0):");
	for (int sp = 0; sp < 2; sp++) for (int d = 0; d < 2; d++) printf("  %s %.2f %%", KN[sp][d], 100*phb_sum[sp][d][0]/phb_sum[sp][d][1]);
	printf("\n");
	for (int sp = 0; sp < 2; sp++) {
		printf("spin %d: largest 4-step growth of a scale-0 chain below 2^-90: 2^%.1f; log2 of the largest |lambda| before a chain is live:", sp ? 2 : 0, log2(grow4[sp]));
		for (int t = 0; t < NT; t++) printf("  %s: %.1f", THRN[t], dropmax[sp][t]);
		printf("\n");
	}
}

int main(int argc, char** argv) {
	run(argc > 1 ? atoi(argv[1]) : 10000, argc > 2 ? atol(argv[2]) : 20160, argc > 3 ? atoi(argv[3]) : 1, argc > 4 ? atoi(argv[4]) : 0, argc > 5 ? atoi(argv[5]) : 0,
		argc > 6 ? atoi(argv[6]) : 0, argc > 7 ? atoi(argv[7]) : 0, argc > 8 ? atoi(argv[8]) : 0);
	return 0;
}
