// Fused FFT chains of the SHT for gfx950.
//
// Every long transform (ring FFT of nphi points, theta FFTs of N, M, Ncc points) is a four-step transform
// X = a*b: pass 1 runs a-point transforms over the residues mod b, pass 2 b-point transforms that produce the residues
// mod a.  When two consecutive transforms share the modulus g (N = g*bN, M = g*g2, Ncc = ac*g) the residue class that
// pass 2 of one transform produces is exactly the class pass 1 of the next one consumes -- the spectrum resize between
// them maps class r to class r -- so both passes run back to back on the same lines in LDS:
//
//   analysis  (leg on the map's rings -> weighted leg on the CC grid), per pair of columns (m, m+1):
//     RA1  mirror-pair extension, FFT_g           -> Y1      RA2  FFT_bN, shift/pad to M, IFFT_g2     -> Z2
//     RA3  IFFT_g, x |sin| series, FFT_g          -> V3      RA4  FFT_g2, keep |k| <= lmax, IFFT_ac   -> U4
//     RA5  IFFT_g, separate the pair, weights     -> leg_cc
//   synthesis (leg on the CC grid -> ring spectra h[ring][m]):
//     RS1  mirror-pair extension, FFT_gs -> Y    RS2  FFT_bs, keep |k| <= lmax, shift, IFFT_aNs -> Z    RS3  IFFT_gs, separate, transpose -> h
//   ring FFTs: MA1/MA2 (two real rings per complex line; pass 2 unpacks the pair and writes leg[m][ring] directly),
//              MS1/MS2 (Hermitian pair load straight from h[ring][m]; pass 2 writes the two rings).
//
// Every intermediate array is written once and read once; one side of each access is fully contiguous, the other
// side moves runs of T*16 bytes (T = lines per tile, a multiple of 8: whole 128-byte lines, measured at copy speed
// on MI355X with tools/stride_bw.hip).  All global loads of a tile are issued before the first LDS write.
// Replaces ducc0's ring FFTs / resample_theta inside synthesis_2d / analysis_2d (pixell/curvedsky.py:907-924, 1032-1046).
#include "fftchain.hpp"
#include "fft_dev.hpp"
#include "fft_static_dev.hpp"
#include "chain_dev.hpp"
#include <algorithm>
#include <set>
#include <type_traits>
#include <cmath>

namespace pxs {

#ifndef PXS_CH_PTS
#define PXS_CH_PTS 2560    /* complex points per tile */
#endif
#ifdef PXS_HOST_SIM
static constexpr int CH_NT = 1, CH_MAXE = PXS_CH_PTS;
#else
#ifndef PXS_CH_NT
#define PXS_CH_NT 512      /* threads per workgroup: measured at config 3 (ring FFT + theta resampling, one stream) 256: 129 ms, 512: 115 ms */
#endif
static constexpr int CH_NT = PXS_CH_NT, CH_MAXE = (PXS_CH_PTS + PXS_CH_NT - 1)/PXS_CH_NT;
#endif
static constexpr int CH_TILE_PTS = PXS_CH_PTS;
static constexpr int CH_NMAX = 512;           // longest LDS sub-transform of a chain stage      // points per tile = CH_NT * CH_MAXE on the device

struct TileC { int outer, t0, nl, comp, q0; };

// alignas(64): a stage's own fields start on a 64-byte boundary whatever the base holds.  The compiler merges the scalar loads of the
// kernel arguments into aligned 16- to 64-byte loads, so the fields' offsets modulo 64 decide which loads merge and, through the
// schedule, the registers: with the base 40 bytes shorter and unaligned StResize 112/150 T = 16 went from 64 to 66 VGPRs (8 -> 7 waves)
// and StColOut 120 T = 16 from 54 to 55 with their own text unchanged; aligned, both are back (profiles/chain_static_kernel_resources.txt).
// The alignment does not protect against other changes: rerun tools/kres.py on this file whenever a stage struct changes.
struct alignas(64) StageBase {
	// radix 7 compiled into the stage's kernel (MAXR = 9 stages): the theta stages, for ducc0's ring counts.  Its code costs the kernels
	// that hold it 2-4 % (same box, tools/fft2_ab.sh: enmap.fft 17.3 -> 17.7 ms, enmap.ifft 32.2 -> 33.7), so the 2-D FFT stages leave it out
	static constexpr bool R7 = true;
	// threads per workgroup.  Per-stage A/B at C3 (profiles/r04b_ntlab_c3.txt): 512 wins for every stage (256: ring stages
	// +15-25 %, StResize / StSigma +5-9 %; 384: 0 to +10 %) except the transposing split StSplit<1>: from_cc 12.27 -> 11.45 ms with 256
	static constexpr int NT = CH_NT;
	// most points a tile of the stage may hold (the kernel's per-thread element count follows from it)
	static constexpr int PTS = CH_TILE_PTS;
	LdsFft fa, fb;
	int T; int ntile;
	FastDiv dT, dna, dnb, dnt;
	// four-step twiddle of the stage's output, W_X^{(t0 + li) e} = W_X^{t0 e} * W_X^{li e}: the first factor is gathered once per tile
	// from the full table btw (into LDS), the second comes from a small table tws[e][li] shared by all tiles (coalesced reads).
	// (One gather per point from the full table made every wave instruction touch 64 cache lines.)
	const double2* btw; const double2* tws;
	// Prefetch ahead: a workgroup of a stage that loads whole rows touches the rows of the tile `pf` workgroups ahead (one dword per
	// 128-byte line, issued after its own loads, consumed by nothing until the kernel ends), so that tile's loads hit the L2 when its
	// workgroup starts -- on the same XCD: workgroups go round-robin to the 8 XCDs and pf is a multiple of 8.  Measured at C3 / C4
	// (tools/chain_lab.py, 5 repetitions, profiles/r04b_prefetch_ahead.txt): pf = 24, 48: +2 %; 96: -0.5 %; 128 ... 256: -2.5 % (to_cc
	// 30.0 -> 28.4 ms, C4 11.6 -> 10.8); 384 ... 768: -2 % (from_cc 17.1 -> 16.5); 1536: 0; 3072: +6 %.  PXS_CH_PF overrides (0: off).
	int pf;
	static constexpr int PF = 256;
	// stages that load strided runs name the 128-byte lines of a tile themselves (pfaddr), PFI per thread at most.  Only the first stage of
	// the 2-D FFTs does: for StFirst of the theta chains and the ring stages MA1 / MS1 it was measured and lost (the ring stages, held to
	// 64 VGPRs, spill with it: profiles/r04b_prefetch_ahead.txt); enmap.ifft of 21600 x 43200: 32.2 -> 30.2 ms.
	static constexpr int PFI = 0;
	__device__ __forceinline__ const void* pfaddr(const TileC&, int) const { return nullptr; }
};

// (Tried: persistent workgroups that issue the global loads of their NEXT tile into registers before the LDS passes of the current
// one.  The prefetch registers pushed the single-transform stages to 151-169 VGPRs and the two-transform stages to 256 (172 with
// 512-thread workgroups), and config 3 got slower: ring FFT 58 -> 67 ms, theta resampling 71 -> 129 ms (102 ms with 512 threads).
// One tile per workgroup, many workgroups per CU in different phases, stays.)
// (Tried in round 3, tools/chain_lab.py, profiles/r03_chain_lab_fused_passes.jsonl: fusing the first radix pass of a transform with
// the global loads (each thread fetches the R inputs of its butterflies) and the last pass with the store -- 7 instead of 10 LDS
// write sweeps and barriers in a two-transform stage.  93 VGPRs (two instead of three workgroups per CU), or 80 with spills under
// __launch_bounds__: C3 chain stages 110.6 ms unfused, 124.8-136.8 ms fused; C4 27.0 / 28.4-30.4.  Not kept.)
// S::MINW = 8 asks the compiler for <= 64 VGPRs (8 waves per SIMD = four 512-thread workgroups per CU where the LDS allows):
// the ring stages, whose passes use radices up to 8 (S::MAXR), gain 6-12 % from it; with radix 9 compiled in the same bound spills.
#ifndef PXS_HOST_SIM
#define PXS_CH_BOUNDS __launch_bounds__(NT, S::MINW)
#else
#define PXS_CH_BOUNDS
#endif
template<class S, int NT, int MAXE> __global__ PXS_CH_BOUNDS void chain_kernel(const S s)
{
	PXS_SHARED(double2, lds);
	const int na = s.fa.n, nb = s.fb.n;
	const int nlast = S::TWO ? nb : na, nslast = S::TWO ? s.fb.ns : s.fa.ns;
	// (two transforms of one length share the W_n table: StSigma at g = 320 then fits three times on a CU instead of twice)
	const bool same_tw = S::TWO && nb == na;
	double2* twa = lds; double2* twb = same_tw ? lds : lds + na; double2* twx = lds + na + (same_tw ? 0 : nb); double2* buf = twx + (S::HAS_TW ? nlast : 0);
	TileC c;
	if (!s.decode((int)blockIdx.x, c)) return;
	const bool have_tw = S::HAS_TW && s.btw != nullptr;
	const int T = s.T;
	int pf_val = 0;
	{	// ---- load: every global load of the tile is in flight before the first LDS write
		const int total = T*na;
		double2 v[MAXE]; int pos[MAXE];
#pragma unroll
		for (int u = 0; u < MAXE; u++) {
			const int idx = threadIdx.x + u*NT; pos[u] = -1;
			if (idx < total) {
				uint32_t li, e;
				if (S::LOAD_LINE_FAST) { e = fdiv(idx, s.dT); li = idx - e*T; }
				else { li = fdiv(idx, s.dna); e = idx - li*na; }
				v[u] = s.load(c, (int)li, (int)e);
				if (S::INV_A) v[u].y = -v[u].y;
				pos[u] = (int)li*s.fa.ns + s.fa.perm[e];
			}
		}
		if ((S::LOADK == 0 || S::PFI > 0) && s.pf > 0 && (long)blockIdx.x + s.pf < (long)gridDim.x) {	// (issued after the tile's own loads: the wait before the LDS writes below does not include it)
			TileC c2;
			if (s.decode((int)blockIdx.x + s.pf, c2)) {
				if (S::LOADK == 0) {	// whole rows: one dword per 128-byte line
					const int per = (na*16 + 127) >> 7, i = threadIdx.x;
					if (i < T*per) {
						const int li = i/per, seg = i - li*per;
						const double2* r = s.row(c2, li);
						if (r) pf_val = *reinterpret_cast<const int*>(reinterpret_cast<const char*>(r) + seg*128);
					}
				} else {	// runs of T elements at a stride: the stage names the lines, at most S::PFI per thread
#pragma unroll
					for (int it = 0; it < S::PFI; it++) {
						const void* q = s.pfaddr(c2, (int)threadIdx.x + it*NT);
						if (q) pf_val += *reinterpret_cast<const int*>(q);
					}
				}
			}
		}
		for (int k = threadIdx.x; k < na; k += NT) twa[k] = s.fa.tw[k];
		if (!same_tw) for (int k = threadIdx.x; k < nb; k += NT) twb[k] = s.fb.tw[k];
		if (have_tw) for (int k = threadIdx.x; k < nlast; k += NT) twx[k] = s.btw[(long)c.t0*k];
#pragma unroll
		for (int u = 0; u < MAXE; u++) if (pos[u] >= 0) buf[pos[u]] = v[u];
	}
	PXS_LDS_BARRIER();
	lds_fft<NT, S::MAXR, S::R7>(buf, twa, s.fa, T);
	if (S::TWO) {	// ---- second transform on the same lines: pull its inputs out of the first one's output (lines fastest across lanes)
		const int total = T*nb;
		double2 v[MAXE]; int pos[MAXE];
#pragma unroll
		for (int u = 0; u < MAXE; u++) {
			const int idx = threadIdx.x + u*NT; pos[u] = -1;
			if (idx < total) {
				const uint32_t e = fdiv(idx, s.dT), li = idx - e*T;
				{ const double2* Al = buf + li*s.fa.ns; v[u] = s.mid(c, (int)li, (int)e, [&](int k) { return Al[k]; }); }
				if (S::INV_B) v[u].y = -v[u].y;
				pos[u] = (int)li*s.fb.ns + s.fb.perm[e];
			}
		}
		PXS_LDS_BARRIER();
#pragma unroll
		for (int u = 0; u < MAXE; u++) if (pos[u] >= 0) buf[pos[u]] = v[u];
		PXS_LDS_BARRIER();
		lds_fft<NT, S::MAXR, S::R7>(buf, twb, s.fb, T);
	}
	{	// ---- store
		const int total = T*nlast;
		const FastDiv dl = S::TWO ? s.dnb : s.dna;
		for (int idx = threadIdx.x; idx < total; idx += NT) {
			uint32_t li, e;
			if (S::STORE_LINE_FAST) { e = fdiv(idx, s.dT); li = idx - e*T; } else { li = fdiv(idx, dl); e = idx - li*nlast; }
			double2 w = make_double2(1, 0);
			if (have_tw) w = cmul(twx[e], s.tws[e*T + li]);
			s.store(c, (int)li, (int)e, [&](int l2, int e2) { return buf[l2*nslast + e2]; }, w);
		}
	}
#ifndef PXS_HOST_SIM
	if (S::LOADK == 0 || S::PFI > 0) asm volatile("" :: "v"(pf_val));
#endif
}

// ---------------------------------------------------------------------------------------------------------------
// theta chains
// ---------------------------------------------------------------------------------------------------------------
// pass 1 of the first transform of a chain: circle index j = b*j1 + j2, line = j2, a-point FFT over j1, four-step twiddle
struct StFirst : StageBase {
	static constexpr int SID = 0;
	static constexpr bool TWO = false, INV_A = false, INV_B = false, LOAD_LINE_FAST = true, STORE_LINE_FAST = true, HAS_TW = true;
	static constexpr int MAXR = 9, MINW = 1;
	PairSrc src; int b; double2* Y; long ldY; int npair; FastDiv dnp;       // outer = comp*npair + pair
	static constexpr int LOADK = 1, STOREK = 0;
	__device__ __forceinline__ const double2* row(const TileC&, int) const { return nullptr; }
	__device__ __forceinline__ bool decode(int bx, TileC& c) const {
		c.outer = fdiv(bx, dnt); c.t0 = (bx - c.outer*ntile)*T; c.nl = min(T, b - c.t0);
		c.comp = fdiv(c.outer, dnp); c.q0 = c.outer - c.comp*npair; return true; }
	__device__ __forceinline__ double2 load(const TileC& c, int li, int e) const {
		if (li >= c.nl) return make_double2(0, 0);
		return src.get(c.comp, c.q0, b*e + c.t0 + li); }
	template<class AF> __device__ __forceinline__ double2 mid(const TileC&, int, int, AF&&) const { return make_double2(0, 0); }
	template<class VF> __device__ __forceinline__ void store(const TileC& c, int li, int e, VF&& val, double2 w) const {
		if (li >= c.nl) return;
		Y[((long)c.outer*fa.n + e)*ldY + c.t0 + li] = cmul(val(li, e), w); }
};

// ... of the 2-D FFTs (plain mode; lengths are 2-3-5-smooth there, split_balanced)
struct StFirst2D : StFirst {
	static constexpr int SID = 10;      // (its own kernel: a stage id of its own in the static table and the per-stage switches)
	static constexpr bool R7 = false;
	// the tile's samples are runs of nl elements at j = b e + t0 of row q0: every 8th element names a 128-byte line
	static constexpr int PFI = 2;
	__device__ __forceinline__ const void* pfaddr(const TileC& c, int i) const {
		const int segs = (c.nl + 7) >> 3;
		const int e = i/segs; if (e >= fa.n) return nullptr;
		return src.leg + (long)c.comp*src.cstride + (long)c.q0*src.ld + (b*e + c.t0 + 8*(i - e*segs)); }
};

// pass 2 of transform X1 (forward, b1 points) + spectrum resize + pass 1 of transform X2 (backward, a2 points); shared modulus g.
// in: Y[outer][k1 < g][j2 < b1]; out: Z[outer][k1' < a2][k1 < g] (row stride ldZ).
// resize rule: signed frequency kappa of the X2 slot; zero beyond kmax (or beyond X1/2); Nyquist bin of X1 halved when nyq;
// optional phase table ph[|kappa|], conjugated for kappa < 0.
struct StResize : StageBase {
	static constexpr int SID = 1;
	static constexpr bool TWO = true, INV_A = false, INV_B = true, LOAD_LINE_FAST = false, STORE_LINE_FAST = true, HAS_TW = true;
	#ifndef PXS_RESIZE_MINW
#define PXS_RESIZE_MINW 1      /* 8 (at most 64 VGPRs, 20 bytes of scratch per lane, four workgroups per CU where the LDS allows) measured: to_cc 29.9 -> 34.1 ms at C3, 11.4 -> 13.0 at C4 */
#endif
	static constexpr int MAXR = 9, MINW = PXS_RESIZE_MINW;
	const double2* Y; long ldY; double2* Z; long ldZ;
	int g, X1, X2, kmax, nyq; const double2* ph; FastDiv dg;
	int adj;      // transposed padding rule (X1 > X2): conjugate phase, and the Nyquist slot of X2 collects 1/2 of both +-X2/2 bins of X1
	static constexpr int LOADK = 0, STOREK = 0;
	__device__ __forceinline__ const double2* row(const TileC& c, int li) const { return li < c.nl ? Y + ((long)c.outer*g + c.t0 + li)*ldY : nullptr; }
	__device__ __forceinline__ bool decode(int bx, TileC& c) const {
		c.outer = fdiv(bx, dnt); c.t0 = (bx - c.outer*ntile)*T; c.nl = min(T, g - c.t0); return true; }
	__device__ __forceinline__ double2 load(const TileC& c, int li, int e) const {
		if (li >= c.nl) return make_double2(0, 0);
		return Y[((long)c.outer*g + c.t0 + li)*ldY + e]; }
	template<class AF> __device__ __forceinline__ double2 mid(const TileC& c, int li, int e, AF&& A) const {
		if (li >= c.nl) return make_double2(0, 0);
		const int k1 = c.t0 + li;
		const int jp = g*e + k1;
		const int kap = (2*jp <= X2) ? jp : jp - X2;
		const int ak = kap < 0 ? -kap : kap;
		if ((kmax >= 0 && ak > kmax) || 2*ak > X1) return make_double2(0, 0);
		const int k = kap >= 0 ? kap : kap + X1;
		const uint32_t k2 = fdiv((uint32_t)(k - k1), dg);
		double2 v = A((int)k2);
		if (adj) {
			double2 t = ph ? ph[ak] : make_double2(1, 0);
			if (2*ak == X2 && X1 != X2) {      // both bins are in this line: X1, X2 and hence +-X2/2 are congruent mod g
				const double2 vm = A((int)fdiv((uint32_t)(X1 - ak - k1), dg));
				const double2 r = cadd(cmul(v, cconj(t)), cmul(vm, t));
				return cscale(r, 0.5);
			}
			if (kap >= 0) t.y = -t.y;
			return cmul(v, t);
		}
		if (nyq && 2*ak == X1) v = cscale(v, 0.5);
		if (ph) { double2 t = ph[ak]; if (kap < 0) t.y = -t.y; v = cmul(v, t); }
		return v; }
	template<class VF> __device__ __forceinline__ void store(const TileC& c, int li, int e, VF&& val, double2 w) const {
		if (li >= c.nl) return;
		Z[((long)c.outer*fb.n + e)*ldZ + c.t0 + li] = cmul(cconj(val(li, e)), cconj(w)); }
};

// pass 2 of IFFT_M (g points), pointwise product with the |sin| series samples, pass 1 of FFT_M (g points)
// in: Z[outer][k1' < g2][r < g]; out: V[outer][k1'' < g][k1' < g2]
struct StSigma : StageBase {
	static constexpr int SID = 2;
	static constexpr bool TWO = true, INV_A = true, INV_B = false, LOAD_LINE_FAST = false, STORE_LINE_FAST = true, HAS_TW = true;
	static constexpr int MAXR = 9, MINW = 1;
	const double2* Z; long ldZ; double2* V; long ldV; int g, g2; const double2* sigma;
	static constexpr int LOADK = 0, STOREK = 0;
	__device__ __forceinline__ const double2* row(const TileC& c, int li) const { return li < c.nl ? Z + ((long)c.outer*g2 + c.t0 + li)*ldZ : nullptr; }
	__device__ __forceinline__ bool decode(int bx, TileC& c) const {
		c.outer = fdiv(bx, dnt); c.t0 = (bx - c.outer*ntile)*T; c.nl = min(T, g2 - c.t0); return true; }
	// (c.t0 + li grouped, here and in store: the 32-bit line index that row() and mid() use too; summed into the 64-bit outer*g2 first
	// it cost StSigma 48/48 T = 48 two more VGPRs, 72 against 70 and 68)
	__device__ __forceinline__ double2 load(const TileC& c, int li, int e) const {
		if (li >= c.nl) return make_double2(0, 0);
		return Z[((long)c.outer*g2 + (c.t0 + li))*ldZ + e]; }
	template<class AF> __device__ __forceinline__ double2 mid(const TileC& c, int li, int e, AF&& A) const {
		if (li >= c.nl) return make_double2(0, 0);
		return cmul(cconj(A(e)), sigma[(c.t0 + li) + g2*e]); }
	template<class VF> __device__ __forceinline__ void store(const TileC& c, int li, int e, VF&& val, double2 w) const {
		if (li >= c.nl) return;
		V[((long)c.outer*g + e)*ldV + (c.t0 + li)] = cmul(val(li, e), w); }
};

// last pass of a backward chain (IFFT over r < g for the lines k1 < a, circle index t = k1 + a*k2) + separation of the packed pair
// by reflection symmetry.
// MODE 0: a tile holds TH primary lines and their mirror lines (slots li and li + TH) of one pair;
//         out = leg[(col)*ld + t] * w[t] * scale, rings t < nr_out          (analysis: CC grid, weights)
// MODE 1: a tile holds T/2 pairs x (line, mirror line), slot = 2*pi + which;
//         out = h[t*ld + col] * conj(tab[col]) * scale                      (synthesis: ring-major rows for the ring FFT)
template<int MODE> struct StSplit : StageBase {
	static constexpr int SID = 3 + MODE;
#ifndef PXS_HOST_SIM
	static constexpr int NT = MODE == 1 ? 256 : CH_NT;
#endif
	static constexpr int PF = MODE == 1 ? 512 : 256;      // (per-stage sweep, profiles/r04b_prefetch_ahead.txt: from_cc 16.9 -> 16.3 ms at 512 ... 768)
	static constexpr bool TWO = false, INV_A = true, INV_B = false, LOAD_LINE_FAST = false, STORE_LINE_FAST = true, HAS_TW = false;
	static constexpr int MAXR = 9, MINW = 1;
	const double2* U; long ldU; int a, g, X, mir_c, nr_out, a_odd, ncol, npair;
	double2* out; long ld; const double2* w; const double2* tab; double scale; int TH; FastDiv da;
	long ocstride; int groups; FastDiv dnp, dgr;      // components of a launch: output stride; MODE 0: outer = comp*npair + pair, MODE 1: outer = comp*groups + group
	int self_half;     // self-mirrored output rings get weight 1/2 (adjoint of a mirror extension, which reads them once)
	static constexpr int LOADK = 0, STOREK = 1;
	__device__ __forceinline__ const double2* row(const TileC& c, int li) const {
		int line, pair; slot(c, li, line, pair);
		return line >= 0 ? U + (((long)c.comp*npair + pair)*a + line)*ldU : nullptr; }
	__device__ __forceinline__ int mirror_line(int k) const { int m = a - k - mir_c; if (m >= a) m -= a; if (m < 0) m += a; return m; }
	__device__ __forceinline__ bool decode(int bx, TileC& c) const {
		c.outer = fdiv(bx, dnt); c.t0 = (bx - c.outer*ntile)*(MODE == 0 ? TH : 1); c.nl = T;
		if (MODE == 0) { c.comp = fdiv(c.outer, dnp); c.q0 = c.outer - c.comp*npair; }
		else { c.comp = fdiv(c.outer, dgr); c.q0 = (c.outer - c.comp*groups)*(T/2); }
		if (MODE == 1) { if (mirror_line(c.t0) < c.t0) return false; }      // the tile of the mirror line does this one
		return true; }
	// line and pair (within its component) of LDS slot li (line < 0: unused slot)
	__device__ __forceinline__ void slot(const TileC& c, int li, int& line, int& pair) const {
		if (MODE == 0) {
			pair = c.q0;
			const int prim = c.t0 + (li < TH ? li : li - TH);
			line = -1;
			if (prim < a) {
				const int m = mirror_line(prim);
				if (li < TH) { if (prim <= m) line = prim; }                   // primary lines: the smaller of (line, mirror)
				else if (prim < m) line = m;
			}
		} else {
			pair = c.q0 + (li >> 1);
			const int m = mirror_line(c.t0);
			line = (li & 1) ? (m != c.t0 ? m : -1) : c.t0;
			if (pair >= npair) line = -1;
		}
	}
	__device__ __forceinline__ double2 load(const TileC& c, int li, int e) const {
		int line, pair; slot(c, li, line, pair);
		if (line < 0) return make_double2(0, 0);
		return U[(((long)c.comp*npair + pair)*a + line)*ldU + e]; }
	template<class AF> __device__ __forceinline__ double2 mid(const TileC&, int, int, AF&&) const { return make_double2(0, 0); }
	template<class VF> __device__ __forceinline__ void store(const TileC& c, int li, int e, VF&& val, double2) const {
		int line, pair; slot(c, li, line, pair);
		if (line < 0) return;
		const int t = line + a*e;
		if (t >= nr_out) return;
		int tm = X - t - mir_c; if (tm >= X) tm -= X; if (tm < 0) tm += X;
		const double2 z = cconj(val(li, e));
		double2 ev, od;
		if (tm == t) { ev = self_half ? cscale(z, 0.5) : z; od = make_double2(0, 0); }
		else {
			const int ml = mirror_line(line);
			const int lp = (ml == line) ? li : (MODE == 0 ? (li < TH ? li + TH : li - TH) : (li ^ 1));
			const int e2 = (int)fdiv((uint32_t)(tm - ml), da);
			const double2 y = cconj(val(lp, e2));
			ev = make_double2(0.5*(z.x + y.x), 0.5*(z.y + y.y)); od = make_double2(0.5*(z.x - y.x), 0.5*(z.y - y.y));
		}
		const int ca = 2*pair;
		double2 va = a_odd ? od : ev, vb = a_odd ? ev : od;
		double2* oc = out + (long)c.comp*ocstride;
		if (MODE == 0) {
			const double f = scale*(w ? w[t].x : 1.0);
			oc[(long)ca*ld + t] = cscale(va, f);
			if (ca + 1 < ncol) oc[(long)(ca + 1)*ld + t] = cscale(vb, f);
		} else {
			const double f = scale*(w ? w[t].x : 1.0);
			oc[(long)t*ld + ca] = cscale(cmul(va, cconj(tab[ca])), f);
			if (ca + 1 < ncol) oc[(long)t*ld + ca + 1] = cscale(cmul(vb, cconj(tab[ca + 1])), f);
		}
	}
};

// ---------------------------------------------------------------------------------------------------------------
// ring FFTs
// ---------------------------------------------------------------------------------------------------------------

// MA1: two real rings as one complex line z = ring(2q) + i ring(2q+1); pixel x = b*j1 + j2, line = j2, a-point FFT over j1
struct StRingA1 : StageBase {
	static constexpr int SID = 5;
	// MA1 reads the map in runs of T reals: 16 lines make whole 128-byte lines.  Where 2560 points hold fewer (C3: 180-point lines, T = 14) the
	// tile may grow to 2880 points (profiles/r04b_tile2880_ab.txt: map2leg of the Q/U pair 14.74 -> 13.76 ms, enmap.fft 17.65 -> 16.78 ms;
	// 2880-point tiles for every stage: nothing elsewhere at C3, +2 % at C4)
	static constexpr int PTS = 2880;
	static constexpr bool TWO = false, INV_A = false, INV_B = false, LOAD_LINE_FAST = true, STORE_LINE_FAST = true, HAS_TW = true;
	static constexpr int MAXR = 8, MINW = 8;
	MapAddr m; int b, npair; double2* Y; long ldY; FastDiv dnp;
	static constexpr int LOADK = 1, STOREK = 0;
	__device__ __forceinline__ const double2* row(const TileC&, int) const { return nullptr; }
	__device__ __forceinline__ bool decode(int bx, TileC& c) const {
		c.outer = fdiv(bx, dnt); c.t0 = (bx - c.outer*ntile)*T; c.nl = min(T, b - c.t0);
		c.comp = fdiv(c.outer, dnp); c.q0 = c.outer - c.comp*npair; return true; }
	__device__ __forceinline__ double2 load(const TileC& c, int li, int e) const {
		if (li >= c.nl) return make_double2(0, 0);
		const int x = b*e + c.t0 + li;
		const int bi = (int)fdiv(c.comp, m.dncb);
		const long o = bi*m.bstride + (c.comp - bi*m.ncb)*m.cstride + m.off0 + (2L*c.q0)*m.rstride + x*m.pstride;
		const double re = rd_real(m.ptr, m.dtype, o).x;
		const double im = (2*c.q0 + 1 < m.nring) ? rd_real(m.ptr, m.dtype, o + m.rstride).x : 0.0;
		return make_double2(re, im); }
	template<class AF> __device__ __forceinline__ double2 mid(const TileC&, int, int, AF&&) const { return make_double2(0, 0); }
	template<class VF> __device__ __forceinline__ void store(const TileC& c, int li, int e, VF&& val, double2 w) const {
		if (li >= c.nl) return;
		Y[((long)c.outer*fa.n + e)*ldY + c.t0 + li] = cmul(val(li, e), w); }
};

// MA2: b-point FFT over j2 for the lines k1 and a - k1 of T/2 ring pairs; bin k = k1 + a*k2 <= mmax is unpacked with its
// partner bin nphi - k (in the mirror line) into the spectra of the two rings and written as leg[m][2q], leg[m][2q+1]
struct StRingA2 : StageBase {
	static constexpr int SID = 6;
	static constexpr int PF = 512;      // (map2leg 21.1 -> 20.75 ms against 256)
	static constexpr bool TWO = false, INV_A = false, INV_B = false, LOAD_LINE_FAST = false, STORE_LINE_FAST = true, HAS_TW = false;
	static constexpr int MAXR = 8, MINW = 8;
	const double2* Y; long ldY; int a, X, npair, groups, nring, mmax; double2* leg; long ldleg; int nm; const double2* tab; double scale; FastDiv da, dgr;
	static constexpr int LOADK = 0, STOREK = 1;
	__device__ __forceinline__ const double2* row(const TileC& c, int li) const {
		int line, q; slot(c, li, line, q);
		return line >= 0 ? Y + (((long)c.comp*npair + q)*a + line)*ldY : nullptr; }
	__device__ __forceinline__ int mirror_line(int k) const { return k == 0 ? 0 : a - k; }
	__device__ __forceinline__ bool decode(int bx, TileC& c) const {
		c.outer = fdiv(bx, dnt); c.t0 = bx - c.outer*ntile; c.nl = T;
		c.comp = fdiv(c.outer, dgr); c.q0 = (c.outer - c.comp*groups)*(T/2);
		return mirror_line(c.t0) >= c.t0; }
	__device__ __forceinline__ void slot(const TileC& c, int li, int& line, int& q) const {
		q = c.q0 + (li >> 1);
		const int ml = mirror_line(c.t0);
		line = (li & 1) ? (ml != c.t0 ? ml : -1) : c.t0;
		if (q >= npair) line = -1;
	}
	__device__ __forceinline__ double2 load(const TileC& c, int li, int e) const {
		int line, q; slot(c, li, line, q);
		if (line < 0) return make_double2(0, 0);
		return Y[(((long)c.comp*npair + q)*a + line)*ldY + e]; }
	template<class AF> __device__ __forceinline__ double2 mid(const TileC&, int, int, AF&&) const { return make_double2(0, 0); }
	template<class VF> __device__ __forceinline__ void store(const TileC& c, int li, int e, VF&& val, double2) const {
		int line, q; slot(c, li, line, q);
		if (line < 0) return;
		const int k = line + a*e;
		if (k > mmax) return;
		const double2 zp = val(li, e);
		double2 zm;
		if (k == 0) zm = zp;
		else {
			const int kp = X - k, ml = mirror_line(line);
			const int lp = (ml == line) ? li : (li ^ 1);
			zm = val(lp, (int)fdiv((uint32_t)(kp - ml), da));
		}
		// X_a = (Z[k] + conj Z[n-k])/2, X_b = -i (Z[k] - conj Z[n-k])/2
		double2 xa = make_double2(0.5*(zp.x + zm.x), 0.5*(zp.y - zm.y));
		const double2 d = make_double2(zp.x - zm.x, zp.y + zm.y);
		double2 xb = make_double2(0.5*d.y, -0.5*d.x);
		const double2 t = tab ? tab[k] : make_double2(1, 0);
		double2* o = leg + ((long)c.comp*nm + k)*ldleg + 2*q;
		o[0] = cscale(cmul(xa, t), scale);
		if (2*q + 1 < nring) o[1] = cscale(cmul(xb, t), scale);
	}
};

// MS1: Hermitian pair load from h[comp][ring][m]: bin k = b*j1 + j2, line = j2, backward a-point transform over j1
struct StRingS1 : StageBase {
	static constexpr int SID = 7;
	static constexpr bool TWO = false, INV_A = true, INV_B = false, LOAD_LINE_FAST = true, STORE_LINE_FAST = true, HAS_TW = true;
	static constexpr int MAXR = 8, MINW = 8;
	const double2* h; long ldh, hcomp; int b, X, npair, nring, mmax; double2* Y; long ldY; FastDiv dnp;      // hcomp: rows of h per component
	static constexpr int LOADK = 1, STOREK = 0;
	__device__ __forceinline__ const double2* row(const TileC&, int) const { return nullptr; }
	__device__ __forceinline__ bool decode(int bx, TileC& c) const {
		c.outer = fdiv(bx, dnt); c.t0 = (bx - c.outer*ntile)*T; c.nl = min(T, b - c.t0);
		c.comp = fdiv(c.outer, dnp); c.q0 = c.outer - c.comp*npair; return true; }
	__device__ __forceinline__ double2 load(const TileC& c, int li, int e) const {
		if (li >= c.nl) return make_double2(0, 0);
		const int k = b*e + c.t0 + li;
		int m; bool cj;
		if (k <= mmax) { m = k; cj = false; }
		else if (X - k <= mmax) { m = X - k; cj = true; }
		else return make_double2(0, 0);
		const double2* r = h + ((long)c.comp*hcomp + 2*c.q0)*ldh + m;
		double2 ha = r[0];
		double2 hb = (2*c.q0 + 1 < nring) ? r[ldh] : make_double2(0, 0);
		if (m == 0) { ha.y = 0; hb.y = 0; }
		if (cj) { ha.y = -ha.y; hb.y = -hb.y; }
		return make_double2(ha.x - hb.y, ha.y + hb.x); }
	template<class AF> __device__ __forceinline__ double2 mid(const TileC&, int, int, AF&&) const { return make_double2(0, 0); }
	template<class VF> __device__ __forceinline__ void store(const TileC& c, int li, int e, VF&& val, double2 w) const {
		if (li >= c.nl) return;
		Y[((long)c.outer*fa.n + e)*ldY + c.t0 + li] = cmul(cconj(val(li, e)), cconj(w)); }
};

// MS2: backward b-point transform over j2 for the lines k1; pixel x = k1 + a*k2: real part -> ring 2q, imaginary part -> ring 2q+1
struct StRingS2 : StageBase {
	static constexpr int SID = 8;
	static constexpr bool TWO = false, INV_A = true, INV_B = false, LOAD_LINE_FAST = false, STORE_LINE_FAST = true, HAS_TW = false;
	static constexpr int MAXR = 8, MINW = 8;
	const double2* Y; long ldY; int a, npair; MapAddr m; FastDiv dnp;
	static constexpr int LOADK = 0, STOREK = 0;
	__device__ __forceinline__ const double2* row(const TileC& c, int li) const { return li < c.nl ? Y + ((long)c.outer*a + c.t0 + li)*ldY : nullptr; }
	__device__ __forceinline__ bool decode(int bx, TileC& c) const {
		c.outer = fdiv(bx, dnt); c.t0 = (bx - c.outer*ntile)*T; c.nl = min(T, a - c.t0);
		c.comp = fdiv(c.outer, dnp); c.q0 = c.outer - c.comp*npair; return true; }
	__device__ __forceinline__ double2 load(const TileC& c, int li, int e) const {
		if (li >= c.nl) return make_double2(0, 0);
		return Y[((long)c.outer*a + c.t0 + li)*ldY + e]; }
	template<class AF> __device__ __forceinline__ double2 mid(const TileC&, int, int, AF&&) const { return make_double2(0, 0); }
	template<class VF> __device__ __forceinline__ void store(const TileC& c, int li, int e, VF&& val, double2) const {
		if (li >= c.nl) return;
		const int x = c.t0 + li + a*e;
		const double2 v = val(li, e);                     // conj of the backward transform: the imaginary part flips sign
		const int bi = (int)fdiv(c.comp, m.dncb);
		const long o = bi*m.bstride + (c.comp - bi*m.ncb)*m.cstride + m.off0 + (2L*c.q0)*m.rstride + x*m.pstride;
		wr_real(m.ptr, m.dtype, o, v.x);
		if (2*c.q0 + 1 < m.nring) wr_real(m.ptr, m.dtype, o + m.rstride, -v.y);
	}
};

// last pass of a transform of the 2-D FFTs (FftChain::fft2_real / fft2_c2c), with the transpose: b-point transform over j2 for line k1
// of T consecutive outer lines kx (columns of the spectrum, or rows of the input); writes out[ky = k1 + a k2][kx] (kx fastest: runs of T
// points; row stride ldo) and, with herm (real input: kx runs over the half spectrum), for 0 < kx < nx - kx the Hermitian image
// out[(ny - ky) % ny][nx - kx] = conj
struct StColOut : StageBase {
	static constexpr int SID = 9;
	static constexpr bool R7 = false;
	static constexpr bool TWO = false, INV_A = false, INV_B = false, LOAD_LINE_FAST = false, STORE_LINE_FAST = true, HAS_TW = false;
	static constexpr int MAXR = 9, MINW = 1;
	const double2* Y; long ldY; int a, nm, ny, nx, groups, conj_out, herm; double2* out; long ldo, ocomp; double scale; FastDiv dgr;
	static constexpr int LOADK = 0, STOREK = 0;
	__device__ __forceinline__ const double2* row(const TileC& c, int li) const { return c.q0 + li < nm ? Y + (((long)c.comp*nm + c.q0 + li)*a + c.t0)*ldY : nullptr; }
	__device__ __forceinline__ bool decode(int bx, TileC& c) const {
		c.outer = fdiv(bx, dnt); c.t0 = bx - c.outer*ntile; c.nl = T;
		c.comp = fdiv(c.outer, dgr); c.q0 = (c.outer - c.comp*groups)*T; return true; }
	__device__ __forceinline__ double2 load(const TileC& c, int li, int e) const {
		const int kx = c.q0 + li;
		if (kx >= nm) return make_double2(0, 0);
		return Y[(((long)c.comp*nm + kx)*a + c.t0)*ldY + e]; }
	template<class AF> __device__ __forceinline__ double2 mid(const TileC&, int, int, AF&&) const { return make_double2(0, 0); }
	template<class VF> __device__ __forceinline__ void store(const TileC& c, int li, int e, VF&& val, double2) const {
		const int kx = c.q0 + li;
		if (kx >= nm) return;
		const int ky = c.t0 + a*e;
		double2 v = cscale(val(li, e), scale);
		double2* oc = out + (long)c.comp*ocomp;
		// (backward transform = conjugate of the forward one of the conjugated input)
		oc[(long)ky*ldo + kx] = conj_out ? cconj(v) : v;
		if (herm && kx > 0 && 2*kx < nx) oc[(long)(ky == 0 ? 0 : ny - ky)*ldo + (nx - kx)] = conj_out ? v : cconj(v);
	}
};

// ---------------------------------------------------------------------------------------------------------------
// The same kernel with its transforms planned at compile time (fft_static_dev.hpp): na, nb, T, the radix sequences and the digit
// reversal are constants, every index split divides by a constant, every loop has a constant trip count.  The stage functors (load,
// mid, store, decode, row, pfaddr), the tables (W_n, tws, btw), the prefetch-ahead and the shared W_n of two equal lengths are
// those of chain_kernel; partial tiles (c.nl < T) stay a run-time condition inside the functors.  Launched for the stage shapes of
// STATIC_TABLE below; chain_kernel serves every other shape.
template<class S, class FA, class FB, int T, int NT> __global__ PXS_CH_BOUNDS void chain_kernel_static(const S s)
{
	PXS_SHARED(double2, lds);
	constexpr int na = FA::n, nb = FB::n;
	static_assert(S::TWO == (nb > 0), "chain_kernel_static: second transform");
	constexpr int nlast = S::TWO ? nb : na, nslast = S::TWO ? FB::ns : FA::ns;
	constexpr bool same_tw = S::TWO && nb == na;
	constexpr int LA = (T*na + NT - 1)/NT, LB = (T*nb + NT - 1)/NT, LS = (T*nlast + NT - 1)/NT;
	static_assert(LA*NT <= SDIV_MAX && LB*NT <= SDIV_MAX && LS*NT <= SDIV_MAX, "chain_kernel_static: index range of sdiv");
	double2* twa = lds; double2* twb = same_tw ? lds : lds + na; double2* twx = lds + na + (same_tw ? 0 : nb); double2* buf = twx + (S::HAS_TW ? nlast : 0);
	TileC c;
	if (!s.decode((int)blockIdx.x, c)) return;
	const bool have_tw = S::HAS_TW && s.btw != nullptr;
	int pf_val = 0;
	{	// ---- load: every global load of the tile is in flight before the first LDS write
		double2 v[LA]; int pos[LA];
#pragma unroll
		for (int u = 0; u < LA; u++) {
			const uint32_t idx = threadIdx.x + u*NT; pos[u] = -1;
			if ((T*na) % NT == 0 || idx < (uint32_t)(T*na)) {
				uint32_t li, e;
				if (S::LOAD_LINE_FAST) { e = sdiv<T>(idx); li = idx - e*T; }
				else { li = sdiv<na>(idx); e = idx - li*na; }
				v[u] = s.load(c, (int)li, (int)e);
				if (S::INV_A) v[u].y = -v[u].y;
				pos[u] = (int)(li*FA::ns + FA::perm(e));
			}
		}
		if ((S::LOADK == 0 || S::PFI > 0) && s.pf > 0 && (long)blockIdx.x + s.pf < (long)gridDim.x) {
			TileC c2;
			if (s.decode((int)blockIdx.x + s.pf, c2)) {
				if (S::LOADK == 0) {
					constexpr int per = (na*16 + 127) >> 7; const uint32_t i = threadIdx.x;
					if (i < (uint32_t)(T*per)) {
						const uint32_t li = sdiv<per>(i), seg = i - li*per;
						const double2* r = s.row(c2, (int)li);
						if (r) pf_val = *reinterpret_cast<const int*>(reinterpret_cast<const char*>(r) + seg*128);
					}
				} else {
#pragma unroll
					for (int it = 0; it < S::PFI; it++) {
						const void* q = s.pfaddr(c2, (int)threadIdx.x + it*NT);
						if (q) pf_val += *reinterpret_cast<const int*>(q);
					}
				}
			}
		}
#pragma unroll
		for (int k0 = 0; k0 < na; k0 += NT) { const int k = k0 + (int)threadIdx.x; if (k < na) twa[k] = s.fa.tw[k]; }
		if constexpr (S::TWO && !same_tw) {
#pragma unroll
			for (int k0 = 0; k0 < nb; k0 += NT) { const int k = k0 + (int)threadIdx.x; if (k < nb) twb[k] = s.fb.tw[k]; }
		}
		if (have_tw) {
#pragma unroll
			for (int k0 = 0; k0 < nlast; k0 += NT) { const int k = k0 + (int)threadIdx.x; if (k < nlast) twx[k] = s.btw[(long)c.t0*k]; }
		}
#pragma unroll
		for (int u = 0; u < LA; u++) if (pos[u] >= 0) buf[pos[u]] = v[u];
	}
	PXS_LDS_BARRIER();
	lds_fft_static<FA, NT, T>(buf, twa);
	if constexpr (S::TWO) {	// ---- second transform on the same lines
		double2 v[LB]; int pos[LB];
#pragma unroll
		for (int u = 0; u < LB; u++) {
			const uint32_t idx = threadIdx.x + u*NT; pos[u] = -1;
			if ((T*nb) % NT == 0 || idx < (uint32_t)(T*nb)) {
				const uint32_t e = sdiv<T>(idx), li = idx - e*T;
				{ const double2* Al = buf + li*FA::ns; v[u] = s.mid(c, (int)li, (int)e, [&](int k) { return Al[k]; }); }
				if (S::INV_B) v[u].y = -v[u].y;
				pos[u] = (int)(li*FB::ns + FB::perm(e));
			}
		}
		PXS_LDS_BARRIER();
#pragma unroll
		for (int u = 0; u < LB; u++) if (pos[u] >= 0) buf[pos[u]] = v[u];
		PXS_LDS_BARRIER();
		lds_fft_static<FB, NT, T>(buf, twb);
	}
	{	// ---- store
#pragma unroll
		for (int u = 0; u < LS; u++) {
			const uint32_t idx = threadIdx.x + u*NT;
			if ((T*nlast) % NT == 0 || idx < (uint32_t)(T*nlast)) {
				uint32_t li, e;
				if (S::STORE_LINE_FAST) { e = sdiv<T>(idx); li = idx - e*T; } else { li = sdiv<nlast>(idx); e = idx - li*nlast; }
				double2 w = make_double2(1, 0);
				if (have_tw) w = cmul(twx[e], s.tws[S::STORE_LINE_FAST ? idx : e*T + li]);
				s.store(c, (int)li, (int)e, [&](int l2, int e2) { return buf[l2*nslast + e2]; }, w);
			}
		}
	}
#ifndef PXS_HOST_SIM
	if (S::LOADK == 0 || S::PFI > 0) asm volatile("" :: "v"(pf_val));
#endif
}

// ---- the compiled table ---------------------------------------------------------------------------------------------------------
// One StaticFft per length and radix set (F<n>: the theta stages and the 2-D FFT stages, radices up to 9; G<n>: the ring stages,
// radices up to 8), one PXS_CS line per stage shape (stage, first transform, second transform or NoFft, lines per tile).
// To add a shape: run the workload with PXS_CHAIN_VERBOSE=1, which prints every stage shape it launches ("chain stage <sid>:
// na= nb= T= ... static 0|1") and the radices FftContext::sub plans for its lengths; add the StaticFft if the length is new,
// with exactly those radices in that order (static_check refuses anything else), then the PXS_CS line; check the kernel's
// registers against its stage's budget (tools/kres.py: ring stages <= 64 VGPRs, no scratch anywhere) and leave it out if it
// does not fit.
struct StaticEntry {
	int sid, na, nb, T, maxr; std::vector<int> ra, rb; std::vector<int> pa, pb;
	void (*launch)(const void* s, long nblk, size_t sh, hipStream_t st);
};
template<class S, class FA, class FB, int T> static void launch_static(const void* sp, long nblk, size_t sh, hipStream_t st) {
	const S& s = *static_cast<const S*>(sp);
#ifndef PXS_HOST_SIM
	static const bool once = [] { (void)hipFuncSetAttribute((const void*)chain_kernel_static<S, FA, FB, T, S::NT>, hipFuncAttributeMaxDynamicSharedMemorySize, 160*1024 - 256); return true; }();
	(void)once;
#endif
	hipLaunchKernelGGL((chain_kernel_static<S, FA, FB, T, S::NT>), dim3((unsigned)nblk), dim3(S::NT), sh, st, s);
}
template<class F> static std::vector<int> radices_of() { std::vector<int> r; for (int p = 0; p < F::nfac; p++) r.push_back(F::radix(p)); return r; }
template<class F> static std::vector<int> perm_of() { std::vector<int> r; for (int j = 0; j < F::n; j++) r.push_back(F::perm_host(j)); return r; }
template<class S, class FA, class FB, int T> static StaticEntry static_entry() {
	static_assert((long)T*(FA::n > FB::n ? FA::n : FB::n) <= S::PTS, "static chain stage: tile too large");
	return StaticEntry{S::SID, FA::n, FB::n, T, S::MAXR, radices_of<FA>(), radices_of<FB>(), perm_of<FA>(), perm_of<FB>(), &launch_static<S, FA, FB, T>};
}
#define PXS_CS(S, FA, FB, T) static_entry<S, FA, FB, T>(),
#include "chain_static_table.hpp"
#undef PXS_CS
static const StaticEntry* static_find(int sid, int na, int nb, int T) {
	for (const StaticEntry& e : static_table()) if (e.sid == sid && e.na == na && e.nb == nb && e.T == T) return &e;
	return nullptr;
}
// PXS_CHAIN_STATIC=0 keeps the run-time kernel for every shape (read per call: the tests compare the two paths on one plan)
static bool static_enabled() { const char* e = getenv("PXS_CHAIN_STATIC"); return e ? atoi(e) != 0 : true; }

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
static bool smooth235(long n) { if (n < 1) return false; for (int p : {2, 3, 5}) while (n % p == 0) n /= p; return n == 1; }
bool FftChain::sub_ok(long n) { return n >= 2 && n <= CH_NMAX && smooth235(n); }

static LdsFft mk(FftContext* fc, long n, int maxr = 9) {
	LdsFft f; memset(&f, 0, sizeof(f));
	if (n <= 0) return f;
	auto v = fc->view(n, maxr);
#ifdef PXS_LAB
	static const int nofft = [] { const char* e = getenv("PXS_CH_NOFFT"); return e ? atoi(e) : 0; }();     // lab builds only: timing experiments (wrong results)
#else
	constexpr int nofft = 0;
#endif
	if (getenv("PXS_CHAIN_VERBOSE")) {
		static std::mutex mu; static std::set<std::pair<long, int>> seen; std::lock_guard<std::mutex> g(mu);
		if (seen.insert(std::make_pair(n, maxr)).second) {
			std::string r; for (int p = 0; p < v.nfac; p++) r += " " + std::to_string(v.hfac[p]);
			fprintf(stderr, "[pxsht] chain fft n=%ld maxr=%d: radices%s\n", n, maxr, r.c_str());
		}
	}
	f.n = v.n; f.nfac = nofft ? 0 : v.nfac; f.ns = v.ns; f.generic = v.generic; f.pass = (const PassDesc*)v.pass; f.perm = v.perm; f.tw = v.tw; f.dn = make_fastdiv((uint32_t)n);
	return f;
}

// W_X^{li e}, e < n, li < T, laid out [e][li] (see StageBase)
const double2* FftChain::small_tw(long X, int n, int T) {
#ifdef PXS_LAB
	{ static const int notw = [] { const char* e = getenv("PXS_CH_NOTW"); return e ? atoi(e) : 0; }(); if (notw) return nullptr; }     // lab builds only: timing experiments (wrong results)
#endif
	std::lock_guard<std::mutex> g(mu_);
	auto key = std::make_tuple(X, n, T);
	auto it = stw_.find(key);
	if (it != stw_.end()) return it->second.as<double2>();
	std::vector<double2> t((size_t)n*T);
	const long double tp = 6.283185307179586476925286766559L;
	for (int e = 0; e < n; e++) for (int li = 0; li < T; li++) {
		const long double ang = tp*(long double)(((long)li*e) % X)/(long double)X;
		t[(size_t)e*T + li] = make_double2((double)cosl(ang), (double)(-sinl(ang)));
	}
	stw_[key] = upload(t);
	return stw_[key].as<double2>();
}

// lines per tile: as many as fit CH_TILE_PTS, in multiples of `mult`
// (Tried for the ring stages, which run at <= 64 VGPRs: tiles shrunk until tile + tables fit 39.5 KiB of LDS, four workgroups per CU.
// Measured at C3 / C4 / C2: ring FFT stages 47.4 / 60.6 / 2.85 ms against 46.4 / 60.8 / 2.83 ms with the full 2560-point tiles.  Removed.)
static int tile_lines(long n_a, long n_b, long nlines, int mult) {
	const long n = std::max(n_a, n_b);
	long T = CH_TILE_PTS / n;
	if (T >= mult) T -= T % mult;
	if (T < 1) T = 1;
	const long cap = ((nlines + mult - 1)/mult)*mult;
	if (T > cap) T = cap;
	return (int)T;
}
// tiles of T consecutive lines; X > 0: the stage applies the four-step twiddle of a length-X transform to its output
template<class S> void FftChain::set_tiles(S& s, int T, long nlines, long X) {
	s.T = T; s.ntile = (int)((nlines + T - 1)/T); s.dT = make_fastdiv((uint32_t)T); s.dnt = make_fastdiv((uint32_t)s.ntile);
	s.dna = make_fastdiv((uint32_t)s.fa.n); s.dnb = make_fastdiv((uint32_t)std::max(1, s.fb.n));
	s.btw = nullptr; s.tws = nullptr;
	if (X > 0) { s.tws = small_tw(X, S::TWO ? s.fb.n : s.fa.n, T); s.btw = s.tws ? fc_->twiddle_table(X) : nullptr; }
}
// the static instance of a stage as planned, or null: its shape is not in the table, or the plan has no passes (PXS_CH_NOFFT, lab builds)
template<class S> static const StaticEntry* static_for(const S& s) {
	const StaticEntry* e = static_find(S::SID, s.fa.n, s.fb.n, s.T);
	if (!e || s.fa.nfac != (int)e->ra.size() || (S::TWO && s.fb.nfac != (int)e->rb.size())) return nullptr;
	return e;
}
template<class S> static void launch_stage(const S& s, long nblk, hipStream_t st, std::vector<ChainShape>* dry) {
	if (nblk <= 0) return;
	const StaticEntry* se = static_for(s);
	if (dry) { dry->push_back(ChainShape{S::SID, s.fa.n, s.fb.n, s.T, se != nullptr}); return; }
	if (!static_enabled()) se = nullptr;
	PXS_REQUIRE((long)s.T*std::max(s.fa.n, s.fb.n) <= S::PTS, "internal: chain tile too large");
	PXS_REQUIRE(nblk < (1L << 31), "internal: chain grid too large");
	size_t sh = sizeof(double2)*((size_t)s.fa.n + (S::TWO && s.fb.n == s.fa.n ? 0 : s.fb.n) + (S::HAS_TW ? std::max(s.fa.n, s.fb.n) : 0) + (size_t)s.T*std::max(s.fa.ns, s.fb.ns) + 2);
	{ static const size_t pad = [] { const char* e = lab_getenv("PXS_CH_LDS_PAD"); return e ? (size_t)atol(e) : (size_t)0; }(); sh += pad; }   // occupancy experiments
	{ static const int pf = [] {      // PXS_CH_PF: every stage; PXS_CH_PF_SID<k>: the stage with S::SID = k
		const std::string name = "PXS_CH_PF_SID" + std::to_string(S::SID);
		const char* e1 = lab_getenv(name.c_str()); const char* e = lab_getenv("PXS_CH_PF");
		return e1 ? atoi(e1) : (e ? atoi(e) : S::PF); }(); const_cast<S&>(s).pf = pf; }
	if (getenv("PXS_CHAIN_VERBOSE")) {
		static std::mutex mu; static std::set<std::tuple<int, int, int, int>> seen; std::lock_guard<std::mutex> g(mu);
		if (seen.insert(std::make_tuple(S::SID, s.fa.n, s.fb.n, s.T)).second)
			fprintf(stderr, "[pxsht] chain stage %d: na=%d nb=%d T=%d LDS %.1f KiB -> %d WG/CU by LDS, %ld workgroups, static %d\n", S::SID, s.fa.n, s.fb.n, s.T, sh/1024.0, (int)((160*1024)/sh), nblk, se ? 1 : 0);
	}
	if (se) { se->launch(&s, nblk, sh, st); return; }
#ifndef PXS_HOST_SIM
	static const bool once = [] { (void)hipFuncSetAttribute((const void*)chain_kernel<S, S::NT, (S::PTS + S::NT - 1)/S::NT>, hipFuncAttributeMaxDynamicSharedMemorySize, 160*1024 - 256); return true; }();
	(void)once;
#endif
	hipLaunchKernelGGL((chain_kernel<S, S::NT, (S::PTS + S::NT - 1)/S::NT>), dim3((unsigned)nblk), dim3(S::NT), sh, st, s);
}

// lines per tile of a stage
template<class S> int FftChain::tile_lines_for(long n_a, long n_b, long nlines, int mult) {
	int T = tile_lines(n_a, n_b, nlines, mult);
	// a stage with a larger cap takes it only to reach `mult` lines (whole 128-byte lines on its strided side)
	if (S::PTS > CH_TILE_PTS && T < mult && (long)mult*std::max(n_a, n_b) <= S::PTS && nlines >= mult) T = mult;
	return T;
}
template<class S> void FftChain::launch_any(S& s, long nblk, hipStream_t st) {
	if (!dry_) static_check(S::MAXR);
	launch_stage(s, nblk, st, dry_);
}

// every table entry against the run-time plans of its lengths (once per radix set of a chain): radices, order and digit reversal
// must be those of FftContext::sub, whose W_n tables the static kernels read.  Returns the number of entries.
int FftChain::static_check(int maxr) {
	std::lock_guard<std::mutex> g(mu_);
	if (maxr > 0 && checked_.count(maxr)) return (int)static_table().size();
	for (const StaticEntry& e : static_table()) {
		if (maxr > 0 && e.maxr != maxr) continue;
		for (int which = 0; which < 2; which++) {
			const int n = which ? e.nb : e.na; if (n <= 0) continue;
			const std::vector<int>& r = which ? e.rb : e.ra; const std::vector<int>& pm = which ? e.pb : e.pa;
			const auto v = fc_->view(n, e.maxr);
			bool ok = !v.generic && v.nfac == (int)r.size() && v.ns == (n | 1);
			for (int p = 0; ok && p < v.nfac; p++) ok = v.hfac[p] == r[p];
			for (int j = 0; ok && j < n; j++) ok = v.hperm[j] == pm[j];
			PXS_REQUIRE(ok, "static chain table: the plan compiled for length " + std::to_string(n) + " (stage " + std::to_string(e.sid) + ") is not the one the FFT engine plans");
		}
	}
	if (maxr > 0) checked_.insert(maxr);
	return (int)static_table().size();
}
// is (stage id, na, nb, T) in the compiled table
bool FftChain::static_has(int sid, int na, int nb, int T) { return static_find(sid, na, nb, T) != nullptr; }
void FftChain::static_shapes(std::vector<ChainShape>& out) { for (const StaticEntry& e : static_table()) out.push_back(ChainShape{e.sid, e.na, e.nb, e.T, true}); }

// balanced split n = a*b with both factors usable
static bool split_balanced(long n, Split& s, long amax = 320) {
	long best = 0; double bestc = 1e300;
	for (long a = 2; a <= 1024 && a <= n/2; a++) if (n % a == 0) {
		const long b = n/a;
		if (!FftChain::sub_ok(a) || !FftChain::sub_ok(b)) continue;
		double c = std::fabs(std::log((double)a/(double)b));
		if (a > amax) c += 10;
		if (b % 8) c += 0.3;
		if (c < bestc) { bestc = c; best = a; }
	}
	if (!best) return false;
	s.a = best; s.b = n/best; return true;
}

bool FftChain::plan_rings(long nphi) {
	nphi_ = nphi; ra_ = Split(); rs_ = Split();
	Split s;
	if (!split_balanced(nphi, s)) return false;
	// analysis: pass 1 tiles are 16 lines (128-byte runs of f64) x a points -> the smaller factor first;
	// synthesis: pass 2 tiles are 16 lines x b points -> the smaller factor last
	ra_.a = std::min(s.a, s.b); ra_.b = nphi/ra_.a;
	rs_.b = std::min(s.a, s.b); rs_.a = nphi/rs_.b;
	// The map side of the ring stages moves 8-byte reals in runs of T lines.  Synthesis (MS2 WRITES the map: a partial 128-byte
	// line is a read-modify-write): the first factor a a multiple of 16 and T a multiple of 16 (b <= 160) make every run whole,
	// aligned lines; the largest such a <= 320 (8 lines of a points still fill a tile in MS1).  Analysis (MA1 reads the map): b the
	// largest multiple of 16 up to 256.  Measured with tools/chain_lab.py (ms, h2map / map2leg of one component): C3 43200 =
	// 240 x 180 -> 320 x 135: 8.13 -> 7.04 (288 x 150: 7.48, 400 x 108: 7.33); C4 10800 = 120 x 90 -> 240 x 45: 3.88 -> 3.45 per 8
	// maps (80 x 135: 3.52, 144 x 75: 3.56); analysis 90 x 120 -> 45 x 240: 3.78 -> 3.45 (C3 stays 180 x 240; 150 x 288: 7.77 vs 7.54).
	for (long a = 320; a >= 16; a -= 16) if (nphi % a == 0 && nphi/a <= 160 && nphi/a >= 2 && sub_ok(a) && sub_ok(nphi/a)) { rs_.a = a; rs_.b = nphi/a; break; }
	for (long b = 256; b >= 16; b -= 16) if (nphi % b == 0 && nphi/b >= 2 && nphi/b <= 320 && sub_ok(b) && sub_ok(nphi/b)) { ra_.b = b; ra_.a = nphi/b; break; }
	{	// experiments: force the first factor of the analysis / synthesis split
		const char* ea = lab_getenv("PXS_RING_A_ANA"); const char* es = lab_getenv("PXS_RING_A_SYN");
		if (ea && atol(ea) > 1 && nphi % atol(ea) == 0 && sub_ok(atol(ea)) && sub_ok(nphi/atol(ea))) { ra_.a = atol(ea); ra_.b = nphi/ra_.a; }
		if (es && atol(es) > 1 && nphi % atol(es) == 0 && sub_ok(atol(es)) && sub_ok(nphi/atol(es))) { rs_.a = atol(es); rs_.b = nphi/rs_.a; }
	}
	return true;
}

static long smooth_at_least(long n, bool even_product_with = false, long g = 1) {
	for (long m = std::max<long>(n, 2);; m++) if (smooth235(m) && (!even_product_with || ((m*g) % 2 == 0))) return m;
}

// lengths the theta stages (StFirst, StResize, StSigma, StSplit: lds_fft with MAXR = 9) transform: radix 7 next to 2, 3, 5
static bool smooth2357(long n) { if (n < 1) return false; for (int p : {2, 3, 5, 7}) while (n % p == 0) n /= p; return n == 1; }
static bool sub_ok7(long n) { return n >= 2 && n <= CH_NMAX && smooth2357(n); }
// ducc0's good_size_complex: the smallest 2^a 3^b 5^c 7^d 11^e >= n.  Its analysis_2d / synthesis_2d run the Legendre stage on a CC grid of
// good_size_complex(lmax + 1) + 1 rings, i.e. a circle of N_cc = 2 good_size_complex(lmax + 1) points.
bool FftChain::sub_ok_theta(long n) { return sub_ok7(n); }
long FftChain::ducc_ncc(int lmax) {
	for (long n = std::max<long>(lmax + 1, 1);; n++) { long r = n; for (int p : {2, 3, 5, 7, 11}) while (r % p == 0) r /= p; if (r == 1) return 2*n; }
}

// How full the tiles of a stage with lines of n points are (tiles hold a multiple of 8 lines, at most CH_TILE_PTS points); lines too long
// for 8 of them (strided side in runs below 128 bytes) count as a quarter less.  Sweeps of the shared moduli with tools/gpu_sweep.sh
// (profiles/r04b_theta_modulus_sweep.txt) follow sum(points of a stage / fill) to ~5 %: C3 analysis 29.8 ms (g = 160, 144, 288, 320) against
// 34-40 (g = 180, 192, 240: half-empty tiles; 480: five-line tiles), C5 3.6-3.75 (72, 96, 288) against 3.9-4.0 (108, 144, 216, 432).
static double tile_fill(long n) {
	long T = CH_TILE_PTS / n; if (T >= 8) T -= T % 8; if (T < 1) T = 1;
	return (double)(T*n)/(double)CH_TILE_PTS*(T >= 8 ? 1.0 : 0.8);
}
// among moduli whose tiles fill alike: 64 ... 160 (16 or more lines per tile in the g-point stages) before larger or much smaller ones
static double modulus_pref(long g) { return 1.0 + 0.02*std::max(0.0, std::log2((double)g/160.0)) + 0.04*std::max(0.0, std::log2(64.0/(double)g)); }
ThetaPlan FftChain::plan_theta(long N, int lmax) {
	ThetaPlan best; double bestc = 1e300;
	static const long gforce = [] { const char* e = lab_getenv("PXS_THETA_G"); return e ? atol(e) : 0L; }();     // experiments: force the shared modulus
	const long Nd = ducc_ncc(lmax);
	auto consider = [&](long g, long ac) {
		ThetaPlan t; t.N = N; t.g = g; t.bN = N/g; t.ac = ac; t.Ncc = g*ac;
		t.g2 = smooth_at_least((N + 2L*lmax + 2 + g - 1)/g); t.M = g*t.g2;
		if ((t.Ncc & 1) || !sub_ok(t.g2) || !sub_ok7(t.ac)) return;
		// synthesis split: gs divides both Ncc and N; RS1 and RS3 run gs-point lines, RS2 lines of max(bs, aNs) points
		long gs_best = 0; double gsc = 1e300;
		static const long gsforce = [] { const char* e = lab_getenv("PXS_THETA_GS"); return e ? atol(e) : 0L; }();     // experiments: force the modulus of the synthesis chain
		for (long gs = 2; gs <= 1024; gs++) if (t.Ncc % gs == 0 && N % gs == 0 && sub_ok7(gs) && sub_ok7(t.Ncc/gs) && sub_ok7(N/gs) && (!gsforce || gs == gsforce)) {
			const double c = ((2.0*t.Ncc + 1.5*N)/tile_fill(gs) + (double)(t.Ncc + N)/tile_fill(std::max(t.Ncc/gs, N/gs)))*modulus_pref(gs);
			if (c < gsc) { gsc = c; gs_best = gs; }
		}
		if (!gs_best) return;
		t.gs = gs_best; t.bs = t.Ncc/gs_best; t.aNs = N/gs_best;
		// cost: a CC ring costs far more (Legendre stage) than a point of FFT traffic; then the points the stages of the default analysis
		// (the fine-CC form: middle circle of 2 N_cc points) and of the synthesis move, each over the fill of its tiles, with a slight
		// preference among equals for moduli of 64 ... 160 (modulus_pref).
		// ducc0's own N_cc wins whenever some g realises it: the fine-CC form of the analysis then cuts the theta spectrum of a map
		// that is not band-limited where ducc0 does (sht.hip, ana_form), and it is the smallest size ducc0 considers good.
		const double lmin = 2.0*lmax + 2, M2 = 2.0*t.Ncc;
		const double ana = (2.0*N + 2.0*M2 + 1.5*t.Ncc)/tile_fill(g) + (N + M2)/tile_fill(std::max(t.bN, 2*t.ac)) + (M2 + t.Ncc)/tile_fill(2*t.ac);
		double c = 60.0*(t.Ncc - lmin)/lmin + (ana*modulus_pref(g) + gsc)/(3.0*N + 4.0*M2 + 2.5*t.Ncc + 3.0*t.Ncc + 2.5*N);
		if (t.Ncc == Nd) c -= 1000.0;
		if (c < bestc) { bestc = c; best = t; best.ok = true; }
	};
	for (long g = 2; g <= 1024 && g <= N/2; g++) if (N % g == 0 && sub_ok7(g) && sub_ok7(N/g) && (!gforce || g == gforce)) {
		consider(g, smooth_at_least((2L*lmax + 2 + g - 1)/g, true, g));
		if (Nd % g == 0) consider(g, Nd/g);
	}
	return best;
}


// ring pairs per pass of the ring-FFT stages: PXS_RING_CHUNK_MB > 0 bounds the intermediate of a pass (experiment: keeping it in
// the 256 MB memory-side cache between the two kernels of a pass); 0 = all pairs at once.  Measured at C3 (ring FFT ms per round
// trip): all at once 47.3, 2048 MB 46.7, 512 MB 47.6, 200 MB 50.9, 128 MB 49.3, 64 MB 55.4 -- the cache does not pay for the
// shorter launches.
static long ring_chunk(long npair, long bytes_per_pair, int mult) {
	size_t budget = 0; env_budget("PXS_RING_CHUNK_MB", 20, budget);      // (per call)
	if (budget == 0) return npair;
	long q = std::max<long>(mult, ((long)budget/std::max<long>(bytes_per_pair, 1))/mult*mult);
	return std::min(q, npair);
}

// ---- one builder per stage kind -------------------------------------------------------------------------------------------------
// A builder takes what varies between the calls of its stage and owns the rest: the zeroed stage and its transforms (new_stage), the
// lines per tile (tile_lines_for; pair_lines where a tile holds pairs of lines), set_tiles, the FastDivs of its own arguments, and
// where the intermediates live: a chain ping-pongs between s1_ and s2_, and a row of n points has the leading dimension pad8(n).
template<class S> S FftChain::new_stage(long na, long nb) {
	S s; memset(&s, 0, sizeof(s));
	s.fa = mk(fc_, na, S::MAXR); s.fb = mk(fc_, nb, S::MAXR);
	return s;
}
template<class S> int FftChain::pair_lines(long n, long nlines) { int T = tile_lines_for<S>(n, 0, nlines, 8); if (T < 2) T = 2; return T - T % 2; }

// columns (m, m+1) of leg[comp][m][ring] packed by parity and mirror-extended to the circle of N points (w: optional weight per ring)
static PairSrc pair_src(const double2* leg, long ld, int nr, long N, int mir_c, int spin, int nm, const double2* w) {
	PairSrc p; memset(&p, 0, sizeof(p));
	p.leg = leg; p.cstride = (long)nm*ld; p.ld = ld; p.nr = nr; p.N = (int)N; p.mir_c = mir_c; p.a_odd = spin & 1; p.ncol = nm; p.w = w;
	return p;
}
// `nlines` plain lines of n points per component (the 2-D FFTs)
static PairSrc plain_src(const double2* src, long nlines, long ld, long n, int conj) {
	PairSrc p; memset(&p, 0, sizeof(p));
	p.leg = src; p.cstride = nlines*ld; p.ld = ld; p.nr = (int)n; p.N = (int)n; p.ncol = (int)nlines; p.plain = 1; p.conj = conj;
	return p;
}
// StFirst / StFirst2D: pass 1 of the a*b-point transform of `npair` lines per component: src -> s1_[outer][k1 < a][j2 < b]
template<class S> void FftChain::run_first(hipStream_t st, const PairSrc& src, long ncomp, long npair, long a, long b) {
	S s = new_stage<S>(a, 0);
	s.src = src; s.b = (int)b; s.Y = s1_.as<double2>(); s.ldY = pad8(b); s.npair = (int)npair; s.dnp = make_fastdiv((uint32_t)npair);
	set_tiles(s, tile_lines_for<S>(a, 0, b, 8), b, a*b);
	launch_any(s, ncomp*npair*s.ntile, st);
}
// StResize: pass 2 of the forward transform of X1 = g*fa points, resize, pass 1 of the backward one of X2 = g*fb points:
// s1_[outer][k1 < g][j2 < fa] -> s2_[outer][k1' < fb][k1 < g]
void FftChain::run_resize(hipStream_t st, long nouter, long fa, long fb, long g, int kmax, int nyq, int adj, const double2* ph) {
	StResize s = new_stage<StResize>(fa, fb);
	s.Y = s1_.as<double2>(); s.ldY = pad8(fa); s.Z = s2_.as<double2>(); s.ldZ = pad8(g);
	s.g = (int)g; s.X1 = (int)(g*fa); s.X2 = (int)(g*fb); s.kmax = kmax; s.nyq = nyq; s.adj = adj; s.ph = ph; s.dg = make_fastdiv((uint32_t)g);
	set_tiles(s, tile_lines_for<StResize>(fa, fb, g, 8), g, g*fb);
	launch_any(s, nouter*s.ntile, st);
}
// StSigma: s2_[outer][k1' < g2][r < g] -> s1_[outer][k1'' < g][k1' < g2] on the fine circle of M = g*g2 points
void FftChain::run_sigma(hipStream_t st, long nouter, long g, long g2, const double2* sigma) {
	StSigma s = new_stage<StSigma>(g, g);
	s.Z = s2_.as<double2>(); s.ldZ = pad8(g); s.V = s1_.as<double2>(); s.ldV = pad8(g2); s.g = (int)g; s.g2 = (int)g2; s.sigma = sigma;
	set_tiles(s, tile_lines_for<StSigma>(g, g, g2, 8), g2, g*g2);
	launch_any(s, nouter*s.ntile, st);
}
// StSplit<MODE>: last pass of the backward transform of X = a*g points from s2_[comp][pair][k1 < a][r < g], the pair apart, rings t < nr_out:
// MODE 0 -> out[comp][col][t] * w[t]; MODE 1 -> out[comp][t][col] * conj(tab[col]) * w[t] * scale.  ocstride: elements of out per component
template<int MODE> void FftChain::run_split(hipStream_t st, long ncomp, long npair, int nm, int spin, long a, long g, int mir_c, int nr_out,
                                            double2* out, long ld, long ocstride, const double2* w, const double2* tab, double scale, int self_half) {
	using S = StSplit<MODE>;
	S s = new_stage<S>(g, 0);
	const int T = pair_lines<S>(g, MODE == 0 ? 2*a : 2*npair), TH = T/2;
	// MODE 0: tiles of TH primary lines (of a/2 + 1) and their mirror lines; MODE 1: one tile per line and group of TH pairs (ntile = a)
	set_tiles(s, T, MODE == 0 ? (long)((a/2 + 1 + TH - 1)/TH)*T : a*T, 0);
	s.TH = MODE == 0 ? TH : 0; s.groups = MODE == 0 ? 1 : (int)((npair + TH - 1)/TH);
	s.U = s2_.as<double2>(); s.ldU = pad8(g); s.a = (int)a; s.g = (int)g; s.X = (int)(a*g); s.mir_c = mir_c; s.nr_out = nr_out; s.a_odd = spin & 1; s.ncol = nm; s.npair = (int)npair;
	s.out = out; s.ocstride = ocstride; s.ld = ld; s.w = w; s.tab = tab; s.scale = scale; s.self_half = self_half;
	s.da = make_fastdiv((uint32_t)a); s.dnp = make_fastdiv((uint32_t)npair); s.dgr = make_fastdiv((uint32_t)s.groups);
	launch_any(s, ncomp*(MODE == 0 ? npair : (long)s.groups)*s.ntile, st);
}
// StColOut: last pass of the a*b-point transform of `nlines` lines per component from s1_, transposed into out[k][line] (row stride ldo,
// ocomp elements per component); herm_nx > 0: the lines are the half spectrum of herm_nx real points, write the Hermitian image too
void FftChain::run_colout(hipStream_t st, long npre, long nlines, long a, long b, double2* out, long ldo, long ocomp, int conj, double scale, long herm_ny, long herm_nx) {
	StColOut s = new_stage<StColOut>(b, 0);
	const int T = tile_lines_for<StColOut>(b, 0, nlines, 8);
	set_tiles(s, T, a*T, 0);          // one tile per line: ntile = a
	s.Y = s1_.as<double2>(); s.ldY = pad8(b); s.a = (int)a; s.nm = (int)nlines; s.ny = (int)herm_ny; s.nx = (int)herm_nx; s.herm = herm_nx > 0 ? 1 : 0;
	s.conj_out = conj; s.out = out; s.ldo = ldo; s.ocomp = ocomp; s.scale = scale;
	s.groups = (int)((nlines + T - 1)/T); s.dgr = make_fastdiv((uint32_t)s.groups);
	launch_any(s, npre*s.groups*a, st);
}

void FftChain::map2leg(hipStream_t st, const MapDesc& m, int nc, int mmax, double2* leg, long ldleg, const double2* tab, double scale) {
	PXS_REQUIRE(rings_ok() && m.nphi == nphi_, "internal: ring chain not planned");
	const long npair_all = (m.nring + 1)/2, a = ra_.a, b = ra_.b, ldY = pad8(b);
	const int T2 = pair_lines<StRingA2>(b, 2*npair_all);
	const long qchunk = ring_chunk(npair_all, (long)sizeof(double2)*nc*a*ldY, T2/2);
	ensure1(sizeof(double2)*(size_t)nc*qchunk*a*ldY);
	if (!dry_) pass_ring.begin();
	for (long q_lo = 0; q_lo < npair_all; q_lo += qchunk) {
		const long npair = std::min(qchunk, npair_all - q_lo);
		if (!dry_) pass_ring.add(npair);
		const int nring = m.nring - (int)(2*q_lo);           // rings from the first pair of this pass on (the odd-last-ring tests are local)
		{	StRingA1 s = new_stage<StRingA1>(a, 0);
			s.m = map_addr(m); s.m.off0 += 2*q_lo*m.ring_stride; s.m.nring = nring;
			s.b = (int)b; s.npair = (int)npair; s.Y = s1_.as<double2>(); s.ldY = ldY; s.dnp = make_fastdiv((uint32_t)npair);
			set_tiles(s, tile_lines_for<StRingA1>(a, 0, b, 16), b, nphi_);
			launch_any(s, (long)nc*npair*s.ntile, st);
		}
		{	StRingA2 s = new_stage<StRingA2>(b, 0);
			set_tiles(s, T2, a*T2, 0);          // one tile per line: ntile = a
			s.Y = s1_.as<double2>(); s.ldY = ldY; s.a = (int)a; s.X = (int)nphi_; s.npair = (int)npair; s.nring = nring; s.mmax = mmax;
			s.groups = (int)((npair + T2/2 - 1)/(T2/2)); s.da = make_fastdiv((uint32_t)a); s.dgr = make_fastdiv((uint32_t)s.groups);
			s.leg = leg + 2*q_lo; s.ldleg = ldleg; s.nm = mmax + 1; s.tab = tab; s.scale = scale;
			launch_any(s, (long)nc*s.groups*a, st);
		}
	}
	if (!dry_) PXS_HIP(hipGetLastError());
}

void FftChain::h2map(hipStream_t st, const double2* h, long ldh, const MapDesc& m, int nc, int mmax, long hcomp) {
	PXS_REQUIRE(rings_ok() && m.nphi == nphi_, "internal: ring chain not planned");
	if (!dry_) pass_ring.begin();
	if (dry_ ? line_h2map_takes(nphi_, mmax) : line_h2map(st, h, ldh, m, nc, mmax, hcomp)) return;      // (ring lengths compiled into ringline.hip: one kernel, no intermediate)
	const long npair_all = (m.nring + 1)/2, a = rs_.a, b = rs_.b, ldY = pad8(b);
	const long qchunk = ring_chunk(npair_all, (long)sizeof(double2)*nc*a*ldY, 1);
	ensure1(sizeof(double2)*(size_t)nc*qchunk*a*ldY);
	if (!dry_) pass_ring.begin();
	for (long q_lo = 0; q_lo < npair_all; q_lo += qchunk) {
		const long npair = std::min(qchunk, npair_all - q_lo);
		if (!dry_) pass_ring.add(npair);
		const int nring = m.nring - (int)(2*q_lo);
		{	StRingS1 s = new_stage<StRingS1>(a, 0);
			s.h = h + 2*q_lo*ldh; s.ldh = ldh; s.hcomp = hcomp > 0 ? hcomp : m.nring; s.b = (int)b; s.X = (int)nphi_; s.npair = (int)npair; s.nring = nring; s.mmax = mmax;
			s.Y = s1_.as<double2>(); s.ldY = ldY; s.dnp = make_fastdiv((uint32_t)npair);
			set_tiles(s, tile_lines_for<StRingS1>(a, 0, b, 8), b, nphi_);
			launch_any(s, (long)nc*npair*s.ntile, st);
		}
		{	StRingS2 s = new_stage<StRingS2>(b, 0);
			s.Y = s1_.as<double2>(); s.ldY = ldY; s.a = (int)a; s.npair = (int)npair; s.m = map_addr(m); s.m.off0 += 2*q_lo*m.ring_stride; s.m.nring = nring;
			s.dnp = make_fastdiv((uint32_t)npair);
			set_tiles(s, tile_lines_for<StRingS2>(b, 0, a, 16), a, 0);
			launch_any(s, (long)nc*npair*s.ntile, st);
		}
	}
	if (!dry_) PXS_HIP(hipGetLastError());
}

// components per pass of a theta chain: all of them unless the two ping-pong buffers would exceed PXS_CHAIN_SCRATCH_GB (12) each
static int theta_comp_chunk(int nc, size_t need1_per_comp, size_t need2_per_comp) {
	size_t budget = (size_t)12 << 30; env_budget("PXS_CHAIN_SCRATCH_GB", 30, budget);      // (per call: the sizing of the scratch and the loop read the same value)
	const size_t per = sizeof(double2)*std::max(need1_per_comp, need2_per_comp);
	return (int)std::max<size_t>(1, std::min<size_t>((size_t)nc, budget/std::max<size_t>(per, 1)));
}
// points per component that a theta chain keeps in s1_ (n1) and s2_ (n2): the largest of the intermediates its builders put there
static void theta_need(ThetaOp op, const ThetaPlan& tp, int nm, size_t& n1, size_t& n2) {
	const size_t npair = (size_t)(nm + 1)/2;
	if (op == TH_TO_CC) { n1 = npair*std::max(tp.g*FftChain::pad8(tp.bN), tp.g*FftChain::pad8(tp.g2)); n2 = npair*std::max(tp.g2*FftChain::pad8(tp.g), tp.ac*FftChain::pad8(tp.g)); }
	else if (op == TH_FROM_CC_ADJ) { n1 = npair*tp.g*FftChain::pad8(tp.bN); n2 = npair*tp.ac*FftChain::pad8(tp.g); }
	else if (op == TH_FROM_CC) { n1 = npair*tp.gs*FftChain::pad8(tp.bs); n2 = npair*tp.aNs*FftChain::pad8(tp.gs); }
	else { n1 = npair*std::max(tp.g*FftChain::pad8(tp.ac), tp.g*FftChain::pad8(tp.g2)); n2 = npair*std::max(tp.g2*FftChain::pad8(tp.g), tp.bN*FftChain::pad8(tp.g)); }
}
void FftChain::theta_scratch(ThetaOp op, const ThetaPlan& tp, int nm, int nc, size_t& b1, size_t& b2) {
	size_t n1, n2; theta_need(op, tp, nm, n1, n2);
	const int cc = theta_comp_chunk(nc, n1, n2);
	b1 = sizeof(double2)*n1*cc; b2 = sizeof(double2)*n2*cc;
}
void FftChain::ring_scratch(long nring, int nc, bool analysis, size_t& b1, int mmax) const {
	if (!analysis && mmax >= 0 && line_h2map_takes(nphi_, mmax)) { b1 = 0; return; }
	const long npair = (nring + 1)/2, a = analysis ? ra_.a : rs_.a, b = analysis ? ra_.b : rs_.b;
	b1 = sizeof(double2)*(size_t)nc*npair*a*pad8(b);       // (ring_chunk only shrinks it)
}
// the loop of a theta chain over the component chunks that fit its scratch: stages(c0, ncl) runs the chain for
// the ncl components from c0 on.
// All components of a chunk go through each stage in ONE launch (outer index = component * npair + pair; batched maps are
// components here): 64 maps of 5400 rings are 5 launches of ~150 000 workgroups instead of 320 of ~10 000 with their tails.
template<class F> void FftChain::theta_chunks(ThetaOp op, const ThetaCall& c, F&& stages) {
	const int nc = c.nc; size_t n1, n2; theta_need(op, *c.tp, c.nm, n1, n2);
	const int cchunk = theta_comp_chunk(nc, n1, n2);
	ensure1(sizeof(double2)*n1*cchunk); ensure2(sizeof(double2)*n2*cchunk);
	if (!dry_) pass_theta.begin();
	for (int c0 = 0; c0 < nc; c0 += cchunk) {
		if (!dry_) pass_theta.add(std::min(cchunk, nc - c0));
		stages(c0, (long)std::min(cchunk, nc - c0));
	}
	if (!dry_) PXS_HIP(hipGetLastError());
}

// The four stage lists.  c.map is leg on the map's rings for the two that read them, h for the two that write them.
void FftChain::theta(hipStream_t st, ThetaOp op, const ThetaCall& c) {
	if (!dry_) pass_theta.begin();      // (stays empty where the single-kernel form takes the call)
	if (op == TH_TO_CC) to_cc(st, c); else if (op == TH_FROM_CC_ADJ) from_cc_adjoint(st, c); else if (op == TH_FROM_CC) from_cc(st, c); else if (op == TH_TO_CC_ADJ) to_cc_adjoint(st, c);
}

void FftChain::to_cc(hipStream_t st, const ThetaCall& c) {
	if (line_takes(*c.tp, true, c.sig_half)) { if (!dry_) line_analysis(st, true, c); return; }
	const ThetaPlan& tp = *c.tp; const long npair = (c.nm + 1)/2, g = tp.g, bN = tp.bN, g2 = tp.g2, ac = tp.ac;
	const double2* ph = c.ph;
#ifdef PXS_LAB
	{ static const int noph = [] { const char* e = getenv("PXS_CH_NOPH"); return e ? atoi(e) : 0; }(); if (noph) ph = nullptr; }     // timing experiments only (wrong results)
#endif
	theta_chunks(TH_TO_CC, c, [&](int c0, long ncl) {
		run_first<StFirst>(st, pair_src(c.map + (size_t)c0*c.nm*c.ldmap, c.ldmap, c.nr, tp.N, c.mir_c, c.spin, c.nm, nullptr), ncl, npair, g, bN);      // RA1
		// RA2.  M > N (the interpolant form; the fine-CC form on grids below ~2 lmax rings): zero padding, Nyquist bin of N split;
		// M <= N (the fine-CC form on larger grids): low pass, |k| < M/2 kept
		run_resize(st, ncl*npair, bN, g2, g, tp.M > tp.N ? -1 : (int)(tp.M/2 - 1), tp.M > tp.N ? 1 : 0, 0, ph);
		run_sigma(st, ncl*npair, g, g2, c.sigma);      // RA3
		run_resize(st, ncl*npair, g2, ac, g, c.lmax, 0, 0, nullptr);      // RA4: keep |k| <= lmax
		run_split<0>(st, ncl, npair, c.nm, c.spin, ac, g, 0, c.ncc, c.cc + (size_t)c0*c.nm*c.ldcc, c.ldcc, (long)c.nm*c.ldcc, c.wcc, nullptr, 1.0, 0);      // RA5
	});
}

// exact transpose of from_cc (theta upsampling CC grid -> map rings): leg on the map's rings -> leg on the CC grid, for grids
// without self-mirrored rings (F1).  With U = S F_N^-1 D(e^{ik theta0}) Pad F_Ncc E (E: mirror extension of the CC samples,
// S: sampling at the rings), U^T = E^T F_Ncc^-1 Trunc D(e^{-ik theta0}) F_N S^T up to the scalar; E^T A S^T = R A E' for any
// operator A that commutes with the reflection (E': mirror extension of the ring samples, R: restriction to the CC rings) except
// at the CC pole rings, which E' counts twice: weight 1/2 there (c.wcc).  So: RA1, the resize N -> N_cc directly, RA5.
void FftChain::from_cc_adjoint(hipStream_t st, const ThetaCall& c) {
	if (line_takes(*c.tp, false, nullptr)) { if (!dry_) line_analysis(st, false, c); return; }
	const ThetaPlan& tp = *c.tp; const long npair = (c.nm + 1)/2, g = tp.g, bN = tp.bN, ac = tp.ac;
	theta_chunks(TH_FROM_CC_ADJ, c, [&](int c0, long ncl) {
		// (wring: quadrature weights of the map's rings: the weights form of the analysis)
		run_first<StFirst>(st, pair_src(c.map + (size_t)c0*c.nm*c.ldmap, c.ldmap, c.nr, tp.N, c.mir_c, c.spin, c.nm, c.wring), ncl, npair, g, bN);
		run_resize(st, ncl*npair, bN, ac, g, c.lmax, 0, 0, c.ph);
		run_split<0>(st, ncl, npair, c.nm, c.spin, ac, g, 0, c.ncc, c.cc + (size_t)c0*c.nm*c.ldcc, c.ldcc, (long)c.nm*c.ldcc, c.wcc, nullptr, 1.0, 0);
	});
}

// exact adjoint of to_cc (adjoint_analysis_2d): leg on the CC grid -> ring spectra h[c][ring][m] on the map's rings.
// With to_cc = W R F_Ncc^-1 T F_M Sigma F_M^-1 P F_N E' (E': parity mirror extension of the ring samples, P: phase, Nyquist split and
// zero padding N -> M, T: truncation to |k| <= lmax, R: restriction to the CC rings, W: weights) the adjoint is
// E'^T F_N^-1 P^H F_M Sigma F_M^-1 T^T F_Ncc R^T W.  R^T zero-extends, but E'^T keeps only the part of the result with the column's
// parity (times 2), every operator in between commutes with the reflection, so the zero extension may be replaced by the parity
// mirror extension of W x with weight 1/2 off the poles: the chain then has the shape of from_cc -- pairs of columns of opposite
// parity packed into one sequence and separated by reflection symmetry at the end, written ring-major for the ring FFT.
void FftChain::to_cc_adjoint(hipStream_t st, const ThetaCall& c) {
	const ThetaPlan& tp = *c.tp; const long npair = (c.nm + 1)/2, g = tp.g, bN = tp.bN, g2 = tp.g2, ac = tp.ac;
	theta_chunks(TH_TO_CC_ADJ, c, [&](int c0, long ncl) {
		// weighted mirror-pair extension on the CC circle, pass 1 of FFT_Ncc
		run_first<StFirst>(st, pair_src(c.cc + (size_t)c0*c.nm*c.ldcc, c.ldcc, c.ncc, tp.Ncc, 0, c.spin, c.nm, c.wcc), ncl, npair, g, ac);
		// pass 2 of FFT_Ncc, |k| <= lmax embedded in the M spectrum, pass 1 of IFFT_M
		run_resize(st, ncl*npair, ac, g2, g, c.lmax, 0, 0, nullptr);
		// pass 2 of IFFT_M, x |sin| series, pass 1 of FFT_M
		run_sigma(st, ncl*npair, g, g2, c.sigma);
		// pass 2 of FFT_M, transposed padding M -> N (conjugate phase, Nyquist bins combined), pass 1 of IFFT_N
		// (M <= N: transpose of the low pass = zero padding of |k| < M/2)
		run_resize(st, ncl*npair, g2, bN, g, tp.M > tp.N ? -1 : (int)(tp.M/2 - 1), 0, 1, c.ph);
		// pass 2 of IFFT_N, the two parities apart, rings of the map, ring-major
		run_split<1>(st, ncl, npair, c.nm, c.spin, bN, g, c.mir_c, c.nr, c.map + (size_t)c0*c.nr*c.ldmap, c.ldmap, (long)c.nr*c.ldmap, nullptr, c.tab, c.scale, 1);
	});
}

void FftChain::from_cc(hipStream_t st, const ThetaCall& c) {
	const ThetaPlan& tp = *c.tp; const long npair = (c.nm + 1)/2, gs = tp.gs, bs = tp.bs, aN = tp.aNs;
	theta_chunks(TH_FROM_CC, c, [&](int c0, long ncl) {
		run_first<StFirst>(st, pair_src(c.cc + (size_t)c0*c.nm*c.ldcc, c.ldcc, c.ncc, tp.Ncc, 0, c.spin, c.nm, nullptr), ncl, npair, gs, bs);      // RS1
		run_resize(st, ncl*npair, bs, aN, gs, c.lmax, 0, 0, c.ph);      // RS2
		run_split<1>(st, ncl, npair, c.nm, c.spin, aN, gs, c.mir_c, c.nr, c.map + (size_t)c0*c.nr*c.ldmap, c.ldmap, (long)c.nr*c.ldmap, c.wring, c.tab, c.scale, 0);      // RS3
	});
}

// 2-D FFT of real maps [npre][ny][nx] -> complex [npre][ny][nx] (enmap.fft of a map, pixell/enmap.py:1307-1323), through the
// chain stages: MA1 / MA2 transform two real rows per complex line and leave the half spectrum transposed, F[kx <= nx/2][y]; the
// column transforms then run along contiguous rows (StFirst in plain mode, StColOut), and the last pass writes out[ky][kx] and its
// Hermitian image.  Traffic: 7 x (8 bytes per pixel) + the complex output = 4.5 N x 16 bytes against 7.5 N x 16 for the same
// transform as a complex one over both axes.  false: no usable factorisation (the caller takes the generic engine).
bool FftChain::fft2_real(hipStream_t st, const void* in, int in_dtype, double2* out, long npre, long ny, long nx, bool forward, double scale) {
	Split sy;
	// (plan_rings notes the width before it knows whether it can split it: a chain kept per stream must not take a width it refused
	// in an earlier transform for a planned one)
	if (nx < 4 || ny < 4 || !split_balanced(ny, sy) || ((nphi_ != nx || !rings_ok()) && !plan_rings(nx))) return false;
	const long nm = nx/2 + 1, ldF = pad8(ny), a = std::min(sy.a, sy.b), b = ny/a;
	if (getenv("PXS_CHAIN_VERBOSE")) fprintf(stderr, "[pxsht] fft2_real %ld x %ld x %ld: rows %s, columns %ld x %ld\n", npre, ny, nx, describe().c_str(), a, b);
	PXS_REQUIRE(npre*nm < (1L << 31)/std::max<long>(a, b), "fft2_real: too many lines");
	// F (half spectrum, transposed) lives in s2_, the four-step intermediates of both axes in s1_
	ensure2(sizeof(double2)*(size_t)npre*nm*ldF);
	MapDesc m; m.ptr = in; m.dtype = in_dtype; m.cstride = ny*nx; m.ring_off0 = 0; m.ring_stride = nx; m.pix_stride = 1; m.nring = (int)ny; m.nphi = nx;
	map2leg(st, m, (int)npre, (int)(nm - 1), s2_.as<double2>(), ldF, nullptr, 1.0);
	ensure1(sizeof(double2)*(size_t)npre*nm*a*pad8(b));
	run_first<StFirst2D>(st, plain_src(s2_.as<double2>(), nm, ldF, ny, 0), npre, nm, a, b);
	run_colout(st, npre, nm, a, b, out, nx, ny*nx, forward ? 0 : 1, scale, ny, nx);
	if (!dry_) PXS_HIP(hipGetLastError());
	return true;
}

// 2-D complex FFT [npre][ny][nx] -> [npre][ny][nx] (enmap.ifft, enmap.fft of complex maps) with the same stage kinds: rows (StFirst
// plain over the lines of a row, StColOut into the transposed F[kx][y]), then columns along contiguous rows of F (StFirst plain,
// StColOut into out[ky][kx]).  Backward: conj on the way in and out.  false: no usable factorisation.
bool FftChain::fft2_c2c(hipStream_t st, const double2* in, double2* out, long npre, long ny, long nx, bool forward, double scale) {
	Split sx, sy;
	if (nx < 4 || ny < 4 || !split_balanced(nx, sx) || !split_balanced(ny, sy)) return false;
	const long ax = std::min(sx.a, sx.b), bx = nx/ax, ay = std::min(sy.a, sy.b), by = ny/ay, ldF = pad8(ny);
	if (npre*std::max(nx, ny) >= (1L << 31)/512) return false;
	if (getenv("PXS_CHAIN_VERBOSE")) fprintf(stderr, "[pxsht] fft2_c2c %ld x %ld x %ld: rows %ld x %ld, columns %ld x %ld\n", npre, ny, nx, ax, bx, ay, by);
	ensure1(sizeof(double2)*(size_t)npre*std::max(ny*ax*pad8(bx), nx*ay*pad8(by)));
	ensure2(sizeof(double2)*(size_t)npre*nx*ldF);
	const int conj = forward ? 0 : 1;
	run_first<StFirst2D>(st, plain_src(in, ny, nx, nx, conj), npre, ny, ax, bx);                  // rows y: lines of nx points
	run_colout(st, npre, ny, ax, bx, s2_.as<double2>(), ldF, nx*ldF, 0, 1.0);                      // -> F[kx][y]
	run_first<StFirst2D>(st, plain_src(s2_.as<double2>(), nx, ldF, ny, 0), npre, nx, ay, by);     // columns kx: contiguous lines of ny points
	run_colout(st, npre, nx, ay, by, out, nx, ny*nx, conj, scale);                                 // -> out[ky][kx]
	if (!dry_) PXS_HIP(hipGetLastError());
	return true;
}

} // namespace pxs
