// Fused FFT chains of the SHT for gfx950 (see fftchain.hip): ring FFTs (map <-> leg) and the exact theta resampling
// between the map's rings and the minimal Clenshaw-Curtis grid, as sequences of LDS kernels in which every intermediate
// array is written once and read once.
#pragma once
#include "fft.hpp"
#include <tuple>
#include <map>
#include <set>
#include <vector>
#include <mutex>
#include <memory>

namespace pxs {

struct Lds2;
struct PairSrc;

// factorisation N = a*b of a four-step transform: pass 1 = a-point transforms over the residues mod b,
// pass 2 = b-point transforms producing the residues mod a
struct Split { long a = 0, b = 0; };
// a stage as launched: stage id (S::SID), lengths of its one or two LDS transforms, lines per tile; in the compiled table?
struct ChainShape { int sid, na, nb, T; bool is_static; };

struct ThetaPlan {            // sizes of the theta chains of a grid plan
	bool ok = false;
	long N = 0, M = 0, Ncc = 0;      // map circle, fine circle (|sin| product), CC circle
	long g = 0, bN = 0, g2 = 0, ac = 0;     // analysis: N = g*bN, M = g*g2 (both ways), Ncc = ac*g
	long gs = 0, bs = 0, aNs = 0;            // synthesis: Ncc = gs*bs, N = aNs*gs
};

// the four theta operations between the map's rings and the CC grid, and what one of them takes
enum ThetaOp { TH_NONE = -1, TH_TO_CC = 0, TH_FROM_CC_ADJ = 1, TH_FROM_CC = 2, TH_TO_CC_ADJ = 3 };
struct ThetaCall {
	const ThetaPlan* tp = nullptr;
	int nc = 0, nm = 0, spin = 0, lmax = 0, mir_c = 0;
	double2* map = nullptr; long ldmap = 0; int nr = 0;       // map side: leg[c][m][ring] (read: TH_TO_CC, TH_FROM_CC_ADJ) or h[c][ring][m] (written)
	double2* cc = nullptr; long ldcc = 0; int ncc = 0;        // CC side: leg_cc[c][m][cc ring]
	// tables: shift phase per k; pointwise table on the M circle; weight (.x) per CC ring (TH_FROM_CC_ADJ: 1/N_cc, half at the poles;
	// TH_TO_CC_ADJ: the TH_TO_CC weights halved off the poles); optional weight (.x) per ring of the map; h = ... * conj(tab[m]) * scale
	const double2 *ph = nullptr, *sigma = nullptr, *wcc = nullptr, *wring = nullptr, *tab = nullptr; double scale = 1.0;
	const double* sig_half = nullptr;      // the fine-CC form: entries i <= M/2 of its sigma, which is real and mirror-symmetric (AnaForm::sig_half)
};

class FftChain {
public:
	explicit FftChain(FftContext* fc) : fc_(fc) {}
	// can the engine run its LDS passes on lines of this length (radices 2,3,4,5, length <= 512)?
	static bool sub_ok(long n);
	static bool sub_ok_theta(long n); // ... of the theta stages: radix 7 as well
	static long pad8(long n) { return (n + 7) & ~7L; }
	// ring FFT split of nphi for analysis (map -> leg) and synthesis (h -> map); false: no usable factorisation
	bool plan_rings(long nphi);
	// theta chain sizes for a grid with N circle samples; picks Ncc (even, > 2 lmax + 1) and M (> N + 2 lmax)
	static ThetaPlan plan_theta(long N, int lmax);
	static long ducc_ncc(int lmax);     // 2 good_size_complex(lmax + 1): the circle of the CC grid ducc0 runs its Legendre stage on
	bool rings_ok() const { return ra_.a > 0; }
	std::string describe() const { return "analysis " + std::to_string(ra_.a) + "x" + std::to_string(ra_.b) + ", synthesis " + std::to_string(rs_.a) + "x" + std::to_string(rs_.b); }

	struct MapDesc { const void* ptr; int dtype; long cstride, ring_off0, ring_stride, pix_stride; int nring; long nphi;
	                 long bstride = 0; int ncb = 0; };   // batches: component index k of a call = b*ncb + c lives at b*bstride + c*cstride (ncb = 0: no batch axis)
	// map -> leg[c][m][ring] * tab[m] * scale   (two real rings per complex transform; needs 2 mmax < nphi)
	void map2leg(hipStream_t st, const MapDesc& m, int nc, int mmax, double2* leg, long ldleg, const double2* tab, double scale);
	// h[c][ring][m] (row stride ldh) -> map
	// (hcomp: rows of h per component when the map's rings are a row range of a larger h; 0 = the map's ring count)
	void h2map(hipStream_t st, const double2* h, long ldh, const MapDesc& m, int nc, int mmax, long hcomp = 0);
	// the theta operation `op` on c.nc components, paired by column parity (theta_scratch: what it keeps in the ping-pong scratch).
	// TH_TO_CC: leg on the map's rings -> quadrature-weighted leg on the CC grid.  TH_FROM_CC: band-limited leg on the CC grid ->
	// h[c][ring][m] * conj(tab[m]) * scale on the map's rings.  TH_FROM_CC_ADJ: exact transpose of TH_FROM_CC for grids without
	// self-mirrored rings.  TH_TO_CC_ADJ: exact adjoint of TH_TO_CC, written like TH_FROM_CC.
	void theta(hipStream_t st, ThetaOp op, const ThetaCall& c);
	// 2-D FFT of real [npre][ny][nx] (float32 / float64) into complex128 [npre][ny][nx]; false if nx or ny has no usable factorisation
	bool fft2_real(hipStream_t st, const void* in, int in_dtype, double2* out, long npre, long ny, long nx, bool forward, double scale);
	// 2-D FFT of complex128 [npre][ny][nx] (in == out allowed); false if nx or ny has no usable factorisation
	bool fft2_c2c(hipStream_t st, const double2* in, double2* out, long npre, long ny, long nx, bool forward, double scale);
	// single-kernel form of TH_TO_CC (has_mid) / TH_FROM_CC_ADJ for lines that fit a CU (thetaline.hip): one workgroup per pair of columns,
	// no HBM intermediates.  line_takes: THE test of whether it runs the call -- the circles are a compiled configuration, a middle circle
	// comes with ThetaCall::sig_half, and PXS_THETA_LINE is not 0; the route (which then sizes no theta scratch), the dry run and the launch ask it.
	static bool line_takes(const ThetaPlan& tp, bool has_mid, const double* sig_half);
	void line_analysis(hipStream_t st, bool has_mid, const ThetaCall& c);      // (throws on a call line_takes refuses)
	// single-kernel form of h2map for ring lengths compiled into ringline.hip: one workgroup per ring pair, no HBM intermediate
	bool line_h2map(hipStream_t st, const double2* h, long ldh, const MapDesc& m, int nc, int mmax, long hcomp);
	static bool line_h2map_takes(long nphi, int mmax);
	size_t scratch_bytes() const { return s1_.bytes + s2_.bytes; }
	// scratch a call needs, so that the plan can size it before the first launch of the call
	static void theta_scratch(ThetaOp op, const ThetaPlan& tp, int nm, int nc, size_t& b1, size_t& b2);
	void ring_scratch(long nring, int nc, bool analysis, size_t& b1, int mmax = -1) const;      // (mmax given: 0 for a synthesis that ringline.hip takes)
	void reserve(size_t b1, size_t b2) { s1_.ensure(b1); s2_.ensure(b2); }
	// Compile-time-planned stage kernels (chain_kernel_static, chain_static_table.hpp).  A dry run: between dry_begin and dry_end the
	// calls above launch and allocate nothing and list the stage shapes they would launch, with whether the table holds each.
	void dry_begin(std::vector<ChainShape>* out) { dry_ = out; }
	void dry_end() { dry_ = nullptr; }
	int static_check(int maxr = 0);      // table entries (of the stages with this largest radix; 0: all) against the engine's plans; throws on a mismatch
	static bool static_has(int sid, int na, int nb, int T);
	static void static_shapes(std::vector<ChainShape>& out);
	// passes of the most recent theta chain (components per pass) and of the most recent map2leg / h2map through the two ring stages
	// (ring pairs per pass; none where the single-kernel form took the call); a dry run leaves them alone
	PassLog pass_theta, pass_ring;
private:
	void ensure1(size_t b) { if (!dry_) s1_.ensure(b); }
	void ensure2(size_t b) { if (!dry_) s2_.ensure(b); }
	std::vector<ChainShape>* dry_ = nullptr;
	std::set<int> checked_;
	const double2* small_tw(long X, int n, int T);
	template<class S> void set_tiles(S& s, int T, long nlines, long X);
	template<class S> int tile_lines_for(long n_a, long n_b, long nlines, int mult);
	template<class S> int pair_lines(long n, long nlines);
	template<class S> void launch_any(S& s, long nblk, hipStream_t st);
	// one builder per stage kind (fftchain.hip): each plans, fills in and launches its stage; theta_chunks: the chunk loop of a theta chain
	template<class S> S new_stage(long na, long nb);
	template<class S> void run_first(hipStream_t st, const PairSrc& src, long ncomp, long npair, long a, long b);
	void run_resize(hipStream_t st, long nouter, long fa, long fb, long g, int kmax, int nyq, int adj, const double2* ph);
	void run_sigma(hipStream_t st, long nouter, long g, long g2, const double2* sigma);
	template<int MODE> void run_split(hipStream_t st, long ncomp, long npair, int nm, int spin, long a, long g, int mir_c, int nr_out,
	                                  double2* out, long ld, long ocstride, const double2* w, const double2* tab, double scale, int self_half);
	void run_colout(hipStream_t st, long npre, long nlines, long a, long b, double2* out, long ldo, long ocomp, int conj, double scale, long herm_ny = 0, long herm_nx = 0);
	template<class F> void theta_chunks(ThetaOp op, const ThetaCall& c, F&& stages);
	void to_cc(hipStream_t st, const ThetaCall& c), from_cc(hipStream_t st, const ThetaCall& c), from_cc_adjoint(hipStream_t st, const ThetaCall& c), to_cc_adjoint(hipStream_t st, const ThetaCall& c);
	std::mutex mu_;
	std::map<std::tuple<long, int, int>, DevBuf> stw_;
	FftContext* fc_;
	Split ra_, rs_;           // ring FFT splits: analysis, synthesis
	long nphi_ = 0;
	DevBuf s1_, s2_;          // ping-pong scratch
};

// where the pixels of a map live, in the form the ring-FFT kernels take it (fftchain.hip, ringline.hip)
struct MapAddr { void* ptr; int dtype; long cstride, bstride, off0, rstride, pstride; int nring, ncb; FastDiv dncb; };   // "component" index = b*ncb + c
inline MapAddr map_addr(const FftChain::MapDesc& m) {
	MapAddr a; a.ptr = const_cast<void*>(m.ptr); a.dtype = m.dtype; a.cstride = m.cstride; a.bstride = m.bstride; a.off0 = m.ring_off0; a.rstride = m.ring_stride; a.pstride = m.pix_stride; a.nring = m.nring;
	a.ncb = m.ncb > 0 ? m.ncb : (1 << 30); a.dncb = make_fastdiv((uint32_t)a.ncb);
	return a;
}

} // namespace pxs
