// The SHT plan, the route of a call and what the translation units of the SHT host pipeline share:
//   sht.hip          plan construction, options and queries, route_of, run_core, the C entry points
//   sht_grids.hip    grid arithmetic and quadrature weights (host only)
//   sht_general.hip  ring sets with per-ring length, phase and offset (healpix, profile rings)
//   sht_unfused.hip  the glue kernels, the ring FFT and the theta resamplers through the generic FFT engine
#pragma once
#include "../../include/pxsht.h"
#include "fft.hpp"
#include "legendre.hpp"
#include "fftchain.hpp"
#include <map>
#include <memory>
#include <mutex>
#include <exception>

namespace pxs {

typedef long double LDb;
static const LDb PIl = 3.141592653589793238462643383279502884L;

FftContext& fft_context(int device);
void fft_dense_lines(int device, hipStream_t st, long n, bool forward, long nlines, const double2* in, double2* out);   // api_fft.hip
void fft_release_stream(int device, hipStream_t st);                                                                  // api_fft.hip
const char* get_last_error();
// points plans (points.hip)
struct PointsState;
PointsState* points_create(int ntheta, int nphi, int lmax, int mmax, int device, long npts, const double* d_loc, double eps, hipStream_t st);
void points_free(PointsState* s);
void points_run(PointsState* s, pxs_plan* grid, int spin, int mode, int adjoint, int nb, const AlmArg& alm, const MapArg& map, hipStream_t st);
int64_t points_query(const PointsState* s, const std::string& name);
void points_profile(PointsState* s, bool on);
// ... of a pixel map [ny][nx] instead of an alm (pxm_plan_map_points): pix [{y, x}][npts] in pixels
PointsState* mappoints_create(int ny, int nx, int ydouble, int device, long npts, const double* d_pix, double eps, hipStream_t st);
void mappoints_run(PointsState* s, int ncomp, const void* maps, int mdt, long mstride, void* out, int odt, long ostride, hipStream_t st);
bool points_from_map(const PointsState* s);

// ---- sht_grids.hip: a grid's circle of N samples, ring j at theta = (c + 2 j) pi / N
struct GridInfo { long N; int c; bool ok; };
GridInfo grid_info(const std::string& g, int n);
bool grid_weights_only(const std::string& g);      // DH / F2: analysis is plain quadrature
int grid_maxlmax(const std::string& g, int n);
std::vector<LDb> grid_theta(const std::string& g, int n);
double abs_sin_coef(long q);
std::vector<double> grid_weights(const std::string& g, int n);      // pxs_gridweights; throws
DevBuf ring_weight_table(const std::string& g, int n, int nphi);    // ... / nphi per ring as a double2 table on the device
// ring r is its own mirror image on the circle (the pole rings of CC, one of MW / MWflip)
inline bool self_mirrored(long r, int mir_c, long N) { const long t = 2*r + mir_c; return t == 0 || t == N || t == 2*N; }

// one form of the interpolating analysis: the fine circle of M points, the pointwise table on it, the CC weights (whalf: halved off
// the two pole rings, for the adjoint) and the fused theta chain that holds the circle (tp.ok) -- the unfused engine takes any M.
// sig_half: the fine-CC form's table is real and mirror-symmetric; its entries i <= M/2 as doubles, for the single-kernel engine
struct AnaForm { ThetaPlan tp; DevBuf sigma, sig_half, wcc, whalf; long M = 0; bool fine = false; };
// tables of the theta resampling between the map's grid (circle of N samples, mirror constant mir_c) and the CC grid (circle N_cc, ncc rings)
struct ThetaTables {
	long N = 0; int mir_c = 0; long Ncc = 0; int ncc = 0;
	DevBuf ph_shift, ph_up, wadj;           // e^{-+ i k theta_0}; weights of the transposed upsampling
	DevBuf wgrid, wgrid_ext, wunit_ext;     // built on first use: gridweights / nphi per ring; _ext: self-mirrored rings doubled (ring_weights_ext)
};
// a general ring set: rings of equal length are one dense block of z, for one batched FFT (sht_general.hip)
struct GenRings {
	struct Group { long n, count, zoff; };
	std::vector<Group> groups; long npixz = 0, nblk = 0;
	DevBuf blk_ring, blk_k0, nphi, zoff, rstart, phi0, z;
	int device = 0; std::vector<hipStream_t> streams; std::vector<hipEvent_t> join; hipEvent_t fork = nullptr;
	void setup(int device, int nring, const uint64_t* nphi, const double* phi0, const uint64_t* ringstart);
	void ffts(hipStream_t st, int nc, bool forward);
	GenRings() {} GenRings(const GenRings&) = delete; GenRings& operator=(const GenRings&) = delete; ~GenRings();
};
// begin / end of a profiled stage around a scope (an exception leaves the stage open, as a throwing launch always did)
struct StageScope {
	LegProfile& prof; hipStream_t st; int stage; int live = std::uncaught_exceptions();
	StageScope(LegProfile& prof_, hipStream_t st_, int stage_) : prof(prof_), st(st_), stage(stage_) { prof.begin(st, stage); }
	~StageScope() noexcept(false) { if (std::uncaught_exceptions() == live) prof.end(st, stage); }
};

} // namespace pxs

using namespace pxs;      // (a header of the three sht*.hip files only: pxs_plan is the C ABI's name, outside the namespace)

// How one pxs_synthesis / pxs_analysis call runs.  route_of() decides it ONCE per call, from the plan and the call's arguments; the
// scratch of the call (reserve_call), its batching, the stages it launches (run_core) and the queries all read this one object.
enum RouteKind {
	R_DIRECT,             // synthesis / its adjoint: Legendre stage on the map's own rings
	R_VIA_CC,             // ... on the minimal CC grid, fused theta chain between that grid and the map's rings (grids, bands of F1 grids)
	R_VIA_CC_UNFUSED,     // ... theta resampling through the generic FFT engine (no fused theta chain for this size), one map at a time
	R_VIA_CC_UNFUSED_H,   // ... whose last stage writes the ring-major h directly (plans without a ring chain)
	R_RING_WEIGHTS,       // analysis: quadrature weights on the map's rings + adjoint synthesis there (DH / F2; the weights form off the CC detour)
	R_CC_WEIGHTS,         // analysis: ring weights, transposed theta upsampling, Legendre stage on the CC grid (the weights form with fused chains)
	R_CHAIN,              // analysis: exact quadrature of the theta-interpolant through the fused chains (TH_TO_CC / TH_TO_CC_ADJ)
	R_UNFUSED };          // analysis: ... through the generic FFT engine on dense rows, one map at a time
struct Route {
	RouteKind kind = R_DIRECT;
	bool to_map = true;            // alm -> map (synthesis, adjoint analysis) or map -> alm
	bool batched = true;           // may take several maps per pass (batch_chunk); false: one map at a time
	int nc = 1, deriv1 = 0;        // map components per map
	const LegTables* tb = nullptr;       // (null in the routes the queries make: they size nothing)
	const RingSet* rs = nullptr;         // ring set of the Legendre stage: the plan's rs_map (buffer leg) or rs_cc (buffer leg2)
	// row strides of leg[c][m][ring], leg2[c][m][cc ring], h[c][ring][m] (padded to whole 128-byte lines on the fused routes, dense on
	// the unfused ones; 0: the route does not touch that buffer) and the rings of h per component
	long ld_leg = 0, ld_leg2 = 0, ld_h = 0; int nr_h = 0;
	long ld_leg_alloc = 0;         // leg is SIZED for rows of this stride: ld_leg but for the CC-grid synthesis, see route_of
	// theta operation between the map's grid (nr_th rings: the whole grid for a band) and the CC grid, with the form whose chain and tables it uses
	ThetaOp theta = TH_NONE; bool theta_fused = false, line = false;      // line: the single-kernel engine takes it (thetaline.hip; no intermediates)
	int nr_th = 0; const AnaForm* form = nullptr;
	bool reserve_chain = false;    // the call reserves the ping-pong scratch of the plan's FFT chains
	// bytes the call needs for nb maps per pass: the plan's leg / leg2 / hbuf, the Legendre work arrays, the chain's ping-pong scratch
	struct Scratch { size_t leg = 0, leg2 = 0, h = 0, almt = 0, mom = 0, c1 = 0, c2 = 0, r1 = 0; };
	Scratch scratch(const pxs_plan* p, int nb) const;
};

struct pxs_plan {
	// a plan serves one call at a time (it owns the scratch of the call, and the analysis option is read several times in a call):
	// the entry points that run or reconfigure it take this lock, so two host threads on one cached plan queue up instead of interleaving
	std::mutex call_mu;
	// ... on the device too: the calls are asynchronous, so the lock orders only their issue.  Every call records `used` on its stream
	// after its last launch, and a call that comes on another stream waits for it before its first (PlanUse below): calls on one plan
	// run in the order they were issued, whatever their streams.
	hipEvent_t used = nullptr; hipStream_t used_stream = nullptr; bool used_any = false;
	int device = 0;
	bool is_grid = false;
	std::string geometry;
	int nring = 0, nphi = 0;
	// rows of a larger F1 grid (declination bands through pxs_plan_rings): the grid has nfull rings, the map's first ring is its
	// ring row0.  Such plans share the CC-grid machinery of the grid plans for synthesis and its adjoint.  Grid plans: nfull = nring.
	int nfull = 0, row0 = 0; bool band = false;
	double phi0 = 0;
	long ring_off0 = 0, ring_stride = 0, pix_stride = 1;   // user-map offset of (ring r, pixel x) = ring_off0 + r*ring_stride + x*pix_stride
	int lmax = 0, mmax = 0; long lstride = 1;
	DevBuf d_mstart;
	RingSet rs_map, rs_cc;
	std::map<int, std::unique_ptr<LegTables>> tables;
	LegWork wk;
	DevBuf leg, leg2, hbuf, phase;
	DevBuf b1, b2;               // intermediates of the unfused theta resamplers
	ThetaTables th;              // theta resampling (grid plans, bands of F1 grids); th.ncc == 0: none
	// The two interpolating forms of the analysis.  ana_interp: the |sin| series on M > N + 2 lmax points.  ana_fine: the fine-CC form
	// (ducc0's resample_to_prepared_CC as published: the theta-interpolant, low-passed where the grid has more than 2 N_cc circle samples,
	// is evaluated on the CC grid of N_cc + 1 rings, multiplied by that grid's quadrature weights and carried to the N_cc/2 + 1 rings
	// of the Legendre stage by the transposed upsampling): the chain of the interpolant form with M = 2 N_cc and the weights as the
	// pointwise table; M > 0: its tables exist.  ana_interp.tp is also the chain of the synthesis side.
	AnaForm ana_interp, ana_fine;
	bool general = false; GenRings gen;      // general ring sets
	// points plans (pxs_plan_points): the CC grid plan they were made from (owned by the caller) and the per-point state
	pxs_plan* pgrid = nullptr; PointsState* pts = nullptr;
	~pxs_plan() { if (pts) points_free(pts); if (used) (void)hipEventDestroy(used); }
	DevBuf wring;                // DH / F2 grids: per-ring quadrature weight / nphi (analysis = weighted adjoint synthesis)
	int ana_weights = 2;         // pxs_plan_option("analysis"): 2 = ducc0's route (default: the fine-CC form; ring weights on CC grids with ntheta >= 2 lmax + 2),
	                             // 0 = interpolant (|sin| series on the M circle), 1 = ring weights + adjoint synthesis where ntheta >= 2 lmax + 2;
	                             // PXS_ANALYSIS=ducc0|interpolant|weights presets it
	bool syn_via_cc = false, syn_via_cc0 = false;      // synthesis through the CC grid: spin s / spin 0 (the recurrence of spin 0 is 4x cheaper per ring, the resampling is not)
	FftContext* fc = nullptr;
	// fused FFT chains (fftchain.hip).  chain_rings: ring FFTs through MA1/MA2, MS1/MS2; ana_interp.tp.ok: theta resampling through RA1-5 / RS1-3.
	// These say what the plan CAN do; which of it a call uses, and with which row strides (padded to whole 128-byte lines on the chain
	// routes, dense on the unfused ones kept for aliased rings and lengths without a usable factorisation), is the call's Route.
	std::unique_ptr<FftChain> chain; bool chain_rings = false;
	bool chain_theta() const { return chain_rings && ana_interp.tp.ok; }
	long ld_map() const { return chain_rings ? FftChain::pad8(nring) : nring; }
	long ld_cc()  const { return chain_theta() ? FftChain::pad8(th.ncc) : th.ncc; }
	long ld_h()   const { return chain_rings ? FftChain::pad8(mmax + 1) : mmax + 1; }
	FftChain::MapDesc map_desc(const MapArg& a, int ncb = 0) const {
		FftChain::MapDesc m; m.ptr = a.ptr; m.dtype = a.dtype; m.cstride = a.cstride; m.ring_off0 = ring_off0; m.ring_stride = ring_stride; m.pix_stride = pix_stride; m.nring = nring; m.nphi = nphi;
		m.bstride = a.bstride; m.ncb = ncb; return m; }
	LegProfile prof;
	size_t resample_chunk_bytes = size_t(1) << 40;    // per intermediate buffer of the unfused theta resamplers (chunking to stay in the
	                                                  // Infinity Cache was measured slower: 22.4 -> 26.2 ms at config 2; PXS_RESAMPLE_MB re-enables it)
	// passes of the plan's most recent call (pxs_plan_query "passes_batch", "passes_resample"): maps per pass of run_call; column pairs or
	// columns per pass of the last unfused theta resampler.  The other seams keep theirs where they loop (wk, chain, the FFT context).
	PassLog pass_batch, pass_resample;

	LegTables& table(int spin) {
		auto& p = tables[spin]; if (!p) { p.reset(new LegTables()); p->build(lmax, mmax, spin); }
		return *p; }
	// Legendre stage of a route for nb maps: alm -> the route's buffer on its ring set with its row stride (rs_map: leg, rs_cc: leg2) ...
	DevBuf& leg_buf(const Route& r) { return r.rs == &rs_cc ? leg2 : leg; }
	void leg_syn(hipStream_t st, const Route& r, const AlmArg& a, int nb) {
		const long ld = r.rs == &rs_cc ? r.ld_leg2 : r.ld_leg;
		leg_synthesis(st, *r.rs, *r.tb, wk, a.ptr, a.dtype, a.cstride, d_mstart.as<uint64_t>(), lstride, leg_buf(r).as<double2>(), r.deriv1, &prof, ld, nb, a.bstride, (long)r.nc*(mmax + 1)*ld);
	}
	// ... and its transpose
	void leg_ana(hipStream_t st, const Route& r, const AlmArg& a, int nb) {
		const long ld = r.rs == &rs_cc ? r.ld_leg2 : r.ld_leg;
		leg_analysis(st, *r.rs, *r.tb, wk, leg_buf(r).as<double2>(), a.ptr, a.dtype, a.cstride, d_mstart.as<uint64_t>(), lstride, r.deriv1, &prof, ld, nb, a.bstride, (long)r.nc*(mmax + 1)*ld);
	}
};

// One call on a plan (call_mu held, the plan's device selected): waits, on the call's stream, for the plan's previous call where that
// ran on another stream, and records the plan's last use when the call has issued its launches (also when it ends in an exception:
// what it launched up to there uses the scratch all the same).
struct PlanUse {
	pxs_plan* p; hipStream_t st;
	PlanUse(pxs_plan* p_, hipStream_t st_) : p(p_), st(st_) {
		if (p->used_any && st != p->used_stream) PXS_HIP(hipStreamWaitEvent(st, p->used, 0));
	}
	~PlanUse() {
		if (!p->used && hipEventCreateWithFlags(&p->used, hipEventDisableTiming) != hipSuccess) p->used = nullptr;
		if (p->used && hipEventRecord(p->used, st) == hipSuccess) { p->used_stream = st; p->used_any = true; }
		else { (void)hipStreamSynchronize(st); p->used_any = false; }      // (no event: the call is complete before the next one starts)
	}
	PlanUse(const PlanUse&) = delete; PlanUse& operator=(const PlanUse&) = delete;
};

// ---- sht_general.hip: the ring FFT stage of a general ring set, nc components of one map (the caller holds the stage's StageScope)
void gen_map2leg(pxs_plan* p, hipStream_t st, const MapArg& m, int nc, double2* leg, long ldleg);
void gen_leg2map(pxs_plan* p, hipStream_t st, const double2* leg, long ldleg, const MapArg& m, int nc);

// ---- sht_unfused.hip
// leg[line][ring] *= w[ring].x (the weights forms of the analysis)
void scale_leg_rings(hipStream_t st, double2* leg, long nlines, int nr, long ld, const double2* w);
// leg[c][m][ring] (rows of stride ldleg) * e^{+i m phi0} -> the plan's h[c][ring][m] (rows of stride ldh)
void leg_to_h(pxs_plan* p, hipStream_t st, const double2* leg, long ldleg, long ldh, int nc);
// the ring FFT of one map through the generic FFT engine, dense rows: map -> leg * e^{-i m phi0} / the plan's h -> map
void unfused_map2leg(pxs_plan* p, hipStream_t st, const MapArg& m, int nc, double2* leg);
void unfused_h2map(pxs_plan* p, hipStream_t st, const MapArg& m, int nc);
// the theta operations through the generic FFT engine, dense rows, one map: TH_TO_CC and TH_TO_CC_ADJ (leg instead of h) with the
// tables of a form, TH_FROM_CC (h_out: straight into the ring-major h where the whole map is one chunk)
void resample_to_cc(pxs_plan* p, hipStream_t st, const double2* leg_in, double2* leg_cc, int nc, int spin, const AnaForm& f);
void resample_to_cc_adjoint(pxs_plan* p, hipStream_t st, const double2* leg_cc, double2* leg_out, int nc, int spin, const AnaForm& f);
void resample_from_cc(pxs_plan* p, hipStream_t st, const double2* leg_cc, double2* leg_out, int nc, int spin, double2* h_out = nullptr);
