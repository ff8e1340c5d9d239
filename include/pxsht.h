/* libpxsht -- MI355X (gfx950) spherical-harmonic-transform and FFT kernels behind a C ABI.
 *
 * Drop-in boundary for the one hot path of simonsobs/pixell: the calls that
 * pixell/curvedsky.py and pixell/fft.py make into the third-party ducc0 / pyfftw / numpy
 * libraries.  The reference has no C ABI of its own for this path (its boundary is ducc0's
 * Python keyword interface), so every entry point below cites the reference call site it
 * replaces; INTEGRATION.md shows the ctypes binding a pixell maintainer would add.
 *
 * Conventions
 *  - all data pointers are DEVICE pointers (hipMalloc / torch.cuda tensors) on the plan's
 *    device; the caller owns them.  `stream` is a hipStream_t (NULL = default stream); calls
 *    are asynchronous with respect to the host.
 *  - plans own their device scratch and tables, so a plan serves one call at a time.  On the
 *    device the library sees to that itself: calls on one plan run in the order they were
 *    issued, whatever their streams (each call records an event after its last launch, and
 *    a call that comes on another stream waits for it; a points plan orders against the
 *    grid plan it borrows in the same way).  Streams are told apart by their handles: a
 *    stream must be idle with respect to a plan (synchronised, or its last call on the plan
 *    followed by one on another stream) before it is destroyed.  The calls themselves take the plan's own host
 *    lock, so two host threads on one plan queue up; a thread that sets a plan option and
 *    relies on it in the next call must hold a lock of its own around the pair.
 *  - device memory a plan releases (pxs_plan_destroy, a scratch buffer that grows) may still
 *    be in use by queued work on any stream: the library synchronises the device before
 *    such a block serves another plan or returns to the driver (pxs_memory).
 *  - return value: 0 = OK, <0 = error (pxs_last_error() returns a thread-local message).
 *    No C++ exception crosses the boundary.
 *  - dtype codes: 0 = float32, 1 = float64, 2 = complex64, 3 = complex128.  All arithmetic is
 *    float64 regardless of the I/O dtype.
 *  - alm layout: element (l,m) of component c at alm[c*alm_cstride + mstart[m] + l*lstride]
 *    (curvedsky.alm_info, curvedsky.py:409-447).
 */
#ifndef PXSHT_H
#define PXSHT_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct pxs_plan pxs_plan;

#define PXS_F32  0
#define PXS_F64  1
#define PXS_C64  2
#define PXS_C128 3

#define PXS_MODE_STANDARD 0
#define PXS_MODE_DERIV1   1   /* curvedsky.py:917-920: spin-1 of sqrt(l(l+1)) a_lm -> (d_theta, d_phi/sin) */

/* Plan for transforms on explicit iso-latitude rings.
 * Replaces the geometry arguments of ducc0.sht.experimental.synthesis / adjoint_synthesis
 * (curvedsky.py:936-960, 1068-1084, 328-349, 396-403; ring tables from get_ring_info, get_ring_info_healpix,
 * get_ring_info_radial, curvedsky.py:1170-1234).
 * theta[nring] colatitudes, nphi[nring] pixels per ring (>= 1), phi0[nring] azimuth of pixel 0,
 * ringstart[nring] index of pixel 0 of each ring in the flat map, pixstride: stride between pixels of a ring.
 * Rings of equal length, phase and spacing (CAR maps) take the fused ring FFTs; any other ring set (healpix, profile
 * rings, ring subsets, nphi < mmax) the general path: one batched FFT per ring length.  Equal rings that are consecutive
 * rows of a Fejer-1 grid (a declination band) run their Legendre stage on the Clenshaw-Curtis grid of that grid. */
int pxs_plan_rings(pxs_plan** plan, int nring, const double* theta, const uint64_t* nphi,
                   const double* phi0, const uint64_t* ringstart, int64_t pixstride,
                   int lmax, int mmax, const uint64_t* mstart, int64_t lstride, int device);

/* Plan for a named full-sky equiangular grid ("CC","F1","MW","MWflip","DH","F2"; curvedsky.py:1329-1342), map[ntheta][nphi].
 * Replaces the geometry arguments of ducc0.sht.experimental.{synthesis_2d, adjoint_synthesis_2d,
 * analysis_2d, adjoint_analysis_2d} (curvedsky.py:907-924, 1032-1046).
 * flip_y / flip_x fold curvedsky.map2buffer / buffer2map (curvedsky.py:1384-1411) into the kernels'
 * addressing: with flip_y the map's row 0 is the SOUTHERN-most ring, with flip_x column 0 is the
 * largest phi; phi0 is that of the flipped (ducc-orientation) map, i.e. analyse_geometry().phi0
 * (curvedsky.py:1284). */
int pxs_plan_grid2d(pxs_plan** plan, const char* geometry, int ntheta, int nphi, double phi0,
                    int flip_y, int flip_x, int lmax, int mmax, const uint64_t* mstart,
                    int64_t lstride, int device);

/* Plan for transforms at arbitrary points (ducc0.sht.experimental.synthesis_general / adjoint_synthesis_general, curvedsky.py:993-1016,
 * 1088-1120).  cc_grid_plan: a pxs_plan_grid2d plan of geometry "CC", unflipped, phi0 = 0, ntheta >= lmax + 2, nphi even and >= 2 mmax + 2,
 * both 2 ntheta - 2 and nphi transformable by the FFT engine; it carries lmax, mmax and the alm layout, the caller keeps it alive as long as
 * the points plan.  d_loc: DEVICE f64[npts][2] = (theta in [0, pi], phi any finite value), read while the plan is made (sorted into the
 * plan).  epsilon in [1e-13, 0.1]: relative L2 accuracy of the result.  Transforms run through pxs_synthesis on this plan with the map
 * [comp][npts] (map_cstride = npts): synthesis onto the CC grid, mirror onto the doubled sphere, 2-D FFT, deapodisation and zero padding
 * to the fine grid (oversampling 2), inverse FFT, interpolation with the exponential-of-semicircle kernel; the adjoint is the exact
 * transpose.  The spreading of the adjoint sums in a fixed order (bitwise repeatable); the Legendre stage follows the grid plan's own
 * "deterministic" option.  pxs_plan_query: "kernel_width", "fine_ntheta", "fine_nphi", "npts", "plan_us" (host wall time of
 * making the plan), "stage_us_cc_sht" / "_fft" / "_grid" / "_interp" / "_spread" (device-event microseconds per stage, summed over the
 * calls since pxs_plan_option(plan, "profile", 1), which resets them; each profiled call synchronises its stream).  A plan serves any
 * number of calls, of either direction and of any spin.  Synchronises `stream` once. */
int pxs_plan_points(pxs_plan** plan, const pxs_plan* cc_grid_plan, int64_t npts, const double* d_loc, double epsilon, int device, void* stream);

void pxs_plan_destroy(pxs_plan* plan);

/* alm -> map (adjoint = 0: synthesis[_2d]) or map -> alm (adjoint = 1: adjoint_synthesis[_2d]).
 * spin 0: 1 alm component, 1 map component; spin > 0: 2 and 2; mode DERIV1: 1 and 2 (spin must be 1).
 * alm_cstride / map_cstride: distance between components in elements of the respective dtype.
 * nbatch independent maps per call (the loop over pre-dimensions at curvedsky.py:763-765, 910-924): map b starts at
 * map + b*map_bstride, its alm at alm + b*alm_bstride (elements); nbatch = 1 ignores the batch strides.  The ring FFTs of a
 * batch run as one launch per pass; the plan's scratch bounds the maps per pass (PXS_BATCH_GB, default 64; pxs_plan_query
 * "passes_batch" tells how a call went). */
int pxs_synthesis(pxs_plan* plan, int spin, int mode, int adjoint, int nbatch,
                  void* alm, int alm_dtype, int64_t alm_cstride, int64_t alm_bstride,
                  void* map, int map_dtype, int64_t map_cstride, int64_t map_bstride, void* stream);

/* map -> alm (adjoint = 0: analysis_2d) or alm -> map (adjoint = 1: adjoint_analysis_2d).
 * Only for grid2d plans (curvedsky.py:1018-1048; batch loop :1038-1046); how the integral over theta is taken: pxs_plan_option. */
int pxs_analysis(pxs_plan* plan, int spin, int adjoint, int nbatch,
                 void* map, int map_dtype, int64_t map_cstride, int64_t map_bstride,
                 void* alm, int alm_dtype, int64_t alm_cstride, int64_t alm_bstride, void* stream);

/* Plan options.  "analysis": how pxs_analysis integrates over theta on grid2d plans (CC, F1, MW, MWflip; DH and F2 always take ring
 * weights) -- all forms give the same alm for band-limited maps and differ at the 1e-3 level on maps that are not --
 *   2 (default) "ducc0": the route of ducc0's analysis_2d (ducc0 >= 0.36, src/ducc0/sht/sht.cc: analysis_2d -> resample_to_prepared_CC; the
 *     reference calls it at curvedsky.py:1032-1046) as restated WITHOUT access to the package or its source in the build environment: all
 *     forms agree on band-limited maps (pinned by tests); agreement with ducc0's numerics on maps that are not band-limited -- e.g. its
 *     treatment of the Nyquist bin when the spectrum is resized -- is UNPINNED until checked against an installed ducc0.  The theta-interpolant of the rings -- low-passed to
 *     |k| < N_cc where the grid's circle has at least 2 N_cc samples -- is evaluated on the Clenshaw-Curtis grid of N_cc + 1 rings,
 *     multiplied by that grid's quadrature weights and carried to the N_cc/2 + 1 rings of the Legendre stage by the transposed
 *     band-limited upsampling; N_cc = 2 good_size_complex(lmax + 1) (ducc0's) whenever the grid's circle shares a usable factor with
 *     it (pxs_plan_query "ncc_circle" tells).  A CC grid with ntheta >= 2 lmax + 2 is multiplied by its own weights directly (ducc0:
 *     need_first_resample = false).  Plans without fused theta chains run the same form through the generic FFT engine.
 *   0 "interpolant": exact quadrature of the full theta-interpolant (its product with |sin| on a circle of M > N + 2 lmax points);
 *   1 "weights": ring quadrature weights + adjoint synthesis, the reference's cyl route (curvedsky.py:852-861, 1068-1084:
 *     get_gridweights / nphi, then adjoint_synthesis), applied when ntheta >= 2 lmax + 2 (smaller grids take the default).
 * The adjoint (adjoint = 1) is the exact transpose of the chosen form.  Takes effect for the calls issued after it returns.
 * "build_tables" (value = spin): builds the recurrence tables of that spin now instead of inside the first transform that needs them.
 * "deterministic" (0 | 1; default 0, or 1 when PXS_DETERMINISTIC=1 is set as the plan is made): the Legendre analysis (pxs_analysis,
 *   adjoint synthesis) sums the contributions of the ring chunks of an m with atomic adds in arrival order -- results repeat from
 *   run to run to ~1e-14 of their size, not bit for bit (ducc0 on the CPU is bitwise repeatable).  1 selects ordered sums through
 *   per-chunk partial moments (<= 2 GB of scratch, m in passes; batched calls one map at a time): bitwise repeatable, slower.
 *   The promise is run-to-run repeatability of the SAME call.  A map transformed inside a batch of 4 or more takes the FP64-MFMA
 *   kernels (another summation order) and equals its single-map call to rounding (1e-13), not bit for bit, with or without this
 *   option -- the reference loops over the maps and is identical per map; PXS_SYN_MM_MIN=0 / PXS_ANA_MM_MIN=0 keep batches on the
 *   single-map kernels.
 * "leg_max_batch" (value = n >= 0; default 0 = no bound): at most n maps per launch of the single-map (VALU) Legendre kernels and 8 n per
 *   launch of the FP64-MFMA kernels.  The only limit otherwise is the grid size (2^31 blocks: tens of thousands of maps in one call);
 *   the option exists so that the launch loop can be tested.  Same results.
 * "leg_ana_k" (value = K >= 0; default 0 = the library's rule): ring pairs per lane of the single-map (VALU) Legendre analysis kernels.  The rule
 *   takes 8 (spin 0) / 4 (spin s), fewer on small ring sets, and 6 for spin s where the ring set gives at least 8 waves per m; the option exists
 *   so that every compiled kernel can be tested on a small ring set.  A K without a compiled kernel is an error of the call.  Same results to rounding.
 * Memory budgets from the environment (PXS_BATCH_GB, PXS_PART_GB, PXS_SEED_GB, PXS_CHAIN_SCRATCH_GB in GB; PXS_FFT_TEMP_MB,
 *   PXS_RESAMPLE_MB, PXS_RING_CHUNK_MB in MB) are real numbers of their unit (0.004 GB = 4 MB), read as the plan is made (PXS_PART_GB,
 *   PXS_RESAMPLE_MB), per call (the others) or per transform of the FFT engine (PXS_FFT_TEMP_MB: pxf_fft_nd and plans alike).
 *   PXS_PART_GB=0: one m per pass; PXS_BATCH_GB unset or 0: the default rule (64 GB, at most 40 % of the free memory). */
int pxs_plan_option(pxs_plan* plan, const char* name, int64_t value);

/* What a plan does: "analysis_form" = the form pxs_analysis runs now (0 interpolant, 1 ring weights, 2 fine-CC form of ducc0's
 * route), "ncc_circle" = N_cc, the circle of the CC grid of the Legendre stage (0: none), "ducc_ncc_circle" = ducc0's N_cc for
 * the plan's lmax, "theta_line" = 1 if the theta resampling of pxs_analysis runs as one kernel with the line resident on a CU
 * (the fine-CC form and the ring-weights form on the circle sizes compiled into thetaline.hip; PXS_THETA_LINE=0 switches it off), 0 if as the five-stage chain: same results.
 * "leg_ana_k": ring pairs per lane of the single-map Legendre analysis kernels in the plan's most recent analysis or adjoint synthesis (0: none yet).
 * "leg_executed_flops_ana": FP64 flops the Legendre analysis kernels executed while profiling was on (see pxs_profile_flops).
 * "chain_stages": the distinct FFT chain stage shapes (stage, transform lengths, lines per tile) of the plan's standard calls (analysis
 * under its current option, synthesis of spin 0 and 2); "chain_static": how many of them have a compile-time-planned kernel
 * (csrc/chain_static_table.hpp; PXS_CHAIN_STATIC=0, read per call, runs the run-time kernel for all: same results to rounding);
 * "chain_static_table": entries of that table, each checked against the FFT engine's plan of its lengths (an error if one differs).
 * "passes_<seam>": how many passes the plan's most recent pxs_synthesis / pxs_analysis took at one of the places where a memory budget
 *   cuts a call, counted by the loop that launched them (0: the call did not come by that place); "passes_<seam>_first", "_prev",
 *   "_last": the sizes of the first pass, the one before the last and the last.  Seams and their sizes: "batch" maps per pass of a
 *   batched call (PXS_BATCH_GB); "leg_m" m per range of the ordered Legendre analysis (PXS_PART_GB; of the last map); "theta" components
 *   per pass of a theta chain (PXS_CHAIN_SCRATCH_GB); "ring" ring pairs per pass of the two ring FFT stages (PXS_RING_CHUNK_MB);
 *   "resample" column pairs or columns per pass of an unfused theta resampler (PXS_RESAMPLE_MB; at least 32); "leg_valu" / "leg_mm" maps
 *   per launch of the single-map / FP64-MFMA Legendre kernels (option "leg_max_batch"); of a batched call in several passes: those of
 *   its last pass.  "passes_fft" is device-wide and takes plan = NULL (the current device) as well: lines per pass of the most recent
 *   four-step transform of the FFT engine (PXS_FFT_TEMP_MB), whoever issued it.  Diagnostics: not synchronised with calls in flight. */
int pxs_plan_query(const pxs_plan* plan, const char* name, int64_t* value);

/* ducc0.sht.experimental.get_gridweights (curvedsky.py:501, 855): out[ntheta], sum = 4 pi. Host memory. */
int pxs_gridweights(const char* geometry, int ntheta, double* out);

/* largest lmax analysis_2d supports on the grid (curvedsky.get_ducc_maxlmax, curvedsky.py:1349-1353) */
int pxs_grid_maxlmax(const char* geometry, int ntheta);

/* number of Legendre rings the plan iterates (R_actual of SURVEY 8d) for synthesis / analysis */
int pxs_plan_info(const pxs_plan* plan, int* nring_legendre_syn, int* nring_legendre_ana, int64_t* scratch_bytes);

/* Sizes the planner of the fused FFT chains picks for a theta circle of N samples and band limit lmax (diagnostics, tests):
 * out[10] = {ok, g, bN, g2, M, ac, Ncc, gs, bs, aNs} with N = g*bN, M = g*g2 (fine circle of the |sin| product), Ncc = ac*g
 * (Clenshaw-Curtis circle: Ncc/2+1 rings in the Legendre stage), synthesis: Ncc = gs*bs, N = aNs*gs.  See csrc/fftchain.hip. */
int pxs_debug_theta_plan(int64_t N, int lmax, int64_t* out);
/* Average milliseconds of one group of fused-chain stages of a plan, run `reps` times on scratch data (diagnostics and kernel
 * experiments, tools/chain_lab.py).  kind 0: ring FFTs map -> leg (MA1, MA2), 1: ring FFTs h -> map (MS1, MS2), 2: theta
 * resampling of the analysis (RA1-5), 3: of the synthesis (RS1-3), 4: transposed theta upsampling.  nc components in one call. */
int pxs_debug_chain(pxs_plan* plan, int kind, int nc, int spin, int reps, double* ms);

/* Optional device-side stage timers (hipEvents recorded on the launch stream around each stage):
 * used by bench.py to time the dominant kernel live.  ms[PXS_NSTAGE], counts[PXS_NSTAGE]. */
#define PXS_STAGE_LEG_SYN  0   /* Legendre synthesis kernel (alm2leg) */
#define PXS_STAGE_LEG_ANA  1   /* Legendre analysis kernel (leg2alm) */
#define PXS_STAGE_RING_FFT 2   /* ring FFTs + transposes (map2leg / leg2map) */
#define PXS_STAGE_RESAMPLE 3   /* theta resampling between the map's rings and the Clenshaw-Curtis grid */
#define PXS_NSTAGE 4
int pxs_profile(pxs_plan* plan, int enable);
int pxs_profile_read(pxs_plan* plan, double* ms, int* counts, int reset);
/* FP64 flops the Legendre kernels EXECUTED since profiling was enabled (or since the last reset): flops[0] synthesis, flops[1]
 * analysis.  Counted by the kernels themselves (steps run x ring pairs per lane x FMAs per step x 64 lanes x 2), so bench.py can
 * quote the hardware FMA utilisation next to the algorithmic flop count of SURVEY 8(d) (which credits rings and degrees the
 * kernels skip as polar-dead).  No reference counterpart. */
int pxs_profile_flops(pxs_plan* plan, double* flops, int reset);
/* A wave of the single-map kernels holds K blocks of 64 ring pairs, and the figures above count every block from the step at which its wave starts.  The
 * analysis kernels start the accumulation of a block at the block's own live step: what they executed with that taken into account is
 * pxs_plan_query "leg_executed_flops_ana" (flops, an exact integer; reset together with pxs_profile_flops).  bench.py quotes flops[1], which at C3 is 3.2 % above it. */

/* N-d FFT over `naxes` axes of a strided array: the engine behind fft.engines["hip"].FFTW(a,b,axes,
 * direction) (pixell/fft.py:8-64,133-209) and enmap.fft/ifft (enmap.py:1307-1337).
 * kind 0: c2c (in/out same shape), 1: r2c (out last transformed axis n//2+1), 2: c2r,
 * 3..10: the FFTW r2r kinds REDFT00, REDFT10, REDFT01, REDFT11, RODFT00, RODFT10, RODFT01, RODFT11 (DCT-I..IV, DST-I..IV;
 *   pixell/fft.py:211-290): real in/out of the same shape, unnormalised, `forward` ignored.
 * shape[ndim] is the LOGICAL (real-space) shape; istride/ostride in elements of in/out dtype.
 * forward: e^{-i...}; unnormalised, result multiplied by `scale`. */
int pxf_fft_nd(int ndim, const int64_t* shape, const int64_t* istride, const int64_t* ostride,
               int naxes, const int* axes, int kind, int forward, double scale,
               int in_dtype, int out_dtype, const void* in, void* out, int device, void* stream);

/* alm post-processing on the device (cython/cmisc_core.c of the reference, via alm_info.alm2cl / lmul,
 * curvedsky.py:451-474, 630-712).  d_mstart: DEVICE array u64[mmax+1]; d_lmat: DEVICE f64[N][M][nl].
 * pxa_alm2cl: cl[l] = 1/(2l+1) sum_m a1_lm conj(a2_lm) (m>0 counted twice), one pair of alm per call.
 * pxa_lmatmul: out[a] = sum_b lmat[a][b][l] in[b] (N = M = 1 is almxfl); out may alias in.
 * complex64 alm use single precision arithmetic with the filter rounded to float, as the reference does. */
int pxa_alm2cl(int lmax, int mmax, const uint64_t* d_mstart, int64_t lstride, const void* alm1, const void* alm2, int alm_dtype,
               void* cl, int cl_dtype, int device, void* stream);
int pxa_lmatmul(int N, int M, int lmax, int mmax, const uint64_t* d_mstart, int64_t lstride,
                const void* alm_in, int64_t in_cstride, void* alm_out, int64_t out_cstride, int alm_dtype,
                const double* d_lmat, int nl, int device, void* stream);
/* pxa_rotate_alm: rotation of ncomp alm (triangular, mmax = lmax, components ncomp apart by in_cstride / out_cstride elements) by the
 * Euler angles psi, theta, phi (zyz, active: f'(n) = f(R^-1 n), R = R_z(phi) R_y(theta) R_z(psi); ducc0.sht.rotate_alm as called at
 * curvedsky.py:717-740).  FP64 arithmetic for both dtypes; out may alias in.  Scratch of (1 + 2 min(ncomp, 4)) x 16 x nalm bytes is
 * allocated and freed on `stream` (stream-ordered); no host synchronisation. */
int pxa_rotate_alm(int lmax, int ncomp, const void* alm_in, int64_t in_cstride, void* alm_out, int64_t out_cstride, int alm_dtype,
                   double psi, double theta, double phi, int device, void* stream);
/* The filter bank of the wavelet transforms: one alm in any alm_info layout (lmax, mmax, d_mstart, lstride as for pxa_lmatmul; npre
 * components, one every *_pitch elements) <-> nscale filtered copies.  Copy i is npre dense triangular layouts of band limit L_i
 * (mmax = L_i, stride 1, element (l, m) at m (2 L_i + 1 - m)/2 + l), one every pitch[i] >= (L_i+1)(L_i+2)/2 elements from the DEVICE
 * pointer outs[i] / ins[i]; it holds signal up to lmax_i <= min(lmax, L_i).
 * pxa_bank_split: outs[i](l,m) = filt[i][l] in(l,m) for l <= lmax_i, 0 for lmax_i < l <= L_i; (l,m) the input does not hold count as 0.
 * pxa_bank_merge: out(l,m) = (out(l,m) if accumulate, else 0) + sum_i filt[i][l] ins[i](l,m) over the scales with l <= lmax_i, added in
 *   ascending i by one thread per element (bitwise repeatable); every (l,m) of the output layout is written.
 * Convention for the tables: lmaxs, Ls, outs / ins and the pitches are HOST arrays of nscale entries -- they travel in the kernel
 * arguments, 32 scales per launch (so a bank of up to 32 scales is one launch that loads each input element once); d_filt is a DEVICE
 * table f64[nscale][nl], nl > max lmax_i.  complex64 alm use single precision arithmetic with the filter rounded to float.
 * No host synchronisation; the scale arrays must not overlap the full alm. */
int pxa_bank_split(int nscale, const int* lmaxs, const int* Ls, void* const* outs, const int64_t* out_pitch, int npre,
                   int lmax, int mmax, const uint64_t* d_mstart, int64_t lstride, const void* alm_in, int64_t in_pitch, int alm_dtype,
                   const double* d_filt, int nl, int device, void* stream);
int pxa_bank_merge(int nscale, const int* lmaxs, const int* Ls, void* const* ins, const int64_t* in_pitch, int npre,
                   int lmax, int mmax, const uint64_t* d_mstart, int64_t lstride, void* alm_out, int64_t out_pitch, int alm_dtype,
                   const double* d_filt, int nl, int accumulate, int device, void* stream);

/* flat-sky harmonic helpers around the 2-D map FFT (pixell/enmap.py:1358-1400 map2harm / harm2map / queb_rotmat,
 * :1959-2011 calc_ps2d, :2526-2556 lbin).  d_ly[ny], d_lx[nx]: DEVICE f64 wavenumber axes (enmap.laxes); maps [ny][nx] contiguous.
 * pxm_rotate_queb: in place (a, b) <- (c a - s b, s a + c b) with c + i s = exp(i spin atan2(+-lx, ly)); inverse_sign selects -.
 * pxm_ps2d: out = Re(a conj b).   pxm_lbin: ADDS, per bin floor(|l|/bsize) < nbin, the map value to d_sum and (when both
 * are given) |l| to d_lsum and 1 to d_hit; the caller zeroes the accumulators. */
int pxm_rotate_queb(int ny, int nx, const double* d_ly, const double* d_lx, int spin, int inverse_sign,
                    void* a, void* b, int dtype, int device, void* stream);
int pxm_ps2d(int64_t n, const void* a, const void* b, int dtype, void* out, int out_dtype, int device, void* stream);
int pxm_lbin(int ny, int nx, const double* d_ly, const double* d_lx, double bsize, int nbin,
             const void* map, int dtype, double* d_sum, double* d_lsum, double* d_hit, int device, void* stream);
/* binning by a per-pixel bin table (enmap.rbin, enmap.py:2512-2524; enmap.lbin with a transform of |l|, :2526-2531; both through _bin_helper
 * :2533-2556): ADDS map[i] (f32 | f64, n contiguous pixels) to d_sum[d_bin[i]] for 0 <= d_bin[i] < nbin; d_bin: DEVICE int32[n], made by the host
 * from the geometry alone; the caller zeroes d_sum (DEVICE f64[nbin]) */
int pxm_bin_index(int64_t n, const int32_t* d_bin, int nbin, const void* map, int dtype, double* d_sum, int device, void* stream);
/* data[i] *= vec[(i / inner) % n] on a contiguous complex array of `total` elements; d_vec: DEVICE complex128[n]
 * (the per-axis phase ramps of pixell.fft.shift, fft.py:347-368) */
int pxm_mul_axis(int64_t total, int64_t n, int64_t inner, void* data, int dtype, const void* d_vec, int device, void* stream);

/* curved-sky lensing between the gradient synthesis and the point synthesis of lensing.lens_map_curved (pixell/lensing.py:367-503).
 * pxm_deflect: the observed positions offset by the gradient of the lensing potential (lensing.offset_by_grad, lensing.py:552-589), one
 *   thread per pixel.  Positions: d_pos = NULL -> pixel i of the separable CAR band [ny][nx] (ny*nx = npts) sits at dec0 + (i / nx) ddec,
 *   ra0 + (i % nx) dra (radians; enmap.posmap without the map); otherwise d_pos: DEVICE f64 [{dec, ra}(, psi0)][npts], pos_ncomp = 2 | 3.
 *   d_grad: [2][npts] = (d/ddec, (d/dra)/cos dec) as alm2map(deriv=True) returns it, f32 | f64, components grad_cstride elements apart.
 *   geodesic != 0: the point moves |grad| along the great circle that leaves it in the direction of the gradient, psi = psi0 minus twice
 *   the change of that direction's angle in the local (e_theta, e_phi) basis (the spin-2 rotation of parallel transport); a zero
 *   gradient is the identity.  geodesic = 0: dec + g0, ra + g1/cos dec, reflected at the poles (lensing.pole_wrap, :623-632), psi = 0.
 *   d_loc: DEVICE f64 [npts][2] = (colatitude in [0, pi], ra in [0, 2 pi)), what pxs_plan_points reads; d_psi: DEVICE f64 [npts] or NULL.
 *   FP64 arithmetic for both gradient dtypes.
 * pxm_rotate_pol: in place (a, b) <- (c a - s b, s a + c b), c + i s = exp(i spin psi) (enmap.rotate_pol, enmap.py:1402-1416), for npair
 *   pairs of maps (f32 | f64, npts contiguous pixels each) that share d_psi (DEVICE f64 [npts]): pair p is a + p*pair_stride,
 *   b + p*pair_stride (elements).  spin = 0 does nothing. */
int pxm_deflect(int64_t npts, int ny, int nx, double dec0, double ddec, double ra0, double dra, const double* d_pos, int pos_ncomp,
                const void* d_grad, int grad_dtype, int64_t grad_cstride, int geodesic, double* d_loc, double* d_psi, int device, void* stream);
int pxm_rotate_pol(int64_t npts, int npair, void* a, void* b, int64_t pair_stride, int dtype, const double* d_psi, int spin, int device, void* stream);

/* the Doppler boost of maps (pixell/aberration.py): the values of pixel maps at displaced pixels, and the modulation.
 * pxm_plan_map_points: a plan for the trigonometric interpolation of maps [ny][nx] at npts points (aberration.interpol_map, aberration.py:246-270,
 *   whose ducc0.nufft.u2nu this replaces).  d_pix: DEVICE f64 [{y, x}][npts] in pixels, any finite value (wrapped onto the periodic grid), read
 *   while the plan is made (sorted into the plan).  With g = the map (ydouble = 0, N1 = ny), or the map continued over the pole (ydouble = 1,
 *   N1 = 2 ny: g[ny + r][x] = map[ny - 1 - r][x - nx/2]), N2 = nx and G = fft2(g), the value at (y, x) is
 *   Re sum_{j1, j2} G[j1][j2] exp(2 pi i (k(j1, N1) y / N1 + k(j2, N2) x / N2)) / (N1 N2), k(j, N) = j for j <= (N - 1)/2, j - N above: the whole
 *   band, the Nyquist terms of an even axis split between +N/2 and -N/2 so that real maps give this number with no imaginary part to drop
 *   (two maps travel as one complex grid): half and half, and the corner G[N1/2][N2/2] of two even axes as cos(pi (y + x)).
 *   epsilon in [1e-13, 0.1]: relative L2 accuracy.  N1 and nx must be transformable by the FFT engine.  Synchronises `stream` once.  The plan is
 *   a pxs_plan: pxs_plan_destroy frees it, pxs_plan_query knows "kernel_width", "fine_ntheta", "fine_nphi", "npts", "plan_us" and
 *   "stage_us_fft" / "_grid" / "_interp" as for pxs_plan_points, pxs_plan_option "profile"; pxs_synthesis refuses it.
 * pxm_map_points: d_out[c][i] = the value of map c at point i, for ncomp maps (f32 | f64, ny*nx contiguous pixels each, map_cstride elements
 *   apart) into d_out (f32 | f64, components out_cstride elements apart).  Pairs of maps go through one complex grid each, one pair at a
 *   time: pack (and double), 2-D FFT, deapodise and zero-pad to the fine grid (oversampling 2), inverse FFT, interpolate; the plan keeps
 *   16 B x fine_ntheta x fine_nphi + 16 B x N1 x nx of scratch and 24 B per point.  FP64 arithmetic for both dtypes.  Asynchronous: calls on
 *   one plan from different streams are ordered by the plan's last-use event.  Forward only.
 * pxm_modulate: in place, aberration.apply_modulation (aberration.py:285-354) on ncomp <= 64 maps (f32 | f64, npix contiguous pixels each,
 *   map_cstride elements apart) under the modulation d_A (npix values of the maps' dtype).  mode: PXM_MOD_NONE; PXM_MOD_T2T: map *= A, with
 *   dipole != 0 component 0 gets (A - 1) T0 / map_unit added; PXM_MOD_T2LIN / PXM_MOD_LIN2T: true temperature <-> linearised units (proportional to
 *   flux density at `freq` Hz, about the monopole T0 K, maps in units of map_unit K); PXM_MOD_LIN2LIN: LIN2T under A = 1, then T2LIN.  Bit c of
 *   spin0_mask says component c is a scalar: with dipole != 0 those keep the monopole's own boost (the CMB dipole).  LIN2T takes off
 *   utils.T_cmb = 2.72548 K, not T0, as the reference does.  FP64 arithmetic for both dtypes, differences of Planck functions in closed form. */
enum { PXM_MOD_NONE = 0, PXM_MOD_T2T = 1, PXM_MOD_T2LIN = 2, PXM_MOD_LIN2T = 3, PXM_MOD_LIN2LIN = 4 };
int pxm_plan_map_points(pxs_plan** plan, int ny, int nx, int ydouble, int64_t npts, const double* d_pix, double epsilon, int device, void* stream);
int pxm_map_points(pxs_plan* plan, int ncomp, const void* d_maps, int map_dtype, int64_t map_cstride, void* d_out, int out_dtype, int64_t out_cstride, void* stream);
int pxm_modulate(int64_t npix, int ncomp, void* d_map, int dtype, int64_t map_cstride, const void* d_A, uint64_t spin0_mask,
                 int mode, int dipole, double T0, double freq, double map_unit, int device, void* stream);

/* radially symmetric objects painted into a map, and radial sums read back out around a catalogue (pixell/pointsrcs.py:35-210 sim_objects /
 * radial_sum; cython/srcsim_core.c).  The map is [ncomp][ny][nx] on the separable CAR grid dec0 + y ddec, ra0 + x dra (radians, as in
 * the deflection call above; nx |dra| = 2 pi: the columns wrap), f32 | f64, components map_cstride elements apart.  Pixel and object
 * coordinates are taken as float32; the distance is r = 2 asin sqrt(sin^2(ddec/2) + cos dec cos dec' sin^2(dra/2)).  All arrays DEVICE.
 * pxm_sim_objects: d_obj_dec, d_obj_ra: f32 [nobj]; d_amps: f32 [ncomp][nobj], components amp_cstride apart; d_prof_ids: int32 [nobj] or
 *   NULL (profile 0).  The nprof profiles are laid end to end (nsamp samples in all): profile q is d_prof_rs / d_prof_vs
 *   [d_prof_off[q] .. d_prof_off[q+1]) (d_prof_off: int32 [nprof+1]), rs ascending; d_prof_vmax[k] = max |vs[j]| over the samples j >= k of
 *   the same profile; prof_equi != 0: every profile has rs[k] = k rs[1].  P(r): linear interpolation, vs[0] below rs[0], 0 from the last
 *   sample on.  Object i reaches to rcut_i = rs[min(k+1, n-1)], k the last sample with |vs[k]| >= vmin / max_c |amps[c][i]| (0 if none), capped
 *   by rmax when rmax > 0.  transpose = 0: map[c][p] = op(map[c][p], amps[c][i] P_i(r)) for every object with r <= rcut_i; op: 0 add (in
 *   ascending i), 1 max, 2 min.  The result is the same bit for bit from run to run.  The call waits once for the stream (it reads the total
 *   length of the per-tile object lists back to size them).  transpose != 0 (op 0): d_amps[c][i] += sum_{p: r <= rcut_i} map[c][p] P_i(r),
 *   rcut from the incoming amplitudes; no wait.
 * pxm_radial_sum: d_oprofs[i][c][k] += sum of map[c][p] over the pixels with d_bins[k] <= r < d_bins[k+1] (d_bins: f32 [nbin+1], ascending;
 *   rlast: the value of d_bins[nbin]; equi != 0: d_bins[k] = k d_bins[1]); d_oprofs: f32 [nobj][ncomp][nbin], ncomp nbin <= 12288.  Each pixel
 *   counts once however wide the bins reach. */
int pxm_sim_objects(int ny, int nx, double dec0, double ddec, double ra0, double dra, void* d_map, int map_dtype, int ncomp, int64_t map_cstride,
                    int64_t nobj, const float* d_obj_dec, const float* d_obj_ra, float* d_amps, int64_t amp_cstride, const int32_t* d_prof_ids,
                    int nprof, const int32_t* d_prof_off, int64_t nsamp, const float* d_prof_rs, const float* d_prof_vs, const float* d_prof_vmax,
                    int prof_equi, double vmin, double rmax, int op, int transpose, int device, void* stream);
int pxm_radial_sum(int ny, int nx, double dec0, double ddec, double ra0, double dra, const void* d_map, int map_dtype, int ncomp, int64_t map_cstride,
                   int64_t nobj, const float* d_obj_dec, const float* d_obj_ra, int nbin, const float* d_bins, double rlast, int equi, float* d_oprofs,
                   int device, void* stream);

/* distance transforms (pixell/enmap.py:2127-2215 distance_from / distance_transform / labeled_distance_transform; cython/distances_core.c),
 * on the separable CAR grid dec0 + y ddec, ra0 + x dra of the calls above, FP64 coordinates and arithmetic.  All arrays DEVICE.
 * pxm_find_edges: the edge pixels of d_map [ny][nx] as ascending flat indices.  labeled = 0: d_map is uint8, an edge pixel has value 0
 *   and lies on the border of the array or has a non-zero 4-neighbour; labeled != 0: d_map is int32, an edge pixel is non-zero and lies on
 *   the border or has a 4-neighbour of another value.  d_edges = NULL: only counts; *count (HOST, may be NULL when d_edges is given)
 *   receives the number of edge pixels, and the call waits for the stream to read it.  d_edges: DEVICE int64 [cap], receives the first cap
 *   indices; with count = NULL the call does not wait.  (Count, allocate, fill: two calls, one wait.)
 * pxm_distance_from: d_omap[p] = min_i r(p, i) over the npoint points, r the great-circle distance, exact; d_domains (int32 [ny][nx] or
 *   NULL) the winning i: the comparison is on h = sin^2(ddec/2) + cos dec cos dec' sin^2(dra/2), the lowest i among equal h, and the
 *   winner's distance is evaluated in Vincenty's atan2 form (good on [0, pi]).  Points: d_pt_pix != NULL: int64 [npoint] flat pixel
 *   indices of this grid (the pixel centres); otherwise d_pt_dec, d_pt_ra: f64 [npoint] radians, anywhere on the sphere, RA modulo 2 pi,
 *   duplicates allowed.  rmax > 0: pixels with a distance above rmax get rmax and domain -1 (rmax <= 0: no limit).  npoint = 0: rmax
 *   (infinity without one) and -1 everywhere.  d_skip (uint8 [ny][nx] or NULL): pixels where it is 0 get distance 0 and domain -1 without a
 *   search.  d_omap: f32 | f64 [ny][nx].  d_visits (int32 [ceil(ny/16)][ceil(nx/16)] or NULL): how many points each 16 x 16 pixel tile
 *   looked at (the measure of the pruning: npoint for a brute-force search).  The result is the same bit for bit from run to run; the call
 *   does not wait for the stream. */
int pxm_find_edges(int ny, int nx, const void* d_map, int labeled, int64_t* d_edges, int64_t cap, int64_t* count, int device, void* stream);
int pxm_distance_from(int ny, int nx, double dec0, double ddec, double ra0, double dra, int64_t npoint, const double* d_pt_dec, const double* d_pt_ra,
                      const int64_t* d_pt_pix, double rmax, const uint8_t* d_skip, void* d_omap, int map_dtype, int32_t* d_domains, int32_t* d_visits,
                      int device, void* stream);

/* spline interpolation of maps at positions (pixell/utils.py:630-783 interpol / SplineInterpolator: scipy.ndimage.spline_filter, then
 * map_coordinates(prefilter=False); enmap.at, enmap.project, enmap.py:561-638, 796-842).  All arrays DEVICE, FP64 arithmetic, no wait.
 * pxm_spline_filter: the cubic B-spline coefficients of nmap maps [ny][nx] (f32 | f64, in_mstride elements apart) into d_out, f64
 *   [nmap][ny][nx]: along each axis the solution of B c = f, B the (1/6, 4/6, 1/6) collocation matrix under the extension rule
 *   0 whole-sample mirror (period 2(n-1)), 1 half-sample reflect (period 2n), 2 periodic.  d_tmp: f64 [nmap][ny][nx] scratch of the
 *   caller's (the y pass writes it, the x pass reads it); the input, the scratch and the output are three different arrays.
 * pxm_interpol: d_out[m][i] = the value of map m at point i, in the maps' dtype.  order 0: the nearest sample, maps f32 | f64 | uint8
 *   (code 4) | int32 (code 5); order 1: linear, f32 | f64 maps; order 3: cubic, d_maps being the f64 coefficients of pxm_spline_filter.
 *   Point i is (d_pts[i], d_pts[npts + i]) (f64 [2][npts]) or, with d_pts = NULL, (i / onx, i % onx) of a grid [ony][onx] with
 *   ony onx = npts.  Its pixel coordinate on each axis is off + scale p, then, where per > 0, ref + ((pix - ref + per/2) mod per) - per/2
 *   (enmap.sky2pix(safe=True), enmap.py:509-519).  border (n the axis length, x the coordinate): 0 "nearest": tap indices clamped to
 *   [0, n-1]; 1 "mirror": indices mirrored with period 2(n-1); 2 "constant": cval where x < 0 or x > n-1 on an axis, indices mirrored;
 *   3 "wrap" (scipy's legacy rule): x outside [0, n-1] folded with period n-1, indices mirrored; 4 "grid-wrap": indices modulo n.  Taps:
 *   floor(x + 1/2) (order 0), floor(x), floor(x) + 1 (order 1), floor(x) - 1 .. floor(x) + 2 (order 3).  A coordinate that is not a number
 *   gives cval.
 * pxm_spline_filter_axes: pxm_spline_filter with one extension rule per axis (a map that goes round the sky: periodic along x, mirror along
 *   y); pxm_spline_filter is this call with its rule given twice. */
int pxm_spline_filter(int nmap, int ny, int nx, const void* d_in, int in_dtype, int64_t in_mstride, double* d_tmp, double* d_out, int extension,
                      int device, void* stream);
int pxm_interpol(int nmap, int ny, int nx, const void* d_maps, int map_dtype, int64_t mstride, int64_t npts, const double* d_pts, int ony, int onx,
                 double yoff, double yscale, double xoff, double xscale, double yref, double yper, double xref, double xper,
                 int order, int border, double cval, void* d_out, int device, void* stream);
int pxm_spline_filter_axes(int nmap, int ny, int nx, const void* d_in, int in_dtype, int64_t in_mstride, double* d_tmp, double* d_out,
                           int extension_y, int extension_x, int device, void* stream);

/* catalogue cut-outs (pixell/reproject.py:10-116 thumbnails / thumbnails_ivar, with coordinates.recenter and the polarisation angle of
 * coordinates.transform(pol=True), coordinates.py:25-122, 289-305).  All arrays DEVICE, FP64 arithmetic, no wait (the first call of a
 * stream, or a larger thumbnail than any before on it, allocates the direction table).
 * pxm_thumbnails: d_out[o][m][j][i] = map m, interpolated, where thumbnail pixel (j, i) lies once the thumbnail's centre is put on object o;
 *   d_out: [nobj][nmap][oy][ox] in the maps' dtype.  Maps, dtypes, order, the affine map from (dec, ra) in radians to pixels and the rewind
 *   (ref, per): as in pxm_interpol.  d_obj: f64 [nobj][2] = (dec, ra) in radians.  The thumbnail geometry has crval = (0, 0): pixel (j, i)
 *   has the intermediate coordinates x = (i + 1 - crpix_x) cdelt_x, y = (j + 1 - crpix_y) cdelt_y in degrees and the direction
 *   v = unit vector of (dec = y, ra = x) (proj 0, CAR) or v = (1, x, y)/|.| with x, y in radians (proj 1, TAN: gnomonic about (0, 0)).
 *   Object o at (dec_o, ra_o) turns it into V = Rz(ra_o) Ry(-dec_o) v, read at dec = atan2(V_z, hypot(V_x, V_y)), ra = atan2(V_y, V_x).
 *   border_y, border_x: the border codes of pxm_interpol, one per axis.  A pixel whose position is not a number, or outside a "constant"
 *   axis, gets cval in every map.  pol != 0: components qcomp and ucomp (different, in [0, nmap), float maps) are rotated by -2 psi,
 *   Q' = cos 2psi Q + sin 2psi U, U' = -sin 2psi Q + cos 2psi U, psi = atan2(Re . N, Re . E) the angle of the rotated east vector e of
 *   the thumbnail pixel in the (east, north) frame of the sky position (enmap.rotate_pol(., -psi), reproject.py:93-101); pixels that got
 *   cval are not rotated.  nobj times the workgroups per thumbnail (ceil(oy ox / 256)) must stay below 2^31. */
int pxm_thumbnails(int nmap, int ny, int nx, const void* d_maps, int map_dtype, int64_t mstride,
                   double yoff, double yscale, double xoff, double xscale, double yref, double yper, double xref, double xper,
                   int64_t nobj, const double* d_obj, int oy, int ox, int proj, double cdelt_y, double crpix_y, double cdelt_x, double crpix_x,
                   int order, int border_y, int border_x, double cval, int pol, int qcomp, int ucomp, void* d_out, int device, void* stream);

/* healpix pixel arithmetic (RING scheme, any nside >= 1, Gorski et al. 2005) and healpix <-> CAR reprojection by interpolation
 * (pixell/reproject.py:118-361 map2healpix / healpix2map with method="spline": healpy.pix2ang / ang2pix / get_interp_val,
 * coordinates.transform_euler, enmap.at, enmap.rotate_pol).  All arrays DEVICE unless marked HOST, int64 pixel indices, FP64 arithmetic,
 * no wait.  theta is the colatitude, phi the longitude, radians; phi is taken modulo 2 pi.
 * pxm_healpix_index: mode 0: d_out (f64 [2][n]) = (theta, phi) of the centres of the pixels d_pix_in [n] (not a number for a pixel
 *   outside [0, 12 nside^2)); mode 1: d_pix_out [n] = the pixel that holds (d_theta[i], d_phi[i]) (-1 where they are not numbers);
 *   mode 2: d_pix_out [4][n] and d_out (f64 [4][n]) = the four pixels and weights of the ring-bilinear value there: the two pixels
 *   around phi on the ring above the point and on the ring below, linear in phi on each ring and in theta between them; north of the
 *   first ring (south of the last) the four pixels of that ring share the polar part equally.  Weights are >= 0 and sum to 1.
 * pxm_healpix_interp: d_out[m][i] = map m (ncomp maps [12 nside^2] of f32 | f64, mstride elements apart) at point i: the pixel that
 *   holds it (order 0) or the ring-bilinear value (order 1), in the maps' dtype; not a number where the point is not a number.
 * pxm_map2healpix: d_out[m][i] = scale times map m at the centre of healpix pixel first + i, i < n, interpolated; d_out: [ncomp] rows
 *   ostride elements apart, f32 | f64 by out_dtype (the maps' dtype, or f32 from f64 maps).  Maps, dtypes, order, the affine map from
 *   (dec, ra) in radians to pixels and the rewind (ref, per): as in pxm_interpol; border_y, border_x: as in pxm_thumbnails (a pixel
 *   outside a "constant" axis gets scale cval in every map).  rot (HOST, nine doubles, row-major, or NULL): the centre's direction n is
 *   read at M n, and every pair is rotated by -spin psi, a' = cos(spin psi) a + sin(spin psi) b, b' = -sin(spin psi) a + cos(spin psi) b,
 *   psi = atan2(M e_ra(n) . e_dec(M n), M e_ra(n) . e_ra(M n)) (enmap.rotate_pol(., -psi, spin), reproject.py:239-243).  pairs (HOST,
 *   int [npair][2]): (first component, spin) of the pairs (c, c + 1), which do not overlap; without rot they have no effect.
 *   ncomp <= 32.
 * pxm_healpix2map: d_out[m][y][x] = healpix map m at pixel (y, x) of the separable geometry dec = dec0 + y ddec, ra = ra0 + x dra
 *   (wcs.separable_geometry), order 0 | 1 as in pxm_healpix_interp, times d_rowfac[y] (f64 [ny], or NULL); rot and pairs as in
 *   pxm_map2healpix, with n the direction of the output pixel.  d_out in the maps' dtype.  ncomp <= 32. */
int pxm_healpix_index(int mode, int64_t nside, int64_t n, const int64_t* d_pix_in, const double* d_theta, const double* d_phi, int64_t* d_pix_out, double* d_out,
                      int device, void* stream);
int pxm_healpix_interp(int64_t nside, int ncomp, const void* d_maps, int map_dtype, int64_t mstride, int64_t n, const double* d_theta, const double* d_phi,
                       int order, void* d_out, int device, void* stream);
int pxm_map2healpix(int ncomp, int ny, int nx, const void* d_maps, int map_dtype, int64_t mstride,
                    double yoff, double yscale, double xoff, double xscale, double yref, double yper, double xref, double xper,
                    int order, int border_y, int border_x, double cval, int64_t nside, int64_t first, int64_t n, const double* rot,
                    int npair, const int* pairs, double scale, void* d_out, int out_dtype, int64_t ostride, int device, void* stream);
int pxm_healpix2map(int ncomp, int64_t nside, const void* d_maps, int map_dtype, int64_t mstride, int ny, int nx, double dec0, double ddec, double ra0, double dra,
                    int order, const double* rot, int npair, const int* pairs, const double* d_rowfac, void* d_out, int device, void* stream);

/* connected components, per-label reductions and the per-pixel solve of the source finder (pixell/analysis.py:553-564: scipy.ndimage.label,
 * center_of_mass, maximum; :1052-1060 solve_mapsys: np.linalg.solve / inv per pixel).  All arrays DEVICE unless marked HOST.
 * pxm_label: d_labels (int32 [ny][nx], 16-byte aligned) = 0 where d_mask (uint8 [ny][nx]) is 0 and 1 .. n on its n connected components,
 *   numbered in ascending order of their lowest flat pixel index (scipy.ndimage.label's numbering: a raster-order flood fill): a pure
 *   function of the mask, the same bit for bit from run to run.  connectivity 1: 4-neighbours, 2: 8-neighbours.  wrap_x = 1: column nx-1
 *   is a neighbour of column 0.  ny nx < 2^31.  *count (HOST, may be NULL) receives n, and the call waits for the stream to read it.
 * pxm_label_stats: reductions over the pixels of every label 1 .. nlabel of d_labels (int32 [ny][nx], values 0 .. nlabel, 0 is skipped, from
 *   any source).  d_v, d_w: value and weight maps [ny][nx], f32 | f64 each by its dtype code, or NULL (w = 1; without d_v: sum_v 0, vmax
 *   and vmin NaN, the args -1).  Per label l, at index l-1: d_count (int64) pixels; d_box (int32 [4][nlabel]) ymin, ymax, xmin, xmax;
 *   d_sums (f64 [4][nlabel]) sum w, sum w y, sum w x, sum v; d_vmax, d_vmin (f64) and d_argmax, d_argmin (int64: the lowest flat index
 *   that holds the value; -0 counts as +0).  A label without pixels: count 0, box (ny, -1, nx, -1), NaN, -1.  Everything but the four
 *   sums is independent of the order of execution; the sums are FP64 atomic adds in arrival order.  A label outside 0 .. nlabel makes the
 *   call fail (that pixel is skipped, nothing is written out of range).  The call waits for the stream to learn this.
 * pxm_solve_mapsys: d_flux[a][p] = (K_p^-1 r_p)[a], d_dflux[a][p] = sqrt((K_p^-1)[a][a]) for K_p[a][b] = d_kappa[a][b][p] and
 *   r_p[a] = d_rho[a][p], p < npix, n = 2 .. 8 (others: unsupported); all four arrays of one dtype, f32 | f64, FP64 arithmetic:
 *   Gauss-Jordan elimination with partial pivoting.  A pixel with a zero pivot gets NaN in all its outputs.  No wait. */
int pxm_label(int ny, int nx, const void* d_mask, int connectivity, int wrap_x, int32_t* d_labels, int64_t* count, int device, void* stream);
int pxm_label_stats(int ny, int nx, const int32_t* d_labels, int64_t nlabel, const void* d_v, int v_dtype, const void* d_w, int w_dtype,
                    int64_t* d_count, int32_t* d_box, double* d_sums, double* d_vmax, double* d_vmin, int64_t* d_argmax, int64_t* d_argmin,
                    int device, void* stream);
int pxm_solve_mapsys(int n, int64_t npix, const void* d_kappa, const void* d_rho, void* d_flux, void* d_dflux, int dtype, int device, void* stream);

/* 1 if the engine can transform this length (2,3,5-smooth or prime factors small enough) */
int pxf_fft_supported(int64_t n);
int64_t pxf_fft_good_size(int64_t n);

/* Device memory of the library.  Plans release their scratch into a per-process arena (blocks >= 32 MB, at most PXS_ARENA_GB = 48 GB
 * kept) that the next plan draws from, so that dropping and rebuilding plans does not go through hipMalloc again.  release != 0: give
 * the kept blocks back to the driver now.  stats (may be null): [0] ms spent in hipMalloc so far, [1] hipMalloc calls, [2] bytes they
 * allocated, [3] requests served from the arena, [4] bytes kept in the arena now, [5] bytes in use by plans.  No reference counterpart
 * (ducc0 allocates host memory per call). */
int pxs_memory(int release, double* stats);

const char* pxs_last_error(void);
const char* pxs_version(void);

#ifdef __cplusplus
}
#endif
#endif
