// Device-side pieces shared by the Legendre translation units (legendre.hip: host side, alm kernels, tables; leg_s0.hip: spin-0 kernels;
// leg_spin.hip: spin-s kernels): kernel arguments, block -> (m, ring chunk) order, extended-exponent helpers, the pair map, the lane-sum
// reduction tile of the VALU analysis kernels, the MFMA helpers and the two bodies of the four batched kernels (leg_ana_mm, leg_syn_mm; the
// spin-0 / spin-s side is a policy defined next to the kernels) and the launch helper.  The four VALU kernels keep a copy of the phase skeleton
// each, held together by the macros at the head of leg_s0.hip and leg_spin.hip (leg_spin.hip says why).  Design notes: head of legendre.hip.
#pragma once
#include "legendre.hpp"
#include <cmath>
#include <algorithm>
#include <initializer_list>

namespace pxs {

static constexpr double SC_BIG   = 0x1p+400;
static constexpr double SC_SMALL = 0x1p-800;
static constexpr int    SC_STEP  = 800;
// A chain counts as LIVE -- its wave or workgroup leaves phase A and starts the full-cost accumulating steps -- when it is at scale 0
// AND its value has reached LEG_LIVE.  (Until this constant existed, scale 0 alone did: the largest |lambda| of the wave was then about
// 2^-400, and the steps from there to ~2^-100 of the final size ran at full cost on terms nobody can see: 3.9 % of the accumulating
// steps of a lmax 10^4 transform.)
// The bound.  Phase A tests once per 4 steps, so what a wave drops are the values of a chain at the test that found it below LEG_LIVE
// and at the three steps after it (the value after the fourth step is tested again).  A chain value is the normalised lambda over
// the step's alpha (LegTables::alpha, folded into the pre-scaled alm and the moments), so |lambda| = |value| |alpha|.
//  * Growth.  Below its turning point lambda_lm grows monotonically and one degree multiplies it by less than x / eps_{l+1} <
//    x sqrt(2 m / (l - m)), x = cos(theta).  A chain that starts AT scale 0 has sin^m(theta) >= 2^-400, so m x^2 / 2 <~ 400 ln 2 and
//    2 m x^2 < 1110 whatever m is: three spin-0 steps (6 degrees) grow it by < 1110^3 / sqrt(6!) < 2^26, four by < 1110^4 / sqrt(8!)
//    < 2^33; spin-s steps are one degree each and grow less.  (The "< 2^60 in 4 steps" of the phase-A comment below is the bound
//    for ANY chain, x = 1 at m = 6 10^4: it guards the overflow, where chains below scale 0 count too.  The 2^30 one can read off a
//    lmax 10^4 table next to l = m is the same thing as the 2^33 here, seen at one size.)
//  * |alpha| <= alpha_0 = sqrt(2 m + 3) c_m ~ 0.6 m^(3/4): 2^9 at m = 10^4, < 2^12 up to m = 10^5; it falls like 1/k from there.
//  So every dropped term has |lambda| < 2^-140 2^26 2^12 = 2^-102 < 2^-100 up to lmax 10^5.  Counted over every chain of the lmax 10^4
//  ring set (the chains that come up from below scale 0 included; tools/leg_live_count.cpp): largest 4-step growth 2^32.3 (spin 0),
//  2^18.6 (spin 2); largest dropped |lambda| 2^-111.8 (spin 0), 2^-126.8 (spin 2), and 2^-110.3 / 2^-126.4 at lmax 4 10^4.  2^-130 leaves
//  2^-102.1 and 2^-100.6 at those two sizes -- no margin -- and saves 0.2 % more steps; 2^-140 it is.
// A synthesised pixel is therefore off by less than nl 2^-100 max|a_lm| and an analysis moment by less than nring 2^-100 max|ring data|:
// absolute errors, relative to the input's largest value, not to the pixel's or moment's own size.
// Phase B's per-lane join is unchanged (scale 0).  The constant is compile-time: seeds, both directions and all eight kernels
// start under the same rule within a process by construction.
static constexpr double LEG_LIVE = 0x1p-140;
#define LEG_IS_LIVE(v, sc) ((sc) == 0 && fabs(v) >= LEG_LIVE)

// Block starts.  A wave holds K blocks of 64 ring pairs, block K - 1 the most equatorial.  It leaves phase A when its first chain is live, which is almost always one of
// block K - 1; the more polar blocks then hold zeros or values below LEG_LIVE for hundreds of steps more.  Every block runs its recurrence FMAs from the wave's
// start on, but its ACCUMULATION FMAs (4 of 6 per step for spin 0, 8 of 12 for spin s) only from its own start: the first 4-step test, counted from the wave's
// start, at which one of its own chains or a chain of a more polar block of the wave is live (leg_live_upto; tools/leg_live_count.cpp, column (c), is the same rule on
// the CPU).  Starts are wave-uniform and monotone -- block K - 1 with the wave, then K - 2, ... -- so a wave runs its phases B and C as a sequence of loops
// compiled for NB = 1 .. K started blocks (the *_ANA_STAGE macros of leg_s0.hip / leg_spin.hip), switching at a 4-step test; loop NB = K is the former loop.  What
// this drops is bounded as what LEG_LIVE drops (above): values of chains that are not live.  An analysis block fetches its ring data when it starts.
// The ANALYSIS kernels do this.  Measured on MI355X at C3, parent and result alternating (profiles/README.md, "Block starts", table "the tree as it is"): leg_ana
// 112.03 -> 109.25 ms per step (spreads 0.50 / 0.58), C2 leg_ana 8.71 -> 8.26.  The synthesis kernels were built the same way, passed the same tests and came out level
// (same section, table "all four kernels gated": leg_syn 84.62 -> 84.11 ms at spreads of 1.0 / 1.1, leg_syn_spin<3> 68.48 -> 69.05 ms in the kernel trace) with fewer blocks per wave to gate (K = 4 / 3); they keep the one loop
// for all blocks, and the seed tail of a synthesis record is written (LEG_NEVER) and not read.
// Seeded launches read the starts off the seed record instead of testing: the last 64 ints of a (wave, m) record held the step reached in [0] and nothing else;
// [1 + c] now holds the start step of block c (LEG_NEVER: none), written by lane c + 1 both times so that the two stores stay in order.  No byte is added.
#define LEG_NEVER 0x7fffffff
template<int C, int K> __device__ __forceinline__ bool leg_live_upto(const double (&v)[K], const int (&sc)[K]) {
	bool act = false;
#pragma unroll
	for (int s = 0; s <= C; s++) act |= LEG_IS_LIVE(v[s], sc[s]);
	return act;
}

struct double4_t { double a, b, c, d; };
// Wave-uniform table rows are fetched through the constant address space: that makes them scalar loads (s_load_dwordx8)
// even in kernels that also store to global memory inside their loops.  Without it the analysis kernels, whose flush
// stores precede later row loads, got per-lane global_load broadcasts for every coefficient row (SQ_INSTS_SMEM 5.5e7
// against SQ_INSTS_VMEM_RD 2.2e9 for leg_ana_spin<6> at config 3; the synthesis kernels had 4e9 scalar loads).
#ifdef PXS_HOST_SIM
#define LDC(p, i) ((p)[i])
#else
typedef double pxs_d4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ double4_t ldc_row(const double4_t* p, long i) {
	const __attribute__((address_space(4))) pxs_d4* c = (const __attribute__((address_space(4))) pxs_d4*)(unsigned long long)p;
	const pxs_d4 v = c[i]; double4_t r; r.a = v.x; r.b = v.y; r.c = v.z; r.d = v.w; return r;
}
#define LDC(p, i) ldc_row((p), (i))
#endif
// one double of a wave-uniform table through the constant address space (s_load_dwordx2)
#ifdef PXS_HOST_SIM
#define LDCD(p, i) ((p)[i])
#else
__device__ __forceinline__ double ldc_double(const double* p, long i) {
	const __attribute__((address_space(4))) double* c = (const __attribute__((address_space(4))) double*)(unsigned long long)p;
	return c[i];
}
#define LDCD(p, i) ldc_double((p), (i))
#endif

// Row prefetch in phase C of the spin-0 synthesis (leg_syn_s0).  A wave needs (a, b') of a step, b' = b or, in a polar wave, a + b: 16 bytes from the compact tables
// LegK::coef2 / coef2p, two steps in one s_load_dwordx8.  Scalar loads return out of order, so the only wait there is for any of them is lgkmcnt(0), and it drains
// whatever was requested a moment ago too: left to the compiler, the rows of the next step pair were requested at the bottom of the loop body and awaited at its top
// (the per-step s_cselect between the polar and the plain column read a freshly loaded row), and every trip exposed a scalar-load latency.  The loop now has ONE
// drain per step pair, PXS_ROWS_DRAIN, with the rows of the NEXT pair (table and pre-scaled alm) requested right behind it -- up to PXS_ROWS_ISSUED nothing else is
// scheduled -- and nothing but the rows that were complete at the drain read before the next one: a full step pair of the wave's FMAs lies between request and wait
// (tools/leg_prefetch_distance.py reads the distances off the assembly: 0-4 FMAs before, 12 K after).  The arithmetic is the same expression on the same values in
// the same order.  Measured on MI355X at C3, parent and result in one session, launches with the seeds loaded (profiles/leg_prefetch_ab.txt): leg_syn_s0<4>
// 20.29 -> 16.89 ms, its waitcnt share of the wave cycles 46 -> 25 %.
// The other three VALU kernels run the same loop.  leg_ana_s0 reads the compact rows too; the spin-s kernels read the 32-byte rows, of which polar waves need the
// columns a, c, d (a loop of their own for plain waves on the compact rows cost a wave per SIMD: leg_spin.hip, "Row sets").  The analysis kernels have the drain
// BETWEEN the two steps of a pair -- the ds_writes of the reduction count on lgkmcnt too and are a step old there -- and flush a full tile at that drain; a row set
// there spans the second step of a pair and the first of the next.  The flush is conditional, and a scheduling barrier holds within its basic block only: PXS_DONE
// keeps the FMAs of the step in front of the drain in front of it.  Every load has its step pair of distance (24 K / 12 K FMAs), results are bit for bit what the
// former loops gave.  When first built, at 3-4 waves per SIMD, these three loops gained 0.6-1.4 ms each at C3, at or inside three times the spread: the waitcnt share
// fell (leg_syn_spin<3> 29 -> 19 %, leg_ana_spin<4> 16 -> 7 %, leg_ana_s0<8> 21 -> 12 %) and the issue stalls rose by as much, the other waves of the SIMD already
// issuing into most of the time one wave waits.  They are what lets the analysis run at TWO waves per SIMD with more ring pairs per lane (leg_ana_k, legendre.hip);
// figures: profiles/README.md, "Analysis K".
struct coef2x2_t { double a0, b0, a1, b1; };
#ifdef PXS_HOST_SIM
#define LDC2(p, i) (coef2x2_t{(p)[i].x, (p)[i].y, (p)[(i)+1].x, (p)[(i)+1].y})
#define PXS_ROWS_DRAIN()
#define PXS_ROWS_ISSUED()
#else
typedef double pxs_d4a16 __attribute__((ext_vector_type(4), aligned(16)));
__device__ __forceinline__ coef2x2_t ldc_row2(const double2* p, long i) {
	const __attribute__((address_space(4))) pxs_d4a16* c = (const __attribute__((address_space(4))) pxs_d4a16*)(unsigned long long)(p + i);
	const pxs_d4a16 v = *c; coef2x2_t r; r.a0 = v.x; r.b0 = v.y; r.a1 = v.z; r.b1 = v.w; return r;
}
#define LDC2(p, i) ldc_row2((p), (i))
// s_waitcnt lgkmcnt(0) (vmcnt and expcnt left open), as an instruction the compiler's own wait insertion sees
#define PXS_ROWS_DRAIN() do { __builtin_amdgcn_s_waitcnt(0xc07f); __builtin_amdgcn_sched_barrier(0); } while (0)
#define PXS_ROWS_ISSUED() __builtin_amdgcn_sched_barrier(0)
#endif
// A per-lane double that has to be computed by this point.  The analysis kernels put their conditional flush behind the drain, and a scheduling barrier holds within
// its basic block only: without this the compiler sinks the FMAs of the step in front of the drain past the flush's branch, and the rows they read stay live across
// the point where the next ones are to be requested (the requests then follow a step late).  No instruction.
#ifdef PXS_HOST_SIM
#define PXS_DONE(x)
#else
#define PXS_DONE(x) asm volatile("" : "+v"(x))
#endif

struct LegK {
	int lmax, mmax, spin, nm, npairs, nring, nwave;
	long ld;                            // row stride of leg[m][ring] (>= nring; rows padded to whole 128-byte lines)
	long nrows;
	const long* row; const double4_t* coef; const double* alpha;
	const int* ring_n; const int* ring_s; const double* cth; const double* sth; const double* sh2; const double* ch2;
	double* almt; double* part; double* mom;
	double2* leg;
	double ofs;
	int m0; long rowbase, rows_chunk;   // analysis processes m in chunks to bound the partial-moment scratch
	int nmc, xcd;                       // m count of this launch; XCD-aware block order on/off
	int* first;                         // analysis: see LegWork::first
	int atomic;                         // analysis: waves add their sums into mom (part = mom) instead of writing per-wave partial moments
	// recurrence seeds: the state of every chain at the end of phase A, per (m, wave): [nd][K][64] doubles, [ni][K][64] + 64 ints
	// (the first of the last 64: the step reached).  mode 0: off, 1: run phase A and record, 2: load instead of running it
	int seed_mode; double* seed_d; int* seed_i;
	// executed-work counters (profiling on: pxs_profile; null otherwise): per slot count[0] synthesis, count[1] analysis (wave counts), count[2], count[3] (not executed; PXS_COUNT_AT), in FMA instructions
	// per lane: every wave adds (steps it ran) x K x (recurrence FMAs per ring pair and step: 2 per two degrees for spin 0, 4 per degree for spin s; phase A
	// included where it ran) + per block (steps from the block's start) x (accumulation FMAs: 4 / 8).  x 64 lanes x 2 = the FP64 flops the hardware executed in
	// the recurrences and accumulations (rings dropped as polar-dead and (wave, m) pairs skipped entirely are not in it, masked-off lanes are).
	double* count;
	// maps of a batched call in one launch: the waves of one m of ALL maps sit next to each other in an XCD's queue, so the maps
	// share the coefficient rows in L2 and the scalar cache.  Strides in elements of leg (double2), almt and mom (double).
	int nb; long leg_bs, almt_bs, mom_bs;
	int nmaps;                          // MFMA kernels (leg_ana_s0_mm): nb counts GROUPS of maps there, nmaps the maps themselves
	const double2* coef2; const double2* coef2p;      // compact step tables (a, b) / (a, a + b; spin 0) (LegTables::d_coef2): phase C of the non-polar VALU waves, the MFMA kernels
};
// (PXS_NCOUNT slots, one picked by the block index: 200 000 waves adding to ONE address cost ~10 ms per C3 step and 24 ms per C4 step)
#define PXS_NCOUNT 1024
// A slot holds four sums: [dir] the wave count -- every block of a wave counted with all its FMAs from the wave's start, the figure pxs_profile_flops has always
// reported and bench.py and tests/test_leg_ana_blocks.py set against the model's column (b) -- and [2 + dir] what of it was NOT executed: the accumulation FMAs of
// the blocks of the analysis kernels between the wave's start and their own ("Block starts" above).  Wave count minus that is the executed count, column (c): plan
// query "leg_executed_flops_ana".  A kernel whose blocks all start with the wave adds to [dir] alone, one atomic per wave as before.
#ifdef PXS_HOST_SIM
#define PXS_COUNT_AT(i, expr) if (a.count != nullptr && lane == 0) atomicAdd(a.count + 4*(blockIdx.x & (PXS_NCOUNT - 1)) + (i), (double)(expr))
#else
#define PXS_COUNT_AT(i, expr) if (a.count != nullptr && lane == 0) unsafeAtomicAdd(a.count + 4*(blockIdx.x & (PXS_NCOUNT - 1)) + (i), (double)(expr))
#endif
#define PXS_COUNT(dir, expr) PXS_COUNT_AT(dir, expr)
// ... of the kernels with block starts, at the wave's start: wave count = the recurrence FMAs `rec` (every block, from here on, and phase A where it ran) + the accumulation
// FMAs `acc` of each of the K blocks from here on; not executed: those of K - 1 blocks (block K - 1 starts with the wave), less what a block still runs when it starts
// (PXS_COUNT_BLOCK: its accumulation FMAs from there on)
#define PXS_COUNT2(dir, rec, acc, K_) { PXS_COUNT_AT(dir, (rec) + (K_)*(acc)); if ((K_) > 1) PXS_COUNT_AT(2 + (dir), ((K_) - 1)*(acc)); }
#define PXS_COUNT_BLOCK(dir, acc) PXS_COUNT_AT(2 + (dir), -(acc))

// Block -> (m, ring chunk).  Every wave of one m streams the same coefficient rows (32 B per l) through the
// scalar cache; workgroups are dealt round-robin to the 8 XCDs, each with a private L2.  With the plain
// (chunk, m) grid the nwave readers of a stream were spread over all XCDs and drifted apart, and FETCH_SIZE
// showed every one of them going to the fabric (49 GB per leg_syn_spin launch at config 3 = nwave x the
// table).  This order gives all chunks of one m the same `block % 8`, back to back in that XCD's queue, so
// one reader misses and the others hit in L2.
// (Workgroups of 2-4 independent waves of the same m -- to share the rows in the CU's scalar cache -- were measured twice:
// with __launch_bounds__(256) and the lane taken as threadIdx.x & 63 every kernel got slower even at one wave per workgroup
// (config 3: leg_syn 106 -> 113 ms, leg_ana 144 -> 151 ms), 4 waves per workgroup 128 / 165 ms.  One wave per workgroup stays.
// A third time with the waves per workgroup NW a template parameter of the four VALU kernels, so that NW = 1 compiles to the code below, NW waves on
// adjacent chunks of one m, one reduction tile per wave: FETCH_SIZE fell (C3, NW = 4: leg_syn_s0<4> 14.3 -> 10.4 GB per launch, leg_ana_spin<4>
// 8.6 -> 7.8, leg_syn_spin<3> 25.5 -> 24.0) but the time did not follow it: C3 -7 % to +11 % per kernel at NW = 2 / 4 and up to +50 % at NW = 8, lmax 8000
// up to +21 % (leg_ana_spin<4>, NW = 4), C2 +5 %; a workgroup needs NW free wave slots on one CU at once, and the waves of a group end far apart.
// Where grouping had gained it had made the number of blocks per m odd (C3, NW = 4: 20 chunks in 5 groups; where it lost, even: C2: 8 in 2):
// that is what leg_blocks_per_m now does for one wave per workgroup, and with it no NW > 1 is ahead.  profiles/README.md, "Wave groups".)
// An m takes an ODD number of blocks: with an even count of chunks and maps, nwave nb, one block more that returns at once (leg_blocks_per_m).  The
// chunks of an m differ in cost by an order of magnitude -- the equatorial ones run every step, the polar ones few or none -- and an XCD deals its
// queue to its shader engines and CUs in turn: with an even period the heavy chunks of every m meet the same part of the XCD, the light ones the
// rest, and the kernel ends on the heavy part alone; an odd period walks through them.  (The cause is inferred from the rule, not read off a counter;
// the rule is what is measured: odd counts are faster at every size tried.)  Measured on MI355X, kernel by kernel against the even count
// (profiles/README.md, "Wave groups"): C3 (20 chunks of 256 pairs) leg_ana_spin<4> 96.8 -> 92.5 ms, leg_ana_s0<8> (10 chunks) 25.3 -> 24.4,
// leg_syn_s0<4> 21.5 -> 20.5, leg_syn_spin<3> (27 chunks, odd before) level; lmax 8000: -5 %, -9 %, -1 %; C2: -11 %, -9 %, +1 %.  What a wave
// computes and where it puts it is keyed on wv and untouched.
__host__ __device__ constexpr unsigned leg_blocks_per_m(unsigned nwave, unsigned nb) { return (nwave*nb) | 1u; }
static_assert(leg_blocks_per_m(20, 1) == 21 && leg_blocks_per_m(27, 1) == 27 && leg_blocks_per_m(4, 8) == 33 && leg_blocks_per_m(3, 2) == 7, "blocks per m: odd, at most one more than chunks x maps");
__device__ __forceinline__ bool leg_block(const LegK& a, int& wv, int& m, int& bb) {
	if (!a.xcd) { wv = blockIdx.x; m = blockIdx.y + a.m0; bb = blockIdx.z; return true; }
	const unsigned b = blockIdx.x, x = b & 7u, j = b >> 3;
	const unsigned per_m = leg_blocks_per_m((unsigned)a.nwave, (unsigned)a.nb);
	const unsigned ml = j / per_m, r = j - ml*per_m;
	bb = (int)(r / (unsigned)a.nwave);
	wv = (int)(r - (unsigned)bb*a.nwave);
	const unsigned mi = ml*8u + x;
	m = (int)mi + a.m0;
	return mi < (unsigned)a.nmc && bb < a.nb;      // (bb == nb: the block that makes the count odd)
}
static inline dim3 leg_grid(const LegK& a) { return a.xcd ? dim3((unsigned)(8*((a.nmc+7)/8)*leg_blocks_per_m(a.nwave, a.nb))) : dim3(a.nwave, a.nmc, a.nb); }

// ---------------------------------------------------------------------------------
// scaled powers
// ---------------------------------------------------------------------------------
__device__ __forceinline__ void frexp_norm(double& m, int& e) { int d; m = frexp(m, &d); e += d; }

// x^n as mant * 2^e, mant in [0.5,1) (or 0)
__device__ __forceinline__ void pow_scaled(double x, int n, double& mant, int& e) {
	double rm = 0.5; int re = 1;
	int be = 0; double bm = frexp(x, &be);
	while (n) {
		if (n & 1) { rm *= bm; re += be; frexp_norm(rm, re); }
		bm *= bm; be *= 2; frexp_norm(bm, be);
		n >>= 1;
	}
	mant = rm; e = re;
}
// value = mant*2^e  ->  v*2^(800*scale), scale <= 0, |v| <= 2^400
__device__ __forceinline__ void to_scaled(double mant, int e, double& v, int& scale) {
	if (mant == 0.0) { v = 0.0; scale = 0; return; }
	int s = (e >= 0) ? (e + SC_STEP/2)/SC_STEP : -((-e + SC_STEP/2)/SC_STEP);
	if (s > 0) s = 0;
	v = ldexp(mant, e - SC_STEP*s); scale = s;
}

// A wave is 'polar' when all its rings have cos^2 > PXS_POLAR_COS2: it then runs the recurrences in the variable -sin^2(theta) (spin 0) or
// -2 sin^2(theta/2) (spin s) instead of cos^2(theta) or cos(theta), with the step coefficient adjusted accordingly (table columns c,d).  This keeps full relative precision near the
// poles, where x = cos(theta) rounds away the information about theta: there the recurrence sits at its double root (step coefficient
// 2 - (l theta)^2-ish) and an ABSOLUTE error eps in the coefficient grows like l^2 eps -- 4e-13 of the map rms on the rings next to the poles at
// lmax 240, 3e-12 at lmax 600 (tests/test_grid_fuzz.py found it), against 1e-14 elsewhere.  The form is exact algebra for every ring but cancels
// towards the equator (a (1 - sin^2) + b: the spin-0 equator ring of a wave forced into it went from 4e-14 to 7e-13 at lmax 240), so a wave takes it
// only if its MOST EQUATORIAL ring still has cos^2 > 0.1 (theta < 71.5 deg: at most one digit of the coefficient).  Until round 5 the bound was 1/2:
// a wave spans 256-512 ring pairs, so grids below 1024-2048 rings -- and the CC-grid detour of the synthesis up to lmax ~2000 -- never ran their
// polar rings in this form; with 0.1 that shrinks to 644-1288 rings (below which l^2 eps stays under ~4e-12).
#ifndef PXS_POLAR_COS2
#define PXS_POLAR_COS2 0.1
#endif
__device__ __forceinline__ bool mm_wave_polar(const LegK& a, int end) {      // a wave of the ring pairs up to `end` (exclusive; wave-uniform)
	const double c = a.cth[min(end, a.npairs) - 1];   // its most equatorial pair (pairs are ordered pole first)
	return c*c > PXS_POLAR_COS2;
}
// Ring pair -> (wave, block s, lane) of the VALU kernels, the one definition of it.  A wave holds 64 K consecutive ring pairs, pole first, in K blocks of 64;
// the nwave K 64 - npairs slots without a pair sit in front of pair 0, in wave 0, the polar wave, which is dead or late for almost every m.  (They used to sit behind
// the last pair, in the most equatorial wave, which is live from the smallest l on for every m: its empty lanes ran every step.)  Every wave's most equatorial pair
// -- the one that decides when the wave leaves phase A -- lies `pad` pairs polewards of where it lay, so no wave starts earlier than before.
// (the MFMA kernels keep their own partition: wave w of workgroup wv holds the pairs from 64 (W wv + w) on)
__host__ __device__ constexpr int leg_pair_of(int npairs, int nwave, int K, int wv, int s, int lane) { return (wv*K + s)*64 + lane - (nwave*K*64 - npairs); }
__host__ __device__ constexpr int leg_wave_last_pair(int npairs, int K, int wv) { return leg_pair_of(npairs, (npairs + 64*K - 1)/(64*K), K, wv, K - 1, 63); }      // the wave's most equatorial pair; >= 0 whenever npairs > 0 (the wave count is the launch's: make_legk)
// (1451 pairs = 7 192 + 107 = 5 256 + 171 = 2 512 + 427: wave 0 holds 107, 171, 427 pairs for K = 3, 4, 8, the last wave ends at the last pair, a full set has no padding)
static_assert(leg_wave_last_pair(1451, 3, 0) == 106 && leg_wave_last_pair(1451, 4, 0) == 170 && leg_wave_last_pair(1451, 8, 0) == 426, "pair map: first wave");
static_assert(leg_wave_last_pair(1451, 3, 7) == 1450 && leg_wave_last_pair(1451, 4, 5) == 1450 && leg_wave_last_pair(1451, 8, 2) == 1450, "pair map: last wave");
static_assert(leg_pair_of(1451, 8, 3, 0, 0, 0) == -85 && leg_pair_of(1451, 8, 3, 0, 1, 21) == 0 && leg_pair_of(512, 2, 4, 0, 0, 0) == 0 && leg_wave_last_pair(30, 4, 0) == 29, "pair map: padding");
__device__ __forceinline__ int leg_pair(const LegK& a, int wv, int K, int s, int lane) { return leg_pair_of(a.npairs, a.nwave, K, wv, s, lane); }
__device__ __forceinline__ bool leg_pair_valid(const LegK& a, int p) { return (unsigned)p < (unsigned)a.npairs; }
__device__ __forceinline__ bool leg_wave_polar(const LegK& a, int wv, int K) { return mm_wave_polar(a, leg_wave_last_pair(a.npairs, K, wv) + 1); }

// make a VGPR copy of a wave-uniform value once, so that v_fma_f64 can take it as the addend next to
// an SGPR multiplicand (gfx950 allows one scalar source per VALU op; without this the compiler
// re-materialises the constant for every use with two v_mov_b32)
#ifdef PXS_HOST_SIM
#define PXS_VCOPY(dst, src) double dst = (src)
#else
#define PXS_VCOPY(dst, src) double dst; asm("v_mov_b64 %0, %1" : "=v"(dst) : "s"(src))
#endif

// a per-lane value the compiler has to take as new at this point.  The synthesis epilogue of the MFMA kernels takes its lane through it: computed from the lane
// itself, its map index was shared with the one of the B operands (MmSynB::init) and kept through the tile loop as sign-extended 64-bit values, which
// leg_syn_spin_mm<2>, at the 128-VGPR line, paid with 36 bytes of scratch (24 before there was one body; none with this)
#ifdef PXS_HOST_SIM
#define PXS_FRESH_INT(x) (x)
#else
__device__ __forceinline__ int pxs_fresh_int(int x) { asm("" : "+v"(x)); return x; }
#define PXS_FRESH_INT(x) pxs_fresh_int(x)
#endif
// ... and one the compiler may not compute ahead of this point either: the analysis kernels take the lane through it where a slot fetches its ring data in phase B.
// Computed from the lane itself, the addresses of every slot's ring indices were kept from the head of the phase-B loop on (leg_ana_spin<3> 132 -> 122 VGPRs
// and a fourth wave per SIMD with it, leg_ana_spin<6> 230 -> 206, leg_ana_s0<8> 159 -> 156)
#ifdef PXS_HOST_SIM
#define PXS_LATE_INT(x) (x)
#else
__device__ __forceinline__ int pxs_late_int(int x) { asm volatile("" : "+v"(x)); return x; }
#define PXS_LATE_INT(x) pxs_late_int(x)
#endif

// (An L2 prefetch of the coefficient streams via global_load_lds into an LDS sink was tried to hide SMEM
// miss latency and measured SLOWER on MI355X: leg_syn 10.8 -> 12.4 ms at config 2; removed.)

#ifdef PXS_HOST_SIM
#define PXS_UNIFORM_INT(x) (x)
#define PXS_UNIFORM_LONG(x) (x)
#else
#define PXS_UNIFORM_INT(x) __builtin_amdgcn_readfirstlane(x)
// (a wave-uniform table offset that the compiler keeps in VGPRs turns every coefficient row load of the loops below into a per-lane
// global_load: seen when the seed stores entered the kernels -- leg_syn 101 -> 123 ms at config 3)
#define PXS_UNIFORM_LONG(x) ((long)(((unsigned long)(unsigned)__builtin_amdgcn_readfirstlane((int)((unsigned long)(x) >> 32)) << 32) | (unsigned long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned long)(x))))
#endif
// leg_pair with the block's first pair taken through v_readfirstlane: for leg_syn_s0, which is held to 72 VGPRs and spills 52 bytes with it against 68 without (44 before
// the padding moved; profiles/leg_kernel_resources.txt).  Not for the analysis kernels: leg_ana_s0<8> 159 -> 168, leg_ana_spin<4> 152 -> 156 VGPRs.
__device__ __forceinline__ int leg_pair_u(const LegK& a, int wv, int K, int s, int lane) { return PXS_UNIFORM_INT(leg_pair(a, wv, K, s, 0)) + lane; }
// Recurrence seeds.  Phase A (recurrence only, no accumulation, until the first lane of the wave is live, LEG_LIVE) is the same
// for every transform on a plan: ~18 % of the steps of a live (wave, m) at a third of the cost of an accumulating step, i.e.
// ~5 % of the Legendre time, plus the sin^m start values.  The first launch on a ring set records the state it ends in, later
// launches load it: K x 20 bytes (spin 0) or K x 40 bytes (spin s) per lane (S0_SEEDED_PHASE_A, leg_s0.hip; SPIN_SEEDED_PHASE_A, leg_spin.hip).

// Phase B history: it used to be a per-step loop with per-lane gating (cndmask) and a rescale test in every step:
// 207 instructions per step for leg_ana_spin<6> against 97 per step in the fast loop, ~18 % of the kernel time in a
// phase that covers ~8 % of the steps.  (Rejected before that: merging the gated steps into the fast pair loop behind
// a wave-uniform `if (pend)`: leg_syn 118 -> 172 ms at config 3; a branch-free pair-wise gated loop: VGPRs 124 -> 192.)
// Now phase B runs the ungated fast steps and only tests / rescales every 4 steps, see the kernels.

// Workgroups are ONE wave: lanes run in lockstep and a wave's LDS operations execute in order, so
// cross-lane visibility of the LDS tile only needs the LDS counter drained -- not an s_barrier, whose
// compiler-inserted s_waitcnt vmcnt(0) would also wait for the (slow, fire-and-forget) global store
// of the previous flush.  (The simulator's lanes do not run in lockstep: there it is the rendezvous of the lanes of ONE wave, pxsim::wave_sync, the
// same thing whatever the waves per workgroup -- a block barrier would deadlock waves of differing trip counts, as the lab build with NW waves
// per workgroup had them.)
#ifdef PXS_HOST_SIM
#define PXS_WAVE_LDS_SYNC() pxsim::wave_sync()
#else
#define PXS_WAVE_LDS_SYNC() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
#endif
// The sums over the rings of a wave (4 values per recurrence step) are collected for LEG_FSTEPS steps in an LDS tile and
// flushed together: output j = 4*step + row of the tile is then owned by lane j, which adds up its partial sums and
// contributes ONE value to a contiguous 512-byte store (or atomic add).  Measured on MI355X at config 3 (leg_ana per round
// trip, same box): no reduction at all 105.5 ms, lane swaps + LDS writes +22.7 ms, and the former flush (every 4 steps, 4
// lanes per output, two shuffles, 128-byte stores) +14 ms; this flush +3.3 ms.  What remains is the lane-swap stage: 6 swaps,
// 3 adds and a ds_write per step next to 48 FMAs, every one of them a 4-cycle VALU issue for a wave64 (10/58 = the measured
// share).  More ring pairs per lane would amortise it, but the kernels sit at the 3-waves-per-SIMD VGPR line already.
#define LEG_FSTEPS 16
#ifdef PXS_HOST_SIM
// simulator path: every lane writes its 4 sums, lane j adds row j over the 64 lanes
#define LEG_RED_STRIDE 66
#define LEG_RED_DOUBLES (4*LEG_FSTEPS*LEG_RED_STRIDE)
__device__ __forceinline__ double leg_flush_sum(const double* red, int lane) {
	const double* r = red + lane*LEG_RED_STRIDE;
	double s0 = 0, s1 = 0, s2 = 0, s3 = 0;
	for (int i = 0; i < 64; i += 4) { s0 += r[i]; s1 += r[i+1]; s2 += r[i+2]; s3 += r[i+3]; }
	return (s0 + s1) + (s2 + s3);
}
__device__ __forceinline__ int leg_flush_col(int lane) { return lane; }
#define LEG_RED_PUT(kk, t0, t1, t2, t3) \
	red[((kk)*4+0)*LEG_RED_STRIDE + lane] = t0; red[((kk)*4+1)*LEG_RED_STRIDE + lane] = t1; \
	red[((kk)*4+2)*LEG_RED_STRIDE + lane] = t2; red[((kk)*4+3)*LEG_RED_STRIDE + lane] = t3;
#else
// MI355X path: reduce-scatter across lanes with the gfx950 lane-swap instructions.  Stage 1
// (v_permlane32_swap on the pairs (t0,t1), (t2,t3)) leaves sum(t0|t2) in lanes 0-31 and sum(t1|t3) in
// lanes 32-63; stage 2 (v_permlane16_swap) leaves ONE value per lane, already summed over the 4 lanes
// {l, l+16, l+32, l+48}: the four 16-lane rows of the wave hold t0, t2, t1, t3.  One ds_write_b64 per step (4x fewer
// LDS bytes than transposing all partial sums; the LDS write port was the limiter); row r of step kk goes to
// red[(4 kk + r)*18 .. +16], so that lane j = 4 kk + r reads its 16 partial sums as 8 aligned 16-byte words.
// (Tried and rejected: v_mfma_f64_4x4x4 with B = 1 as a lane adder: correct, but 8 dependent f64 MFMAs per step made the
// kernel matrix-pipe bound.  Round 3, with the lane layout from tools/mfma_probe.hip -- A at lane 16k+4b+i, B at 16k+4b+j, D at
// 16i+4b+j -- and B_r = [j == r]: four MFMAs accumulate the four sums of a step into ONE register, 4 issues + a ds_write instead
// of 9 VALU ops + a ds_write, 160 / 168 VGPRs: leg_ana_spin<4> 105.9 -> 112.9 ms, leg_ana_s0<8> 26.9 -> 31.0 ms at config 3: the
// f64 MFMA shares the FMA pipe's throughput on MI355X, it does not add to it. transposing all four sums through LDS: 145.1 against 142.1 ms.)
#define LEG_RED_STRIDE 18
#define LEG_RED_DOUBLES (4*LEG_FSTEPS*LEG_RED_STRIDE)
__device__ __forceinline__ void leg_swap32(double& a, double& b) {
	const unsigned alo = __double2loint(a), ahi = __double2hiint(a), blo = __double2loint(b), bhi = __double2hiint(b);
	const auto r0 = __builtin_amdgcn_permlane32_swap(alo, blo, false, false);
	const auto r1 = __builtin_amdgcn_permlane32_swap(ahi, bhi, false, false);
	a = __hiloint2double(r1[0], r0[0]); b = __hiloint2double(r1[1], r0[1]);
}
__device__ __forceinline__ void leg_swap16(double& a, double& b) {
	const unsigned alo = __double2loint(a), ahi = __double2hiint(a), blo = __double2loint(b), bhi = __double2hiint(b);
	const auto r0 = __builtin_amdgcn_permlane16_swap(alo, blo, false, false);
	const auto r1 = __builtin_amdgcn_permlane16_swap(ahi, bhi, false, false);
	a = __hiloint2double(r1[0], r0[0]); b = __hiloint2double(r1[1], r0[1]);
}
__device__ __forceinline__ double leg_flush_sum(const double* red, int lane) {
	const double2* r = reinterpret_cast<const double2*>(red + lane*LEG_RED_STRIDE);
	// two rounds of 4 loads, not unrolled: all 16 values at once cost 16-20 more VGPRs at the point where every chain is live
	// (leg_ana_s0<8> 174 VGPRs = 2 waves per SIMD instead of 3)
	double sum = 0;
#pragma unroll 1
	for (int h = 0; h < 8; h += 4) {
		const double2 a = r[h], b = r[h+1], c = r[h+2], d = r[h+3];
		sum += ((a.x + a.y) + (b.x + b.y)) + ((c.x + c.y) + (d.x + d.y));
	}
	return sum;
}
// lane j = 4 kk + r holds row r of step kk: rows are t0, t2, t1, t3
__device__ __forceinline__ int leg_flush_col(int lane) { const int r = lane & 3; return (lane & ~3) | ((r == 1) ? 2 : (r == 2) ? 1 : r); }
#define LEG_RED_PUT(kk, t0, t1, t2, t3) { \
	double a_ = t0, b_ = t1, c_ = t2, d_ = t3; \
	leg_swap32(a_, b_); leg_swap32(c_, d_); \
	double u_ = a_ + b_, v_ = c_ + d_; \
	leg_swap16(u_, v_); \
	red[((kk)*4 + (lane >> 4))*LEG_RED_STRIDE + (lane & 15)] = u_ + v_; }
#endif
// nkk steps of the tile -> dst[4 step + c] (c = 0..3: the sums t0..t3 of the step).  atomic: several waves add into the same
// rows (dst pre-zeroed); otherwise dst belongs to this wave alone
__device__ __forceinline__ void leg_flush(double* red, double* __restrict__ dst, int lane, int nkk, int atomic) {
	PXS_WAVE_LDS_SYNC();
	if (lane < 4*nkk) {
		const double sum = leg_flush_sum(red, lane);
		double* q = dst + leg_flush_col(lane);
#ifdef PXS_HOST_SIM
		if (atomic) atomicAdd(q, sum); else *q = sum;
#else
		if (atomic) unsafeAtomicAdd(q, sum); else *q = sum;
#endif
	}
	PXS_WAVE_LDS_SYNC();
}


#define MM_PSTRIDE 65
#define MM_WAVES 8
#define MM_ESTRIDE 17
#ifdef PXS_HOST_SIM
struct mm_acc { double v[4]; double& operator[](int i) { return v[i]; } };
static inline mm_acc mm_mfma(double av, double bv, mm_acc c) {      // D[4r + lane/16][lane%16] += sum_kk A[i][kk] B[kk][j], A at lane i + 16 kk, B at lane j + 16 kk
	pxsim::BlockCtx* cx = pxsim::t_ctx; const int w = pxsim::wave_id(), l = pxsim::lane_id();
	uint64_t* s = cx->wslot->data() + (size_t)w*128;
	memcpy(&s[l], &av, 8); memcpy(&s[64 + l], &bv, 8); cx->wbar[w]->wait();
	for (int r = 0; r < 4; r++) {
		const int i = 4*r + (l >> 4), j = l & 15;
		double sum = c.v[r];
		for (int kk = 0; kk < 4; kk++) { double x, y; memcpy(&x, &s[i + 16*kk], 8); memcpy(&y, &s[64 + j + 16*kk], 8); sum = fma(x, y, sum); }
		c.v[r] = sum;
	}
	cx->wbar[w]->wait();
	return c;
}
static inline void mm_lds_add(double* p, double v) { atomicAdd(p, v); }
#define MM_WAVE_SYNC() pxsim::t_ctx->wbar[pxsim::wave_id()]->wait()
#else
typedef double mm_acc __attribute__((ext_vector_type(4)));
__device__ __forceinline__ mm_acc mm_mfma(double av, double bv, mm_acc c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, c, 0, 0, 0); }
__device__ __forceinline__ void mm_lds_add(double* p, double v) { (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
#define MM_WAVE_SYNC() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
#endif
// step coefficient a x^2 + b' with both a and b' wave-uniform: gfx950 takes one scalar source per VALU op, so b' is copied to a VGPR
// right at its use (left to the compiler, the copies of all 16 steps of a tile were made early and lived in 64 VGPRs: spills)
__device__ __forceinline__ double mm_coef(double ca, double x2, double cb) { PXS_VCOPY(vb_, cb); return fma(ca, x2, vb_); }
// ---- what the four MFMA kernels (leg_{ana,syn}_{s0,spin}_mm) share ----
// A chain is one recurrence of one ring pair in extended-exponent form (S0Chain, leg_s0.hip; SpinChain, leg_spin.hip): step(ca, cb) advances it by one
// step with the table row (ca, cb) and returns the value it had, sc < 0 says that it is still below scale 0, rescale() brings it closer, park_sign()
// gives the parked values of four steps from kq on their sign in the P tile.
// the (a, b') of the 16 steps from k0 on: four s_load_dwordx16
__device__ __forceinline__ void mm_load_cf(double (&cf)[32], const double* __restrict__ tab, int k0) {
#pragma unroll
	for (int i = 0; i < 32; i++) cf[i] = LDCD(tab, 2L*k0 + i);
}
// Park the 16 steps k0 ... k0 + 15 of the chain as rows of the wave's P tile (rows of STRIDE doubles, the lane's column).  kw: first step this wave contributes to
// (a multiple of 4), n: steps of this m, pend: some chain of the wave is below scale 0 (phase B: such a chain contributes nothing yet and is rescaled every 4 steps).
template<int STRIDE, class Chain>
__device__ __forceinline__ void mm_park_tile(Chain& C, const double (&cf)[32], int k0, int kw, int n, bool& pend, double* __restrict__ ptile, int lane) {
#pragma unroll
	for (int q4 = 0; q4 < 4; q4++) {
		const int kq = k0 + 4*q4;
		double p[4] = {0, 0, 0, 0};
		if (kq >= kw && kq < n) {
#pragma unroll
			for (int i = 0; i < 4; i++) p[i] = C.step(cf[8*q4 + 2*i], cf[8*q4 + 2*i + 1]);
			if (pend) {
				if (C.sc < 0) { p[0] = p[1] = p[2] = p[3] = 0.0; C.rescale(); }
				pend = __any(C.sc < 0);
			}
			C.park_sign(kq, p);
			// rows beyond the last step of this m stay out of the sums (their table rows belong to the next m)
			if (kq + 1 >= n) p[1] = 0.0;
			if (kq + 2 >= n) p[2] = 0.0;
			if (kq + 3 >= n) p[3] = 0.0;
		}
#pragma unroll
		for (int i = 0; i < 4; i++) ptile[(4*q4 + i)*STRIDE + lane] = p[i];
	}
}
// B operands of the synthesis kernels: lane (j, kk) of MFMA step-quad q holds column j & 3 of map 4 (bb NG + g) + (j >> 2) at step q + 4 kk of the tile, read from
// the pre-scaled alm.  SIGNED (spin s): columns 2, 3 (a-) times sgn_l = (-1)^(par + step)
template<int NG, bool SIGNED> struct MmSynB {
	const double* src[NG]; bool ok[NG]; int kk4, cc, par;
	__device__ __forceinline__ void init(const LegK& a, int bb, long row0, int lane, int par_) {
		const int jcol = lane & 15; kk4 = lane >> 4; cc = jcol & 3; par = par_;
#pragma unroll
		for (int g = 0; g < NG; g++) {
			const int map = (bb*NG + g)*4 + (jcol >> 2);
			ok[g] = map < a.nmaps;
			src[g] = a.almt + (long)(ok[g] ? map : 0)*a.almt_bs + 4*row0 + cc + 16*kk4;
		}
	}
	__device__ __forceinline__ void load(int k0, int n, double (*b)[4]) const {
#pragma unroll
		for (int g = 0; g < NG; g++)
#pragma unroll
			for (int q = 0; q < 4; q++) {
				const int row = k0 + q + 4*kk4;
				const double v = (ok[g] && row < n) ? src[g][4L*(k0 + q)] : 0.0;
				b[g][q] = (SIGNED && cc >= 2 && ((par + row) & 1)) ? -v : v;
			}
	}
};
// Flush of tile tf of the analysis kernels (after the barrier that ends it): the W waves share out the 4 NG rows of the reduction tile; register r of group g holds rows
// 4 r + lane / 16 of the tile, column lane % 16 = 4 (map in the group) + c.  It is issued behind the MFMAs of the NEXT tile (the two reduction tiles alternate), off the
// path from the barrier to that tile's recurrence.  SIGNED (spin s): c >= 2 (mu-) times sgn of the row, (-1)^(par + row)
template<int NG, int W, bool SIGNED>
__device__ __forceinline__ void mm_flush(const LegK& a, double* __restrict__ red, int tf, int w, int lane, int bb, int n, long row0, int par) {
	double* __restrict__ redf = red + (tf & 1)*NG*4*64;
	for (int cidx = w; cidx < 4*NG; cidx += W) {
		const int g = cidx >> 2, r = cidx & 3;
		double* rp = redf + cidx*64 + lane;
		double v = *rp; *rp = 0.0;
		const int krow = 16*tf + 4*r + (lane >> 4), map = (bb*NG + g)*4 + ((lane & 15) >> 2), c = lane & 3;
		if (krow < n && map < a.nmaps) {
			if (SIGNED && c >= 2 && ((par + krow) & 1)) v = -v;
			double* dst = a.mom + (long)map*a.mom_bs + 4*(row0 + krow) + c;
#ifdef PXS_HOST_SIM
			atomicAdd(dst, v);
#else
			unsafeAtomicAdd(dst, v);
#endif
		}
	}
}
// LDS: [W][16][MM_PSTRIDE] P tiles + [2][4 NG][64] reduction tiles (the staging area of the prologue, 64 W entries of MM_ESTRIDE doubles, lies over both)
__host__ __device__ constexpr int mm_lds_doubles(int NG, int W) { return W*16*MM_PSTRIDE + 2*NG*4*64 > 64*W*MM_ESTRIDE ? W*16*MM_PSTRIDE + 2*NG*4*64 : 64*W*MM_ESTRIDE; }
static inline size_t mm_ana_lds(int NG, int W) { return sizeof(double)*(size_t)mm_lds_doubles(NG, W) + 16; }

#define MMS_PSTRIDE 68
static inline size_t mm_syn_lds() { return sizeof(double)*16*MMS_PSTRIDE; }
#ifdef PXS_HOST_SIM
#define MMS_XOR2(v) __shfl_xor((v), 2)
#else
__device__ __forceinline__ double mms_xor2(double v) {      // value of lane ^ 2 (quad permute [2, 3, 0, 1])
	const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), 0x4e, 0xf, 0xf, true), hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), 0x4e, 0xf, 0xf, true);
	return __hiloint2double(hi, lo);
}
#define MMS_XOR2(v) mms_xor2(v)
#endif

// ---- the MFMA kernels: one analysis body, one synthesis body ----
// leg_ana_mm<Sys, NG, W> is the body of leg_ana_s0_mm / leg_ana_spin_mm, leg_syn_mm<Sys, NG> that of leg_syn_s0_mm / leg_syn_spin_mm; Sys = S0Mm (leg_s0.hip)
// or SpinMm (leg_spin.hip) supplies
//   Chain, init(a, p, m, half, polar, C): the chain of a slot and its start value;  SLOTS: ring pairs per wave (64, or 32 pairs x 2 half-wave chains);
//   steps(a, m, par): step count of the m and the parity of its first step (spin s; a count <= 0 ends the kernel or leaves the wave idle);
//   table(a, polar, row0): the compact step table (a, b') the tiles read;  phase_a(a, C, row0, polar, n): phase A, returns the step reached;
//   SIGNED: the last two columns carry sgn_l (MmSynB, mm_flush);
//   Data, load(...), park(...): the 16 doubles a thread parks per slot and group of 4 maps in the analysis prologue, BREG_SYNC: a wave sync after the B registers
//   of a group are read;  store<NG>(...): the synthesis epilogue.
template<class Sys, int NG, int W> __device__ __forceinline__ void leg_ana_mm(const LegK& a)
{
	PXS_SHARED(double, sh);
	double* __restrict__ ptile = sh;                              // [W][16][MM_PSTRIDE]
	double* __restrict__ red = sh + W*16*MM_PSTRIDE;              // [2][4 NG][64]: the accumulators of a tile summed over the waves
	int* __restrict__ s_kmin = reinterpret_cast<int*>(sh + mm_lds_doubles(NG, W));
	const int tid = threadIdx.x, lane = tid & 63, w = PXS_UNIFORM_INT(tid >> 6), half = lane/Sys::SLOTS;
	int wv, m, bb;
	if (!leg_block(a, wv, m, bb)) return;
	int par;
	const int n = Sys::steps(a, m, par);
	if (n <= 0) return;
	const long row0 = PXS_UNIFORM_LONG(a.row[m]);
	const int pbase = wv*Sys::SLOTS*W;
	const bool polar = mm_wave_polar(a, pbase + Sys::SLOTS*(w + 1));      // (per wave: its own pairs, its own coefficient stream)
	const int pmine_ = pbase + Sys::SLOTS*w + (lane & (Sys::SLOTS - 1));       // ring pair of this lane's chain: wave w owns the pairs [SLOTS w, SLOTS (w + 1)) of the chunk
	typename Sys::Chain C;
	const bool alive = Sys::init(a, pmine_, m, half, polar, C);
	if (tid == 0) *s_kmin = n;
	__syncthreads();
	// phase A, per wave: recurrence only until the first lane of the wave is live; kw = the first step this wave contributes to
	const bool wave_alive = __any(alive);
	const int kw = PXS_UNIFORM_INT(wave_alive ? Sys::phase_a(a, C, row0, polar, n) : n + 16);
	if (lane == 0) atomicMin(s_kmin, kw);
	__syncthreads();
	const int kmin = PXS_UNIFORM_INT(*s_kmin);
	if (kmin >= n) return;      // (workgroup-uniform) no ring of this chunk carries signal at this m
	// B operands through the LDS: thread = slot (a chain of a ring pair), 4 maps per round
	double breg[NG][16];
	{
		const bool ok = pmine_ < a.npairs;
		const int rn = ok ? a.ring_n[pmine_] : -1, rs = ok ? a.ring_s[pmine_] : -1;
		const double x = ok ? a.cth[pmine_] : 0.0;
		double* __restrict__ ent = sh + tid*MM_ESTRIDE;
		const double* __restrict__ rd = sh + (64*w + 16*(lane >> 4))*MM_ESTRIDE + (lane & 15);
#pragma unroll
		for (int g = 0; g < NG; g++) {
			typename Sys::Data d;
			Sys::load(a, m, (bb*NG + g)*4, rn, rs, d);
			if (g > 0) __syncthreads();      // the reads of the previous round
			Sys::park(d, x, half, ent);
			__syncthreads();
#pragma unroll
			for (int q = 0; q < 16; q++) breg[g][q] = rd[q*MM_ESTRIDE];
			if (Sys::BREG_SYNC) MM_WAVE_SYNC();
		}
		__syncthreads();
		for (int i = tid; i < 2*NG*4*64; i += 64*W) red[i] = 0.0;
		__syncthreads();
	}
	const double* __restrict__ tab = Sys::table(a, polar, row0);      // (a, b') of step k at tab[2 k]
	bool pend = __any(C.sc < 0);
	double* __restrict__ pmine = ptile + w*16*MM_PSTRIDE;
	const double* __restrict__ pread = pmine + (lane & 15)*MM_PSTRIDE + 16*(lane >> 4);
	double cf[32]; int cf_tile = -1;      // coefficients of the 16 steps of tile cf_tile, requested a tile ahead
	long ntile = 0;
	auto flush = [&](int tf) { mm_flush<NG, W, Sys::SIGNED>(a, red, tf, w, lane, bb, n, row0, par); };
	int tlast = -1;
	for (int t = kmin >> 4; 16*t < n; t++) {
		const int k0 = 16*t;
		double* __restrict__ redt = red + (t & 1)*NG*4*64;
		if (k0 + 16 > kw) {      // (wave-uniform) this wave has steps in the tile
			ntile++;
			if (cf_tile != t) mm_load_cf(cf, tab, k0);
			mm_park_tile<MM_PSTRIDE>(C, cf, k0, kw, n, pend, pmine, lane);
			MM_WAVE_SYNC();
			double av[4];
#pragma unroll
			for (int q = 0; q < 4; q++) av[q] = pread[q];
			MM_WAVE_SYNC();
			if (k0 + 16 < n) { mm_load_cf(cf, tab, k0 + 16); cf_tile = t + 1; }      // the rows of the next tile, on their way during the MFMAs (requested after the first A operands have landed)
			mm_acc acc[NG];
#pragma unroll
			for (int g = 0; g < NG; g++) { acc[g][0] = 0; acc[g][1] = 0; acc[g][2] = 0; acc[g][3] = 0; }
#pragma unroll
			for (int q = 0; q < 16; q++) {
				const double aq = q < 4 ? av[q] : pread[q];
#pragma unroll
				for (int g = 0; g < NG; g++) acc[g] = mm_mfma(aq, breg[g][q], acc[g]);
			}
			if (tlast >= 0) { flush(tlast); tlast = -1; }
#pragma unroll
			for (int g = 0; g < NG; g++)
#pragma unroll
				for (int r = 0; r < 4; r++) mm_lds_add(redt + (g*4 + r)*64 + lane, acc[g][r]);
		}
		if (tlast >= 0) flush(tlast);
		tlast = t;
		__syncthreads();
	}
	if (tlast >= 0) flush(tlast);
	PXS_COUNT(1, ntile*(NG*256L + 32L) + (wave_alive ? (long)kw*2 : 0L));
}

template<class Sys, int NG> __device__ __forceinline__ void leg_syn_mm(const LegK& a)
{
	PXS_SHARED(double, pmine);      // [16][MMS_PSTRIDE]
	const int lane = threadIdx.x, half = lane/Sys::SLOTS;
	int wv, m, bb;
	if (!leg_block(a, wv, m, bb)) return;
	int par;
	const int n = Sys::steps(a, m, par);
	const long row0 = PXS_UNIFORM_LONG(a.row[m]);
	const int pbase = wv*Sys::SLOTS;
	const bool polar = mm_wave_polar(a, pbase + Sys::SLOTS);
	typename Sys::Chain C;
	const bool alive = Sys::init(a, pbase + (lane & (Sys::SLOTS - 1)), m, half, polar, C);
	mm_acc acc[NG][4];
#pragma unroll
	for (int g = 0; g < NG; g++)
#pragma unroll
		for (int rb = 0; rb < 4; rb++) { acc[g][rb][0] = 0; acc[g][rb][1] = 0; acc[g][rb][2] = 0; acc[g][rb][3] = 0; }
	long ntile = 0;
	// phase A: recurrence only until the first lane of the wave is live (a wave without a live ring skips the loop below)
	const bool wave_alive = n > 0 && __any(alive);
	const int kw = PXS_UNIFORM_INT(wave_alive ? Sys::phase_a(a, C, row0, polar, n) : max(n, 0) + 16);      // (explicitly wave-uniform: left as a select, the loop below was compiled as divergent and the prefetched coefficient rows went to VGPRs)
	{
		const double* __restrict__ tab = Sys::table(a, polar, row0);      // (a, b') of step k at tab[2 k]
		MmSynB<NG, Sys::SIGNED> B; B.init(a, bb, row0, lane, par);
		bool pend = __any(C.sc < 0);
		const double* __restrict__ pread = pmine + 4*(lane >> 4)*MMS_PSTRIDE + (lane & 15);
		double cf[32];      // coefficients of the 16 steps of the tile, requested a tile ahead (every tile from the wave's first one on is run)
		double bcur[NG][4], bnxt[NG][4];
		B.load(16*(kw >> 4), n, bcur);
		if (kw < n) mm_load_cf(cf, tab, 16*(kw >> 4));
		for (int t = kw >> 4; 16*t < n; t++) {
			const int k0 = 16*t;
			ntile++;
			mm_park_tile<MMS_PSTRIDE>(C, cf, k0, kw, n, pend, pmine, lane);
			MM_WAVE_SYNC();
			double av[4];
#pragma unroll
			for (int rb = 0; rb < 4; rb++) av[rb] = pread[16*rb];
			MM_WAVE_SYNC();
			if (k0 + 16 < n) { mm_load_cf(cf, tab, k0 + 16); B.load(k0 + 16, n, bnxt); }      // the rows of the next tile (coefficients and pre-scaled alm), on their way during the MFMAs
#pragma unroll
			for (int q = 0; q < 4; q++)
#pragma unroll
				for (int rb = 0; rb < 4; rb++) {
					const double aq = q == 0 ? av[rb] : pread[q*MMS_PSTRIDE + 16*rb];
#pragma unroll
					for (int g = 0; g < NG; g++) acc[g][rb] = mm_mfma(aq, bcur[g][q], acc[g][rb]);
				}
			MM_WAVE_SYNC();      // the A operands are out of the tile before the next one is written
#pragma unroll
			for (int g = 0; g < NG; g++)
#pragma unroll
				for (int q = 0; q < 4; q++) bcur[g][q] = bnxt[g][q];
		}
	}
	Sys::template store<NG>(a, m, bb, pbase, PXS_FRESH_INT(lane), acc);      // (the epilogue's map index and addresses are computed here, after the loop)
	PXS_COUNT(0, ntile*(NG*256L + 32L) + (wave_alive ? (long)kw*2 : 0L));
}

// ---- launches ----
// the kernel of (direction, form, K or ng) is picked next to the kernels (launch_leg_s0, launch_leg_spin); ng: groups of 4 maps per wave / workgroup (0: VALU form)
typedef void (*LegKernel)(const LegK);
// (waves per workgroup of the MFMA analysis measured at C4: 2 waves 95 ms, 4: 78, 8: 77, 16: 82 per 64 maps)
static inline bool leg_mm_lds_optin(std::initializer_list<LegKernel> ks) {
	for (LegKernel k : ks) (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, 160*1024 - 256);
	return true;
}
static inline void leg_launch(LegKernel k, bool analysis, int ng, dim3 grid, hipStream_t st, const LegK& a) {
	const int W = analysis && ng ? MM_WAVES : 1;
	const size_t lds = ng ? (analysis ? mm_ana_lds(ng, MM_WAVES) : mm_syn_lds()) : analysis ? sizeof(double)*LEG_RED_DOUBLES : 0;
	hipLaunchKernelGGL(k, grid, dim3(64*W), lds, st, a);
}
void launch_leg_s0(bool analysis, int ng, int K, dim3 grid, hipStream_t st, const LegK& a);
void launch_leg_spin(bool analysis, int ng, int K, dim3 grid, hipStream_t st, const LegK& a);

} // namespace pxs
