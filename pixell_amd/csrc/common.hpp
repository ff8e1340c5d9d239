// Shared host-side helpers for libpxsht (gfx950 only).
#pragma once
#include "hostsim.hpp"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <stdexcept>

namespace pxs {

enum : int { PXS_OK = 0, PXS_ERR_ARG = -1, PXS_ERR_HIP = -2, PXS_ERR_UNSUPPORTED = -3, PXS_ERR_NOMEM = -4 };

struct Error : std::runtime_error {
	int code;
	Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

void set_last_error(const std::string& msg);

#define PXS_HIP(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) \
	throw pxs::Error(pxs::PXS_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)
#define PXS_REQUIRE(cond, msg) do { if (!(cond)) throw pxs::Error(pxs::PXS_ERR_ARG, std::string(msg)); } while (0)
// the body of every extern "C" entry point: an exception becomes the last error and its code, anything else returns 0
#define PXS_TRY try {
#define PXS_CATCH } catch (const pxs::Error& e) { pxs::set_last_error(e.what()); return e.code; } \
	catch (const std::exception& e) { pxs::set_last_error(e.what()); return pxs::PXS_ERR_ARG; } return 0;

static constexpr double PXS_PI = 3.14159265358979323846;

// Device memory of the library goes through one per-process arena (arena.hip): blocks of 32 MB and more that a plan releases are
// kept (up to PXS_ARENA_GB, default 48) and handed to the next plan that asks for a similar size instead of going back to the driver
// -- the scratch of a plan is tens of GB, hipMalloc maps it at a box-dependent rate, and a program that drops its plans between
// workloads (bench.py's legs, sht.clear_plans()) paid for it again each time.  pxs_memory() reports and releases.
void* dev_alloc(size_t bytes);
void dev_free(void* p, size_t bytes);
size_t dev_capacity(void* p);      // true size of a live arena block (it may exceed what its user asked for), 0 for anything else

// simple owning device buffer
struct DevBuf {
	void* p = nullptr; size_t bytes = 0;
	DevBuf() {}
	explicit DevBuf(size_t n) { alloc(n); }
	DevBuf(const DevBuf&) = delete; DevBuf& operator=(const DevBuf&) = delete;
	DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
	DevBuf& operator=(DevBuf&& o) noexcept { release(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; return *this; }
	~DevBuf() { release(); }
	void alloc(size_t n) { release(); if (n) { p = dev_alloc(n); bytes = n; } }
	void ensure(size_t n) {
		if (n <= bytes) return;
		if (p && dev_capacity(p) >= n) { bytes = n; return; }      // a reused block with room to spare: grow in place (releasing it would hand the same block back after a device synchronisation)
		alloc(n);
	}
	void release() { if (p) { dev_free(p, bytes); p = nullptr; bytes = 0; } }
	template<class T> T* as() const { return reinterpret_cast<T*>(p); }
};

// Scratch that a library call keeps between calls, one buffer per (slot, device, stream): calls on two streams must not share it, calls
// on one stream are ordered by the stream.  The reference is found under the registry's lock and stays valid until the stream is
// released (entries never move); the caller grows it with ensure() and launches outside the lock.  Growing hands the old block to the
// arena, which synchronises the device before the block serves anybody else: the stream's earlier kernels may still read it.
enum ScratchSlot : int { SCR_FOURSTEP, SCR_BLUESTEIN, SCR_C2R, SCR_ALM2CL, SCR_SRC_FIXED, SCR_SRC_PAIRS, SCR_DISTANCE, SCR_THUMBS, SCR_LABEL };
DevBuf& stream_scratch(ScratchSlot slot, int device, void* stream);
void stream_scratch_release(int device, void* stream);      // a stream is about to be destroyed: a recycled handle must not inherit a stale buffer

inline unsigned blocks_of(long n) { return (unsigned)((n + 255)/256); }      // workgroups of 256 lanes for n items
struct Carve {      // consecutive 16-byte aligned pieces of one buffer
	size_t at = 0;
	size_t take(size_t bytes) { const size_t o = at; at += (bytes + 15)/16*16; return o; }
};

template<class T> inline DevBuf upload(const std::vector<T>& v) {
	DevBuf b(v.size()*sizeof(T));
	if (!v.empty()) PXS_HIP(hipMemcpy(b.p, v.data(), v.size()*sizeof(T), hipMemcpyHostToDevice));
	return b;
}

// exact unsigned division by a small runtime constant: q = umulhi(x, mul) (valid for x*d < 2^32)
struct FastDiv { uint32_t mul; uint32_t d; };
inline FastDiv make_fastdiv(uint32_t d) {
	FastDiv f; f.d = d;
	f.mul = d <= 1 ? 0u : (uint32_t)(((1ull << 32) + d - 1) / d);
	return f;
}

enum DType : int { PX_F32 = 0, PX_F64 = 1, PX_C64 = 2, PX_C128 = 3, PX_U8 = 4, PX_I32 = 5 };      // (the integer types: maps that pxm_interpol copies from)
inline int dtype_bytes(int dt) { return dt == PX_U8 ? 1 : dt == PX_F32 || dt == PX_I32 ? 4 : dt == PX_C128 ? 16 : 8; }      // of one element

// the alm and the maps of an SHT call as the C ABI hands them over: component c of batch member b starts at element
// b*bstride + c*cstride of `dtype`; from(b): the same arrays from batch member b on
struct AlmArg { void* ptr; int dtype; long cstride, bstride;
	AlmArg from(long b) const { return AlmArg{(char*)ptr + dtype_bytes(dtype)*(size_t)b*bstride, dtype, cstride, bstride}; } };
struct MapArg { void* ptr; int dtype; long cstride, bstride;
	MapArg from(long b) const { return MapArg{(char*)ptr + dtype_bytes(dtype)*(size_t)b*bstride, dtype, cstride, bstride}; } };

// Tuning and experiment switches (tile shapes, ring pairs per lane, planner overrides, alternative paths kept for A/B runs) are read
// from the environment in LAB builds only (-DPXS_LAB, tools/build_variants.sh); the product build compiles their defaults in.  What
// the product reads from the environment is listed in DESIGN.md ("Environment switches").
#ifdef PXS_LAB
inline const char* lab_getenv(const char* name) { return getenv(name); }
#else
inline const char* lab_getenv(const char*) { return nullptr; }
#endif

// A memory budget of the product's environment (PXS_*_GB: shift 30, PXS_*_MB: shift 20): a real number of that unit, so that
// PXS_BATCH_GB=0.004 means 4 MB and whole numbers mean what they always did.  false: unset or empty (the caller keeps its default).
// Read where it applies -- as a plan is made or per call -- never once per process.
inline bool env_budget(const char* name, int shift, size_t& bytes) {
	const char* e = getenv(name);
	if (!e || !*e) return false;
	const double v = strtod(e, nullptr);
	bytes = v > 0 ? (size_t)(v*(double)(size_t(1) << shift)) : 0;
	return true;
}
// The passes a call took at one of the places where the library cuts it to stay within such a budget, counted by the loop that
// launches them (pxs_plan_query "passes_<seam>"): n passes, the sizes of the first, the last and the one before the last
struct PassLog {
	long n = 0, first = 0, prev = 0, last = 0;
	void begin() { n = first = prev = last = 0; }
	void add(long size) { if (n == 0) first = size; prev = n ? last : 0; last = size; n++; }
};

} // namespace pxs
