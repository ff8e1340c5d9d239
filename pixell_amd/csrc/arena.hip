// Device-memory arena of libpxsht (see common.hpp) and its accounting: how long the library spent in hipMalloc is the first thing to
// know about a slow first call (round 5: first alm2map of a fresh process 162 ms on one box, 1248 ms on another, same code).
#include "common.hpp"
#include <chrono>
#include <climits>
#include <map>
#include <mutex>
#include <tuple>
#include <unordered_map>

namespace pxs {
namespace {
// A released block may still be read or written by kernels of its last owner: the library's calls are asynchronous, and a block comes
// back (a plan destroyed, a buffer grown by DevBuf::ensure) with no runtime call at all.  So every pooled block carries the number of
// device synchronisations the arena had made on its device when it was pooled (its "epoch"), and before a block pooled since the last
// one is handed out again, or given back to the driver, the arena synchronises that device once: all blocks pooled up to then are
// idle from there on.  A steady state reuses nothing and pays nothing; the one synchronisation inside a transform call is that of a
// scratch buffer which grows (DevBuf::ensure) into a block pooled a moment ago, its own old block included when the new size is
// within a quarter of it (a reused block with slack grows in place instead: dev_capacity).
struct Block { void* p; int dev; unsigned long epoch; };
struct Arena {
	std::mutex mu;
	std::multimap<size_t, Block> pool;                       // released blocks by their true size
	std::unordered_map<void*, std::pair<int, size_t>> owner; // (device, true size) of every live block >= MINB (noted at allocation: no runtime call when a block comes back,
	                                                         // which may be from a static destructor after the HIP runtime has shut down).  The true size: a pooled block of S bytes
	                                                         // serves requests down to 0.8 S, and is accounted, pooled again and matched by S whatever its user asked for
	std::unordered_map<int, unsigned long> epoch;            // device synchronisations made by the arena, per device
	size_t pooled = 0, live = 0, cap = size_t(48) << 30;
	double malloc_ms = 0; long nmalloc = 0, nreuse = 0; size_t malloc_bytes = 0;
	Arena() { const char* e = getenv("PXS_ARENA_GB"); if (e) cap = (size_t)atol(e) << 30; }
	static constexpr size_t MINB = size_t(32) << 20;
	// (mu held) work that may touch a block pooled on `dev` at `stamp` is complete on return
	void settle(int dev, unsigned long stamp) {
		unsigned long& ep = epoch[dev];
		if (stamp < ep) return;
		int cur = 0; (void)hipGetDevice(&cur);
		if (cur != dev) (void)hipSetDevice(dev);
		const hipError_t e = hipDeviceSynchronize();
		if (cur != dev) (void)hipSetDevice(cur);
		if (e != hipSuccess) throw Error(PXS_ERR_HIP, std::string("hipDeviceSynchronize before the reuse of an arena block: ") + hipGetErrorString(e));
		ep++;
	}
	void drop_all() {      // (mu held)
		for (auto& kv : pool) { try { settle(kv.second.dev, kv.second.epoch); } catch (const Error&) {} (void)hipFree(kv.second.p); }
		pool.clear(); pooled = 0;
	}
};
Arena& arena() { static Arena* a = new Arena; return *a; }      // (never destroyed: buffers with static storage duration are released through it while the process exits)
}

void* dev_alloc(size_t n) {
	Arena& a = arena();
	std::lock_guard<std::mutex> g(a.mu);
	int dev = 0; (void)hipGetDevice(&dev);
	if (n >= Arena::MINB) {      // a released block of this size or up to a quarter more, on this device
		for (auto it = a.pool.lower_bound(n); it != a.pool.end() && it->first <= n + n/4; ++it) if (it->second.dev == dev) {
			a.settle(dev, it->second.epoch);      // (throws with the block still pooled)
			void* p = it->second.p; const size_t sz = it->first;
			a.pooled -= sz; a.live += sz; a.pool.erase(it); a.nreuse++;
			a.owner[p] = std::make_pair(dev, sz);
			return p;
		}
	}
	void* p = nullptr;
	const auto t0 = std::chrono::steady_clock::now();
	hipError_t e = hipMalloc(&p, n);
	if (e != hipSuccess && !a.pool.empty()) { a.drop_all(); e = hipMalloc(&p, n); }      // out of memory: give the kept blocks back first
	a.malloc_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	if (e != hipSuccess) throw Error(PXS_ERR_NOMEM, std::string("hipMalloc of ") + std::to_string(n >> 20) + " MB: " + hipGetErrorString(e));
	a.nmalloc++; a.malloc_bytes += n; a.live += n;
	if (n >= Arena::MINB) a.owner[p] = std::make_pair(dev, n);
	return p;
}

size_t dev_capacity(void* p) {
	if (!p) return 0;
	Arena& a = arena();
	std::lock_guard<std::mutex> g(a.mu);
	auto it = a.owner.find(p);
	return it == a.owner.end() ? 0 : it->second.second;
}

void dev_free(void* p, size_t n) {      // no runtime call unless the block goes back to the driver
	if (!p) return;
	Arena& a = arena();
	std::lock_guard<std::mutex> g(a.mu);
	int dev = -1;
	auto it = a.owner.find(p);
	if (it != a.owner.end()) { dev = it->second.first; n = it->second.second; a.owner.erase(it); }      // (the block's true size, which may exceed what its user asked for)
	a.live -= std::min(a.live, n);
	if (n >= Arena::MINB && a.pooled + n <= a.cap) {
		// (the device the block lives on, not the thread's current one: a plan may be destroyed from a thread that has another device selected)
		if (dev < 0) { dev = 0; (void)hipGetDevice(&dev); }
		auto ep = a.epoch.find(dev);
		a.pool.emplace(n, Block{p, dev, ep == a.epoch.end() ? 0ul : ep->second}); a.pooled += n;
		return;
	}
	(void)hipFree(p);      // (hipFree waits for the device)
}

namespace {
struct Scratch { std::mutex mu; std::map<std::tuple<int, void*, int>, DevBuf> tab; };      // (device, stream, slot): std::map nodes do not move
Scratch& scratch() { static Scratch* s = new Scratch; return *s; }      // (never destroyed, like the arena its buffers go back to)
}
DevBuf& stream_scratch(ScratchSlot slot, int device, void* stream) {
	Scratch& s = scratch();
	std::lock_guard<std::mutex> g(s.mu);
	return s.tab[std::make_tuple(device, stream, (int)slot)];
}
void stream_scratch_release(int device, void* stream) {
	Scratch& s = scratch();
	std::lock_guard<std::mutex> g(s.mu);
	s.tab.erase(s.tab.lower_bound(std::make_tuple(device, stream, 0)), s.tab.upper_bound(std::make_tuple(device, stream, INT_MAX)));
}
} // namespace pxs

extern "C" int pxs_memory(int release, double* stats) {
	pxs::Arena& a = pxs::arena();
	std::lock_guard<std::mutex> g(a.mu);
	if (release) a.drop_all();
	if (stats) { stats[0] = a.malloc_ms; stats[1] = (double)a.nmalloc; stats[2] = (double)a.malloc_bytes; stats[3] = (double)a.nreuse; stats[4] = (double)a.pooled; stats[5] = (double)a.live; }
	return 0;
}
