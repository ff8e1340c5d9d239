// General ring sets of the SHT plans: per-ring nphi, phi0 and ringstart (healpix, profile rings; ducc's synthesis / adjoint_synthesis
// contract, curvedsky.py:328-349, 396-403, 537, 553, 936-960): their tables, kernels and ring FFT stage.
#include "sht_plan.hpp"
#include <algorithm>

namespace pxs {

// Rings are grouped by length; z holds one complex line per ring, group after group, so that every group is a dense
// [rings][n] block for one batched FFT.  A block of 256 threads works on 256 consecutive elements of one ring (blk_ring, blk_k0).
struct GenK {
	int nring, nm, nc; long ldleg, leg_cstride, zc, map_cstride, pix_stride;
	const int* blk_ring; const int* blk_k0; const int* nphi; const long* zoff; const long* rstart; const double* phi0;
	double scale;
};
// ring spectrum with aliasing: H[k] = sum_{m = k mod n, m <= mmax} f_m leg[m][r] e^{i m phi0_r}, f_0 = 1, f_m = 2: the real ring is
// Re of the backward DFT of H
__global__ __launch_bounds__(256) void gen_fold(const GenK g, const double2* __restrict__ leg, double2* __restrict__ z)
{
	const int r = g.blk_ring[blockIdx.x], k = g.blk_k0[blockIdx.x] + (int)threadIdx.x, c = blockIdx.y;
	const int n = g.nphi[r];
	if (k >= n) return;
	const double ph = g.phi0[r];
	const double2* col = leg + (long)c*g.leg_cstride + r;
	double ar = 0, ai = 0;
	for (int m = k; m < g.nm; m += n) {
		const double2 a = col[(long)m*g.ldleg];
		double sn, cs; sincos((double)m*ph, &sn, &cs);
		const double f = m ? 2.0 : 1.0;
		ar += f*(a.x*cs - a.y*sn); ai += f*(a.x*sn + a.y*cs);
	}
	z[(long)c*g.zc + g.zoff[r] + k] = make_double2(ar, ai);
}
template<class T> __global__ __launch_bounds__(256) void gen_scatter(const GenK g, const double2* __restrict__ z, T* __restrict__ map)
{
	const int r = g.blk_ring[blockIdx.x], j = g.blk_k0[blockIdx.x] + (int)threadIdx.x, c = blockIdx.y;
	if (j >= g.nphi[r]) return;
	map[(long)c*g.map_cstride + g.rstart[r] + (long)j*g.pix_stride] = (T)z[(long)c*g.zc + g.zoff[r] + j].x;
}
template<class T> __global__ __launch_bounds__(256) void gen_gather(const GenK g, const T* __restrict__ map, double2* __restrict__ z)
{
	const int r = g.blk_ring[blockIdx.x], j = g.blk_k0[blockIdx.x] + (int)threadIdx.x, c = blockIdx.y;
	if (j >= g.nphi[r]) return;
	z[(long)c*g.zc + g.zoff[r] + j] = make_double2((double)map[(long)c*g.map_cstride + g.rstart[r] + (long)j*g.pix_stride], 0.0);
}
// leg[m][r] = scale e^{-i m phi0_r} F_r[m mod n_r]
__global__ __launch_bounds__(256) void gen_unfold(const GenK g, const double2* __restrict__ z, double2* __restrict__ leg)
{
	const int r = blockIdx.x*256 + (int)threadIdx.x, c = blockIdx.z;
	if (r >= g.nring) return;
	const int n = g.nphi[r]; const double ph = g.phi0[r];
	const double2* line = z + (long)c*g.zc + g.zoff[r];
	for (int m = blockIdx.y; m < g.nm; m += gridDim.y) {
		const double2 a = line[m % n];
		double sn, cs; sincos((double)m*ph, &sn, &cs);
		leg[(long)c*g.leg_cstride + (long)m*g.ldleg + r] = make_double2(g.scale*(a.x*cs + a.y*sn), g.scale*(a.y*cs - a.x*sn));
	}
}

// tables of a general ring set: groups of equal length, z offsets, the block table of the gen_* kernels
void GenRings::setup(int device_, int nring, const uint64_t* nphi_, const double* phi0_, const uint64_t* ringstart) {
	device = device_; std::vector<int> order(nring);
	for (int r = 0; r < nring; r++) { order[r] = r; PXS_REQUIRE(nphi_[r] >= 1 && nphi_[r] < (1ull << 31), "pxs_plan_rings: bad nphi"); }
	std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return nphi_[a] < nphi_[b]; });
	std::vector<int> np(nring), br, bk; std::vector<long> zo(nring), rs(nring); std::vector<double> ph(phi0_, phi0_ + nring);
	long off = 0;
	groups.clear();
	for (int i = 0; i < nring; i++) {
		const int r = order[i];
		np[r] = (int)nphi_[r]; rs[r] = (long)ringstart[r]; zo[r] = off;
		if (groups.empty() || groups.back().n != (long)nphi_[r]) groups.push_back(Group{(long)nphi_[r], 0, off});
		groups.back().count++;
		for (long k0 = 0; k0 < (long)nphi_[r]; k0 += 256) { br.push_back(r); bk.push_back((int)k0); }
		off += (long)nphi_[r];
	}
	npixz = off; nblk = (long)br.size();
	blk_ring = upload(br); blk_k0 = upload(bk); nphi = upload(np); zoff = upload(zo); rstart = upload(rs); phi0 = upload(ph);
	if (groups.size() >= 8) {
		const int ns = 16;      // side streams of ffts(): nside 2048, lmax 4096, 3 components took 282 ms on one stream, 94 ms on 16
		streams.resize(ns); join.resize(ns);
		for (int i = 0; i < ns; i++) { PXS_HIP(hipStreamCreateWithFlags(&streams[i], hipStreamNonBlocking)); PXS_HIP(hipEventCreateWithFlags(&join[i], hipEventDisableTiming)); }
		PXS_HIP(hipEventCreateWithFlags(&fork, hipEventDisableTiming));
	}
}
GenRings::~GenRings() {
	for (auto s : streams) if (s) { fft_release_stream(device, s); (void)hipStreamDestroy(s); }
	for (auto e : join) if (e) (void)hipEventDestroy(e);
	if (fork) (void)hipEventDestroy(fork);
}
// one batched FFT per (component, length).  A healpix map has 2 nside lengths with two to four rings each: the launches are
// dealt round-robin to side streams that fork from / join the caller's stream, so that the many small transforms overlap
void GenRings::ffts(hipStream_t st, int nc, bool forward) {
	const size_t njobs = (size_t)nc*groups.size();
	const size_t ns = njobs >= 16 ? streams.size() : 0;
	if (ns) {
		PXS_HIP(hipEventRecord(fork, st));
		for (size_t i = 0; i < ns; i++) PXS_HIP(hipStreamWaitEvent(streams[i], fork, 0));
	}
	size_t job = 0;
	for (int c = 0; c < nc; c++)
		for (const auto& gr : groups) {
			double2* zl = z.as<double2>() + (size_t)c*npixz + gr.zoff;
			fft_dense_lines(device, ns ? streams[job % ns] : st, gr.n, forward, gr.count, zl, zl);
			job++;
		}
	for (size_t i = 0; i < ns; i++) { PXS_HIP(hipEventRecord(join[i], streams[i])); PXS_HIP(hipStreamWaitEvent(st, join[i], 0)); }
}

} // namespace pxs

// the kernels' view of the plan's ring set for nc components (which also sizes z: general ring sets size their own scratch here)
static GenK gen_args(pxs_plan* p, int nc, long ldleg, long map_cstride) {
	GenRings& gn = p->gen;
	gn.z.ensure(sizeof(double2)*(size_t)nc*gn.npixz);
	GenK g; g.nring = p->nring; g.nm = p->mmax + 1; g.nc = nc; g.ldleg = ldleg; g.leg_cstride = (long)(p->mmax + 1)*ldleg; g.zc = gn.npixz;
	g.map_cstride = map_cstride; g.pix_stride = p->pix_stride;
	g.blk_ring = gn.blk_ring.as<int>(); g.blk_k0 = gn.blk_k0.as<int>(); g.nphi = gn.nphi.as<int>(); g.zoff = gn.zoff.as<long>();
	g.rstart = gn.rstart.as<long>(); g.phi0 = gn.phi0.as<double>(); g.scale = 1.0;
	return g;
}

void gen_map2leg(pxs_plan* p, hipStream_t st, const MapArg& m, int nc, double2* leg, long ldleg) {
	const GenK g = gen_args(p, nc, ldleg, m.cstride);
	double2* z = p->gen.z.as<double2>(); const dim3 grid((unsigned)p->gen.nblk, nc);
	if (m.dtype == PX_F32) hipLaunchKernelGGL(gen_gather<float>, grid, dim3(256), 0, st, g, (const float*)m.ptr, z);
	else                     hipLaunchKernelGGL(gen_gather<double>, grid, dim3(256), 0, st, g, (const double*)m.ptr, z);
	p->gen.ffts(st, nc, true);
	hipLaunchKernelGGL(gen_unfold, dim3((p->nring + 255)/256, std::min(p->mmax + 1, 4096), nc), dim3(256), 0, st, g, (const double2*)z, leg);
}

void gen_leg2map(pxs_plan* p, hipStream_t st, const double2* leg, long ldleg, const MapArg& m, int nc) {
	const GenK g = gen_args(p, nc, ldleg, m.cstride);
	double2* z = p->gen.z.as<double2>(); const dim3 grid((unsigned)p->gen.nblk, nc);
	hipLaunchKernelGGL(gen_fold, grid, dim3(256), 0, st, g, leg, z);
	p->gen.ffts(st, nc, false);
	if (m.dtype == PX_F32) hipLaunchKernelGGL(gen_scatter<float>, grid, dim3(256), 0, st, g, (const double2*)z, (float*)m.ptr);
	else                     hipLaunchKernelGGL(gen_scatter<double>, grid, dim3(256), 0, st, g, (const double2*)z, (double*)m.ptr);
}
