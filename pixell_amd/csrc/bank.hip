// The alm filter bank of the wavelet transforms (pixell_amd/wavelets.py): one full-resolution alm <-> a list of filtered, band-limited
// copies, each in the dense triangular layout of its own band limit.
//   split:  out_i(l,m) = f_i[l] in(l,m)   for l <= lmax_i,   0 for lmax_i < l <= L_i           (every scale in ONE launch, in(l,m) loaded once)
//   merge:  out(l,m)   = (out(l,m) +) sum_i f_i[l] a_i(l,m)  over the scales with l <= lmax_i   (a gather, summed in ascending i: no atomics)
// These replace, per scale, curvedsky.transfer_alm (a gather / scatter through host-built index arrays) followed by alm_info.lmul.
// Pure streaming: bytes moved are 16 (N + sum_i N_i) for complex128 (N elements of the full alm, N_i of scale i).  For fixed m, l is
// contiguous on both sides (lstride 1), so lanes run along l; blockIdx.y is m, blockIdx.z the component.  Every global access is 16 bytes
// wide where it can be: one complex128 per lane, or the complex64 pair (l even, l+1) per lane where that pair sits on a 16-byte boundary
// of the array in question (decided per row and per array: the row starts of the layouts involved differ in parity), else two 8-byte ones.
// The per-scale tables travel in the kernel arguments (no upload, no host synchronisation); the filters are a device table.
#include "../../include/pxsht.h"
#include "common.hpp"

namespace pxs {

static constexpr int BANK_MAX = 32;          // scales per launch: 32 x 24 bytes of kernel arguments
struct BankScale { void* p; long pitch; int lmax, L; };
struct BankTab { BankScale s[BANK_MAX]; };

struct alignas(16) c64x2 { float2 a, b; };

// first element of column m in the dense triangular layout of band limit L (element (l, m) at tri(L, m) + l)
__device__ __forceinline__ long tri(int L, int m) { return ((long)m*(2*L + 1 - m))/2; }

// complex128: one element per lane
__global__ __launch_bounds__(256) void bank_split_c128(BankTab T, int nscale, int ltop, int lmax, int mmax, const uint64_t* __restrict__ mstart, long lstride,
		const double2* __restrict__ in, long in_pitch, const double* __restrict__ filt, int nl)
{
	const int m = blockIdx.y, c = blockIdx.z;
	const int l = m + blockIdx.x*256 + threadIdx.x;
	if (l > ltop) return;
	double2 v = make_double2(0.0, 0.0);
	if (m <= mmax && l <= lmax) v = in[c*in_pitch + (long)mstart[m] + l*lstride];
	for (int i = 0; i < nscale; i++) {
		const BankScale S = T.s[i];
		if (l > S.L) continue;
		double2 r = make_double2(0.0, 0.0);
		if (l <= S.lmax) { const double f = filt[(long)i*nl + l]; r = make_double2(f*v.x, f*v.y); }
		((double2*)S.p)[c*S.pitch + tri(S.L, m) + l] = r;
	}
}

__global__ __launch_bounds__(256) void bank_merge_c128(BankTab T, int nscale, int lmax, int mmax, const uint64_t* __restrict__ mstart, long lstride,
		double2* __restrict__ out, long out_pitch, const double* __restrict__ filt, int nl, int accumulate)
{
	const int m = blockIdx.y, c = blockIdx.z;
	const int l = m + blockIdx.x*256 + threadIdx.x;
	if (l > lmax) return;
	const long o = c*out_pitch + (long)mstart[m] + l*lstride;
	double2 acc = accumulate ? out[o] : make_double2(0.0, 0.0);
	for (int i = 0; i < nscale; i++) {
		const BankScale S = T.s[i];
		if (l > S.lmax) continue;
		const double f = filt[(long)i*nl + l];
		const double2 a = ((const double2*)S.p)[c*S.pitch + tri(S.L, m) + l];
		acc.x += f*a.x; acc.y += f*a.y;
	}
	out[o] = acc;
}

// complex64: the pair (l0 even, l0 + 1) per lane; ok0 / ok1 say which of the two exist in the row
__device__ __forceinline__ void ld_pair(const float2* p, bool ok0, bool ok1, float2& a, float2& b) {
	if (ok0 && ok1 && (((uintptr_t)p) & 15) == 0) { const c64x2 t = *(const c64x2*)p; a = t.a; b = t.b; return; }
	a = ok0 ? p[0] : make_float2(0.0f, 0.0f);
	b = ok1 ? p[1] : make_float2(0.0f, 0.0f);
}
__device__ __forceinline__ void st_pair(float2* p, bool ok0, bool ok1, float2 a, float2 b) {
	if (ok0 && ok1 && (((uintptr_t)p) & 15) == 0) { c64x2 t; t.a = a; t.b = b; *(c64x2*)p = t; return; }
	if (ok0) p[0] = a;
	if (ok1) p[1] = b;
}

__global__ __launch_bounds__(256) void bank_split_c64(BankTab T, int nscale, int ltop, int lmax, int mmax, const uint64_t* __restrict__ mstart, long lstride,
		const float2* __restrict__ in, long in_pitch, const double* __restrict__ filt, int nl)
{
	const int m = blockIdx.y, c = blockIdx.z;
	const int l0 = (m & ~1) + 2*(blockIdx.x*256 + threadIdx.x), l1 = l0 + 1;
	if (l0 > ltop) return;
	float2 v0 = make_float2(0.0f, 0.0f), v1 = v0;
	if (m <= mmax) {
		const bool ok0 = l0 >= m && l0 <= lmax, ok1 = l1 <= lmax;
		const float2* p = in + c*in_pitch + (long)mstart[m] + l0*lstride;
		if (lstride == 1) ld_pair(p, ok0, ok1, v0, v1);
		else { if (ok0) v0 = p[0]; if (ok1) v1 = p[lstride]; }
	}
	for (int i = 0; i < nscale; i++) {
		const BankScale S = T.s[i];
		if (l0 > S.L) continue;
		float2 r0 = make_float2(0.0f, 0.0f), r1 = r0;
		if (l0 <= S.lmax) { const float f = (float)filt[(long)i*nl + l0]; r0 = make_float2(f*v0.x, f*v0.y); }
		if (l1 <= S.lmax) { const float f = (float)filt[(long)i*nl + l1]; r1 = make_float2(f*v1.x, f*v1.y); }
		st_pair((float2*)S.p + c*S.pitch + tri(S.L, m) + l0, l0 >= m, l1 <= S.L, r0, r1);
	}
}

__global__ __launch_bounds__(256) void bank_merge_c64(BankTab T, int nscale, int lmax, int mmax, const uint64_t* __restrict__ mstart, long lstride,
		float2* __restrict__ out, long out_pitch, const double* __restrict__ filt, int nl, int accumulate)
{
	const int m = blockIdx.y, c = blockIdx.z;
	const int l0 = (m & ~1) + 2*(blockIdx.x*256 + threadIdx.x), l1 = l0 + 1;
	if (l0 > lmax) return;
	const bool ok0 = l0 >= m, ok1 = l1 <= lmax;
	float2* po = out + c*out_pitch + (long)mstart[m] + l0*lstride;
	float2 acc0 = make_float2(0.0f, 0.0f), acc1 = acc0;
	if (accumulate) {
		if (lstride == 1) ld_pair(po, ok0, ok1, acc0, acc1);
		else { if (ok0) acc0 = po[0]; if (ok1) acc1 = po[lstride]; }
	}
	for (int i = 0; i < nscale; i++) {
		const BankScale S = T.s[i];
		if (l0 > S.lmax) continue;
		float2 a0, a1;
		ld_pair((const float2*)S.p + c*S.pitch + tri(S.L, m) + l0, ok0, l1 <= S.lmax, a0, a1);
		const float f0 = (float)filt[(long)i*nl + l0];
		acc0.x += f0*a0.x; acc0.y += f0*a0.y;
		if (l1 <= S.lmax) { const float f1 = (float)filt[(long)i*nl + l1]; acc1.x += f1*a1.x; acc1.y += f1*a1.y; }
	}
	if (lstride == 1) st_pair(po, ok0, ok1, acc0, acc1);
	else { if (ok0) po[0] = acc0; if (ok1) po[lstride] = acc1; }
}

static void check_bank(const char* who, int nscale, const int* lmaxs, const int* Ls, void* const* ptrs, const int64_t* pitches, int npre,
		int lmax, int mmax, const uint64_t* d_mstart, const void* full, int dtype, const double* d_filt, int nl)
{
	const std::string w(who);
	PXS_REQUIRE(nscale >= 1 && lmaxs && Ls && ptrs && pitches, w + ": bad scale tables");
	PXS_REQUIRE(npre >= 1 && npre <= 65535 && lmax >= 0 && lmax < 65535 && mmax >= 0 && mmax <= lmax && d_mstart && full && d_filt, w + ": bad arguments");
	PXS_REQUIRE(dtype == PX_C64 || dtype == PX_C128, w + ": alm must be complex64 or complex128");
	for (int i = 0; i < nscale; i++) {
		PXS_REQUIRE(ptrs[i] && lmaxs[i] >= 0 && lmaxs[i] <= lmax && Ls[i] >= lmaxs[i] && Ls[i] < 65535, w + ": a scale needs 0 <= lmax_i <= min(lmax, L_i)");
		PXS_REQUIRE(lmaxs[i] < nl, w + ": the filter table is shorter than a scale's band limit");
		PXS_REQUIRE(pitches[i] >= ((int64_t)Ls[i] + 1)*(Ls[i] + 2)/2, w + ": a scale's pitch is shorter than its triangular layout");
	}
}
} // namespace pxs

using namespace pxs;

extern "C" {

int pxa_bank_split(int nscale, const int* lmaxs, const int* Ls, void* const* outs, const int64_t* out_pitch, int npre,
                   int lmax, int mmax, const uint64_t* d_mstart, int64_t lstride, const void* alm_in, int64_t in_pitch, int alm_dtype,
                   const double* d_filt, int nl, int device, void* stream)
{
	PXS_TRY
	check_bank("pxa_bank_split", nscale, lmaxs, Ls, outs, out_pitch, npre, lmax, mmax, d_mstart, alm_in, alm_dtype, d_filt, nl);
	PXS_HIP(hipSetDevice(device));
	for (int i0 = 0; i0 < nscale; i0 += BANK_MAX) {
		const int n = std::min(BANK_MAX, nscale - i0);
		BankTab T; int ltop = 0;
		for (int i = 0; i < n; i++) { T.s[i] = BankScale{outs[i0+i], (long)out_pitch[i0+i], lmaxs[i0+i], Ls[i0+i]}; ltop = std::max(ltop, Ls[i0+i]); }
		const double* f = d_filt + (size_t)i0*nl;
		if (alm_dtype == PX_C128)
			hipLaunchKernelGGL(bank_split_c128, dim3((ltop+256)/256, ltop+1, npre), dim3(256), 0, (hipStream_t)stream, T, n, ltop, lmax, mmax, d_mstart, (long)lstride,
				(const double2*)alm_in, (long)in_pitch, f, nl);
		else
			hipLaunchKernelGGL(bank_split_c64, dim3((ltop/2+256)/256, ltop+1, npre), dim3(256), 0, (hipStream_t)stream, T, n, ltop, lmax, mmax, d_mstart, (long)lstride,
				(const float2*)alm_in, (long)in_pitch, f, nl);
	}
	PXS_HIP(hipGetLastError());
	PXS_CATCH
}

int pxa_bank_merge(int nscale, const int* lmaxs, const int* Ls, void* const* ins, const int64_t* in_pitch, int npre,
                   int lmax, int mmax, const uint64_t* d_mstart, int64_t lstride, void* alm_out, int64_t out_pitch, int alm_dtype,
                   const double* d_filt, int nl, int accumulate, int device, void* stream)
{
	PXS_TRY
	check_bank("pxa_bank_merge", nscale, lmaxs, Ls, ins, in_pitch, npre, lmax, mmax, d_mstart, alm_out, alm_dtype, d_filt, nl);
	PXS_HIP(hipSetDevice(device));
	for (int i0 = 0; i0 < nscale; i0 += BANK_MAX) {
		const int n = std::min(BANK_MAX, nscale - i0);
		BankTab T;
		for (int i = 0; i < n; i++) T.s[i] = BankScale{ins[i0+i], (long)in_pitch[i0+i], lmaxs[i0+i], Ls[i0+i]};
		const double* f = d_filt + (size_t)i0*nl;
		const int acc = (accumulate || i0 > 0) ? 1 : 0;          // later groups of scales add onto the first
		if (alm_dtype == PX_C128)
			hipLaunchKernelGGL(bank_merge_c128, dim3((lmax+256)/256, mmax+1, npre), dim3(256), 0, (hipStream_t)stream, T, n, lmax, mmax, d_mstart, (long)lstride,
				(double2*)alm_out, (long)out_pitch, f, nl, acc);
		else
			hipLaunchKernelGGL(bank_merge_c64, dim3((lmax/2+256)/256, mmax+1, npre), dim3(256), 0, (hipStream_t)stream, T, n, lmax, mmax, d_mstart, (long)lstride,
				(float2*)alm_out, (long)out_pitch, f, nl, acc);
	}
	PXS_HIP(hipGetLastError());
	PXS_CATCH
}

} // extern "C"
