// The SHT stages that do not run as fused chains (fftchain.hip): the glue kernels between the stages, the ring FFT through the generic
// FFT engine (aliased rings, lengths without a usable factorisation) and the theta resampling through it.
//
// The theta resampling integrates the trigonometric interpolant exactly: mirror-extend each m column to the full circle with parity
// (-1)^(m+s), FFT, resize the spectrum onto a fine grid of M points, multiply by the pointwise table of the form there, FFT back, keep
// |k| <= lmax and evaluate on the CC grid.  All index remaps are fused into the FFT load/store functors (fft.hpp).
#include "sht_plan.hpp"
#include "fft_dev.hpp"
#include <algorithm>

namespace pxs {

// v * t (conj(t) if conj) * scale
__device__ __forceinline__ double2 tab_mul(double2 v, double2 t, bool conj, double scale) {
	if (conj) t.y = -t.y;
	v = cmul(v, t);
	return make_double2(v.x*scale, v.y*scale);
}
// the mirror image of sample j on a circle of N samples with mirror constant c: (-j - c) mod N
__device__ __forceinline__ long mirror_index(long N, int j, int c) { long mj = N - j - c; if (mj >= N) mj -= N; if (mj < 0) mj += N; return mj; }
// A line Z holds even(theta) + odd(theta) of two columns of opposite parity on the full circle: the two parts at sample j,
// (Z[j] +- Z[mirror(j)])/2 (a self-mirrored sample is all even), as a = the first column's (odd parity: a_odd) and b = the second's
__device__ __forceinline__ void split_even_odd(const double2* __restrict__ Z, long N, int j, int c, bool a_odd, double2& a, double2& b) {
	const long mj = mirror_index(N, j, c); const double2 z = Z[j];
	double2 ev = z, od = make_double2(0, 0);
	if (mj != j) { const double2 y = Z[mj]; ev = make_double2(0.5*(z.x + y.x), 0.5*(z.y + y.y)); od = make_double2(0.5*(z.x - y.x), 0.5*(z.y - y.y)); }
	a = make_double2(a_odd ? od.x : ev.x, a_odd ? od.y : ev.y);
	b = make_double2(a_odd ? ev.x : od.x, a_odd ? ev.y : od.y);
}

// ---- glue kernels ----------------------------------------------------------------------
// 32x32 tile transpose through LDS times tab[c] (conjugated if conj_tab) * scale; c runs with blockIdx.x, r with blockIdx.y.
// C_IS_ROW false: out[b][c][r] = in[b][r][c] * tab[c]; true: out[b][r][c] = in[b][c][r] * tab[c] (ldin, ldout: row strides)
template<bool C_IS_ROW> __global__ __launch_bounds__(256) void transpose_tab(const double2* __restrict__ in, double2* __restrict__ out,
		int nr, int nc, long in_bstride, long out_bstride, long ldin, long ldout, const double2* __restrict__ tab, int conj_tab, double scale)
{
	PXS_SHARED(double2, tile);   // [32][33]
	const int b = blockIdx.z;
	const int r0 = blockIdx.y*32, c0 = blockIdx.x*32;
	const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
	in += (long)b*in_bstride; out += (long)b*out_bstride;
	for (int j = ty; j < 32; j += 8) {
		const int r = r0 + (C_IS_ROW ? tx : j), c = c0 + (C_IS_ROW ? j : tx);
		if (r < nr && c < nc) tile[j*33 + tx] = in[C_IS_ROW ? (long)c*ldin + r : (long)r*ldin + c];
	}
	__syncthreads();
	for (int j = ty; j < 32; j += 8) {
		const int r = r0 + (C_IS_ROW ? j : tx), c = c0 + (C_IS_ROW ? tx : j);
		if (r < nr && c < nc) out[C_IS_ROW ? (long)r*ldout + c : (long)c*ldout + r] = tab_mul(tile[tx*33 + j], tab[c], conj_tab != 0, scale);
	}
}

// ring pairs were transformed as one complex line z = a + i b; rows hold Z[0..k] then Z[n-1..n-k] (k = mmax).
// X_a[m] = (Z[m] + conj(Z[n-m]))/2, X_b[m] = -i (Z[m] - conj(Z[n-m]))/2  ->  leg[b][m][2q], leg[b][m][2q+1], times tab[m]*scale.
__global__ __launch_bounds__(256) void unpack_pair_transpose(const double2* __restrict__ in, double2* __restrict__ out,
		int nr, int nm, long in_bstride, long out_bstride, const double2* __restrict__ tab, double scale)
{
	PXS_SHARED(double2, tile);   // two [32][33] tiles
	double2* tp = tile; double2* tm = tile + 32*33;
	const int b = blockIdx.z;
	const int q0 = blockIdx.y*32, m0 = blockIdx.x*32;
	const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
	const int npair = (nr + 1)/2, k = nm - 1, rowlen = 2*k + 1;
	in += (long)b*in_bstride; out += (long)b*out_bstride;
	for (int j = ty; j < 32; j += 8) {
		const int q = q0 + j, m = m0 + tx;
		if (q < npair && m < nm) {
			tp[j*33 + tx] = in[(long)q*rowlen + m];
			tm[j*33 + tx] = in[(long)q*rowlen + (m == 0 ? 0 : k + m)];
		}
	}
	__syncthreads();
	for (int j = ty; j < 32; j += 8) {
		const int m = m0 + j, q = q0 + tx;
		if (q < npair && m < nm) {
			const double2 zp = tp[tx*33 + j], zm = tm[tx*33 + j];
			// conj(zm) = (zm.x, -zm.y)
			double2 xa = make_double2(0.5*(zp.x + zm.x), 0.5*(zp.y - zm.y));
			const double2 d  = make_double2(zp.x - zm.x, zp.y + zm.y);
			double2 xb = make_double2(0.5*d.y, -0.5*d.x);                 // -i d / 2
			// (written out, not through tab_mul: there the compiler contracts the other product of xa's imaginary part into the FMA,
			// which rounds differently, and the results of this path are kept bitwise)
			const double2 t = tab[m];
			xa = make_double2((xa.x*t.x - xa.y*t.y)*scale, (xa.x*t.y + xa.y*t.x)*scale);
			xb = make_double2((xb.x*t.x - xb.y*t.y)*scale, (xb.x*t.y + xb.y*t.x)*scale);
			out[(long)m*nr + 2*q] = xa;
			if (2*q + 1 < nr) out[(long)m*nr + 2*q + 1] = xb;
		}
	}
}

// aliased rings (mmax >= nphi): leg[b][m][r] = h[b][r][m mod nphi] * tab[m]   (rare; simple gather)
__global__ __launch_bounds__(256) void gather_alias(const double2* __restrict__ in, double2* __restrict__ out,
		int nr, int nm, int ncin, int nphi, long in_bstride, long out_bstride, const double2* __restrict__ tab, double scale)
{
	const long idx = (long)blockIdx.x*blockDim.x + threadIdx.x;
	const int b = blockIdx.y;
	if (idx >= (long)nr*nm) return;
	const int m = (int)(idx / nr), r = (int)(idx - (long)m*nr);
	out[(long)b*out_bstride + idx] = tab_mul(in[(long)b*in_bstride + (long)r*ncin + (m % nphi)], tab[m], false, scale);
}

// leg[line][ring] *= w[ring] (DH / F2 analysis: plain quadrature weights)
__global__ __launch_bounds__(256) void scale_rings(double2* __restrict__ leg, long nlines, int nr, long ld, const double2* __restrict__ w)
{
	const long idx = (long)blockIdx.x*blockDim.x + threadIdx.x;
	if (idx >= nlines*nr) return;
	const long line = idx / nr; const int j = (int)(idx - line*nr);
	double2& v = leg[line*ld + j]; const double f = w[j].x;
	v.x *= f; v.y *= f;
}

// transpose of the parity mirror extension: out[line][j] = in[line][j] + sgn * in[line][mirror(j)], j < nr
// (self-mirrored samples -- pole rings -- are kept for even parity and dropped for odd parity)
__global__ __launch_bounds__(256) void fold_mirror(const double2* __restrict__ in, double2* __restrict__ out,
		int nr, long N, int c, long nlines, int par0)
{
	const long idx = (long)blockIdx.x*blockDim.x + threadIdx.x;
	if (idx >= nlines*nr) return;
	const long line = idx / nr; const int j = (int)(idx - line*nr);
	const bool odd = ((line + par0) & 1) != 0;
	const long mj = mirror_index(N, j, c);
	double2 v = in[line*N + j];
	if (mj == j) { if (odd) v = make_double2(0, 0); }
	else { const double2 w = in[line*N + mj]; if (odd) { v.x -= w.x; v.y -= w.y; } else { v.x += w.x; v.y += w.y; } }
	out[line*nr + j] = v;
}

// undo the pair packing of the theta FFTs (split_even_odd): out[line 2p][j], out[line 2p + 1][j] = the two parts * w[j] * scale
// for the real rings j < nr
__global__ __launch_bounds__(256) void split_pair(const double2* __restrict__ Z, double2* __restrict__ out,
		int nr, long N, int c, long npairs, long nlines, int par0, const double2* __restrict__ w, double scale)
{
	const long idx = (long)blockIdx.x*blockDim.x + threadIdx.x;
	if (idx >= npairs*nr) return;
	const long pr = idx / nr; const int j = (int)(idx - pr*nr);
	double2 a, b; split_even_odd(Z + pr*N, N, j, c, (par0 & 1) != 0, a, b);
	const double f = scale*(w ? w[j].x : 1.0);
	const long la = 2*pr, lb = la + 1;
	out[la*nr + j] = make_double2(a.x*f, a.y*f);
	if (lb < nlines) out[lb*nr + j] = make_double2(b.x*f, b.y*f);
}

// split_pair fused with the transpose of the ring FFT (synthesis through the CC grid): Z[pair][N] -> h[ring][m] * conj(tab[m]) * scale,
// through a 32 (m) x 32 (ring) LDS tile; saves writing and re-reading leg[m][ring] (2 x 10 GB at config 3)
__global__ __launch_bounds__(256) void split_pair_transposed(const double2* __restrict__ Z, double2* __restrict__ out,
		int nr, int nm, long N, int c, int par0, const double2* __restrict__ tab, double scale)
{
	PXS_SHARED(double2, tile);                       // [32 m][33]
	const int r0 = blockIdx.y*32, m0 = blockIdx.x*32;
	const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // tx: ring within tile, ty: 0..7
	const bool a_odd = (par0 & 1) != 0;              // parity of column 0; m0 is even, so of every even column
	for (int pj = ty; pj < 16; pj += 8) {            // 16 pairs = 32 columns m0 + 2 pj, m0 + 2 pj + 1
		const long pr = (m0 >> 1) + pj; const int j = r0 + tx;
		double2 a = make_double2(0, 0), b = a;
		if (j < nr && 2*pr < nm) split_even_odd(Z + pr*N, N, j, c, a_odd, a, b);
		tile[(2*pj)*33 + tx] = a;
		tile[(2*pj+1)*33 + tx] = b;
	}
	__syncthreads();
	for (int j = ty; j < 32; j += 8) {
		const int r = r0 + j, m = m0 + tx;
		if (r < nr && m < nm) out[(long)r*nm + m] = tab_mul(tile[tx*33 + j], tab[m], true, scale);
	}
}

} // namespace pxs

void scale_leg_rings(hipStream_t st, double2* leg, long nlines, int nr, long ld, const double2* w) {
	hipLaunchKernelGGL(scale_rings, dim3(blocks_of(nlines*nr)), dim3(256), 0, st, leg, nlines, nr, ld, w);
	PXS_HIP(hipGetLastError());
}

void leg_to_h(pxs_plan* p, hipStream_t st, const double2* leg, long ldleg, long ldh, int nc) {
	const int nm = p->mmax + 1, nr = p->nring;
	hipLaunchKernelGGL(transpose_tab<true>, dim3((nm+31)/32, (nr+31)/32, nc), dim3(256), sizeof(double2)*32*33, st, leg, p->hbuf.as<double2>(), nr, nm,
		(long)nm*ldleg, (long)nr*ldh, ldleg, ldh, (const double2*)p->phase.p, 1, 1.0);
}

// n lines of an FFT of the generic engine, dense along the line: line i reads from i*is and writes to i*os
static FftDims lines(long n, long is, long os) { FftDims d; d.n_i = n; d.is_i = is; d.os_i = os; return d; }

// (the unfused ring FFT of a map sizes its own packed spectra in hbuf; rings shorter than 2 mmax + 1 alias and go unpaired)
void unfused_map2leg(pxs_plan* p, hipStream_t st, const MapArg& m, int nc, double2* leg) {
	const int nm = p->mmax + 1, nr = p->nring;
	FftLoad ld; ld.ptr = (const char*)m.ptr + dtype_bytes(m.dtype)*p->ring_off0; ld.dtype = m.dtype;
	FftStore sf;
	if (2L*p->mmax < p->nphi) {
		// two real rings per complex transform; the pruned two-sided spectrum (|k| <= mmax) is unpacked in the transpose
		const int npair = (nr + 1)/2; const long rowlen = 2L*p->mmax + 1;
		p->hbuf.ensure(sizeof(double2)*(size_t)nc*std::max<size_t>((size_t)npair*rowlen, (size_t)nr*nm));
		FftDims d = lines(npair, p->ring_stride, rowlen); d.n_o1 = nc; d.is_o1 = m.cstride; d.os_o1 = (long)npair*rowlen; d.is_e = p->pix_stride;
		ld.mode = LD_REAL_PAIR; ld.pair_lines = nr;
		sf.ptr = p->hbuf.p; sf.two_sided_k = p->mmax; sf.compact_two_sided = 1;
		p->fc->exec(st, p->nphi, true, d, ld, sf);
		hipLaunchKernelGGL(unpack_pair_transpose, dim3((nm+31)/32, (npair+31)/32, nc), dim3(256), sizeof(double2)*2*32*33, st, (const double2*)p->hbuf.p, leg, nr, nm,
			(long)npair*rowlen, (long)nr*nm, (const double2*)p->phase.p, 1.0);
		return;
	}
	const int ncin = std::min(nm, p->nphi);           // distinct FFT bins needed (m >= nphi alias onto m mod nphi)
	p->hbuf.ensure(sizeof(double2)*(size_t)nc*nr*nm);
	FftDims d = lines(nr, p->ring_stride, ncin); d.n_o1 = nc; d.is_o1 = m.cstride; d.os_o1 = (long)nr*ncin; d.is_e = p->pix_stride;
	sf.ptr = p->hbuf.p; sf.ne = ncin;
	p->fc->exec(st, p->nphi, true, d, ld, sf);
	if (ncin == nm)
		hipLaunchKernelGGL(transpose_tab<false>, dim3((nm+31)/32, (nr+31)/32, nc), dim3(256), sizeof(double2)*32*33, st, (const double2*)p->hbuf.p, leg, nr, nm,
			(long)nr*nm, (long)nr*nm, (long)nm, (long)nr, (const double2*)p->phase.p, 0, 1.0);
	else
		hipLaunchKernelGGL(gather_alias, dim3(blocks_of((long)nr*nm), nc), dim3(256), 0, st, (const double2*)p->hbuf.p, leg, nr, nm, ncin, p->nphi,
			(long)nr*ncin, (long)nr*nm, (const double2*)p->phase.p, 1.0);
}

void unfused_h2map(pxs_plan* p, hipStream_t st, const MapArg& m, int nc) {
	const int nm = p->mmax + 1, nr = p->nring;
	const bool pairs = 2L*p->mmax < p->nphi;      // two rings per complex transform: Z = X_a + i X_b, real part -> ring 2q, imaginary part -> ring 2q+1
	FftDims d = lines(pairs ? (nr + 1)/2 : nr, nm, p->ring_stride); d.n_o1 = nc; d.is_o1 = (long)nr*nm; d.os_o1 = m.cstride; d.os_e = p->pix_stride;
	FftLoad ld; ld.ptr = p->hbuf.p; ld.ne = nm;
	FftStore sf; sf.ptr = (char*)m.ptr + dtype_bytes(m.dtype)*p->ring_off0; sf.dtype = m.dtype;
	if (pairs) { ld.mode = LD_HERM_PAIR; ld.pair_lines = nr; sf.real_pair = 1; sf.pair_lines = nr; }
	else { ld.mode = LD_HERM; ld.herm_fold = 1; }
	p->fc->exec(st, p->nphi, false, d, ld, sf);
}

// lines per pass of a resampler whose largest intermediate row has rowlen points; sizes b1 / b2 for it
static long resample_chunk(pxs_plan* p, long nlines_all, long rowlen) {
	const long chunk = std::max<long>(32, std::min<long>(nlines_all, (long)(p->resample_chunk_bytes/(sizeof(double2)*rowlen))));
	p->b1.ensure(sizeof(double2)*(size_t)chunk*std::max(p->th.N, p->th.Ncc));
	p->b2.ensure(sizeof(double2)*(size_t)chunk*rowlen);
	return chunk;
}

// leg on the map's rings [c][m][nring] -> weighted leg on the CC grid [c][m][ncc].
// Columns m and m+1 have opposite theta-parity, so their mirror extensions are the even and the odd part
// of ONE sequence: each pair shares the whole 4-FFT chain (every stage is linear and commutes with the
// reflection theta -> -theta) and is separated again at the end -- half the FFT work.
// (f: the fine circle, the pointwise table on it and the CC weights of the form of the analysis -- the |sin| series on
// M > N + 2 lmax points, or ducc0's route: the CC weights on M = 2 N_cc points, with the spectrum cut to |k| < M/2 when M <= N)
void resample_to_cc(pxs_plan* p, hipStream_t st, const double2* leg_in, double2* leg_cc, int nc, int spin, const AnaForm& f) {
	const ThetaTables& t = p->th; const int nm = p->mmax+1, nr = p->nring; const long M = f.M, N = t.N, Ncc = t.Ncc;
	const long npair_all = (nm + 1)/2, chunk = resample_chunk(p, npair_all, M);
	StageScope stage(p->prof, st, PXS_STAGE_RESAMPLE);
	p->pass_resample.begin();      // (the passes of the last component: every component takes the same ones)
	for (int c = 0; c < nc; c++)
	for (long p0 = 0; p0 < npair_all; p0 += chunk) {
		const long np = std::min<long>(chunk, npair_all - p0);
		if (c == nc - 1) p->pass_resample.add(np);
		const long m0 = 2*p0, nlines = std::min<long>(2*np, nm - m0);
		{	// (a) packed mirror extension of lines (2i, 2i+1), forward FFT_N
			FftLoad ld; ld.ptr = leg_in + ((size_t)c*nm + m0)*nr; ld.mode = LD_MIRROR_PAIR; ld.ne = nr; ld.mir_c = t.mir_c;
			ld.par0 = (spin + (int)m0) & 1; ld.pair_lines = nlines;
			FftStore sf; sf.ptr = p->b1.p;
			p->fc->exec(st, N, true, lines(np, nr, N), ld, sf);
		}
		{	// (b) shift to theta0 = 0, pad to M, backward FFT_M, multiply by the pointwise table
			FftLoad ld; ld.ptr = p->b1.p; ld.mode = LD_SPEC; ld.ne = N; ld.nyq_half = M > N ? 1 : 0; ld.kmax = M > N ? -1 : M/2 - 1; ld.mul = t.ph_shift.as<double2>();
			FftStore sf; sf.ptr = p->b2.p; sf.mul = f.sigma.as<double2>();
			p->fc->exec(st, M, false, lines(np, N, M), ld, sf);
		}
		{	// (c) forward FFT_M in place; only |k| <= lmax are needed
			FftLoad ld; ld.ptr = p->b2.p;
			FftStore sf; sf.ptr = p->b2.p; sf.two_sided_k = p->lmax;
			p->fc->exec(st, M, true, lines(np, M, M), ld, sf);
		}
		{	// (d) truncate to |k| <= lmax, backward FFT_Ncc onto the full CC circle
			FftLoad ld; ld.ptr = p->b2.p; ld.mode = LD_SPEC; ld.ne = M; ld.kmax = p->lmax;
			FftStore sf; sf.ptr = p->b1.p;
			p->fc->exec(st, Ncc, false, lines(np, M, Ncc), ld, sf);
		}
		// (e) separate the pair by reflection symmetry, keep rings 0..ncc-1, apply the quadrature weights
		hipLaunchKernelGGL(split_pair, dim3(blocks_of(np*t.ncc)), dim3(256), 0, st, (const double2*)p->b1.p,
			leg_cc + ((size_t)c*nm + m0)*t.ncc, t.ncc, Ncc, 0, np, nlines, (spin + (int)m0) & 1, f.wcc.as<double2>(), 1.0);
	}
	PXS_HIP(hipGetLastError());
}

// exact transpose of resample_to_cc: leg on the CC grid [c][m][ncc] -> leg on the map's rings [c][m][nring]
void resample_to_cc_adjoint(pxs_plan* p, hipStream_t st, const double2* leg_cc, double2* leg_out, int nc, int spin, const AnaForm& f) {
	const ThetaTables& t = p->th; const int nm = p->mmax+1, nr = p->nring; const long M = f.M, N = t.N, Ncc = t.Ncc;
	const long chunk = resample_chunk(p, nm, M);
	StageScope stage(p->prof, st, PXS_STAGE_RESAMPLE);
	p->pass_resample.begin();      // (the passes of the last component: every component takes the same ones)
	for (int c = 0; c < nc; c++)
	for (long m0 = 0; m0 < nm; m0 += chunk) {
		const long nl = std::min<long>(chunk, nm - m0);
		if (c == nc - 1) p->pass_resample.add(nl);
		{	// (d)^H: weights, zero-extend the rings to the Ncc circle, forward FFT_Ncc
			FftLoad ld; ld.ptr = leg_cc + ((size_t)c*nm + m0)*t.ncc; ld.ne = t.ncc; ld.mul = f.wcc.as<double2>();
			FftStore sf; sf.ptr = p->b1.p;
			p->fc->exec(st, Ncc, true, lines(nl, t.ncc, Ncc), ld, sf);
		}
		{	// (c)^H: embed |k| <= lmax into the M spectrum, backward FFT_M, multiply by the pointwise table
			FftLoad ld; ld.ptr = p->b1.p; ld.mode = LD_SPEC; ld.ne = Ncc; ld.kmax = p->lmax;
			FftStore sf; sf.ptr = p->b2.p; sf.mul = f.sigma.as<double2>();
			p->fc->exec(st, M, false, lines(nl, Ncc, M), ld, sf);
		}
		{	// (b)^H first half: forward FFT_M in place (only |k| <= N/2 needed)
			FftLoad ld; ld.ptr = p->b2.p;
			FftStore sf; sf.ptr = p->b2.p; sf.two_sided_k = M > N ? N/2 : -1;
			p->fc->exec(st, M, true, lines(nl, M, M), ld, sf);
		}
		{	// (b)^H second half + (a)^H FFT: truncate M -> N with the Nyquist combination and conj phase, backward FFT_N
			// (M <= N: the transpose of the low pass, zero padding of |k| < M/2)
			FftLoad ld; ld.ptr = p->b2.p; ld.mode = LD_SPEC_ADJ; ld.ne = M; ld.nyq_half = M > N ? 1 : 0; ld.kmax = M > N ? -1 : M/2 - 1; ld.mul = t.ph_shift.as<double2>();
			FftStore sf; sf.ptr = p->b1.p;
			p->fc->exec(st, N, false, lines(nl, M, N), ld, sf);
		}
		// (a)^H: fold the mirror images back onto the rings
		hipLaunchKernelGGL(fold_mirror, dim3(blocks_of(nl*nr)), dim3(256), 0, st, (const double2*)p->b1.p,
			leg_out + ((size_t)c*nm + m0)*nr, nr, N, t.mir_c, nl, (spin + (int)m0) & 1);
	}
	PXS_HIP(hipGetLastError());
}

// band-limited leg on the CC grid [c][m][ncc] -> leg on the map's rings [c][m][nring] (exact for degree <= lmax);
// columns (m, m+1) packed as in resample_to_cc
void resample_from_cc(pxs_plan* p, hipStream_t st, const double2* leg_cc, double2* leg_out, int nc, int spin, double2* h_out) {
	const ThetaTables& t = p->th; const int nm = p->mmax+1, nr = p->nring; const long N = t.N, Ncc = t.Ncc;
	const long npair_all = (nm + 1)/2, chunk = resample_chunk(p, npair_all, N);
	StageScope stage(p->prof, st, PXS_STAGE_RESAMPLE);
	p->pass_resample.begin();      // (the passes of the last component: every component takes the same ones)
	for (int c = 0; c < nc; c++)
	for (long p0 = 0; p0 < npair_all; p0 += chunk) {
		const long np = std::min<long>(chunk, npair_all - p0);
		if (c == nc - 1) p->pass_resample.add(np);
		const long m0 = 2*p0, nlines = std::min<long>(2*np, nm - m0);
		{	// packed mirror extension of the CC rings to the full circle, forward FFT_Ncc
			FftLoad ld; ld.ptr = leg_cc + ((size_t)c*nm + m0)*t.ncc; ld.mode = LD_MIRROR_PAIR; ld.ne = t.ncc; ld.mir_c = 0;
			ld.par0 = (spin + (int)m0) & 1; ld.pair_lines = nlines;
			FftStore sf; sf.ptr = p->b1.p;
			p->fc->exec(st, Ncc, true, lines(np, t.ncc, Ncc), ld, sf);
		}
		{	// keep |k| <= lmax, shift to the target grid's theta0, backward FFT_N onto the full circle
			FftLoad ld; ld.ptr = p->b1.p; ld.mode = LD_SPEC; ld.ne = Ncc; ld.kmax = p->lmax; ld.mul = t.ph_up.as<double2>();
			FftStore sf; sf.ptr = p->b2.p;
			p->fc->exec(st, N, false, lines(np, Ncc, N), ld, sf);
		}
		if (h_out && np == npair_all)	// separate the pair straight into the ring-major layout of the ring FFT (times e^{+i m phi0})
			hipLaunchKernelGGL(split_pair_transposed, dim3((nm+31)/32, (nr+31)/32), dim3(256), sizeof(double2)*32*33, st, (const double2*)p->b2.p,
				h_out + (size_t)c*nr*nm, nr, nm, N, t.mir_c, spin & 1, (const double2*)p->phase.p, 1.0/(double)Ncc);
		else	// separate the pair, keep the real rings
			hipLaunchKernelGGL(split_pair, dim3(blocks_of(np*nr)), dim3(256), 0, st, (const double2*)p->b2.p,
				leg_out + ((size_t)c*nm + m0)*nr, nr, N, t.mir_c, np, nlines, (spin + (int)m0) & 1, (const double2*)nullptr, 1.0/(double)Ncc);
	}
	PXS_HIP(hipGetLastError());
}
