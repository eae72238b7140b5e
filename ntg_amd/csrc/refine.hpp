// refine.hpp -- ntg_batch_refine: the coefficients of a spline on a finer knot grid, exactly (knot insertion, no fitting, no sampling).
//
// Fine coefficient j of an output is the blossom of the coarse spline at the fine knots t[j+1 .. j+k-1]: the de Boor triangle on the coarse
// knots tau, started from the k coarse coefficients c[mu-k+1 .. mu] of the span tau[mu] <= t[j] < tau[mu+1].  Level by level, widest knot
// differences first (w = k-1 .. 1, argument t[j+w]):
//     a = (t[j+w] - tau[mu-s]) / (tau[mu+w-s] - tau[mu-s]),   d[s] <- (1 - a) d[s+1] + a d[s],   s = 0 .. w-1,   d[s] = c[mu-s] at the start,
// and d[0] is the result.  Every denominator spans the non-empty interval [tau[mu], tau[mu+1]].  The form (1 - a) d0 + a d1 is kept on
// purpose: on identical grids every a that reaches d[0] is exactly 1, so the coefficients come back bit for bit.
// Neither augmented knot vector is materialised: both are read through the fine break sequence (RefKnots below, the rule of AugKnots in
// basis.hip); a coarse break takes the value of its partner among the fine breaks, so the inclusion of the knot vectors is exact although
// the two break sequences were accumulated separately (linspace) and differ in the last bits.
//
//   refine_shared_kernel  both plans on their own grids: the weights do not depend on the problem.  A workgroup runs the triangle on the k
//                         unit vectors once per fine coefficient and basis class (one thread per weight) -> band alpha[n_to][k] in LDS, then streams problems from
//                         a persistent loop: coalesced read of one x_from row into LDS, one thread per fine coefficient (k multiply-adds on
//                         LDS operands), coalesced store of the x_to row.  8 (nC_from + nC_to) bytes of HBM traffic per problem.
//   refine_pp_kernel      per-problem grids: one wavefront per problem (four problems per workgroup pass), its two break sequences and its
//                         x_from row staged in LDS, the conditions checked into the error word, the triangle run on the coefficients.
// No scratch: every private array below is indexed by unrolled loop counters only.  No atomics but the error word's.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include "ntg_dev.hpp"

#define NTG_REFINE_NT 256
#define NTG_REFINE_TOL 1e-12          // two breaks are partners when they differ by at most this times the knot range
#define NTG_REFINE_LDS_MAX (64 * 1024)
// error word of the per-problem path: (problem << 32) | (code << 24) | break -- the smallest wins, so it names the first offending problem
#define NTG_REFINE_E_ENDS 1           // first / last breaks do not agree
#define NTG_REFINE_E_PARTNER 2        // a break of `from` has no partner among `to`'s
#define NTG_REFINE_E_ORDER 3          // two breaks of `from` share a partner

struct RefineOut { int k, mf, mt, lf, lt, nf, nt, icf, ict, rep, aoff; };   // rep: first output with the same two spline spaces; aoff: its band in LDS
struct RefineArgs {
	int nout, batch, nCf, nCt, na, lmax_f, lmax_t;   // na: doubles of all bands; lmax: longest break sequences
	RefineOut o[NTG_MAX_OUT];
	const double *bf[NTG_MAX_OUT], *bt[NTG_MAX_OUT];   // break sequences of every output (shared grids); [0]: [batch][l + 1] (per-problem grids)
	const double *xf; double *xt;
	unsigned long long *err;
};

static inline size_t ntg_refine_lds(const RefineArgs &A, int pp)
{
	if (pp) return (size_t)(NTG_REFINE_NT / 64) * ((size_t)(A.lmax_t + 1 + A.nCf) * 8 + (size_t)(A.lmax_f + 2) * 4);
	return (size_t)(A.na + A.nCf + A.lmax_t + 1) * 8 + ((size_t)4 * A.nCt + A.lmax_f + 1) * 4;
}

// index of the break of tb[0 .. l] nearest to v
__host__ __device__ static inline int refine_partner(const double *tb, int l, double v)
{
	int lo = 0, hi = l;
	while (hi - lo > 1) {
		const int mid = (lo + hi) >> 1;
		if (tb[mid] <= v) lo = mid; else hi = mid;
	}
	return fabs(tb[hi] - v) < fabs(v - tb[lo]) ? hi : lo;
}

// augmented knots (0-based) read through the fine break sequence; pi != nullptr: the coarse knots, break b of `from` = tb[pi[b]]
struct RefKnots {
	const double *tb; const int *pi; int l, k, m, n;   // n = l (k - m) + m coefficients
	__device__ __forceinline__ int brk(int idx) const { return idx < k ? 0 : (idx >= n ? l : 1 + (idx - k) / (k - m)); }
	__device__ __forceinline__ double operator()(int idx) const { const int b = brk(idx); return tb[pi ? pi[b] : b]; }
};

// the knots one fine coefficient's triangle reads: tl[s] = tau[mu - s], tr[s] = tau[mu + 1 + s], tx[s] = t[j + 1 + s], s = 0 .. k - 2
struct RefTri {
	double tl[NTG_MAX_ORDER - 1], tr[NTG_MAX_ORDER - 1], tx[NTG_MAX_ORDER - 1];
	__device__ __forceinline__ void load(const RefKnots &tau, const RefKnots &t, int k, int j, int mu)
	{
#pragma unroll
		for (int s = 0; s < NTG_MAX_ORDER - 1; s++) {
			const bool on = s < k - 1;
			tl[s] = on ? tau(mu - s) : 0.0; tr[s] = on ? tau(mu + 1 + s) : 1.0; tx[s] = on ? t(j + 1 + s) : 0.0;
		}
	}
	// d[s] = c[mu - s] on entry; returns the fine coefficient
	__device__ __forceinline__ double run(int k, double (&d)[NTG_MAX_ORDER]) const
	{
#pragma unroll
		for (int w = NTG_MAX_ORDER - 1; w >= 1; w--) {
			if (w < k) {
				const double x = tx[w - 1];
#pragma unroll
				for (int s = 0; s < w; s++) {
					const double a = (x - tl[s]) / (tr[w - 1 - s] - tl[s]);
					d[s] = (1.0 - a) * d[s + 1] + a * d[s];
				}
			}
		}
		return d[0];
	}
};

// span of fine coefficient j: the last coarse knot index mu with tau[mu] <= t[j], found on break indices (pi is increasing, pi[0] = 0)
__device__ __forceinline__ int refine_span(const RefKnots &tau, const RefKnots &t, int j)
{
	const int bj = t.brk(j);
	int lo = 0, hi = tau.l;   // pi[lo] <= bj < pi[hi] (the last break is never reached: t[j] lies before it for every coefficient)
	while (hi - lo > 1) {
		const int mid = (lo + hi) >> 1;
		if (tau.pi[mid] <= bj) lo = mid; else hi = mid;
	}
	return tau.k - 1 + lo * (tau.k - tau.m);
}

template <int NT>
__global__ void __launch_bounds__(NT)
refine_shared_kernel(RefineArgs A)
{
	extern __shared__ __attribute__((aligned(16))) char smem_raw[];
	double *alpha = reinterpret_cast<double *>(smem_raw);   // bands of every basis class, [n_to][k] each: weight of c[mu - s] at [j][s]
	double *xrow = alpha + A.na;                             // [nC_from]
	double *tb = xrow + A.nCf;                               // fine breaks of the class being set up
	int *mul = reinterpret_cast<int *>(tb + A.lmax_t + 1);   // [nC_to] span of a class's coefficients (at its first output's slots)
	int *cb = mul + A.nCt, *ao = cb + A.nCt, *kk = ao + A.nCt;   // [nC_to] each: index of c[mu] in xrow, offset of the weights, order
	int *pi = kk + A.nCt;                                    // partners of the coarse breaks
	const int tid = threadIdx.x;
	for (int o = 0; o < A.nout; o++) {
		const RefineOut R = A.o[o];
		if (R.rep != o) continue;
		__syncthreads();   // the class before is done with tb / pi
		for (int i = tid; i <= R.lt; i += NT) tb[i] = A.bt[o][i];
		__syncthreads();
		for (int i = tid; i <= R.lf; i += NT) pi[i] = refine_partner(tb, R.lt, A.bf[o][i]);
		__syncthreads();
		const RefKnots tau{tb, pi, R.lf, R.k, R.mf, R.nf}, t{tb, nullptr, R.lt, R.k, R.mt, R.nt};
		for (int e = tid; e < R.nt * R.k; e += NT) {   // one thread per weight: the triangle on unit vector q
			const int j = e / R.k, q = e - j * R.k;
			const int mu = refine_span(tau, t, j);
			RefTri tri; tri.load(tau, t, R.k, j, mu);
			double d[NTG_MAX_ORDER];
#pragma unroll
			for (int s = 0; s < NTG_MAX_ORDER; s++) d[s] = s == q ? 1.0 : 0.0;
			alpha[R.aoff + e] = tri.run(R.k, d);
			if (q == 0) mul[R.ict + j] = mu;
		}
	}
	__syncthreads();
	for (int o = 0; o < A.nout; o++) {
		const RefineOut R = A.o[o];
		const int rict = A.o[R.rep].ict;
		for (int j = tid; j < R.nt; j += NT) { cb[R.ict + j] = R.icf + mul[rict + j]; ao[R.ict + j] = R.aoff + j * R.k; kk[R.ict + j] = R.k; }
	}
	__syncthreads();
	for (int b = blockIdx.x; b < A.batch; b += gridDim.x) {
		const double *src = A.xf + (size_t)b * A.nCf;
		for (int i = tid; i < A.nCf; i += NT) xrow[i] = src[i];
		__syncthreads();
		double *dst = A.xt + (size_t)b * A.nCt;
		for (int e = tid; e < A.nCt; e += NT) {
			const double *al = alpha + ao[e], *c = xrow + cb[e];
			const int k = kk[e];
			double acc = 0.0;
			for (int s = 0; s < k; s++) acc += al[s] * c[-s];
			dst[e] = acc;
		}
		__syncthreads();
	}
}

// per-problem grids: one basis class in each plan, so every output has the shape of output 0
template <int NT>
__global__ void __launch_bounds__(NT)
refine_pp_kernel(RefineArgs A)
{
	extern __shared__ __attribute__((aligned(16))) char smem_raw[];
	constexpr int NW = NT / 64;
	const RefineOut R = A.o[0];
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	// the doubles of every wave first (fine breaks, x_from row), then the ints (partners, the wave's error flag)
	double *tb = reinterpret_cast<double *>(smem_raw) + (size_t)wave * (R.lt + 1 + A.nCf);
	double *xrow = tb + R.lt + 1;
	int *pi = reinterpret_cast<int *>(reinterpret_cast<double *>(smem_raw) + (size_t)NW * (R.lt + 1 + A.nCf)) + (size_t)wave * (R.lf + 2);
	int *bad = pi + R.lf + 1;
	const int per_pass = gridDim.x * NW;
	for (int b0 = 0; b0 < A.batch; b0 += per_pass) {   // (the same trip count for every wave of the grid: the barriers below are uniform)
		const int b = b0 + blockIdx.x * NW + wave;
		const bool on = b < A.batch;
		__syncthreads();
		if (on) {
			const double *kt = A.bt[0] + (size_t)b * (R.lt + 1), *src = A.xf + (size_t)b * A.nCf;
			for (int i = lane; i <= R.lt; i += 64) tb[i] = kt[i];
			for (int i = lane; i < A.nCf; i += 64) xrow[i] = src[i];
			if (lane == 0) *bad = 0;
		}
		__syncthreads();
		if (on) {
			const double *kf = A.bf[0] + (size_t)b * (R.lf + 1);
			const double tol = NTG_REFINE_TOL * (tb[R.lt] - tb[0]);
			for (int i = lane; i <= R.lf; i += 64) {
				const double v = kf[i];
				const int p = refine_partner(tb, R.lt, v);
				pi[i] = p;
				int code = 0;
				if (!(fabs(tb[p] - v) <= tol)) code = (i == 0 || i == R.lf) ? NTG_REFINE_E_ENDS : NTG_REFINE_E_PARTNER;
				else if ((i == 0 && p != 0) || (i == R.lf && p != R.lt)) code = NTG_REFINE_E_ENDS;
				if (code) { *bad = 1; atomicMin(A.err, ((unsigned long long)b << 32) | ((unsigned long long)code << 24) | (unsigned long long)i); }
			}
		}
		__syncthreads();
		if (on) {
			for (int i = lane + 1; i <= R.lf; i += 64)
				if (pi[i] <= pi[i - 1]) { *bad = 1; atomicMin(A.err, ((unsigned long long)b << 32) | ((unsigned long long)NTG_REFINE_E_ORDER << 24) | (unsigned long long)i); }
		}
		__syncthreads();
		if (on && !*bad) {
			const RefKnots tau{tb, pi, R.lf, R.k, R.mf, R.nf}, t{tb, nullptr, R.lt, R.k, R.mt, R.nt};
			double *dst = A.xt + (size_t)b * A.nCt;
			for (int e = lane; e < A.nCt; e += 64) {
				const int o = e / R.nt, j = e - o * R.nt;
				const int mu = refine_span(tau, t, j);
				RefTri tri; tri.load(tau, t, R.k, j, mu);
				const double *c = xrow + o * R.nf + mu;
				double d[NTG_MAX_ORDER];
#pragma unroll
				for (int s = 0; s < NTG_MAX_ORDER; s++) d[s] = s < R.k ? c[-s] : 0.0;
				dst[e] = tri.run(R.k, d);
			}
		}
	}
}
