// kkt.hpp -- kkt_kernel: first-order optimality residuals of a batch of points (ntg_batch_kkt), fused: r = g - A' lam_A - J' lam_c on the
// band ntg_batch_eval just wrote, the violation and signed complementarity of every linear and nonlinear row, the maxima per problem.
// The dense Jacobian (ntg.c:250-253: the cJac NPSOL hands back next to clambda) is never formed.  Included by certs.hip only: the pass is
// the same for every family, built in or loaded.
//
// Mapping: one workgroup per problem, persistent workgroups walk the chunk.  r and x live in LDS for the whole pass.
//   1. r <- g, max |g|                                   lanes = coefficients
//   2. linear rows: a . x from the sparse row (CSR of the equality rows, ICSR of the declared inequalities: the values the solver reads,
//      this problem's own after ntg_plan_set_grids), violation and complementarity            lanes = rows
//   3. r -= A' lam_A (CSC / ICSC) and r -= J' lam_c, both with lanes = coefficients: a lane owns one word of r and subtracts into it in a
//      fixed ascending row order, so no two lanes ever add into one word.  J' lam_c is a GATHER on the band: coefficient cl of output o lies
//      in the block of the breakpoints bp with off[bp] <= cl < off[bp] + k, a contiguous range because off is non-decreasing (bisection on
//      the offset table in LDS); the lane reads jband[row][koff[o] + cl - off[bp]] for the initial rows, every trajectory row (j, bp) of the
//      range and the final rows.  Consecutive lanes are consecutive coefficients: where their ranges overlap they read consecutive words of
//      the same band row.  No row is skipped on lam = 0 (a skipped product could differ from the computed one by the sign of a zero).
//   4. nonlinear rows: violation and complementarity      lanes = rows, coalesced reads of c, lam, bl, bu
//   5. the six maxima: 64 lanes by DPP / permlane exchanges, the waves through LDS, in wave order.
// Maxima only, every sum owned by one lane in a fixed order: no floating-point atomics, the result does not depend on the order in which
// anything ran nor on the batch around a problem.  A NaN anywhere in a maximum's inputs stays in it (an audit must not lose one).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "ntg_dev.hpp"
#include "wave_ops.hpp"

// the larger of the two; a NaN, once in, stays
__device__ __forceinline__ double kkt_max(double a, double b) { return (b > a || b != b) ? b : a; }

template <int BIT>
__device__ __forceinline__ void kkt_xchg_step(double (&m)[NTG_KKT_NRES])
{
#pragma unroll
	for (int i = 0; i < NTG_KKT_NRES; i++) m[i] = kkt_max(m[i], lane_xchg<BIT>(m[i]));
}

// one row with value v, multiplier lam and bounds [bl, bu] (|.| >= NTG_INF_BOUND: absent): its violation max(bl - v, v - bu, 0) into viol,
// its complementarity lam+ s_lo + lam- s_up (slacks clipped to [0, 1], 1 for an absent bound) into comp
__device__ __forceinline__ void kkt_row(double v, double lam, double bl, double bu, double &viol, double &comp)
{
	const bool hl = fabs(bl) < NTG_INF_BOUND, hu = fabs(bu) < NTG_INF_BOUND;
	double w = 0.0;
	if (hl) w = kkt_max(w, bl - v);
	if (hu) w = kkt_max(w, v - bu);
	viol = kkt_max(viol, w);
	const double slo = hl ? fmin(fmax(v - bl, 0.0), 1.0) : 1.0, sup = hu ? fmin(fmax(bu - v, 0.0), 1.0) : 1.0;
	comp = kkt_max(comp, fmax(lam, 0.0) * slo + fmax(-lam, 0.0) * sup);
}

// the first breakpoint in [lo, P) whose block offset exceeds v, P if there is none (off is non-decreasing)
__device__ __forceinline__ int kkt_first_above(const int *off, int lo, int P, int v)
{
	int hi = P;
	while (lo < hi) { const int mid = (lo + hi) >> 1; if (off[mid] > v) hi = mid; else lo = mid + 1; }
	return lo;
}

template <int NT>
__global__ void __launch_bounds__(NT)
kkt_kernel(NtgDims D, NtgTables T, KktArgs a)
{
	extern __shared__ __attribute__((aligned(16))) char smem_raw[];
	__shared__ double s_red[NT / 64][NTG_KKT_NRES];
	const int nC = D.nC, P = D.P, sumk = D.sumk, nclin = D.nclin, ncnln = D.ncnln, ntot = nC + nclin + ncnln, npad = (nC + 1) & ~1;
	double *s_r = reinterpret_cast<double *>(smem_raw);   // [npad]
	double *s_x = s_r + npad;                             // [npad]
	int *s_off = reinterpret_cast<int *>(s_x + npad);     // [nclass][P]
	const int tid = threadIdx.x;
	for (int i = tid; i < D.nclass * P; i += NT) s_off[i] = T.off[i];
	for (int bl = blockIdx.x; bl < a.nb; bl += gridDim.x) {
		const int b = a.b0 + bl;   // bl: problem within this launch (the chunk's scratch is indexed by it), b: problem of the batch
		__syncthreads();           // the offsets are there; the previous problem's readers are done
		const double *g = a.g + (size_t)bl * nC, *x = a.x + (size_t)b * nC;
		const double *lamA = a.lam + (size_t)b * ntot + nC, *lamC = lamA + nclin;   // (the first nC entries are never read)
		const double *blo = a.bl + (size_t)bl * ntot + nC, *bup = a.bu + (size_t)bl * ntot + nC;   // bounds of the rows, linear first
		double m[NTG_KKT_NRES];
#pragma unroll
		for (int i = 0; i < NTG_KKT_NRES; i++) m[i] = 0.0;
		// 1. r <- g
		for (int i = tid; i < nC; i += NT) { const double gv = g[i]; s_r[i] = gv; s_x[i] = x[i]; m[1] = kkt_max(m[1], fabs(gv)); }
		__syncthreads();
		// 2. linear rows, one lane per row: equality e = rowmap[r] >= 0 in the CSR, inequality j = -rowmap[r] - 1 in the ICSR
		for (int r = tid; r < nclin; r += NT) {
			const int rm = T.rowmap[r], e = rm >= 0 ? rm : -rm - 1;
			const int *ptr = rm >= 0 ? T.csr_ptr : T.icsr_ptr, *col = rm >= 0 ? T.csr_col : T.icsr_col;
			const double *val = rm >= 0 ? T.csr_val + (size_t)b * T.pp_lin : T.icsr_val + (size_t)b * T.pp_ilin;
			double ax = 0.0;
			for (int q = ptr[e]; q < ptr[e + 1]; q++) ax += val[q] * s_x[col[q]];
			const double lv = lamA[r];
			kkt_row(ax, lv, blo[r], bup[r], m[2], m[4]);
			m[5] = kkt_max(m[5], fabs(lv));
		}
		// 3. r -= A' lam_A, r -= J' lam_c: one lane per coefficient, rows ascending
		const double *jb = a.jband + (size_t)bl * ncnln * sumk;
		int o = 0;
		for (int c = tid; c < nC; c += NT) {
			double acc = s_r[c];
			if (D.mE > 0) {
				const double *cv = T.csc_val + (size_t)b * T.pp_lin;
				for (int q = T.csc_ptr[c]; q < T.csc_ptr[c + 1]; q++) acc -= cv[q] * lamA[T.erow[T.csc_row[q]]];
			}
			if (D.nI > 0) {
				const double *cv = T.icsc_val + (size_t)b * T.pp_ilin;
				for (int q = T.icsc_ptr[c]; q < T.icsc_ptr[c + 1]; q++) acc -= cv[q] * lamA[T.irow[T.icsc_row[q]]];
			}
			if (ncnln > 0) {
				while (o + 1 < D.nout && D.iC[o + 1] <= c) o++;
				const int cl = c - D.iC[o], k = D.order[o];
				const int *off = s_off + D.cls[o] * P;
				// breakpoints [lo, hi) whose block holds cl: cl - k < off[bp] <= cl
				const int lo = kkt_first_above(off, 0, P, cl - k), hi = kkt_first_above(off, lo, P, cl);
				const double *je = jb + D.koff[o] + cl;   // row `row` at breakpoint bp holds this coefficient at je[row * sumk - off[bp]]
				if ((unsigned)(cl - off[0]) < (unsigned)k)
					for (int j = 0; j < D.nnlic; j++) acc -= lamC[j] * je[(long long)j * sumk - off[0]];
				for (int j = 0; j < D.nnltc; j++) {
					const int row0 = D.nnlic + j * P;
					for (int bp = lo; bp < hi; bp++)
						if ((unsigned)(cl - off[bp]) < (unsigned)k) acc -= lamC[row0 + bp] * je[(long long)(row0 + bp) * sumk - off[bp]];
				}
				if ((unsigned)(cl - off[P - 1]) < (unsigned)k)
					for (int j = 0; j < D.nnlfc; j++) { const int row = D.nnlic + D.nnltc * P + j; acc -= lamC[row] * je[(long long)row * sumk - off[P - 1]]; }
			}
			s_r[c] = acc;
			if (a.r) a.r[(size_t)b * nC + c] = acc;
			m[0] = kkt_max(m[0], fabs(acc));
		}
		// 4. nonlinear rows, one lane per row
		for (int i = tid; i < ncnln; i += NT) {
			const double lv = lamC[i];
			kkt_row(a.c[(size_t)bl * ncnln + i], lv, blo[nclin + i], bup[nclin + i], m[3], m[4]);
			m[5] = kkt_max(m[5], fabs(lv));
		}
		// 5. the maxima of the workgroup
		if (a.res) {
			kkt_xchg_step<1>(m); kkt_xchg_step<2>(m); kkt_xchg_step<4>(m); kkt_xchg_step<8>(m); kkt_xchg_step<16>(m); kkt_xchg_step<32>(m);
			if ((tid & 63) == 0) {
#pragma unroll
				for (int i = 0; i < NTG_KKT_NRES; i++) s_red[tid >> 6][i] = m[i];
			}
			__syncthreads();
			if (tid < NTG_KKT_NRES) {
				double v = s_red[0][tid];
				for (int w = 1; w < NT / 64; w++) v = kkt_max(v, s_red[w][tid]);
				a.res[(size_t)b * NTG_KKT_NRES + tid] = v;
			}
		}
	}
}

static hipError_t launch_kkt(const NtgDims &D, const NtgTables &T, const KktArgs &a)
{
	if (a.nb <= 0) return hipSuccess;
	auto kfn = kkt_kernel<NTG_KKT_NT>;
	const size_t lds = ntg_kkt_lds(D);
	if (lds > NTG_KKT_LDS_MAX) return hipErrorInvalidValue;   // (ntg_batch_kkt refuses such a plan before it gets here)
	if (lds > 64 * 1024) {
		const hipError_t e = hipFuncSetAttribute((const void *)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
		if (e != hipSuccess) return e;
	}
	hipLaunchKernelGGL(kfn, dim3(a.grid), dim3(NTG_KKT_NT), lds, a.st, D, T, a);
	return hipGetLastError();
}
