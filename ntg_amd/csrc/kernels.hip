// kernels.hip -- hand-written HIP kernels for gfx950 (MI355X) and their launchers.
//
//   basis_kernel    PGS knots/interv/bsplvb/bsplvd at every collocation point
//                   (reference call sites colloc.c:92-111; the Fortran is absent from the
//                   reference tree, algorithm from de Boor's PGS)
//   linrows_kernel  banded rows of the linear-constraint matrix (constraints.c:198-261)
//   bounds_kernel   bounds() (constraints.c:5-33)
//   host*_kernel    the evaluation of host-callback plans: Z = M C (compute_z, lds_tables.hpp) and the
//                   banded gradient / quadrature pass (cost_phase2, eval.hpp) around functors run on the host
//   (eval_kernel and sqp_kernel, the evaluation and the npsol_() call of ntg.c:250 for the compiled
//   families, are instantiated per family in fam_*.hip from eval.hpp and sqp_kernel.hpp)
//   check_kernel    trajectory rows of solved problems between the breakpoints (check.hpp; the
//                   last step of its reduction, check_final_kernel, is here)
//   cost_kernel     running cost of solved problems at arbitrary times, weighted sum per problem
//                   (cost.hpp; the sum over the time tiles, cost_final_kernel, is here)
//   verify_kernel   a family's analytic derivatives against central differences at the breakpoints
//                   (verify.hpp; the maximum over the breakpoint tiles, verify_final_kernel, is here)
//   kkt_kernel      first-order optimality residuals of a batch on the banded Jacobian (kkt.hpp)
//   envelope_*      bounds of every flag entry and linear trajectory row over whole pieces of the
//                   knot intervals, from the Bezier control polygons (envelope.hpp)
//   envelope_sos_*  the same for the nonlinear trajectory rows declared as sums of squares, by the
//                   Bezier product of those polygons (envelope_sos.hpp)
//   extrema_*       minimum and maximum of those rows over the horizon, enclosed to a tolerance, by
//                   bisection of the same polygons from a work list in LDS (extrema.hpp)
//   separation_kernel  smallest squared distance of pairs of bodies over the horizon: the squared
//                   difference of two trajectories as a sum-of-squares row, by that bisection (separation.hpp)
//   forms_*         minimum and maximum over the horizon of quadratic forms of the flag declared at the
//                   call: general Bezier products of the polygons, by that bisection (forms.hpp)
//
// Mapping to CDNA4: one workgroup per problem; breakpoints (then coefficients) across the
// lanes; basis tables, knots/breakpoints and the coefficient vector staged in LDS; the only
// HBM traffic inside a solve is the quasi-Newton history (coalesced, 8 B/lane); reductions are
// 64-lane wavefront shuffles + one LDS hop across the waves of the workgroup.
#include <hip/hip_runtime.h>
#include <math.h>
#include <algorithm>
#include "linesearch.hpp"
#include "nwt_map.hpp"
#include "lds_tables.hpp"
#include "eval.hpp"
#include "family_module.hpp"
#include "refine.hpp"
#include "envelope.hpp"
#include "envelope_sos.hpp"
#include "extrema.hpp"
#include "separation.hpp"
#include "forms.hpp"
#include "kkt.hpp"
#include "verify.hpp"


// ------------------------------------------------------------------------------------------
// PGS on the device.  The augmented knot vector is never materialised: t(idx) is read through
// the break sequence (knots(): first/last break k times, interior breaks k-m times).
// ------------------------------------------------------------------------------------------
struct AugKnots {
	const double *brk; int l, k, m;
	__device__ __forceinline__ double operator()(int idx1) const // 1-based like the Fortran
	{
		const int idx = idx1 - 1, n = l * (k - m) + m;
		if (idx < k) return brk[0];
		if (idx >= n) return brk[l];
		return brk[1 + (idx - k) / (k - m)];
	}
};

// interv on the break sequence (2nd-edition rule at the right end), 1-based interval index
__device__ __forceinline__ int interv_breaks(const double *brk, int l, double x)
{
	const int lxt = l + 1;
	if (x < brk[0]) return 1;
	if (x >= brk[lxt - 1]) {
		for (int i = lxt - 1; i >= 1; i--)
			if (brk[i - 1] < brk[lxt - 1]) return i;
		return 1;
	}
	int lo = 1, hi = lxt;
	while (hi - lo > 1) {
		const int mid = (lo + hi) >> 1;
		if (x >= brk[mid - 1]) lo = mid; else hi = mid;
	}
	return lo;
}

// bsplvb/bsplvd (PGS).  db is [nderiv][k] (m-major) == Fortran dbiatx(k,nderiv) column-major.
__device__ void bsplvd_dev(const AugKnots &t, int k, double x, int left, int nderiv, double *db)
{
	double a[NTG_MAX_ORDER * NTG_MAX_ORDER];
	double deltal[NTG_MAX_ORDER], deltar[NTG_MAX_ORDER];
	int j = 1;
	const int mhigh = max(min(nderiv, k), 1), kp1 = k + 1;
#define DB(r, c) db[((c) - 1) * k + ((r) - 1)]
#define A_(r, c) a[((c) - 1) * k + ((r) - 1)]
	auto raise = [&](int jhigh, double *biatx) {
		while (j < jhigh) {
			const int jp1 = j + 1;
			deltar[j - 1] = t(left + j) - x;
			deltal[j - 1] = x - t(left + 1 - j);
			double saved = 0.0;
			for (int i = 1; i <= j; i++) {
				const double term = biatx[i - 1] / (deltar[i - 1] + deltal[jp1 - i - 1]);
				biatx[i - 1] = saved + deltar[i - 1] * term;
				saved = deltal[jp1 - i - 1] * term;
			}
			biatx[jp1 - 1] = saved;
			j = jp1;
		}
	};
	db[0] = 1.0;
	raise(kp1 - mhigh, db);
	if (mhigh == 1) return;
	int ideriv = mhigh;
	for (int m = 2; m <= mhigh; m++) {
		int jp1mid = 1;
		for (int jj = ideriv; jj <= k; jj++) { DB(jj, ideriv) = DB(jp1mid, 1); jp1mid++; }
		ideriv--;
		raise(kp1 - ideriv, db);
	}
	int jlow = 1;
	for (int i = 1; i <= k; i++) {
		for (int jj = jlow; jj <= k; jj++) A_(jj, i) = 0.0;
		jlow = i;
		A_(i, i) = 1.0;
	}
	for (int m = 2; m <= mhigh; m++) {
		const int kp1mm = kp1 - m;
		const double fkp1mm = (double)kp1mm;
		int il = left, i = k;
		for (int ld = 1; ld <= kp1mm; ld++) {
			const double factor = fkp1mm / (t(il + kp1mm) - t(il));
			for (int jj = 1; jj <= i; jj++) A_(i, jj) = (A_(i, jj) - A_(i - 1, jj)) * factor;
			il--; i--;
		}
		for (i = 1; i <= k; i++) {
			double sum = 0.0;
			const int jl = i > m ? i : m;
			for (int jj = jl; jj <= k; jj++) sum = A_(jj, i) * DB(jj, m) + sum;
			DB(i, m) = sum;
		}
	}
#undef DB
#undef A_
}

// one thread per (grid, breakpoint); the grid's break sequence is staged in LDS
__global__ void basis_kernel(int ngrids, int l, int k, int m, int d, int P,
                             const double *__restrict__ knots, const double *__restrict__ bps,
                             long long knots_stride, long long bps_stride,
                             double *__restrict__ blk, int *__restrict__ off)
{
	extern __shared__ __attribute__((aligned(16))) char smem_raw[];
	double *sbrk = reinterpret_cast<double *>(smem_raw);
	const int g = blockIdx.y;
	if (g >= ngrids) return;
	for (int i = threadIdx.x; i <= l; i += blockDim.x) sbrk[i] = knots[g * knots_stride + i];
	__syncthreads();
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= P) return;
	const double x = bps[g * bps_stride + i];
	const int ivl = interv_breaks(sbrk, l, x);        // colloc.c:107 on the un-augmented knots
	const int left = k + (ivl - 1) * (k - m);         // == interv_ on the augmented knots (colloc.c:98)
	AugKnots t{sbrk, l, k, m};
	double db[NTG_MAX_ORDER * NTG_MAX_ORDER];
	bsplvd_dev(t, k, x, left, d, db);
	double *o = blk + ((size_t)g * P + i) * k * d;
	for (int q = 0; q < k; q++)
		for (int r = 0; r < d; r++) o[q * d + r] = db[r * k + q];   // FTranspose (colloc.c:100-101)
	off[(size_t)g * P + i] = (ivl - 1) * (k - m);                   // colloc.c:108
}

// ------------------------------------------------------------------------------------------
// linear-constraint rows (constraints.c:198-261 through colloc.c:243-316, band entries only)
// row order [lic; ltc constraint-major x breakpoint; lfc]; one thread per (row, band column)
// ------------------------------------------------------------------------------------------
__global__ void linrows_kernel(NtgDims D, NtgTables T, const double *__restrict__ lic,
                               const double *__restrict__ ltc, const double *__restrict__ lfc,
                               double *__restrict__ aband, int *__restrict__ rbp)
{
	const int idx = blockIdx.x * blockDim.x + threadIdx.x;
	if (idx >= D.nclin * D.sumk) return;
	const int r = idx / D.sumk, kc = idx % D.sumk;
	int o = 0;
	while (o + 1 < D.nout && D.koff[o + 1] <= kc) o++;
	const int q = kc - D.koff[o];
	const double *row; int bp;
	if (r < D.nlic) { row = lic + (size_t)r * D.nz; bp = 0; }
	else if (r < D.nlic + D.nltc * D.P) { const int rr = r - D.nlic; row = ltc + (size_t)(rr / D.P) * D.nz; bp = rr % D.P; }
	else { row = lfc + (size_t)(r - D.nlic - D.nltc * D.P) * D.nz; bp = D.P - 1; }
	const int c = D.cls[o], k = D.order[o], d = D.d[o];
	const double *b = T.blk + D.cls_blk[c] + ((size_t)bp * k + q) * d;
	double acc = 0.0;
	for (int l = 0; l < d; l++) acc += row[D.iz[o] + l] * b[l];
	aband[idx] = acc;
	if (kc == 0) rbp[r] = bp;
}

// bounds(): constraints.c:5-33
__global__ void bounds_kernel(NtgDims D, int batch, const double *__restrict__ lower,
                              const double *__restrict__ upper, double *__restrict__ bl,
                              double *__restrict__ bu, double big)
{
	const int ntot = D.nC + D.nclin + D.ncnln;
	const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (idx >= (long long)batch * ntot) return;
	const int b = idx / ntot, e = idx % ntot;
	double lo, up;
	if (e < D.nC) { lo = -big; up = big; }
	else {
		int r = e - D.nC, s;
		if (r < D.nlic) s = r;
		else if ((r -= D.nlic) < D.nltc * D.P) s = D.nlic + r / D.P;
		else if ((r -= D.nltc * D.P) < D.nlfc) s = D.nlic + D.nltc + r;
		else if ((r -= D.nlfc) < D.nnlic) s = D.nlic + D.nltc + D.nlfc + r;
		else if ((r -= D.nnlic) < D.nnltc * D.P) s = D.nlic + D.nltc + D.nlfc + D.nnlic + r / D.P;
		else { r -= D.nnltc * D.P; s = D.nlic + D.nltc + D.nlfc + D.nnlic + D.nnltc + r; }
		lo = lower[(size_t)b * D.nbounds + s]; up = upper[(size_t)b * D.nbounds + s];
	}
	bl[idx] = lo; bu[idx] = up;
}

// ------------------------------------------------------------------------------------------
// host-callback path of the ntg() drop-in: the user's C function pointers run on the host
// between two kernels -- updateZ (colloc.c:344-367) and the banded assembly + quadrature.
// ------------------------------------------------------------------------------------------
// Z in the reference layout Z[iZ[o] + d_o*bp + r], iZ[o] = iz[o]*P (colloc.c:328-331); only the
// declared active variables are written (the buffer persists like GZ, ntg.c:119)
template <int NT>
__global__ void __launch_bounds__(NT)
hostz_kernel(NtgDims D, NtgTables T, SmemLayout L, const double *__restrict__ x, u64 maskI, u64 maskT,
             u64 maskF, double *__restrict__ Z)
{
	extern __shared__ __attribute__((aligned(16))) char smem_raw[];
	Smem S(smem_raw, L, D, T);
	stage_tables<NT>(D, T, S, smem_raw, L);
	for (int i = threadIdx.x; i < D.nC; i += NT) S.x[i] = x[i];
	lds_sync();
	for (int i = threadIdx.x; i < D.P; i += NT) {
		const u64 mask = maskT | (i == 0 ? maskI : 0ull) | (i == D.P - 1 ? maskF : 0ull);
		if (!mask) continue;
		double z[NTG_MAX_NZ];
		compute_z<0, 0, 3>(D, S, S.x, i, mask, z);
		for (int o = 0; o < D.nout; o++)
			for (int r = 0; r < D.d[o]; r++)
				if ((mask >> (D.iz[o] + r)) & 1ull) Z[(size_t)D.iz[o] * D.P + (size_t)D.d[o] * i + r] = z[D.iz[o] + r];
	}
}

// fT [P], dfT [P][nz] = what ucf returned at each breakpoint; fdI/fdF [nz+1] = (df, f) of icf/fcf
template <int NT>
__global__ void __launch_bounds__(NT)
hostcost_kernel(NtgDims D, NtgTables T, SmemLayout L, const double *__restrict__ fT,
                const double *__restrict__ dfT, const double *__restrict__ fdI,
                const double *__restrict__ fdF, double *__restrict__ F, double *__restrict__ g)
{
	extern __shared__ __attribute__((aligned(16))) char smem_raw[];
	Smem S(smem_raw, L, D, T);
	stage_tables<NT>(D, T, S, smem_raw, L);
	const int P = D.P, nz = D.nz;
	for (int i = threadIdx.x; i < P; i += NT) S.fvals[i] = D.nucf ? fT[i] : 0.0;
	lds_sync();
	for (int e = threadIdx.x; e < P * nz; e += NT) { const int i = e / nz, v = e % nz; if (D.tav_row[v] >= 0) S.dfz[D.tav_row[v] * (P + 1) + i] = D.nucf ? S.wts[i] * dfT[e] : 0.0; }
	for (int v = threadIdx.x; v <= nz; v += NT) { S.dfi[v] = D.nicf ? fdI[v] : 0.0; S.dff[v] = D.nfcf ? fdF[v] : 0.0; }
	double gn2;
	const double val = cost_phase2<0, 0, NT, 3, 4>(D, S, S.vecs, &gn2, CoefMap<4>(), D.nicf != 0, D.nfcf != 0, 0.0, 0.0, nullptr, nullptr);
	if (threadIdx.x == 0) *F = val;
	for (int i = threadIdx.x; i < D.nC; i += NT) g[i] = S.vecs[i];
}

// dc [ncnln][nz]: row r holds the user's dc[constraint][variable] for constraint row r
// (rows: initial; trajectory constraint-major x breakpoint; final).  One lane per row.
__global__ void hostcon_kernel(NtgDims D, NtgTables T, const double *__restrict__ dc,
                               double *__restrict__ jband, double *__restrict__ cjac)
{
	const int row = blockIdx.x * blockDim.x + threadIdx.x;
	if (row >= D.ncnln) return;
	int bp;
	if (row < D.nnlic) bp = 0;
	else if (row < D.nnlic + D.nnltc * D.P) bp = (row - D.nnlic) % D.P;
	else bp = D.P - 1;
	const double *dcrow = dc + (size_t)row * D.nz;
	for (int o = 0; o < D.nout; o++) {
		const int k = D.order[o], cc = D.cls[o], d = D.d[o];
		const int col0 = D.iC[o] + T.off[cc * D.P + bp];
		for (int q = 0; q < k; q++) {
			double a = 0.0;
			for (int r = 0; r < d; r++) {
				const int chr = T.chrow[cc * NTG_MAX_ORDER + r];
				if (chr >= 0) a += dcrow[D.iz[o] + r] * T.rowv[chr + q * D.P + bp];
			}
			if (jband) jband[(size_t)row * D.sumk + D.koff[o] + q] = a;
			if (cjac) cjac[(size_t)(col0 + q) * D.ncnln + row] = a;
		}
	}
}

hipError_t ntg_launch_hostz(const NtgDims &D, const NtgTables &T, const SmemLayout &L, const double *x, u64 mI,
                            u64 mT, u64 mF, double *Z, hipStream_t st)
{
	auto kfn = hostz_kernel<128>;
	if (L.total > 64 * 1024) (void)hipFuncSetAttribute((const void *)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, L.total);
	hipLaunchKernelGGL(kfn, dim3(1), dim3(128), L.total, st, D, T, L, x, mI, mT, mF, Z);
	return hipGetLastError();
}
hipError_t ntg_launch_hostcost(const NtgDims &D, const NtgTables &T, const SmemLayout &L, const double *fT,
                               const double *dfT, const double *fdI, const double *fdF, double *F, double *g,
                               hipStream_t st)
{
	auto kfn = hostcost_kernel<128>;
	if (L.total > 64 * 1024) (void)hipFuncSetAttribute((const void *)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, L.total);
	hipLaunchKernelGGL(kfn, dim3(1), dim3(128), L.total, st, D, T, L, fT, dfT, fdI, fdF, F, g);
	return hipGetLastError();
}
hipError_t ntg_launch_hostcon(const NtgDims &D, const NtgTables &T, const double *dc, double *jband, double *cjac,
                              hipStream_t st)
{
	if (D.ncnln == 0) return hipSuccess;
	hipLaunchKernelGGL(hostcon_kernel, dim3((D.ncnln + 63) / 64), dim3(64), 0, st, D, T, dc, jband, cjac);
	return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// receding-horizon (MPC) shift, SURVEY.md §8f rank 2: after a solve, advance every problem to the
// breakpoint `sbp` of its own solution: (1) the linear initial-constraint bounds are re-pinned to
// the flat flag of the old solution at that breakpoint, b_r = sum_v lic[r][v] z_v(sbp) (the role
// NPSOL's warm start arrays istate/clambda/R were meant for, ntg.h:64-68, never used by the
// reference); (2) the coefficient vector is shifted by `sknot` knot intervals, C_new[j] =
// C_old[j + sknot (k-m)], the tail holding the last coefficient -- the warm start of the next solve.
// One workgroup per problem.
// ------------------------------------------------------------------------------------------
__global__ void mpc_shift_kernel(NtgDims D, NtgTables T, int batch, int sbp, int sknot, const double *__restrict__ lic,
                                 double *__restrict__ x, double *__restrict__ lower, double *__restrict__ upper)
{
	extern __shared__ __attribute__((aligned(16))) char smem_raw[];
	double *sx = (double *)smem_raw, *z = sx + ((D.nC + 1) & ~1);
	const int b = blockIdx.x, tid = threadIdx.x;
	if (b >= batch) return;
	for (int i = tid; i < D.nC; i += blockDim.x) sx[i] = x[(size_t)b * D.nC + i];
	__syncthreads();
	// flat flag of the old solution at breakpoint sbp (every derivative, Zvalue of colloc.c:318-326)
	for (int v = tid; v < D.nz; v += blockDim.x) {
		int o = 0;
		while (o + 1 < D.nout && D.iz[o + 1] <= v) o++;
		const int r = v - D.iz[o], k = D.order[o], d = D.d[o], c = D.cls[o];
		const double *bq = T.blk + (size_t)b * T.pp_blk + D.cls_blk[c] + (size_t)sbp * k * d;   // (per-problem grids: this problem's blocks)
		const double *cx = sx + D.iC[o] + T.off[c * D.P + sbp];
		double a = 0.0;
		for (int q = 0; q < k; q++) a += bq[q * d + r] * cx[q];
		z[v] = a;
	}
	__syncthreads();
	for (int r = tid; r < D.nlic; r += blockDim.x) {
		double a = 0.0;
		for (int v = 0; v < D.nz; v++) a += lic[(size_t)r * D.nz + v] * z[v];
		lower[(size_t)b * D.nbounds + r] = a;
		upper[(size_t)b * D.nbounds + r] = a;
	}
	for (int c = tid; c < D.nC; c += blockDim.x) {
		int o = 0;
		while (o + 1 < D.nout && D.iC[o + 1] <= c) o++;
		const int cl = c - D.iC[o], sh = sknot * (D.order[o] - D.mult[o]), src = cl + sh;
		x[(size_t)b * D.nC + c] = sx[D.iC[o] + (src < D.ncoef[o] ? src : D.ncoef[o] - 1)];
	}
}

hipError_t ntg_launch_mpc_shift(const NtgDims &D, const NtgTables &T, int batch, int sbp, int sknot, const double *lic,
                                double *x, double *lower, double *upper, hipStream_t st)
{
	if (batch <= 0) return hipSuccess;
	const size_t sm = (size_t)(((D.nC + 1) & ~1) + D.nz + 2) * 8;
	hipLaunchKernelGGL(mpc_shift_kernel, dim3(batch), dim3(128), sm, st, D, T, batch, sbp, sknot, lic, x, lower, upper);
	return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// launchers (called from plan.cpp, plan_build.cpp)
// ------------------------------------------------------------------------------------------
static inline int align16(int x) { return (x + 15) & ~15; }

// derivative orders named by the trajectory-constraint active variables: the channels the row emission of the banded Jacobian lists
// (eval_constraints / emit_decode; an upper bound is all the layout needs)
static int ntg_emit_channels(const NtgDims &D)
{
	unsigned um = 0;
	for (int o = 0; o < D.nout; o++)
		for (int r = 0; r < D.d[o] && r < NTG_MAX_ORDER; r++)
			if ((D.tcon_mask >> (D.iz[o] + r)) & 1ull) um |= 1u << r;
	return std::max(1, __builtin_popcount(um));
}

SmemLayout ntg_make_layout(const NtgDims &D, int nthreads, int nvec, int with_x, int hrc_pairs, int qp)
{
	SmemLayout L;
	int p = 0;
	const int npad = (D.nC + 1) & ~1;
	L.rowv = p; p = align16(p + D.row_total * 8);
	L.colp = p; p = align16(p + D.col_total * 4);
	L.chrow = p; p = align16(p + D.nclass * NTG_MAX_ORDER * 4);
	L.chcol = p; p = align16(p + D.nclass * NTG_MAX_ORDER * 4);
	L.off = p; p = align16(p + D.nclass * D.P * 4);
	L.bps = p; p = align16(p + D.P * 8);
	L.wts = p; p = align16(p + D.P * 8);
	L.x = p; if (with_x) p = align16(p + npad * 8);
	// [row][P+1] + a zero tail: the column form reads W consecutive entries from a column's first breakpoint
	{
		// the structured Newton mode borrows this area between evaluations: solve vectors and factorisation panels of every group
		// evaluation layout (nvec == 0): the cost pass touches the cost's rows only, and the constraint pass wants room for the
		// derivative rows of ONE constraint (it chunks over the constraints)
		const int ncomp = __builtin_popcountll(D.tcon_mask);
		L.dfz_rows = nvec > 0 ? D.ntav : std::max(D.ntav_cost, (ncomp * D.P + D.P) / (D.P + 1));
		if (L.dfz_rows < 1) L.dfz_rows = 1;
		L.tav_rows = nvec > 0 ? D.ntav : D.ntav_cost;
		int dfz_bytes = (L.dfz_rows * (D.P + 1) + ntg_dfz_tail(D)) * 8;
		if (D.nwt_on && nvec > 0) dfz_bytes = std::max(dfz_bytes, nwt_map(D, nthreads, qp, D.nwt_cg).bytes);   // (solve layouts only: the evaluation kernels never factor anything)
		L.dfz = p; L.nwt_y = p; p = align16(p + dfz_bytes);
	}
	L.fvals = p; p = align16(p + D.P * 8);
	L.red = p; p = align16(p + nwt_map(D, nthreads, qp, D.nwt_cg).red_doubles * 8);   // two halves of 16 values x waves (block_sum) + the Newton mode's flag words
	L.dfi = p; p = align16(p + (D.nz + 1) * 8);
	L.dff = p; p = align16(p + (D.nz + 1) * 8);
	// evaluation layouts (nvec == 0) carry no solver state: no vectors, multipliers or line-search records (config D's evaluation sits
	// 640 bytes under the two-workgroups-per-CU line)
	L.vecs = p; if (nvec > 0) p = align16(p + (nvec * npad + 2 * D.nclin + 2) * 8);
	L.lam = p; if (nvec > 0) p = align16(p + (D.nclin + 1) * 8);
	L.rho = L.c2 = p; L.hrc_n = hrc_pairs; p = align16(p + 2 * hrc_pairs * 8);   // (rho_i, c2_i) of a short quasi-Newton memory; longer ones keep them with the pair in HBM
	L.oinfo = p; p = align16(p + D.nout * 10 * 4);
	L.tavrow = p; p = align16(p + D.nz * 4);
	L.tcomp = p; p = align16(p + D.nz * 4);
	L.ls = p; if (nvec > 0) p = align16(p + 2 * (int)sizeof(LineSearch));   // double buffered (see sqp_kernel)
	L.tI = p; p = align16(p + (D.nI + 1) * 8);   // multiplier estimates of the linear inequality rows
	L.q_idx = L.q_col = L.q_val = p;
	L.with_lin = nvec > 0;
	if (D.q_use && L.with_lin) {
		L.q_idx = p; p = align16(p + D.nC * 2);
		L.q_col = p; p = align16(p + D.q_nt * D.q_w * 4);
		L.q_val = p; p = align16(p + D.q_nt * D.q_w * 8);
	}
	L.csr_ptr = L.csr_col = L.csr_val = L.csc_ptr = L.csc_row = L.csc_val = L.sinv_ptr = L.sinv_col = L.sinv_val = p;
	if (D.lin_lds && L.with_lin) {
		L.csr_ptr = p; p = align16(p + (D.nclin + 1) * 4);
		L.csr_col = p; p = align16(p + D.lin_nnz * 4);
		L.csr_val = p; p = align16(p + D.lin_nnz * 8);
		L.csc_ptr = p; p = align16(p + (D.nC + 1) * 4);
		L.csc_row = p; p = align16(p + D.lin_nnz * 4);
		L.csc_val = p; p = align16(p + D.lin_nnz * 8);
		L.sinv_ptr = p; p = align16(p + (D.nclin + 1) * 4);
		L.sinv_col = p; p = align16(p + D.sinv_nnz * 4);
		L.sinv_val = p; p = align16(p + D.sinv_nnz * 8);
	}
	// row emission of the banded Jacobian (eval_constraints): [64 lanes] (pair index | row slot) + [NTG_MAX_ORDER][64 lanes] (scratch offset,
	// table offset) + the number of listed channels -- decoded once per workgroup instead of once per problem
	L.emit = -1;
	if (nvec == 0 && D.nnltc > 0) { L.emit = p; p = align16(p + 64 * 4 + ntg_emit_channels(D) * 64 * 8 + 16); }
	L.total = p;
	return L;
}

// family dispatch: every family, built in (its translation unit fam_*.hip picks between its tuned -- compile-time nout / order -- instances
// and the generic one) or loaded from a module, launches through its descriptor (family_module.hpp, family_registry.cpp)
hipError_t ntg_launch_eval(const NtgDims &D, const NtgTables &T, const SmemLayout &L, const EvalArgs &a)
{
	const NtgFamily *f = ntg_family(D.family);
	return f ? f->launch_eval(D, T, L, a) : hipErrorInvalidValue;
}

hipError_t ntg_launch_sqp(const NtgDims &D, const NtgTables &T, const SmemLayout &L, const SolveParams &sp, const SqpArgs &a)
{
	const NtgFamily *f = ntg_family(D.family);
	return f ? f->launch_sqp(D, T, L, sp, a) : hipErrorInvalidValue;
}

hipError_t ntg_launch_check(const NtgDims &D, const NtgTables &T, const CheckArgs &a)
{
	const NtgFamily *f = ntg_family(D.family);
	return f ? f->launch_check(D, T, a) : hipErrorInvalidValue;
}

// ntg_batch_check, last step: the maximum over a problem's time tiles (check_kernel left one (violation, key) pair per tile; key = row *
// ntimes + time index, -1: none).  Equal violations: the smaller key.  One thread per problem, tiles in order.
__global__ void check_final_kernel(int batch, int ntiles, int ntimes, const double *__restrict__ pviol, const long long *__restrict__ pkey,
                                   double *__restrict__ viol, int *__restrict__ where)
{
	const int b = blockIdx.x * blockDim.x + threadIdx.x;
	if (b >= batch) return;
	double bv = 0.0; long long bk = -1;
	for (int i = 0; i < ntiles; i++) {
		const double v = pviol[(size_t)b * ntiles + i]; const long long k = pkey[(size_t)b * ntiles + i];
		if (v > bv || (v == bv && k >= 0 && (bk < 0 || k < bk))) { bv = v; bk = k; }
	}
	if (viol) viol[b] = bv;
	if (where) { where[2 * b] = bk < 0 ? -1 : (int)(bk / ntimes); where[2 * b + 1] = bk < 0 ? -1 : (int)(bk % ntimes); }
}
hipError_t ntg_launch_check_final(int batch, int ntiles, int ntimes, const double *pviol, const long long *pkey, double *viol, int *where, hipStream_t st)
{
	hipLaunchKernelGGL(check_final_kernel, dim3((batch + 127) / 128), dim3(128), 0, st, batch, ntiles, ntimes, pviol, pkey, viol, where);
	return hipGetLastError();
}

// ntg_batch_cost (cost.hpp): the family's cost_kernel instance ...
hipError_t ntg_launch_cost(const NtgDims &D, const NtgTables &T, const CostArgs &a)
{
	const NtgFamily *f = ntg_family(D.family);
	return f ? f->launch_cost(D, T, a) : hipErrorInvalidValue;
}

// ... and its last step: the sum over a problem's time tiles (cost_kernel left one weighted partial sum per tile).  One thread per
// problem, tiles in order.
__global__ void cost_final_kernel(int batch, int ntiles, const double *__restrict__ pcost, double *__restrict__ cost)
{
	const int b = blockIdx.x * blockDim.x + threadIdx.x;
	if (b >= batch) return;
	double s = pcost[(size_t)b * ntiles];
	for (int i = 1; i < ntiles; i++) s += pcost[(size_t)b * ntiles + i];
	cost[b] = s;
}
hipError_t ntg_launch_cost_final(int batch, int ntiles, const double *pcost, double *cost, hipStream_t st)
{
	hipLaunchKernelGGL(cost_final_kernel, dim3((batch + 127) / 128), dim3(128), 0, st, batch, ntiles, pcost, cost);
	return hipGetLastError();
}

// ntg_batch_verify (verify.hpp): the family's verify_kernel instance ...
hipError_t ntg_launch_verify(const NtgDims &D, const NtgTables &T, const VerifyArgs &a)
{
	const NtgFamily *f = ntg_family(D.family);
	return f ? f->launch_verify(D, T, a) : hipErrorInvalidValue;
}

// ... and its last step: the maximum over a problem's breakpoint tiles (verify_kernel left one (value, key) pair per tile, slot and kind),
// tiles in order under verify_take's total order, and the key taken apart into {function, breakpoint, flag entry}.  One thread per problem
// and (slot, kind); kind 0 goes to err / where, kind 1 to leak / leak_where, each of which may be null.
__global__ void verify_final_kernel(int batch, int ntiles, int nbps, int nz, const double *__restrict__ pval, const long long *__restrict__ pkey,
                                    double *__restrict__ err, int *__restrict__ where, double *__restrict__ leak, int *__restrict__ leak_where)
{
	constexpr int NQ = 2 * NTG_VERIFY_NSLOT;
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= batch * NQ) return;
	const int b = i / NQ, q = i - b * NQ, slot = q >> 1, kind = q & 1;
	double bv = pval[(size_t)b * ntiles * NQ + q]; long long bk = pkey[(size_t)b * ntiles * NQ + q];
	for (int t = 1; t < ntiles; t++) verify_take(bv, bk, pval[((size_t)b * ntiles + t) * NQ + q], pkey[((size_t)b * ntiles + t) * NQ + q]);
	double *ov = kind ? leak : err; int *ow = kind ? leak_where : where;
	const size_t o = (size_t)b * NTG_VERIFY_NSLOT + slot;
	if (ov) ov[o] = bv;
	if (ow) {
		const long long pt = bk >= 0 ? bk / nz : -1;
		ow[3 * o] = bk >= 0 ? (int)(pt / nbps) : -1; ow[3 * o + 1] = bk >= 0 ? (int)(pt % nbps) : -1; ow[3 * o + 2] = bk >= 0 ? (int)(bk % nz) : -1;
	}
}
hipError_t ntg_launch_verify_final(int batch, int ntiles, int nbps, int nz, const double *pval, const long long *pkey, double *err, int *where, double *leak,
                                   int *leak_where, hipStream_t st)
{
	const long long n = (long long)batch * 2 * NTG_VERIFY_NSLOT;
	hipLaunchKernelGGL(verify_final_kernel, dim3((unsigned)((n + 127) / 128)), dim3(128), 0, st, batch, ntiles, nbps, nz, pval, pkey, err, where, leak, leak_where);
	return hipGetLastError();
}

// ntg_batch_kkt (kkt.hpp): one pass for every family, built in or loaded.  hipErrorInvalidValue: one problem's vectors exceed the LDS.
hipError_t ntg_launch_kkt(const NtgDims &D, const NtgTables &T, const KktArgs &a) { return launch_kkt(D, T, a); }

hipError_t ntg_launch_basis(int ngrids, int l, int k, int m, int d, int P, const double *knots, const double *bps,
                            long long knots_stride, long long bps_stride, double *blk, int *off, hipStream_t st)
{
	const int nt = 64;
	dim3 grid((P + nt - 1) / nt, ngrids);
	hipLaunchKernelGGL(basis_kernel, grid, dim3(nt), (size_t)(l + 1) * 8, st, ngrids, l, k, m, d, P, knots, bps,
	                   knots_stride, bps_stride, blk, off);
	return hipGetLastError();
}

// Receding horizon: the multiplier estimates of the trajectory rows move sbp breakpoints towards the start (row (j, i) <- row (j, i + sbp));
// what enters the window at its end starts at 0.  alw: [batch][2][nal], estimates in the second half (what a warm-started solve reads).
// One workgroup per (problem, trajectory constraint); the read of element i + sbp happens before any lane writes it (two phases).
__global__ void mpc_shift_lambda_kernel(NtgDims D, int batch, int sbp, double *__restrict__ alw)
{
	extern __shared__ double s_row[];
	const int b = blockIdx.x / D.nnltc, j = blockIdx.x % D.nnltc, P = D.P, nal = D.ncnln + D.nI;
	if (b >= batch) return;
	double *t = alw + (size_t)b * 2 * nal + nal + D.nnlic + (size_t)j * P;
	for (int i = threadIdx.x; i < P; i += blockDim.x) s_row[i] = i + sbp < P ? t[i + sbp] : 0.0;
	__syncthreads();
	for (int i = threadIdx.x; i < P; i += blockDim.x) t[i] = s_row[i];
}
hipError_t ntg_launch_mpc_shift_lambda(const NtgDims &D, int batch, int sbp, double *alw, hipStream_t st)
{
	if (D.nnltc <= 0) return hipSuccess;
	hipLaunchKernelGGL(mpc_shift_lambda_kernel, dim3(batch * D.nnltc), dim3(128), (size_t)D.P * 8, st, D, batch, sbp, alw);
	return hipGetLastError();
}

// SplineInterp (colloc.c:449-484) for a batch: flat flag of every problem at ntimes shared points in time.
// tblk [class][t][q][r] and toff [class][t] come from basis_kernel run on the times instead of the breakpoints;
// one thread per (problem, time, flag entry), consecutive threads = consecutive flag entries of one time.
// Per-problem grids: every problem has its own times, basis blocks and offsets (pp != 0: tblk [batch][t][q][r], toff [batch][t]; one class).
__global__ void interp_kernel(NtgDims D, int batch, int ntimes, const double *__restrict__ x, const double *__restrict__ tblk,
                              const int *__restrict__ toff, const int *__restrict__ tblk_base, double *__restrict__ z, int pp)
{
	const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	const long long total = (long long)batch * ntimes * D.nz;
	if (idx >= total) return;
	const int v = (int)(idx % D.nz), t = (int)((idx / D.nz) % ntimes), b = (int)(idx / ((long long)D.nz * ntimes));
	int o = 0;
	while (o + 1 < D.nout && D.iz[o + 1] <= v) o++;
	const int r = v - D.iz[o], c = D.cls[o], kk = D.order[o], d = D.d[o];
	const double *blk = tblk + (pp ? (size_t)b * ntimes * kk * d : (size_t)tblk_base[c]) + ((size_t)t * kk) * d;
	const double *cx = x + (size_t)b * D.nC + D.iC[o] + toff[(pp ? (size_t)b : (size_t)c) * ntimes + t];
	double acc = 0.0;
	for (int q = 0; q < kk; q++) acc += blk[q * d + r] * cx[q];   // colloc.c:476-481
	z[idx] = acc;
}

hipError_t ntg_launch_interp(const NtgDims &D, int batch, int ntimes, const double *x, const double *tblk, const int *toff,
                             const int *tblk_base, double *z, hipStream_t st, int pp)
{
	const long long total = (long long)batch * ntimes * D.nz;
	if (total == 0) return hipSuccess;
	hipLaunchKernelGGL(interp_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, D, batch, ntimes, x, tblk, toff, tblk_base, z, pp);
	return hipGetLastError();
}

// ntg_batch_refine (refine.hpp): coefficients on a finer knot grid.  pp != 0: per-problem grids.  hipErrorInvalidValue: the tables exceed the LDS.
hipError_t ntg_launch_refine(const RefineArgs &A, int pp, int ncu, hipStream_t st)
{
	const size_t lds = ntg_refine_lds(A, pp);
	if (lds > NTG_REFINE_LDS_MAX) return hipErrorInvalidValue;   // (ntg_batch_refine refuses such a pair before it gets here)
	if (pp) {
		const int groups = (A.batch + NTG_REFINE_NT / 64 - 1) / (NTG_REFINE_NT / 64);
		hipLaunchKernelGGL(refine_pp_kernel<NTG_REFINE_NT>, dim3(std::min(groups, 8 * ncu)), dim3(NTG_REFINE_NT), lds, st, A);
	} else {
		// persistent workgroups: each builds its weights once, so each should stream several problems; no more than fill the device
		const int grid = std::max(1, std::min((A.batch + 7) / 8, 8 * ncu));
		hipLaunchKernelGGL(refine_shared_kernel<NTG_REFINE_NT>, dim3(grid), dim3(NTG_REFINE_NT), lds, st, A);
	}
	return hipGetLastError();
}

// The time certificates (envelope.hpp, envelope_sos.hpp, extrema.hpp).  Each has a kernel for per-problem grids (kpp: one problem per wave,
// a workgroup per nt / 64 problems) and one for shared grids (ksh: persistent workgroups; each builds its weights once, so each should
// stream several of the `units` of work: a workgroup for every four of them, no more than fill the device), both in the instance with the
// smallest private polygons that hold the plan's largest order (KM = 6 or NTG_MAX_ORDER).
template <class Args>
static hipError_t launch_cert(void (*kpp)(Args), void (*ksh)(Args), const Args &A, int nt, int units, int ncu, size_t lds, hipStream_t st)
{
	const int groups = (A.g.batch + nt / 64 - 1) / (nt / 64);
	auto kfn = A.g.pp ? kpp : ksh;
	if (lds > 64 * 1024) {
		const hipError_t e = hipFuncSetAttribute((const void *)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
		if (e != hipSuccess) return e;
	}
	const int grid = A.g.pp ? std::min(groups, 8 * ncu) : std::max(1, std::min((units + 3) / 4, 8 * ncu));
	hipLaunchKernelGGL(kfn, dim3(grid), dim3(nt), lds, st, A);
	return hipGetLastError();
}
#define NTG_CERT_LAUNCH(name, NT, units)                                                                                    \
	(A.g.kmax <= 6 ? launch_cert(name##_pp_kernel<NT, 6>, name##_shared_kernel<NT, 6>, A, NT, units, ncu, lds, st) \
	               : launch_cert(name##_pp_kernel<NT, NTG_MAX_ORDER>, name##_shared_kernel<NT, NTG_MAX_ORDER>, A, NT, units, ncu, lds, st))

// hipErrorInvalidValue: the tables exceed the LDS (the entry points refuse such a plan before it gets here).  On shared grids a workgroup of
// the two envelope calls takes one problem at a time ...
hipError_t ntg_launch_envelope(const EnvArgs &A, int ncu, hipStream_t st)
{
	const size_t lds = ntg_envelope_lds(A);
	if (lds > NTG_ENVELOPE_LDS_MAX || A.g.kmax > NTG_MAX_ORDER) return hipErrorInvalidValue;
	if (A.g.batch <= 0) return hipSuccess;
	return NTG_CERT_LAUNCH(envelope, NTG_ENVELOPE_NT, A.g.batch);
}
hipError_t ntg_launch_envelope_sos(const SosArgs &A, int ncu, hipStream_t st)
{
	const size_t lds = ntg_envelope_sos_lds(A);
	if (lds > NTG_ENVELOPE_LDS_MAX || A.g.kmax > NTG_MAX_ORDER || A.sos.nrow > NTG_SOS_MAXROWS) return hipErrorInvalidValue;
	if (A.g.batch <= 0) return hipSuccess;
	return NTG_CERT_LAUNCH(envelope_sos, NTG_ENVELOPE_NT, A.g.batch);
}
// ... and one of ntg_batch_extrema a pass of four problems, one per wave
hipError_t ntg_launch_extrema(const ExtArgs &A, int ncu, hipStream_t st)
{
	const size_t lds = ntg_extrema_lds(A);
	if (lds > NTG_EXTREMA_LDS_MAX || A.g.kmax > NTG_MAX_ORDER || A.sos.nrow > NTG_SOS_MAXROWS) return hipErrorInvalidValue;
	if (A.g.batch <= 0) return hipSuccess;
	return NTG_CERT_LAUNCH(extrema, NTG_EXTREMA_NT, (A.g.batch + NTG_EXTREMA_NT / 64 - 1) / (NTG_EXTREMA_NT / 64));
}
// ... and one of ntg_batch_forms likewise
hipError_t ntg_launch_forms(const FormArgs &A, int ncu, hipStream_t st)
{
	const size_t lds = ntg_forms_lds(A);
	if (lds > NTG_EXTREMA_LDS_MAX || A.g.kmax > NTG_MAX_ORDER || A.nform > NTG_FORM_MAXFORMS) return hipErrorInvalidValue;
	if (A.g.batch <= 0 || A.nform <= 0) return hipSuccess;
	return NTG_CERT_LAUNCH(forms, NTG_EXTREMA_NT, (A.g.batch + NTG_EXTREMA_NT / 64 - 1) / (NTG_EXTREMA_NT / 64));
}
#undef NTG_CERT_LAUNCH
// ... and one of ntg_batch_separation a pass of four pairs.  Shared grids only: the entry point refuses per-problem grids, so there is no kpp
hipError_t ntg_launch_separation(const SepArgs &A, int ncu, hipStream_t st)
{
	const size_t lds = ntg_separation_lds(A);
	constexpr int NT = NTG_EXTREMA_NT;
	if (lds > NTG_EXTREMA_LDS_MAX || A.g.kmax > NTG_MAX_ORDER || A.g.pp || A.g.nclass != 1) return hipErrorInvalidValue;
	if (A.npairs <= 0 || A.g.batch <= 0) return hipSuccess;
	const int units = (A.npairs + NT / 64 - 1) / (NT / 64);
	return A.g.kmax <= 6 ? launch_cert<SepArgs>(nullptr, separation_kernel<NT, 6>, A, NT, units, ncu, lds, st)
	                     : launch_cert<SepArgs>(nullptr, separation_kernel<NT, NTG_MAX_ORDER>, A, NT, units, ncu, lds, st);
}

// Flat flag -> state and input of the kinematic car, the map of examples/kincar.c:68-92 (kincar_flat_reverse), for every car
// of every problem at every time of an ntg_batch_interp result: z [n][nz] with the flag of car c at entries 6 c .. 6 c + 5
// (x, x', x'', y, y', y'') -> out [n][ncars][5] = x, y, theta, v, delta.  One thread per (sample, car).
__global__ void kincar_reverse_kernel(long long nsamp, int nz, int ncars, double wheelbase, int reverse_gear,
                                      const double *__restrict__ z, double *__restrict__ out)
{
	const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (idx >= nsamp * ncars) return;
	const long long smp = idx / ncars; const int c = (int)(idx - smp * ncars);
	const double *f = z + smp * nz + 6 * c;
	const double xd = f[1], xdd = f[2], yd = f[4], ydd = f[5];
	const double th = reverse_gear ? atan2(-yd, -xd) : atan2(yd, xd);   // kincar.c:78-86
	double sn, cs;
	sincos(th, &sn, &cs);
	const double thdot_v = ydd * cs - xdd * sn, v = xd * cs + yd * sn;   // kincar.c:89-90
	double *o = out + idx * 5;
	o[0] = f[0]; o[1] = f[3]; o[2] = th; o[3] = v; o[4] = atan2(thdot_v, v * v / wheelbase);   // kincar.c:91 (pow(u[0], 2.0) / b)
}
hipError_t ntg_launch_kincar_reverse(long long nsamp, int nz, int ncars, double wheelbase, int reverse_gear, const double *z, double *out, hipStream_t st)
{
	const long long total = nsamp * ncars;
	if (total == 0) return hipSuccess;
	hipLaunchKernelGGL(kincar_reverse_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, nsamp, nz, ncars, wheelbase, reverse_gear, z, out);
	return hipGetLastError();
}

// receding-horizon bookkeeping: how many problems of the last re-solve did not end with inform 0
__global__ void count_notconv_kernel(int batch, const int *__restrict__ inform, int *__restrict__ count)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	const int bad = (i < batch && inform[i] != 0) ? 1 : 0;
	const unsigned long long m = __ballot(bad);
	if ((threadIdx.x & 63) == 0 && m) atomicAdd(count, __popcll(m));
}
hipError_t ntg_launch_count_notconv(int batch, const int *inform, int *count, hipStream_t st)
{
	hipLaunchKernelGGL(count_notconv_kernel, dim3((batch + 255) / 256), dim3(256), 0, st, batch, inform, count);
	return hipGetLastError();
}

hipError_t ntg_launch_linrows(const NtgDims &D, const NtgTables &T, const double *lic, const double *ltc,
                              const double *lfc, double *aband, int *rbp, hipStream_t st)
{
	const int total = D.nclin * D.sumk;
	if (total == 0) return hipSuccess;
	hipLaunchKernelGGL(linrows_kernel, dim3((total + 127) / 128), dim3(128), 0, st, D, T, lic, ltc, lfc, aband, rbp);
	return hipGetLastError();
}

hipError_t ntg_launch_bounds(const NtgDims &D, int batch, const double *lo, const double *up, double *bl, double *bu,
                             hipStream_t st)
{
	const long long total = (long long)batch * (D.nC + D.nclin + D.ncnln);
	if (total == 0) return hipSuccess;
	hipLaunchKernelGGL(bounds_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, D, batch, lo, up, bl, bu,
	                   1.7976931348623157e308);
	return hipGetLastError();
}


