// lds_tables.hpp -- the LDS view of a plan: the carve-up of dynamic LDS (Smem), staging of the plan's tables into it,
// Z = M C at a breakpoint (compute_z) with the channel-mask helpers, the column form's reader and the lanes' coefficient
// map.  Used by eval.hpp, direction.hpp and sqp_kernel.hpp, and by the host-callback kernels of hostpath.hip.
#pragma once
#include <hip/hip_runtime.h>
#include "ntg_dev.hpp"

// ------------------------------------------------------------------------------------------
// LDS carve-up shared by eval_kernel and sqp_kernel
// ------------------------------------------------------------------------------------------
struct Smem {
	double *rowv; unsigned int *colp; int *chrow, *chcol;
	int *off; double *bps, *wts;
	double *x, *dfz, *fvals, *red, *dfi, *dff, *vecs, *lam, *rho, *c2;
	// sparse linear-constraint operator: LDS copies when they fit, HBM/L2 otherwise
	const int *csr_ptr, *csr_col, *csc_ptr, *csc_row, *sinv_ptr, *sinv_col; const double *csr_val, *csc_val, *sinv_val;
	int *oinfo, *tavrow, *tcomp;   // per-output scalars, flag->row map, flag->compact trajectory-constraint index, in LDS
	short *q_idx; int *q_col; double *q_val;
	int tav_rows;   // SmemLayout::tav_rows
	mutable int red_sel;   // which half of the reduction scratch the next block_sum writes (wave uniform)
	__device__ __forceinline__ Smem(char *base, const SmemLayout &L, const NtgDims &D, const NtgTables &T, int b = 0)
	{
		rowv = (double *)(base + L.rowv); colp = (unsigned int *)(base + L.colp);
		chrow = (int *)(base + L.chrow); chcol = (int *)(base + L.chcol);
		off = (int *)(base + L.off); bps = (double *)(base + L.bps);
		wts = (double *)(base + L.wts);
		x = (double *)(base + L.x); dfz = (double *)(base + L.dfz); fvals = (double *)(base + L.fvals);
		red = (double *)(base + L.red); dfi = (double *)(base + L.dfi); dff = (double *)(base + L.dff);
		vecs = (double *)(base + L.vecs); lam = (double *)(base + L.lam); rho = (double *)(base + L.rho);
		c2 = (double *)(base + L.c2);
		if (D.lin_lds && L.with_lin) {
			csr_ptr = (const int *)(base + L.csr_ptr); csr_col = (const int *)(base + L.csr_col); csr_val = (const double *)(base + L.csr_val);
			csc_ptr = (const int *)(base + L.csc_ptr); csc_row = (const int *)(base + L.csc_row); csc_val = (const double *)(base + L.csc_val);
			sinv_ptr = (const int *)(base + L.sinv_ptr); sinv_col = (const int *)(base + L.sinv_col); sinv_val = (const double *)(base + L.sinv_val);
		} else {
			csr_ptr = T.csr_ptr; csr_col = T.csr_col; csr_val = T.csr_val + (size_t)b * T.pp_lin;
			csc_ptr = T.csc_ptr; csc_row = T.csc_row; csc_val = T.csc_val + (size_t)b * T.pp_lin;
			sinv_ptr = T.sinv_ptr; sinv_col = T.sinv_col; sinv_val = T.sinv_val + (size_t)b * T.pp_sinv;
		}
		oinfo = (int *)(base + L.oinfo); tavrow = (int *)(base + L.tavrow); tcomp = (int *)(base + L.tcomp);
		q_idx = (short *)(base + L.q_idx); q_col = (int *)(base + L.q_col); q_val = (double *)(base + L.q_val);
		tav_rows = L.tav_rows; red_sel = 0;
	}
};

// b: the problem whose grid is staged (matters only with per-problem grids, NtgTables::pp_*)
template <int NT>
__device__ __forceinline__ void stage_tables(const NtgDims &D, const NtgTables &T0, const Smem &S, char *base, const SmemLayout &L, int b = 0)
{
	const int tid = threadIdx.x;
	NtgTables T = T0;
	T.rowv += (size_t)b * T0.pp_rowv; T.bps += (size_t)b * T0.pp_bps;
	T.csr_val += (size_t)b * T0.pp_lin; T.csc_val += (size_t)b * T0.pp_lin; T.sinv_val += (size_t)b * T0.pp_sinv; T.q_val += (size_t)b * T0.pp_q;
	for (int i = tid; i < D.row_total; i += NT) S.rowv[i] = T.rowv[i];
	for (int i = tid; i < D.col_total; i += NT) S.colp[i] = T.colp[i];
	for (int i = tid; i < D.nclass * NTG_MAX_ORDER; i += NT) { S.chrow[i] = T.chrow[i]; S.chcol[i] = T.chcol[i]; }
	for (int i = tid; i < D.nclass * D.P; i += NT) S.off[i] = T.off[i];
	for (int i = tid; i < D.P; i += NT) {
		S.bps[i] = T.bps[i];
		// trapezoid weight of breakpoint i: integrator.c:21-24 regrouped per node
		double w = 0.0;
		if (i > 0) w += (T.bps[i] - T.bps[i - 1]) / 2;
		if (i < D.P - 1) w += (T.bps[i + 1] - T.bps[i]) / 2;
		S.wts[i] = w;
	}
	if (D.lin_lds && L.with_lin) {
		int *rp = (int *)(base + L.csr_ptr), *rc = (int *)(base + L.csr_col), *cp = (int *)(base + L.csc_ptr), *cr = (int *)(base + L.csc_row);
		double *rv = (double *)(base + L.csr_val), *cv = (double *)(base + L.csc_val), *sv = (double *)(base + L.sinv_val);
		int *sp_ = (int *)(base + L.sinv_ptr), *sc = (int *)(base + L.sinv_col);
		for (int i = tid; i <= D.mE; i += NT) rp[i] = T.csr_ptr[i];
		for (int i = tid; i <= D.nC; i += NT) cp[i] = T.csc_ptr[i];
		for (int i = tid; i < D.lin_nnz; i += NT) { rc[i] = T.csr_col[i]; rv[i] = T.csr_val[i]; cr[i] = T.csc_row[i]; cv[i] = T.csc_val[i]; }
		for (int i = tid; i <= D.mE; i += NT) sp_[i] = T.sinv_ptr[i];
		for (int i = tid; i < D.sinv_nnz; i += NT) { sc[i] = T.sinv_col[i]; sv[i] = T.sinv_val[i]; }
	}
	// per-output scalars: k, m, preconditioner block, d, iC, iz, channel base, offset-table base, column-form width, ncoef
	for (int o = tid; o < D.nout; o += NT) {
		int *q = S.oinfo + o * 10;
		q[0] = D.order[o]; q[1] = D.mult[o]; q[2] = D.n0_blk[o]; q[3] = D.d[o]; q[4] = D.iC[o]; q[5] = D.iz[o];
		q[6] = D.cls[o] * NTG_MAX_ORDER; q[7] = D.cls[o] * D.P; q[8] = D.cls_W[D.cls[o]]; q[9] = D.ncoef[o];
	}
	for (int v = tid; v < D.nz; v += NT) {
		S.tavrow[v] = D.tav_row[v] < L.tav_rows ? D.tav_row[v] : -1;
		S.tcomp[v] = ((D.tcon_mask >> v) & 1ull) ? __popcll(D.tcon_mask & ((1ull << v) - 1ull)) : -1;   // see eval_constraints
	}
	for (int r = tid; r < L.dfz_rows; r += NT) S.dfz[r * (D.P + 1) + D.P] = 0.0;   // the row's extra element stays 0
	for (int i = tid; i < ntg_dfz_tail(D); i += NT) S.dfz[L.dfz_rows * (D.P + 1) + i] = 0.0;   // overrun of the last columns' reads (times 0)
	if (D.q_use && L.with_lin) {
		for (int i = tid; i < D.nC; i += NT) S.q_idx[i] = T.q_idx[i];
		for (int i = tid; i < D.q_nt * D.q_w; i += NT) { S.q_col[i] = T.q_col[i]; S.q_val[i] = T.q_val[i]; }
	}
}

// Z = M C at one breakpoint for the declared active variables (colloc.c:318-326,344-367);
// entries that are not active stay 0 like the reference's calloc'd GZ (ntg.c:119).
// CHM (channel mask, compile time): the instance was picked because the trajectory-cost active variables are exactly
// "derivative r of EVERY output, for the r in CHM" (kincar: CHM = 4, the second derivatives).  Rows, masks and channel
// tests that the general code looks up at run time are then constants.
__host__ __device__ constexpr int chm_count(int chm) { return (chm & 1) + ((chm >> 1) & 1) + ((chm >> 2) & 1) + ((chm >> 3) & 1) + ((chm >> 4) & 1); }
__host__ __device__ constexpr int chm_rank(int chm, int r) { return chm_count(chm & ((1 << r) - 1)); }
__host__ __device__ constexpr u64 chm_full_mask(int chm, int nout, int dm)
{
	u64 m = 0;
	for (int o = 0; o < nout; o++) for (int r = 0; r < dm; r++) if ((chm >> r) & 1) m |= 1ull << (dm * o + r);
	return m;
}
// does the plan match a channel-mask instance?  Running cost only, its active variables = derivative channels CHM of every
// output, no other weighted-gradient rows
static inline bool ntg_chm_match(const NtgDims &D, int chm, int dm)
{
	// (with trajectory constraints the mask is the one of the augmented-Lagrangian evaluation: cost and constraint variables)
	return D.nucf && !D.nicf && !D.nfcf && D.nnlic == 0 && D.nnlfc == 0 && (D.tcost_mask | D.tcon_mask) == chm_full_mask(chm, D.nout, dm) &&
	       D.ntav == D.nout * chm_count(chm);
}

template <int NOUT, int K, int DM, int CHM = 0>
__device__ __forceinline__ void compute_z(const NtgDims &D, const Smem &S, const double *sx, int bp,
                                          u64 mask, double *z, bool chm_ok = false)
{
	const int nout = NOUT > 0 ? NOUT : D.nout, P = D.P;
	if (NOUT > 0 && K > 0 && CHM != 0 && chm_ok) {
		// every output, the derivative channels of CHM, nothing else: no masks, no channel tests
		constexpr int KK = K > 0 ? K : 1, NCH = chm_count(CHM);
		double b[NCH > 0 ? NCH : 1][KK];
#pragma unroll
		for (int r = 0; r < DM; r++) {
			if (!((CHM >> r) & 1)) continue;
			const int ch = S.chrow[r];
#pragma unroll
			for (int q = 0; q < KK; q++) b[chm_rank(CHM, r)][q] = S.rowv[ch + q * P + bp];
		}
		const int ofs = S.off[bp], nco = D.ncoef[0];
#pragma unroll
		for (int o = 0; o < (NOUT > 0 ? NOUT : 1); o++) {
			const double *cx = sx + o * nco + ofs;
			double xv[KK];
#pragma unroll
			for (int q = 0; q < KK; q++) xv[q] = cx[q];
#pragma unroll
			for (int r = 0; r < DM; r++) {
				double acc = 0.0;
				if ((CHM >> r) & 1) {
#pragma unroll
					for (int q = 0; q < KK; q++) acc += b[chm_rank(CHM, r)][q] * xv[q];
				}
				z[DM * o + r] = acc;
			}
		}
		return;
	}
	if (NOUT > 0 && K > 0 && DM > 3 && D.uniform) {
		// one basis class, compile-time order, many derivatives: the coefficients of one output stay in
		// registers while its active derivative rows stream from LDS (keeping all DM rows would not fit)
		constexpr int KK = K > 0 ? K : 1;
		const int ofs = S.off[bp], nco = D.ncoef[0];
#pragma unroll
		for (int o = 0; o < (NOUT > 0 ? NOUT : 1); o++) {
			const double *cx = sx + o * nco + ofs;
			double xv[KK];
#pragma unroll
			for (int q = 0; q < KK; q++) xv[q] = cx[q];
#pragma unroll
			for (int r = 0; r < DM; r++) {
				double acc = 0.0;
				const int ch = S.chrow[r];
				if (((mask >> (DM * o + r)) & 1ull) && ch >= 0) {   // wave-uniform
#pragma unroll
					for (int q = 0; q < KK; q++) acc += S.rowv[ch + q * P + bp] * xv[q];
				}
				z[DM * o + r] = acc;
			}
		}
		return;
	}
	if (NOUT > 0 && K > 0 && D.uniform) {
		// one basis class, compile-time order, maxderiv == 3: the rows of the active derivative
		// channels at this breakpoint are read once into registers and reused by every output
		constexpr int KK = K > 0 ? K : 1;
		double b[3][KK];
#pragma unroll
		for (int r = 0; r < 3; r++) {
			const int ch = S.chrow[r];
			if (ch >= 0) {                                   // wave-uniform
#pragma unroll
				for (int q = 0; q < KK; q++) b[r][q] = S.rowv[ch + q * P + bp];
			} else {
#pragma unroll
				for (int q = 0; q < KK; q++) b[r][q] = 0.0;
			}
		}
		const int ofs = S.off[bp], nco = D.ncoef[0];
#pragma unroll
		for (int o = 0; o < (NOUT > 0 ? NOUT : 1); o++) {
			const double *cx = sx + o * nco + ofs;
			double xv[KK];
#pragma unroll
			for (int q = 0; q < KK; q++) xv[q] = cx[q];
#pragma unroll
			for (int r = 0; r < 3; r++) {
				double acc = 0.0;
				if ((mask >> (3 * o + r)) & 1ull) {           // wave-uniform
#pragma unroll
					for (int q = 0; q < KK; q++) acc += b[r][q] * xv[q];
				}
				z[3 * o + r] = acc;
			}
		}
		return;
	}
#pragma unroll
	for (int o = 0; o < nout; o++) {
		const int k = D.order[o], c = D.cls[o];
		const int d = NOUT > 0 ? DM : D.d[o], iz = NOUT > 0 ? DM * o : D.iz[o];
		const double *cx = sx + D.iC[o] + S.off[c * P + bp];
#pragma unroll
		for (int r = 0; r < (NOUT > 0 ? DM : NTG_MAX_ORDER); r++) {
			if (r >= d) break;
			double acc = 0.0;
			if ((mask >> (iz + r)) & 1ull) {
				const double *rv = S.rowv + S.chrow[c * NTG_MAX_ORDER + r] + bp;
				for (int q = 0; q < k; q++) acc += rv[q * P] * cx[q];
			}
			z[iz + r] = acc;
		}
	}
}

// column form of one collocation-matrix column (W entries, W a multiple of 4), see NtgTables::colp:
// word 0 = first breakpoint i0 of the column (its breakpoints are consecutive), then W/2 words of two 16-bit value
// indices each; a column occupies colp_words(W) words (multiple of 4: read as uint4)
template <int W>
__device__ __forceinline__ void colp_load(const unsigned int *cp, int &i0, unsigned int (&idx)[W])
{
	constexpr int WW = colp_words(W);
	unsigned int w[WW];
	const uint4 *cp4 = (const uint4 *)cp;
#pragma unroll
	for (int s4 = 0; s4 < WW / 4; s4++) { const uint4 t4 = cp4[s4]; w[4 * s4] = t4.x; w[4 * s4 + 1] = t4.y; w[4 * s4 + 2] = t4.z; w[4 * s4 + 3] = t4.w; }
	i0 = (int)w[0];
#pragma unroll
	for (int s = 0; s < W; s++) idx[s] = (w[1 + s / 2] >> (16 * (s & 1))) & 0xffffu;
}

// which coefficients a lane owns (c = tid + e*NT) and where their column-form data sit: decoded
// once per kernel, kept in registers for every evaluation of the solve
template <int EPT>
struct CoefMap {
	int o[EPT], cl[EPT];   // output and local coefficient index of slot e (c = tid + e*NT), o = -1: no coefficient
};
template <int NT, int EPT>
__device__ __forceinline__ void make_coefmap(const NtgDims &D, const Smem &S, CoefMap<EPT> &cm)
{
#pragma unroll
	for (int e = 0; e < EPT; e++) {
		const int c = threadIdx.x + e * NT;
		cm.o[e] = -1; cm.cl[e] = 0;
		if (c < D.nC) {
			int o = 0;
			while (o + 1 < D.nout && D.iC[o + 1] <= c) o++;
			cm.o[e] = o; cm.cl[e] = c - D.iC[o];
		}
	}
}
