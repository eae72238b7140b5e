// layout.cpp -- ntg_make_layout: the carve-up of a workgroup's dynamic LDS (SmemLayout, ntg_dev.hpp) for the evaluation, the host path
// and the solve.  Host code only.  The solve setup (plan_solve.cpp), the evaluation's launch shape (plan.cpp) and ntg_host.cpp size
// their launches with it; the structured Newton mode's share comes from nwt_map.hpp (tests/test_nwt_map.py restates both).
#include <algorithm>
#include "ntg_dev.hpp"
#include "plan.hpp"
#include "nwt_map.hpp"
#include "linesearch.hpp"

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
