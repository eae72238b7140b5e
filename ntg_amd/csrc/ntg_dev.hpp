// ntg_dev.hpp -- shared host/device declarations of the MI355X NTG engine (gfx950 only).
//
// Data layout in HBM (all fp64, indices int32):
//   blk   per basis CLASS (outputs with identical knots/order/mult/maxderiv share one table):
//         [bp][q][r] = D^r B_{off+q}(bps[bp])      == reference block[bp].matrix->elements[q][r]
//         (colloc.c:100-101); classes concatenated, class c starts at cls_blk[c]
//   off   [class][bp]  coefficient offset of the block (colloc.c:104-111)
//   aband [nclin][sumk] banded rows of the linear-constraint matrix A (constraints.c:198-261):
//         row r lives at breakpoint rbp[r]; for output o the k_o entries koff[o].. are the
//         columns iC[o]+off[cls[o]][rbp[r]]+q of the dense A the reference builds
//   x, g  [batch][nC]   coefficient vectors, problem-major (coalesced per workgroup)
//   hist  [batch][memcap][2][nC]  quasi-Newton pairs (s_i, u_i = W_i y_i)
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/ntg_amd.h"

typedef unsigned long long u64;

struct NtgDims {
	int nout, P, nz, nC, nclin, ncnln, nbounds, sumk;
	int nlic, nltc, nlfc, nnlic, nnltc, nnlfc;
	int nicf, nucf, nfcf;
	int family;
	int order[NTG_MAX_OUT], mult[NTG_MAX_OUT], ninterv[NTG_MAX_OUT], d[NTG_MAX_OUT];
	int ncoef[NTG_MAX_OUT], iC[NTG_MAX_OUT], iz[NTG_MAX_OUT], koff[NTG_MAX_OUT], cls[NTG_MAX_OUT];
	int nclass, blk_total;
	int cls_blk[NTG_MAX_OUT], cls_k[NTG_MAX_OUT], cls_d[NTG_MAX_OUT], cls_l[NTG_MAX_OUT], cls_m[NTG_MAX_OUT];
	u64 icost_mask, tcost_mask, fcost_mask, icon_mask, tcon_mask, fcon_mask;
	// running-cost gradient rows kept in LDS: only the flag entries that can be non-zero
	// (the declared trajectory-cost active variables; all of them for host callbacks)
	int ntav, ntav_cost;   // rows of the weighted-gradient area: all trajectory active variables; those of the cost come first
	signed char tav_row[NTG_MAX_NZ];   // flat flag index -> compact row, or -1
	int uniform;                        // 1: one basis class and equal ncoef for every output
	int mE, nI;                         // linear rows kept by projection (equalities) / handled by the AL loop (declared inequalities)
	int lin_nnz, lin_lds;               // sparse A_E (exact zeros dropped); 1: staged in LDS
	int sinv_nnz;                       // sparse (A A')^-1 (block diagonal when the rows decouple)
	int q_use, q_nt, q_w;               // projector Q = A'(AA')^-1 A kept as ELL over its non-zero rows
	int q_pin;                          // 1: the equality rows pin whole coefficients (as many touched columns as rows: the usual initial / final
	                                    // conditions) -- Q is then the identity on its non-zero rows, and g - Q g just zeroes those entries of g
	// collocation matrix of every ACTIVE (class, derivative) channel, in two sparse forms
	int row_total, col_total;           // doubles in rowv / entries in colv+coli
	int cls_W[NTG_MAX_OUT];             // padded (multiple of 4) support width of the column form, per class
	int cls_nc[NTG_MAX_OUT];            // coefficients per output of the class
	int n0_blk[NTG_MAX_OUT];            // which dense preconditioner block an output uses (NtgTables::n0b)
	int ch_row0[NTG_MAX_ORDER], ch_col0[NTG_MAX_ORDER];   // host copy of class 0's channel offsets (NtgTables::chrow/chcol)
	int tav_rmask;                      // union over outputs of the derivative indices with a cost AV
	// column form by VALUE for the lean evaluation kernel (class 0 only): per active derivative channel [nco][colv_stride]
	// doubles = the W basis values of the column at its consecutive breakpoints, then its first breakpoint (as a double);
	// colv_stride = W + 2: lanes that are consecutive columns read 16-byte words from 16 distinct bank groups
	int colv_total, colv_stride, ch_colv0[NTG_MAX_ORDER];
	// breakpoint groups of class 0 (consecutive breakpoints with the same block offset = one knot interval): ig_n groups,
	// group t = breakpoints [igb[t], igb[t+1]); ig_n = 0 when there are more than 64 groups or a group has more than 6 breakpoints
	int ig_n;
	unsigned short igb[66];
	// structured Newton mode (newton.hpp): coupling groups of nwt_go outputs, nwt_ng free coefficients each (interleaved by
	// output), half bandwidth nwt_hb, nwt_cg constraint flag entries per group; nwt_on = 0: the plan does not qualify
	int nwt_on, nwt_ngrp, nwt_go, nwt_ng, nwt_hb, nwt_cg;
	int nwt_tw, nwt_ja, nwt_jb;      // two-sided factorisation (newton.hpp, nwt_factor_pairs): on, block columns eliminated from the top / from the bottom
	int nwt_nfo, nwt_ngf, nwt_hbf;   // free outputs (in no nonlinear row): count, free coefficients and band half width of each; their factor is NtgTables::nwt_lf
	// breakpoint groups (consecutive breakpoints with the same block offset = one knot interval), how many consecutive
	// groups overlap a coefficient (colours of the assembly), and the constraint flag entries of a group packed one byte
	// each: (output within the group) << 4 | derivative
	int nwt_nint, nwt_cover;
	int nwt_tab;   // NtgTables::nwt_tu / nwt_g are there
	u64 nwt_upack;
	int nwt_clo, nwt_chi;               // the free local coefficients of every output: [clo, chi); free index p = (cl - clo) go + o
};

struct NtgTables {
	const double *bps;     // [P]
	const double *blk;     // [blk_total]
	const int *off;        // [nclass][P]
	const double *aband;   // [nclin][sumk]
	const int *rbp;        // [nclin]
	const double *sinv;    // [nclin][nclin]  (A A')^-1
	// preconditioner W0 = Z(Z'H0Z)^-1 Z' as ELL, s-major ([s][nC]) so that lanes with consecutive rows
	// read consecutive words; exact zeros dropped (block diagonal when outputs decouple); nullptr: none
	const double *n0; const unsigned short *n0c; int n0_w;
	// ... or, when W0 is block diagonal by output with equal block sizes: the distinct blocks, each s-major [s][row]
	// (see apply_n0_block); NtgDims::n0_blk maps outputs to blocks
	const double *n0b; int n0b_n, n0b_sp, n0b_nblk;   // rows per block, rows padded to 16 (zeros), distinct blocks
	// sparse A: CSR (rows) and CSC (columns)
	const int *csr_ptr, *csr_col; const double *csr_val;
	const int *csc_ptr, *csc_row; const double *csc_val;
	const int *sinv_ptr, *sinv_col; const double *sinv_val;   // CSR of (A A')^-1
	// rowv[chrow + q*P + bp]  = D^r B_{off(bp)+q}(bps[bp])      (by breakpoint: Z = M C, Jacobian rows)
	// colp[chcol + cl*WW ..] = column cl of the same matrix (its non-zeros sit at consecutive breakpoints): word 0 = the
	// first breakpoint i0, then W 16-bit value indices (q*P+i relative to chrow, two per word; padding = k*P, a stored
	// zero); the s-th entry multiplies the weighted gradient at breakpoint i0+s.  WW = colp_words(W) words per column.
	// chrow/chcol[class*NTG_MAX_ORDER + r] = channel offsets, -1 when no active variable uses D^r
	const double *rowv; const unsigned int *colp; const int *chrow, *chcol;
	const double *colv;    // see NtgDims::colv_total
	// Per-problem grids (ntg_plan_set_grids): the index tables above stay shared, the VALUES become per problem.  Problem b reads
	// rowv + b pp_rowv, bps + b pp_bps, csr_val + b pp_lin, csc_val + b pp_lin, sinv_val + b pp_sinv, q_val + b pp_q, n0b + b pp_n0b
	// (strides in elements; all 0 = one shared grid).
	long long pp_rowv, pp_bps, pp_lin, pp_sinv, pp_q, pp_n0b;
	long long pp_blk;   // ... and blk + b pp_blk (the full basis blocks: the receding-horizon shift evaluates the whole flag)
	long long pp_k0, pp_lf;   // ... nwt_k0 + b pp_k0, nwt_lf + b pp_lf: the structured Newton mode's cost model and free-output factors of every grid (grids.hip, grid_nwt_kernel)
	// linear rows: erow[mE] = original row of equality e; rowmap[nclin] = e, or -(j+1) for inequality j; linflag[slot]
	// = 1 for slots declared as inequalities; inequality rows as CSR (by row) and CSC (by coefficient)
	const int *erow, *rowmap, *linflag, *irow;
	const int *icsr_ptr, *icsr_col, *icsc_ptr, *icsc_row; const double *icsr_val, *icsc_val;
	// structured Newton mode: nwt_map[g][p] = coefficient of free entry p of group g; nwt_pos[c] = g * nwt_ng + p, or -1 for a
	// pinned coefficient; nwt_k0 = cost-model band [g][p][hb+1]; nwt_lo/hi[cl] = breakpoints [lo, hi) in whose block cl lies
	const int *nwt_map, *nwt_pos; const double *nwt_k0; const short *nwt_lo, *nwt_hi;
	// QP-based SQP step in the regime without constraint curvature (the model is the cost model K0, the same for every problem and major):
	// nwt_tu[i][u][p] = (K0^-1 M_i' e_u)[p], the column of W for flag entry u of a group at breakpoint i; nwt_g[k][i][v][u] = e_v' M_k K0^-1 M_i' e_u.
	// A slot's column W J' and its J U over all rows are then short combinations of table rows instead of a band solve and a breakpoint pass
	// (NtgDims::nwt_tab = 1: every coupling group has the same cost model, tables built with the plan)
	const double *nwt_tu, *nwt_g;
	const double *nwt_lf;   // [nwt_nfo][nwt_ngf][nwt_hbf + 1]: band Cholesky factor (diagonal inverted) of the free outputs' cost model, built with the plan
	const short *q_idx;    // [nC] row of coefficient c in the compact Q, or -1
	const unsigned char *q_pinned;   // [nC] 1: coefficient c is pinned by the equality rows (NtgDims::q_pin plans only)
	const int *q_col;      // [q_nt][q_w]
	const double *q_val;   // [q_nt][q_w], zero padded
	// per-problem family parameters (ntg_plan_set_params): problem b reads prm + b pp_prm (nullptr / 0: none set).  Read only on the device,
	// the same row for every lane of a problem; the family callbacks get it through FamCall (families.hpp)
	const double *prm; long long pp_prm;
	// per-problem grids with linear inequality rows: problem b reads icsr_val + b pp_ilin and icsc_val + b pp_ilin (0: one shared grid;
	// grids.hip, grid_ilin_kernel)
	long long pp_ilin;
};

// words per column of the column form (see NtgTables::colp)
__host__ __device__ constexpr int colp_words(int W) { return (W / 2 + 1 + 3) & ~3; }
// zero doubles kept after the last weighted-gradient row: a column's W reads start at its first breakpoint and may run past P
__host__ __device__ inline int ntg_dfz_tail(const NtgDims &D) { int w = 16; for (int c = 0; c < D.nclass; c++) w = D.cls_W[c] > w ? D.cls_W[c] : w; return w; }
// shape tests shared by the per-family dispatchers
static inline bool ntg_all_d(const NtgDims &D, int d) { for (int o = 0; o < D.nout; o++) if (D.d[o] != d) return false; return true; }
// 0 unless a tuned instance may run: one basis class, nC within the lanes' slots, no linear inequality rows (those
// are handled by the generic instances only)
static inline int ntg_uniform_order(const NtgDims &D, int nt, int ept) { return (D.uniform && D.nC <= ept * nt && D.nI == 0) ? D.order[0] : 0; }

// byte offsets into dynamic LDS, computed on the host (layout.cpp: ntg_make_layout)
#define NTG_HRC_LDS 64   // quasi-Newton memories up to this many pairs keep the pair scalars (rho, c2) in LDS, when that costs no residency

struct SmemLayout {
	int rowv, colp, chrow, chcol, off, bps, wts, x, dfz, fvals, red, dfi, dff, vecs, lam, rho, c2;
	int csr_ptr, csr_col, csr_val, csc_ptr, csc_row, csc_val, sinv_ptr, sinv_col, sinv_val, oinfo, tavrow, tcomp, q_idx, q_col, q_val, ls, tI, total;
	int with_lin;   // the linear-constraint operator (projector / CSR tables) is staged: solve layouts only, the evaluation never applies it
	int tav_rows;   // active-variable rows the cost pass may touch: all (solve) or the cost's only (evaluation: the others are not even allocated)
	int dfz_rows;   // rows of the weighted-gradient area: every active variable (solve) or the cost's / one constraint chunk's (evaluation)
	int hrc_n;   // pairs whose scalars (rho, c2) live in LDS at L.rho (0: they travel with the pair in HBM)
	int nwt_y;   // structured Newton mode: byte offset (inside the dfz area, which is idle between evaluations) of the solve vectors; panels follow
	int emit;    // evaluation layouts with trajectory constraint rows: byte offset of the row emission's per-lane decode (eval_constraints), -1: none
};

struct SolveParams {
	int itlim, memcap, ls_maxfev, hessian, fixed_iters;
	int stamps;   // diagnostic: clambda[b][0..7] receives per-phase cycle counts instead of multipliers
	int warm;     // augmented-Lagrangian rows: start from the multiplier estimates the previous solve left in the workspace
	double sr, steplimit, ls_mu, ls_eta;
};

// launcher arguments (host side)
struct EvalArgs { int nt, grid, ncu, batch, mode; const double *x; double *f, *g, *c, *jb, *cj; hipStream_t st; };
struct SqpArgs {
	int nt, big, batch; const double *lo, *up; double *x, *obj; int *inf, *it, *nf; double *cl, *hist, *alw, *vecw, *nwtw; hipStream_t st;
	unsigned int *counter;   // problem queue of the wave kernel (4 bytes inside the workspace)
};
// check_kernel (check.hpp): problems [b0, b0 + nb) of the batch at ntimes times each.  tblk / toff: basis_kernel's output at the times,
// [class][t][q][r] from gbase[c] and [class][t] on the shared grid (pp = 0), [nb][t][q][r] (pp_tab doubles per problem) and [nb][t] on
// per-problem grids (pp = 1).  lbase[c]: first row of class c in the LDS table, sumkd its rows.  rows / lo, up / pviol, pkey may be null:
// row values [batch][nltc + nnltc][ntimes]; bounds [batch][nbounds]; per-tile maxima [batch][ntiles] (violation, row * ntimes + time or -1).
#define NTG_CHECK_NT 128          // lanes of a check_kernel workgroup = times of one tile (host: ntiles and the per-tile pairs' indexing)
#define NTG_CHECK_LDS_STATIC 64   // upper bound of check_kernel's static LDS (the waves' reduction slots, a family's parameter slot)
struct CheckArgs {
	int b0, nb, ntimes, pp, ntiles, ngroups, sumkd;
	int gbase[NTG_MAX_OUT], lbase[NTG_MAX_OUT];
	long long pp_tab, times_stride;
	const double *x, *lo, *up, *times, *tblk, *ltc; const int *toff;
	double *rows, *pviol; long long *pkey;
	hipStream_t st;
};
// dynamic LDS of check_kernel for a plan: the tile's basis table [sum_c k_c d_c][NT + 1], the coefficient row, the offsets [nclass][NT]
static inline size_t ntg_check_lds(const NtgDims &D)
{
	size_t sumkd = 0;
	for (int c = 0; c < D.nclass; c++) sumkd += (size_t)D.cls_k[c] * D.cls_d[c];
	return (sumkd * (NTG_CHECK_NT + 1) + ((D.nC + 1) & ~1)) * 8 + (size_t)D.nclass * NTG_CHECK_NT * 4;
}
// ... and what a workgroup may ask for: 160 KiB less the static part
#define NTG_CHECK_LDS_MAX (160 * 1024 - NTG_CHECK_LDS_STATIC)

// cost_kernel (cost.hpp): the family's running cost at the times of the tile.  t: the tile fields of CheckArgs (b0 .. sumkd, gbase, lbase,
// pp_tab, times_stride, x, times, tblk, toff, st), filled by the walk ntg_batch_check and ntg_batch_cost share and read by the steps of
// time_tile.hpp; its row, bound and maxima fields are not used.  weights in the layout of times (null: no sum); vals [batch][ntimes] and pcost [batch][ntiles] (one weighted partial
// sum per tile) may be null.  LDS: that of check_kernel (ntg_check_lds; the static part is the waves' sums and a family's parameter slot).
struct CostArgs {
	CheckArgs t;
	const double *weights;
	double *vals, *pcost;
};

// verify_kernel (verify.hpp): the family's six callbacks against central differences at the breakpoints.  t: the tile fields of CheckArgs as
// for cost_kernel, filled by the same walk with the plan's (or every problem's own) breakpoints as the times.  pval / pkey
// [batch][ntiles][2 NTG_VERIFY_NSLOT]: per tile and slot the maxima (err, leak) and their keys (function * nbps + breakpoint) * nz + entry, -1: none.
// LDS: that of check_kernel (ntg_check_lds) plus a static part of its own: the waves' maxima and keys, a family's parameter slot.
#define NTG_VERIFY_LDS_STATIC 512
#define NTG_VERIFY_LDS_MAX (160 * 1024 - NTG_VERIFY_LDS_STATIC)
struct VerifyArgs {
	CheckArgs t;
	double *pval; long long *pkey;
};

// basis_kernel's output at the caller's times for problems [b0, b0 + nb) of the batch, as the host's one builder of these tables hands it
// out (plan_times.cpp): the fields of that name in CheckArgs, with the meaning stated there.  The tables are indexed by the problem within
// [b0, b0 + nb), everything of the caller's by the problem of the batch.
struct TimeTables {
	int b0, nb, pp;
	int gbase[NTG_MAX_OUT];
	long long pp_tab;
	const double *tblk; const int *toff;
};
// interp_kernel (times.hip): the flat flag of the problems of t at ntimes times each; x [batch][nC], z [batch][ntimes][nz]
struct InterpArgs {
	TimeTables t;
	int ntimes;
	const double *x; double *z;
};

// kkt_kernel (kkt.hpp): problems [b0, b0 + nb) of the batch, grid persistent workgroups.  x, lam ([batch][nC + nclin + ncnln], the first nC
// entries of a problem never read), res ([batch][NTG_KKT_NRES]) and r ([batch][nC]) are the caller's, indexed by the problem of the batch;
// either of res, r may be null.  g, c, jband (ntg_launch_eval's output) and bl, bu (ntg_launch_bounds') are the chunk's scratch, indexed by
// the problem within the launch.
#define NTG_KKT_NT 256
struct KktArgs {
	int b0, nb, grid;
	const double *x, *lam, *g, *c, *jband, *bl, *bu;
	double *res, *r;
	hipStream_t st;
};
// dynamic LDS of kkt_kernel for a plan: r and x, the offset table [nclass][P]; what a workgroup may ask for: 160 KiB less the static part
// (the waves' reduction slots)
static inline size_t ntg_kkt_lds(const NtgDims &D) { return (size_t)2 * ((D.nC + 1) & ~1) * 8 + (size_t)D.nclass * D.P * 4; }
#define NTG_KKT_LDS_MAX (160 * 1024 - 256)

// The time certificates (envelope.hpp, envelope_sos.hpp, extrema.hpp) enclose trajectory rows by their Bezier polygons on the knot intervals.
// Their kernel arguments are composed of three parts:
//   CertBase  the batch and its basis classes.  c[cl]: a class, its extraction weights [l][k][k] at eoff and interval lengths [l] at hoff in
//             the LDS table of ne doubles.  knots[cl]: the class's break sequence (shared grids); knots[0] = [batch][l + 1] on per-problem
//             grids (pp = 1, one class).  lower / upper [batch][nbounds] (null unless a violation is asked for).
//   CertLin   the linear trajectory rows: ltc [nltc][nz], read through the outputs' cls / d / iC / iz; their bound slots start at slot0.
//   CertSos   the nonlinear trajectory rows declared as sums of squares of shifted flag entries; their bound slots start at slot0.  row[j]: nt
//             terms, the basis class cl of the entries it names, the degree D of its polygon, flag = 1: certified (0: no statement, nothing
//             else of the row is read).  term[j][t]: coefficient offset iC of the output, its derivative order r, the shift's constant s0 and
//             the index poff into the problem's parameter row (np doubles at prm + b pp_prm) or -1.  w: the product tables W_d[i][j] =
//             C(d,i) C(d,j) / C(2d,i+j), d = 0 .. NTG_MAX_ORDER - 1, the upper triangles (i <= j) row by row, d ascending; the kernels
//             unfold them into LDS.
#define NTG_ENVELOPE_NT 256
#define NTG_ENVELOPE_LDS_MAX (64 * 1024)
#define NTG_SOS_MAXROWS 8
#define NTG_SOS_WTRI (NTG_MAX_ORDER * (NTG_MAX_ORDER + 1) * (NTG_MAX_ORDER + 2) / 6)     // doubles of the triangles
#define NTG_SOS_WFULL (NTG_MAX_ORDER * (NTG_MAX_ORDER + 1) * (2 * NTG_MAX_ORDER + 1) / 6) // doubles of the unfolded tables
struct EnvClass { int k, m, l, eoff, hoff; };
struct CertBase {
	int nC, nclass, batch, pp, ne, lmax, kmax, nbounds;
	EnvClass c[NTG_MAX_OUT];
	const double *knots[NTG_MAX_OUT];
	const double *x, *lower, *upper;
};
struct CertLin {
	int nout, nz, nltc, slot0;
	int cls[NTG_MAX_OUT], d[NTG_MAX_OUT], iC[NTG_MAX_OUT], iz[NTG_MAX_OUT];
	const double *ltc;
};
struct SosRow { int nt, cl, D, flag; };
struct SosTerm { int iC, r, poff, pad; double s0; };
struct CertSos {
	int nrow, slot0, np, pad;
	long long pp_prm;
	const double *prm;
	SosRow row[NTG_SOS_MAXROWS];
	SosTerm term[NTG_SOS_MAXROWS][NTG_SOS_MAXTERMS];
	double w[NTG_SOS_WTRI];
};
// table of degree d: offset of its triangle in CertSos::w, of its unfolded [d + 1][d + 1] form in LDS
static inline __host__ __device__ int ntg_sos_wtri(int d) { return d * (d + 1) * (d + 2) / 6; }
static inline __host__ __device__ int ntg_sos_wfull(int d) { return d * (d + 1) * (2 * d + 1) / 6; }

// ntg_batch_envelope (envelope.hpp): every flag entry and every linear trajectory row on the npc = lmax << nsub pieces of the knot intervals.
// Outputs as documented at ntg_batch_envelope, any may be null.
struct EnvArgs {
	CertBase g;
	CertLin lin;
	int nsub, npc;
	double *lo, *hi, *row_lo, *row_hi, *viol; int *where;
};
static_assert(sizeof(EnvArgs) <= 4096, "EnvArgs travels as a kernel argument");
// dynamic LDS: the tables, one coefficient row and one break sequence -- of the workgroup (shared grids) or of each of its waves
static inline size_t ntg_envelope_lds(const EnvArgs &A)
{
	return (size_t)(A.g.pp ? NTG_ENVELOPE_NT / 64 : 1) * (size_t)(A.g.ne + A.g.nC + A.g.lmax + 1) * 8;
}

// ntg_batch_envelope_sos (envelope_sos.hpp): the sum-of-squares rows on the same pieces.  Outputs as documented there, any may be null.
struct SosArgs {
	CertBase g;
	CertSos sos;
	int nsub, npc;
	double *q_lo, *q_hi, *viol; int *where;
};
static_assert(sizeof(SosArgs) <= 4096, "SosArgs travels as a kernel argument");
// dynamic LDS: the unfolded product tables, then the extraction tables, one coefficient row, one parameter row and one break sequence -- of
// the workgroup (shared grids) or of each of its waves
static inline size_t ntg_envelope_sos_lds(const SosArgs &A)
{
	return ((size_t)NTG_SOS_WFULL + (size_t)(A.g.pp ? NTG_ENVELOPE_NT / 64 : 1) * (size_t)(A.g.ne + A.g.nC + A.sos.np + A.g.lmax + 1)) * 8;
}

// The bisection calls (extrema.hpp, separation.hpp, forms.hpp, ratios.hpp) share the level loop of extrema.hpp, and with it:
//   CertBisect  the call's figures and outputs.  koff[cl]: the breaks of class cl in the LDS table of nk doubles (the times of the piece ends
//               need them after the weights are built).  Outputs as documented at ntg_batch_extrema, any may be null.
//   ExtLds      what a wave works with: the workgroup's (or its own) tables and its own rows and work list, all in LDS.
//   BisectLds   where those lie in the dynamic LDS, in doubles and in this order: `front` doubles of tables every wave reads (the product
//               tables); the extraction tables (ne) and breaks (nk) of every class; per wave the coefficient row (nrow), the parameter row
//               (nprm) and the work list of NTG_EXTREMA_CAP elements of W doubles with one key each behind it.  Per-problem grids (pp): the
//               class tables and breaks are the wave's own and lead its part.  The host sizes every launch from this one description
//               (W from the plan, by the rule that picks the instance); the forms and ratios kernels form their pointers from it too,
//               with the W of their instance's piece, staging through ExtStage and handing ExtLds, the read-only view, to everything
//               below.  The extrema and separation kernels carve the same places by hand (extrema.hpp says why).
#define NTG_EXTREMA_NT 256
struct CertBisect {
	int max_depth, sides, nk, pad;
	double tol;
	int koff[NTG_MAX_OUT];
	double *ext, *when, *viol; int *status, *npieces, *where;
};
struct ExtLds {
	const double *wl, *tab, *kns, *xrow, *prow;
	double *list;        // [NTG_EXTREMA_CAP][W]
	long long *keys;     // [NTG_EXTREMA_CAP]: interval << 32 | index of the piece at its level
};
// ... and the same places writable, for the kernel that stages them; everything below the staging gets the view
struct ExtStage {
	double *wl, *tab, *kns, *xrow, *prow, *list;
	long long *keys;
	__host__ __device__ __forceinline__ ExtLds view() const { return ExtLds{wl, tab, kns, xrow, prow, list, keys}; }
};
struct BisectLds {
	int front, ne, nk, nrow, nprm, W, pp;
	__host__ __device__ __forceinline__ size_t wave_doubles() const { return (size_t)(pp ? ne + nk : 0) + nrow + nprm + (size_t)NTG_EXTREMA_CAP * (W + 1); }
	__host__ __device__ __forceinline__ size_t bytes(int nw) const { return ((size_t)front + (pp ? 0 : ne + nk) + (size_t)nw * wave_doubles()) * 8; }
	__host__ __device__ __forceinline__ ExtStage wave(double *base, int w) const   // (inlined: the pointers stay in registers)
	{
		double *tab = base + front + (pp ? (size_t)w * wave_doubles() : 0), *kns = tab + ne;
		double *xrow = kns + nk + (pp ? 0 : (size_t)w * wave_doubles()), *prow = xrow + nrow, *list = prow + nprm;
		return ExtStage{base, tab, kns, xrow, prow, list, reinterpret_cast<long long *>(list + NTG_EXTREMA_CAP * W)};
	}
};
// ... and what a workgroup may ask for: 160 KiB less the static part (the row, term and class tables)
#define NTG_EXTREMA_LDS_MAX (160 * 1024 - 2048)
// doubles of a single polygon as a work-list element; the instance (KM = 6 or NTG_MAX_ORDER) follows from the plan's largest order
static inline __host__ __device__ int ntg_bisect_kd(const CertBase &G) { return G.kmax <= 6 ? 11 : 2 * NTG_MAX_ORDER - 1; }

// ntg_batch_extrema (extrema.hpp): the global minimum and maximum of every certifiable trajectory row over the horizon, each enclosed to tol,
// with the time where the attained value sits.  Rows: the lin.nltc linear trajectory rows, then the sos.nrow nonlinear ones.
struct ExtArgs {
	CertBase g;
	CertLin lin;
	CertSos sos;
	CertBisect q;
};
static_assert(sizeof(ExtArgs) <= 4096, "ExtArgs travels as a kernel argument");
// dynamic LDS: the unfolded product tables in front; a coefficient row and the rows' parameter row per wave
static __host__ __device__ __forceinline__ BisectLds ntg_extrema_layout(const ExtArgs &A, int W) { return BisectLds{NTG_SOS_WFULL, A.g.ne, A.q.nk, A.g.nC, A.sos.np, W, A.g.pp}; }
static inline size_t ntg_extrema_lds(const ExtArgs &A) { return ntg_extrema_layout(A, ntg_bisect_kd(A.g)).bytes(NTG_EXTREMA_NT / 64); }

// ntg_batch_separation (separation.hpp): the smallest squared distance over the horizon of pairs of bodies, each body ndim outputs of one
// basis class.  g holds that ONE class (nclass = 1, its tables at offset 0 of the LDS table, kmax its order) and the batch the pairs'
// problem indices are checked against.  sos: the product tables, and row 0 with ndim terms {coefficient offset t n, derivative deriv, no
// shift} -- the sum of squares of the pair's difference coefficients delta [ndim][n], which a wave stages in place of a coefficient row.
// biC[g][t]: the coefficient offset of coordinate t of body g.  pairs [npairs][4] = {a, b, ga, gb}; sep [npairs] or null.
// Outputs as documented at ntg_batch_separation, any may be null.
struct SepArgs {
	CertBase g;
	CertSos sos;
	int npairs, nbody, ndim, n, max_depth, pad;
	double tol;
	int biC[NTG_MAX_OUT][NTG_SEP_MAXDIM];
	const int *pairs; const double *sep;
	double *min, *when, *viol; int *status, *npieces;
};
static_assert(sizeof(SepArgs) <= 4096, "SepArgs travels as a kernel argument");
// dynamic LDS: the unfolded product tables in front; the breaks of the one class; per wave delta where a coefficient row would be, no
// parameter row.  The limit is ntg_batch_extrema's
static __host__ __device__ __forceinline__ BisectLds ntg_separation_layout(const SepArgs &A, int W) { return BisectLds{NTG_SOS_WFULL, A.g.ne, A.g.lmax + 1, A.ndim * A.n, 0, W, 0}; }
static inline size_t ntg_separation_lds(const SepArgs &A) { return ntg_separation_layout(A, ntg_bisect_kd(A.g)).bytes(NTG_EXTREMA_NT / 64); }

// ntg_batch_forms (forms.hpp): the minimum and maximum over the horizon of quadratic forms of the flat flag that the CALLER declares, each a sum
// of weighted products w (z[u] - a)(z[v] - b) and weighted linear terms w (z[u] - a).  term[f][t] in the kernels' form: the coefficient offsets
// iCu / iCv of the two factors' outputs, their derivative orders ru / rv (the degrees follow from the class: max(k - 1 - r, 0)), the indices
// pu / pv into the problem's row of fprm [batch][nfp] or -1, the kind, the weight w and the shifts' constants su / sv.  row[f]: nt terms, the
// basis class cl of every entry the form names, the degree D of its polygon.  flo / fhi [batch][nform] (null unless a violation is asked
// for).  Outputs (q) as documented at ntg_batch_forms, any may be null.
#define NTG_FORM_LIN 0      // w (z[u] - a)
#define NTG_FORM_PROD 1     // w (z[u] - a)(z[v] - b)
#define NTG_FORM_SQUARE 2   // ... with the same entry, parameter and constant twice: formed as envelope_sos.hpp forms a square
struct FormTerm { int iCu, iCv, pu, pv; short ru, rv, kind, pad; double w, su, sv; };
struct FormRow { int nt, cl, D, t0; };   // t0: the form's first term where the terms of all forms lie in one flat table (MinmaxArgs); 0 here
struct FormArgs {
	CertBase g;
	int nform, nfp;
	CertBisect q;
	FormRow row[NTG_FORM_MAXFORMS];
	FormTerm term[NTG_FORM_MAXFORMS][NTG_FORM_MAXTERMS];
	const double *fprm, *flo, *fhi;
};
static_assert(sizeof(FormArgs) <= 4096, "FormArgs travels as a kernel argument");
// the product tables W_{d,e}[i][j] = C(d,i) C(e,j) / C(d+e,i+j) of every pair of degrees 0 <= d, e < NTG_MAX_ORDER, [d + 1][e + 1] each, e
// fastest: doubles of all of them, and where the table of (d, e) starts
#define NTG_FORM_WALL ((NTG_MAX_ORDER * (NTG_MAX_ORDER + 1) / 2) * (NTG_MAX_ORDER * (NTG_MAX_ORDER + 1) / 2))
static inline __host__ __device__ int ntg_form_woff(int d, int e) { return (NTG_MAX_ORDER * (NTG_MAX_ORDER + 1) / 2) * (d * (d + 1) / 2) + (d + 1) * (e * (e + 1) / 2); }
// dynamic LDS: the product tables (built on the device) in front; a coefficient row and a row of fprm per wave.  The limit is
// ntg_batch_extrema's (the static part is the Pascal triangle the product tables are built from)
static __host__ __device__ __forceinline__ BisectLds ntg_forms_layout(const FormArgs &A, int W) { return BisectLds{NTG_FORM_WALL, A.g.ne, A.q.nk, A.g.nC, A.nfp, W, A.g.pp}; }
static inline size_t ntg_forms_lds(const FormArgs &A) { return ntg_forms_layout(A, ntg_bisect_kd(A.g)).bytes(NTG_EXTREMA_NT / 64); }

// ntg_batch_ratios (ratios.hpp): the minimum and maximum over the horizon of ratios of products of the forms of a FormArgs, R = prod num /
// prod den.  f: the forms exactly as ntg_batch_forms declares them (its outputs are the ratios' [batch][nratio] arrays, flo / fhi the ratios'
// bounds).  r[q]: the forms of each side, the basis class cl of all of them, the degrees dN / dD of the sides and DR = max of both; pn / pd:
// for factor a >= 1 of a side the index of the product table its step of the chain uses.  Table q: degrees pd [q] (the chain so far) and
// pe [q] (the form), (pd + 1)(pe + 1) doubles at poff [q] of the npw doubles all tables have; the kernels build them.  kr: points of the
// private polygons (13 or 25), nw: waves of a workgroup (4, or 2 where the work lists of four do not fit).
#define NTG_RATIO_MAXPAIRS (2 * NTG_RATIO_MAXRATIOS * (NTG_RATIO_MAXFACTORS - 1))
struct RatioRow { unsigned char nnum, nden, cl, dN, dD, DR, num[NTG_RATIO_MAXFACTORS], den[NTG_RATIO_MAXFACTORS], pn[NTG_RATIO_MAXFACTORS - 1], pd[NTG_RATIO_MAXFACTORS - 1]; };
struct RatioArgs {
	FormArgs f;
	unsigned char nratio, npair, kr, nw;
	unsigned short npw, pad;
	RatioRow r[NTG_RATIO_MAXRATIOS];
	unsigned char pd[NTG_RATIO_MAXPAIRS], pe[NTG_RATIO_MAXPAIRS];
	unsigned short poff[NTG_RATIO_MAXPAIRS];
};
static_assert(sizeof(RatioArgs) <= 4096, "RatioArgs travels as a kernel argument");
// dynamic LDS: the forms' product tables and the chains' (both built on the device) in front; a coefficient row and a row of fprm per wave; a
// work-list element is a pair of polygons, numerator first.  The limit is ntg_batch_extrema's
static __host__ __device__ __forceinline__ BisectLds ntg_ratios_layout(const RatioArgs &A, int W) { return BisectLds{NTG_FORM_WALL + A.npw, A.f.g.ne, A.f.q.nk, A.f.g.nC, A.f.nfp, W, A.f.g.pp}; }
static inline size_t ntg_ratios_lds(const RatioArgs &A, int nw) { return ntg_ratios_layout(A, 2 * A.kr).bytes(nw); }

// ntg_batch_trig (trig.hpp): the minimum and maximum over the horizon of sums of sines and cosines of linear combinations of the flat flag that
// the CALLER declares, h = sum_t w_t g_t(theta_t).  term[f][t] in the kernels' form and ORDER: the form's SIN and COS terms first, in declared
// order (row[f].ntrig of them: term t is polygon t of a piece), then its nlin LIN terms in declared order, whose weighted angle polygons are
// summed at level 0 into the one polygon a piece carries behind the trig terms'.  iC / r: coefficient offset of the output and derivative order
// of every entry (the degree follows from the class: max(k - 1 - r, 0)); dt: the largest of those degrees; pp: index into the problem's row of
// fprm [batch][nfp] or -1.  row[f]: the basis class cl of every entry the form names, the degree D of its polygons (the largest dt), and
// W = sum_t |w_t|, declared order.  nprm: doubles of the wave's fprm row in LDS (nfp, padded so that the work list starts at 16 bytes), nw:
// waves of a workgroup (4, or 2 where the work lists of four do not fit).  flo / fhi [batch][nform] (null unless a violation is asked for).
// Outputs (q) as documented at ntg_batch_trig, any may be null.
struct TrigTerm { int iC[NTG_TRIG_MAXENT]; short r[NTG_TRIG_MAXENT]; short kind, nent, dt, pad; int pp, pad2; double coef[NTG_TRIG_MAXENT]; double phase, w; };
struct TrigRow { int ntrig, nlin, cl, D; double W; };
struct TrigArgs {
	CertBase g;
	int nform, nfp, nprm, nw;
	CertBisect q;
	TrigRow row[NTG_TRIG_MAXFORMS];
	TrigTerm term[NTG_TRIG_MAXFORMS][NTG_TRIG_MAXTERMS];
	const double *fprm, *flo, *fhi;
};
static_assert(sizeof(TrigArgs) <= 4096, "TrigArgs travels as a kernel argument");
// doubles of a work-list element: NTG_TRIG_MAXTERMS polygons of KM points (KM = 6 or NTG_MAX_ORDER, by the plan's largest order) and two of
// padding -- an odd number of 16-byte slots, so that the lanes' wide reads of their own pieces spread over the banks
static inline __host__ __device__ int ntg_trig_w(const CertBase &G) { return NTG_TRIG_MAXTERMS * (G.kmax <= 6 ? 6 : NTG_MAX_ORDER) + 2; }
// dynamic LDS: no tables in front; a coefficient row and a row of fprm per wave.  The limit is ntg_batch_extrema's
static __host__ __device__ __forceinline__ BisectLds ntg_trig_layout(const TrigArgs &A, int W) { return BisectLds{0, A.g.ne, A.q.nk, A.g.nC, A.nprm, W, A.g.pp}; }
static inline size_t ntg_trig_lds(const TrigArgs &A, int nw) { return ntg_trig_layout(A, ntg_trig_w(A.g)).bytes(nw); }

// ntg_batch_minmax (minmax.hpp): the minimum and maximum over the horizon of lattice expressions h_g = OUTER_k INNER_j m_kj over quadratic
// forms that the CALLER declares, m = q_form(z) + d.  row / term: the forms in ntg_batch_forms' kernel form, the terms of all forms in ONE
// flat table (row[f].t0 is form f's first).  mem: the members of all groups, group after group, clause after clause; c and pc give d = c +
// fprm_b[pc].  grp[g]: outer / inner (NTG_MINMAX_MIN / _MAX), its nm members from mem[m0], the basis class cl of all its forms, the degree D
// of its polygons (the largest of its forms'), and clast: bit m is set where member m is the last of its clause.  mcap: members the work
// list has room for (8 or 16), pw: doubles of one polygon in it (the instance's points, made odd), nw: waves of a workgroup (4, 2 or 1).
// glo / ghi [batch][ngroup] (null unless a violation is asked for), which [batch][ngroup][2] or null.  Outputs (q) as documented at
// ntg_batch_minmax, any may be null.
#define NTG_MINMAX_MAXMEMTOT 32
struct MinmaxMem { int form, pc; double c; };
struct MinmaxGroup { int outer, inner, nm, m0, cl, D; unsigned int clast; int pad; };
struct MinmaxArgs {
	CertBase g;
	int nform, nfp, ngroup, nw, mcap, pw, pad0, pad1;
	CertBisect q;
	FormRow row[NTG_MINMAX_MAXFORMS];
	FormTerm term[NTG_MINMAX_MAXTERMS];
	MinmaxGroup grp[NTG_MINMAX_MAXGROUPS];
	MinmaxMem mem[NTG_MINMAX_MAXMEMTOT];
	const double *fprm, *glo, *ghi; int *which;
};
static_assert(sizeof(MinmaxArgs) <= 4096, "MinmaxArgs travels as a kernel argument");
// points of the polygons of a call's instance: 6 (every group linear on a plan of largest order <= 6), 11 (that plan, quadratic members) or 19
static inline __host__ __device__ int ntg_minmax_points(const CertBase &G, int dmax) { return G.kmax > 6 ? 2 * NTG_MAX_ORDER - 1 : dmax <= 5 ? 6 : 11; }
// dynamic LDS: the product tables (built on the device) in front; a coefficient row and a row of fprm per wave.  The work list is
// member-major, list[member][slot][pw]: the BisectLds element is the mcap polygons of a slot taken together.  The limit is ntg_batch_extrema's
static __host__ __device__ __forceinline__ BisectLds ntg_minmax_layout(const MinmaxArgs &A) { return BisectLds{NTG_FORM_WALL, A.g.ne, A.q.nk, A.g.nC, A.nfp, A.mcap * A.pw, A.g.pp}; }
static inline size_t ntg_minmax_lds(const MinmaxArgs &A, int nw) { return ntg_minmax_layout(A).bytes(nw); }
