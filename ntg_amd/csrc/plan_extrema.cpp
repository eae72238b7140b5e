// plan_extrema.cpp -- ntg_batch_extrema and ntg_plan_extrema_rows behind include/ntg_amd.h: which trajectory rows of a plan the call
// certifies (a linear row whose outputs share a basis class, from the host mirror of ltc; a nonlinear row by the family's sum-of-squares
// declaration, sos_plan_row), the tables the kernels get as arguments, what the call refuses, and the launch.  The arithmetic is in
// extrema.hpp.  No family callback runs.  It allocates nothing.
#include "plan_priv.hpp"
#include "family_module.hpp"

namespace {
// linear trajectory row i: 1 when the outputs it names belong to one basis class (a row of zeros: class 0)
int lin_row_flag(const ntg_plan *p, int i)
{
	const NtgDims &D = p->D;
	const double *row = p->h_linrows.data() + (size_t)(D.nlic + i) * D.nz;
	int first = -1;
	for (int o = 0; o < D.nout; o++)
		for (int r = 0; r < D.d[o]; r++) {
			if (row[D.iz[o] + r] == 0.0) continue;
			if (first < 0) first = o;
			else if (D.cls[o] != D.cls[first]) return 0;
		}
	return 1;
}
}   // namespace

extern "C" int ntg_plan_extrema_rows(const ntg_plan *p, int *flags)
{
	if (!p || !flags) return fail(NTG_E_BADARG, p ? "null argument" : "null plan");
	const NtgDims &D = p->D;
	const NtgFamily *f = ntg_family(D.family);
	for (int i = 0; i < D.nltc; i++) flags[i] = lin_row_flag(p, i);
	for (int j = 0; j < D.nnltc; j++) flags[D.nltc + j] = sos_plan_row(p, f, j).row.flag;
	return 0;
}

extern "C" int ntg_batch_extrema(const ntg_plan *p, int batch, const double *d_x, double tol, int max_depth, int sides, const double *d_lower, const double *d_upper,
                                 double *d_ext, double *d_when, int *d_status, int *d_npieces, double *d_viol, int *d_where, void *stream)
{
	if (!p) return fail(NTG_E_BADARG, "null plan");
	if (!(tol >= 0.0) || !std::isfinite(tol)) return fail(NTG_E_BADARG, "tol must be finite and >= 0");
	if (max_depth < 0 || max_depth > NTG_EXTREMA_MAX_DEPTH) return fail(NTG_E_BADARG, "max_depth must lie in 0 .. " + std::to_string(NTG_EXTREMA_MAX_DEPTH));
	if (sides < 1 || sides > 3) return fail(NTG_E_BADARG, "sides must be 1 (minimum), 2 (maximum) or 3 (both)");
	if (batch <= 0) return 0;
	if (!d_x) return fail(NTG_E_BADARG, "null argument");
	const bool want_v = d_viol || d_where;
	if (!d_ext && !d_when && !d_status && !d_npieces && !want_v)
		return fail(NTG_E_BADARG, "no output asked for: pass d_ext, d_when, d_status, d_npieces, d_viol or d_where");
	if (want_v && (!d_lower || !d_upper)) return fail(NTG_E_BADARG, "d_viol / d_where need the bounds d_lower and d_upper");
	const NtgDims &D = p->D;
	if (D.family == NTG_FAM_HOST) return fail(NTG_E_UNSUPPORTED, "host-callback plans are not taken by the batch calls");
	if (D.nltc + D.nnltc == 0) return fail(NTG_E_BADARG, "the plan has no trajectory rows (nltc + nnltc == 0)");
	if (p->grid_batch && batch != p->grid_batch) return fail(NTG_E_BADARG, "the plan carries per-problem grids for another batch size");
	if (p->prm_batch && batch != p->prm_batch)
		return fail(NTG_E_BADARG, "the plan carries per-problem parameters for " + std::to_string(p->prm_batch) + " problems, not " + std::to_string(batch));
	const NtgFamily *f = ntg_family(D.family);
	ExtArgs A{};
	SosArgs &S = A.s;
	int ncert = 0, first0 = -1;
	bool need_prm = false;
	for (int i = 0; i < D.nltc; i++) {
		const int fl = lin_row_flag(p, i);
		ncert += fl;
		if (!fl && first0 < 0) first0 = i;
	}
	for (int j = 0; j < D.nnltc; j++) {
		const SosPlanRow R = sos_plan_row(p, f, j);
		ncert += R.row.flag;
		if (!R.row.flag && first0 < 0) first0 = D.nltc + j;
		need_prm = need_prm || R.need_prm;
		if (j < NTG_SOS_MAXROWS) { S.row[j] = R.row; for (int t = 0; t < NTG_SOS_MAXTERMS; t++) S.term[j][t] = R.term[t]; }
	}
	if (ncert == 0)
		return fail(NTG_E_UNSUPPORTED, std::string("no trajectory row of this plan is certified (ntg_plan_extrema_rows): the family ") + (f ? f->name : "?") +
		                                   " declares no nonlinear row as a sum of squares, and no linear row names outputs of one basis class");
	if (D.nnltc > NTG_SOS_MAXROWS) return fail(NTG_E_UNSUPPORTED, "more than " + std::to_string(NTG_SOS_MAXROWS) + " nonlinear trajectory rows");
	if (want_v && first0 >= 0)
		return fail(NTG_E_UNSUPPORTED, "trajectory row " + std::to_string(first0) + " is not certified (ntg_plan_extrema_rows): d_viol / d_where would be a partial "
		                                   "certificate; the other outputs are still served");
	if (need_prm && !p->prm_batch)
		return fail(NTG_E_BADARG, "the certified rows read per-problem parameters: set them with ntg_plan_set_params");
	S.nC = D.nC; S.nclass = D.nclass; S.batch = batch; S.nrow = D.nnltc; S.nbounds = D.nbounds;
	S.slot0 = D.nlic + D.nltc + D.nlfc + D.nnlic;
	S.pp = p->grid_batch ? 1 : 0;
	for (int c = 0; c < D.nclass; c++) {
		EnvClass &C = S.c[c];
		C.k = D.cls_k[c]; C.m = D.cls_m[c]; C.l = D.cls_l[c];
		C.eoff = S.ne; S.ne += C.l * C.k * C.k;
		C.hoff = S.ne; S.ne += C.l;
		A.koff[c] = A.nk; A.nk += C.l + 1;
		S.lmax = std::max(S.lmax, C.l); S.kmax = std::max(S.kmax, C.k);
		S.knots[c] = S.pp ? p->d_grid_knots : p->d_knots[c];
	}
	S.npc = S.lmax;
	S.np = need_prm ? p->prm_n : 0;
	S.prm = need_prm ? p->T.prm : nullptr; S.pp_prm = need_prm ? p->T.pp_prm : 0;
	A.nout = D.nout; A.nz = D.nz; A.nltc = D.nltc; A.slot_lin = D.nlic; A.max_depth = max_depth; A.sides = sides; A.tol = tol;
	for (int o = 0; o < D.nout; o++) { A.cls[o] = D.cls[o]; A.d[o] = D.d[o]; A.iC[o] = D.iC[o]; A.iz[o] = D.iz[o]; }
	if (S.kmax > NTG_MAX_ORDER || ntg_extrema_lds(A) > NTG_EXTREMA_LDS_MAX)
		return fail(NTG_E_UNSUPPORTED, "the tables and work lists of this plan exceed " + std::to_string(NTG_EXTREMA_LDS_MAX / 1024) + " KiB of LDS");
	sos_product_tables(S.w);
	S.x = d_x; S.lower = d_lower; S.upper = d_upper;
	A.ltc = p->d_ltc;
	A.ext = d_ext; A.when = d_when; A.status = d_status; A.npieces = d_npieces; A.viol = d_viol; A.where = d_where;
	HIPCHK(hipSetDevice(p->device));
	HIPCHK(ntg_launch_extrema(A, plan_ncu(p), (hipStream_t)stream));
	return 0;
}
