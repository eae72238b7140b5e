// plan_envelope_sos.cpp -- ntg_batch_envelope_sos and ntg_plan_sos_rows behind include/ntg_amd.h: which nonlinear trajectory rows of a plan
// are certified (the family's declaration, NtgFamily::sos, against the plan's iz / cls), the term table and the product tables the kernels
// get as arguments, what the call refuses, and the launch.  The arithmetic is in envelope_sos.hpp.  No family callback runs.  It allocates
// nothing.
#include "plan_priv.hpp"
#include "family_module.hpp"

// row j of the plan: its terms in the kernels' form (SosPlanRow, plan_priv.hpp)
SosPlanRow sos_plan_row(const ntg_plan *p, const NtgFamily *f, int j)
{
	const NtgDims &D = p->D;
	SosPlanRow R{};
	R.row.cl = D.cls[0];
	NtgSosTerm decl[NTG_SOS_MAXTERMS] = {};
	const int nt = f && f->sos ? f->sos(j, D.nout, decl) : 0;
	if (nt <= 0 || nt > NTG_SOS_MAXTERMS) return R;
	bool ok = true;
	for (int t = 0; t < nt; t++) {
		int o = -1;
		for (int q = 0; q < D.nout; q++) if (decl[t].v >= D.iz[q] && decl[t].v < D.iz[q] + D.d[q]) o = q;
		if (o < 0 || decl[t].pidx >= f->nparam_row) return SosPlanRow{{0, D.cls[0], 0, 0}, {}, false};
		const int r = decl[t].v - D.iz[o], k = D.order[o];
		if (t == 0) R.row.cl = D.cls[o];
		else if (D.cls[o] != R.row.cl) ok = false;
		R.row.D = std::max(R.row.D, 2 * std::max(k - 1 - r, 0));
		R.term[t] = SosTerm{D.iC[o], r, decl[t].pidx >= 0 ? j * f->nparam_row + decl[t].pidx : -1, 0, decl[t].shift};
		R.need_prm = R.need_prm || decl[t].pidx >= 0;
	}
	if (!ok) { R.row.nt = 0; R.row.D = 0; R.need_prm = false; return R; }
	R.row.nt = nt; R.row.flag = 1;
	return R;
}

// C(n, r), exact: n <= 2 (NTG_MAX_ORDER - 1)
static unsigned long long binom(int n, int r)
{
	unsigned long long c = 1;
	for (int i = 1; i <= r; i++) c = c * (unsigned long long)(n - r + i) / (unsigned long long)i;
	return c;
}

void sos_product_tables(double *w)
{
	for (int d = 0; d < NTG_MAX_ORDER; d++) {   // W_d[i][j] = C(d,i) C(d,j) / C(2d,i+j), i <= j: two exact integers, one rounding
		double *q = w + ntg_sos_wtri(d);
		for (int i = 0; i <= d; i++)
			for (int j = i; j <= d; j++) *q++ = (double)(binom(d, i) * binom(d, j)) / (double)binom(2 * d, i + j);
	}
}

extern "C" int ntg_plan_sos_rows(const ntg_plan *p, int *flags)
{
	if (!p || !flags) return fail(NTG_E_BADARG, p ? "null argument" : "null plan");
	const NtgFamily *f = ntg_family(p->D.family);
	for (int j = 0; j < p->D.nnltc; j++) flags[j] = sos_plan_row(p, f, j).row.flag;
	return 0;
}

extern "C" int ntg_batch_envelope_sos(const ntg_plan *p, int batch, const double *d_x, int nsub, const double *d_lower, const double *d_upper,
                                      double *d_q_lo, double *d_q_hi, double *d_viol, int *d_where, void *stream)
{
	if (!p) return fail(NTG_E_BADARG, "null plan");
	if (nsub < 0 || nsub > NTG_ENVELOPE_MAX_NSUB) return fail(NTG_E_BADARG, "nsub must lie in 0 .. " + std::to_string(NTG_ENVELOPE_MAX_NSUB));
	if (batch <= 0) return 0;
	if (!d_x) return fail(NTG_E_BADARG, "null argument");
	const bool want_v = d_viol || d_where;
	if (!d_q_lo && !d_q_hi && !want_v) return fail(NTG_E_BADARG, "no output asked for: pass d_q_lo, d_q_hi, d_viol or d_where");
	if (want_v && (!d_lower || !d_upper)) return fail(NTG_E_BADARG, "d_viol / d_where need the bounds d_lower and d_upper");
	const NtgDims &D = p->D;
	if (D.family == NTG_FAM_HOST) return fail(NTG_E_UNSUPPORTED, "host-callback plans are not taken by the batch calls");
	if (D.nnltc == 0) return fail(NTG_E_BADARG, "the plan has no nonlinear trajectory rows (nnltc == 0)");
	if (p->grid_batch && batch != p->grid_batch) return fail(NTG_E_BADARG, "the plan carries per-problem grids for another batch size");
	if (p->prm_batch && batch != p->prm_batch)
		return fail(NTG_E_BADARG, "the plan carries per-problem parameters for " + std::to_string(p->prm_batch) + " problems, not " + std::to_string(batch));
	const NtgFamily *f = ntg_family(D.family);
	SosArgs A{};
	int ncert = 0, first0 = -1;
	bool need_prm = false;
	for (int j = 0; j < D.nnltc; j++) {
		const SosPlanRow R = sos_plan_row(p, f, j);
		ncert += R.row.flag;
		if (!R.row.flag && first0 < 0) first0 = j;
		need_prm = need_prm || R.need_prm;
		if (j < NTG_SOS_MAXROWS) { A.row[j] = R.row; for (int t = 0; t < NTG_SOS_MAXTERMS; t++) A.term[j][t] = R.term[t]; }
	}
	if (ncert == 0)
		return fail(NTG_E_UNSUPPORTED, std::string("no nonlinear trajectory row of this plan is certified: the family ") + (f ? f->name : "?") +
		                                   " declares none of them as a sum of squares (or the entries they name have no common pieces)");
	if (D.nnltc > NTG_SOS_MAXROWS) return fail(NTG_E_UNSUPPORTED, "more than " + std::to_string(NTG_SOS_MAXROWS) + " nonlinear trajectory rows");
	if (want_v && first0 >= 0)
		return fail(NTG_E_UNSUPPORTED, "nonlinear trajectory row " + std::to_string(first0) + " is not certified (ntg_plan_sos_rows): d_viol / d_where would be a partial "
		                                   "certificate; d_q_lo / d_q_hi are still served");
	if (need_prm && !p->prm_batch)
		return fail(NTG_E_BADARG, "the certified rows read per-problem parameters: set them with ntg_plan_set_params");
	A.nC = D.nC; A.nclass = D.nclass; A.batch = batch; A.nsub = nsub; A.nrow = D.nnltc; A.nbounds = D.nbounds;
	A.slot0 = D.nlic + D.nltc + D.nlfc + D.nnlic;
	A.pp = p->grid_batch ? 1 : 0;
	for (int c = 0; c < D.nclass; c++) {
		EnvClass &C = A.c[c];
		C.k = D.cls_k[c]; C.m = D.cls_m[c]; C.l = D.cls_l[c];
		C.eoff = A.ne; A.ne += C.l * C.k * C.k;
		C.hoff = A.ne; A.ne += C.l;
		A.lmax = std::max(A.lmax, C.l); A.kmax = std::max(A.kmax, C.k);
		A.knots[c] = A.pp ? p->d_grid_knots : p->d_knots[c];
	}
	A.npc = A.lmax << nsub;
	A.np = need_prm ? p->prm_n : 0;
	A.prm = need_prm ? p->T.prm : nullptr; A.pp_prm = need_prm ? p->T.pp_prm : 0;
	if (ntg_envelope_sos_lds(A) > NTG_ENVELOPE_LDS_MAX) return fail(NTG_E_UNSUPPORTED, "the extraction and product tables of this plan exceed 64 KiB of LDS");
	sos_product_tables(A.w);
	A.x = d_x; A.lower = d_lower; A.upper = d_upper;
	A.q_lo = d_q_lo; A.q_hi = d_q_hi; A.viol = d_viol; A.where = d_where;
	HIPCHK(hipSetDevice(p->device));
	HIPCHK(ntg_launch_envelope_sos(A, plan_ncu(p), (hipStream_t)stream));
	return 0;
}
