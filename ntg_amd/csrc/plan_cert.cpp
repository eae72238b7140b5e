// plan_cert.cpp -- the time certificates behind include/ntg_amd.h: ntg_batch_envelope, ntg_batch_envelope_sos, ntg_batch_extrema,
// ntg_batch_separation, ntg_batch_forms, ntg_batch_ratios, ntg_batch_trig, ntg_batch_minmax and the queries ntg_plan_sos_rows and ntg_plan_extrema_rows.  What they share comes first: the refusals (each call tests them between its own
// argument checks, in its own order), which rows of a plan are certified -- a linear trajectory row whose outputs share a basis class, from
// the host mirror of ltc; a nonlinear row by the family's sum-of-squares declaration, NtgFamily::sos, against the plan's iz / cls -- and the
// three parts of the kernels' arguments (CertBase, CertLin, CertSos: ntg_dev.hpp).  An entry point then reads: its own argument checks,
// the setup, its own fields, the launch.  The arithmetic is in envelope.hpp, envelope_sos.hpp, extrema.hpp, separation.hpp, forms.hpp, ratios.hpp, trig.hpp and minmax.hpp.  No family callback runs, so
// the calls serve every built-in family and every loaded module.  They allocate nothing.
#include <cstring>
#include "plan_priv.hpp"
#include "family_module.hpp"

namespace {
// ---------------- refusals ----------------
// an empty batch (1: the call returns 0) and the coefficients
int cert_batch(int batch, const double *d_x)
{
	if (batch <= 0) return 1;
	return d_x ? 0 : fail(NTG_E_BADARG, "null argument");
}
int cert_bounds(bool want_v, const double *d_lower, const double *d_upper)
{
	return want_v && (!d_lower || !d_upper) ? fail(NTG_E_BADARG, "d_viol / d_where need the bounds d_lower and d_upper") : 0;
}
int cert_host(const ntg_plan *p)
{
	return p->D.family == NTG_FAM_HOST ? fail(NTG_E_UNSUPPORTED, "host-callback plans are not taken by the batch calls") : 0;
}
// per-problem grids and (with_prm) per-problem parameters made for another batch size
int cert_batch_size(const ntg_plan *p, int batch, bool with_prm)
{
	if (p->grid_batch && batch != p->grid_batch) return fail(NTG_E_BADARG, "the plan carries per-problem grids for another batch size");
	if (with_prm && p->prm_batch && batch != p->prm_batch)
		return fail(NTG_E_BADARG, "the plan carries per-problem parameters for " + std::to_string(p->prm_batch) + " problems, not " + std::to_string(batch));
	return 0;
}
// tol and max_depth of the bisection calls; sides of those that have both
int cert_levels(double tol, int max_depth)
{
	if (!(tol >= 0.0) || !std::isfinite(tol)) return fail(NTG_E_BADARG, "tol must be finite and >= 0");
	if (max_depth < 0 || max_depth > NTG_EXTREMA_MAX_DEPTH) return fail(NTG_E_BADARG, "max_depth must lie in 0 .. " + std::to_string(NTG_EXTREMA_MAX_DEPTH));
	return 0;
}
int cert_sides(int sides)
{
	return sides < 1 || sides > 3 ? fail(NTG_E_BADARG, "sides must be 1 (minimum), 2 (maximum) or 3 (both)") : 0;
}
// the call's figures and outputs, for the level loop and the epilogue the bisection kernels share (koff / nk: cert_base)
void cert_bisect(CertBisect &Q, double tol, int max_depth, int sides, double *d_ext, double *d_when, int *d_status, int *d_npieces, double *d_viol, int *d_where)
{
	Q.tol = tol; Q.max_depth = max_depth; Q.sides = sides;
	Q.ext = d_ext; Q.when = d_when; Q.status = d_status; Q.npieces = d_npieces; Q.viol = d_viol; Q.where = d_where;
}
int cert_nsub(int nsub)
{
	return nsub < 0 || nsub > NTG_ENVELOPE_MAX_NSUB ? fail(NTG_E_BADARG, "nsub must lie in 0 .. " + std::to_string(NTG_ENVELOPE_MAX_NSUB)) : 0;
}

// ---------------- rows ----------------
// linear trajectory row i: flag 1 when the outputs it names belong to one basis class (a row of zeros: class 0); otherwise the first output
// named and the first one of another class
struct LinRowFlag { int flag, first, other; };
LinRowFlag lin_row_flag(const ntg_plan *p, int i)
{
	const NtgDims &D = p->D;
	const double *row = p->h_linrows.data() + (size_t)(D.nlic + i) * D.nz;
	int first = -1;
	for (int o = 0; o < D.nout; o++)
		for (int r = 0; r < D.d[o]; r++) {
			if (row[D.iz[o] + r] == 0.0) continue;
			if (first < 0) first = o;
			else if (D.cls[o] != D.cls[first]) return {0, first, o};
		}
	return {1, first, -1};
}

// Row j of the plan's nonlinear trajectory rows in the kernels' form.  flag 0: no statement -- the family does not declare the row (or names
// a flag entry the plan does not have), or the entries it names belong to different basis classes; cl is then the class of the first entry
// named, or of output 0.  f: the plan's family (null: declares nothing)
struct SosPlanRow { SosRow row; SosTerm term[NTG_SOS_MAXTERMS]; bool need_prm; };
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

// flag entry v of the plan as (output, derivative order); o < 0: the plan has no such entry
struct FlagEntry { int o, r; };
FlagEntry flag_entry(const NtgDims &D, int v)
{
	for (int q = 0; q < D.nout; q++) if (v >= D.iz[q] && v < D.iz[q] + D.d[q]) return {q, v - D.iz[q]};
	return {-1, 0};
}

// C(n, r), exact: n <= 2 (NTG_MAX_ORDER - 1)
unsigned long long binom(int n, int r)
{
	unsigned long long c = 1;
	for (int i = 1; i <= r; i++) c = c * (unsigned long long)(n - r + i) / (unsigned long long)i;
	return c;
}

// ---------------- the parts of the kernels' arguments ----------------
// the batch and the class tables; koff / nk (extrema): where every class's breaks go
void cert_base(const ntg_plan *p, int batch, const double *d_x, const double *d_lower, const double *d_upper, CertBase &G, int *koff = nullptr, int *nk = nullptr)
{
	const NtgDims &D = p->D;
	G.nC = D.nC; G.nclass = D.nclass; G.batch = batch; G.nbounds = D.nbounds;
	G.pp = p->grid_batch ? 1 : 0;
	for (int c = 0; c < D.nclass; c++) {
		EnvClass &C = G.c[c];
		C.k = D.cls_k[c]; C.m = D.cls_m[c]; C.l = D.cls_l[c];
		C.eoff = G.ne; G.ne += C.l * C.k * C.k;
		C.hoff = G.ne; G.ne += C.l;
		if (koff) { koff[c] = *nk; *nk += C.l + 1; }
		G.lmax = std::max(G.lmax, C.l); G.kmax = std::max(G.kmax, C.k);
		G.knots[c] = G.pp ? p->d_grid_knots : p->d_knots[c];
	}
	G.x = d_x; G.lower = d_lower; G.upper = d_upper;
}
void cert_lin(const ntg_plan *p, CertLin &L)
{
	const NtgDims &D = p->D;
	L.nout = D.nout; L.nz = D.nz; L.nltc = D.nltc; L.slot0 = D.nlic; L.ltc = p->d_ltc;
	for (int o = 0; o < D.nout; o++) { L.cls[o] = D.cls[o]; L.d[o] = D.d[o]; L.iC[o] = D.iC[o]; L.iz[o] = D.iz[o]; }
}
// the product tables W_d[i][j] = C(d,i) C(d,j) / C(2d,i+j), i <= j: two exact integers, one rounding
void cert_products(CertSos &S)
{
	for (int d = 0; d < NTG_MAX_ORDER; d++) {
		double *q = S.w + ntg_sos_wtri(d);
		for (int i = 0; i <= d; i++)
			for (int j = i; j <= d; j++) *q++ = (double)(binom(d, i) * binom(d, j)) / (double)binom(2 * d, i + j);
	}
}
// the rows, terms and product tables; how many rows are certified, the first that is not (or -1), and the parameter row where a term reads it
struct SosCount { int ncert, first0; bool need_prm; };
SosCount cert_sos(const ntg_plan *p, const NtgFamily *f, CertSos &S)
{
	const NtgDims &D = p->D;
	SosCount n{0, -1, false};
	for (int j = 0; j < D.nnltc; j++) {
		const SosPlanRow R = sos_plan_row(p, f, j);
		n.ncert += R.row.flag;
		if (!R.row.flag && n.first0 < 0) n.first0 = j;
		n.need_prm = n.need_prm || R.need_prm;
		if (j < NTG_SOS_MAXROWS) { S.row[j] = R.row; for (int t = 0; t < NTG_SOS_MAXTERMS; t++) S.term[j][t] = R.term[t]; }
	}
	S.nrow = D.nnltc; S.slot0 = D.nlic + D.nltc + D.nlfc + D.nnlic;
	S.np = n.need_prm ? p->prm_n : 0;
	S.prm = n.need_prm ? p->T.prm : nullptr; S.pp_prm = n.need_prm ? p->T.pp_prm : 0;
	cert_products(S);
	return n;
}
// what both calls on sum-of-squares rows refuse about them once they know that some row is certified: more rows than the kernels' tables
// hold, and (after the call's own partial-certificate refusal) parameters that were never set
int cert_sos_fits(const ntg_plan *p)
{
	return p->D.nnltc > NTG_SOS_MAXROWS ? fail(NTG_E_UNSUPPORTED, "more than " + std::to_string(NTG_SOS_MAXROWS) + " nonlinear trajectory rows") : 0;
}
int cert_sos_prm(const ntg_plan *p, const SosCount &n)
{
	return n.need_prm && !p->prm_batch ? fail(NTG_E_BADARG, "the certified rows read per-problem parameters: set them with ntg_plan_set_params") : 0;
}
}   // namespace

extern "C" int ntg_plan_sos_rows(const ntg_plan *p, int *flags)
{
	if (!p || !flags) return fail(NTG_E_BADARG, p ? "null argument" : "null plan");
	const NtgFamily *f = ntg_family(p->D.family);
	for (int j = 0; j < p->D.nnltc; j++) flags[j] = sos_plan_row(p, f, j).row.flag;
	return 0;
}

extern "C" int ntg_plan_extrema_rows(const ntg_plan *p, int *flags)
{
	if (!p || !flags) return fail(NTG_E_BADARG, p ? "null argument" : "null plan");
	for (int i = 0; i < p->D.nltc; i++) flags[i] = lin_row_flag(p, i).flag;
	return ntg_plan_sos_rows(p, flags + p->D.nltc);
}

extern "C" int ntg_batch_envelope(const ntg_plan *p, int batch, const double *d_x, int nsub, const double *d_lower, const double *d_upper,
                                  double *d_lo, double *d_hi, double *d_row_lo, double *d_row_hi, double *d_viol, int *d_where, void *stream)
{
	if (!p) return fail(NTG_E_BADARG, "null plan");
	if (int rc = cert_batch(batch, d_x)) return rc > 0 ? 0 : rc;
	if (int rc = cert_nsub(nsub)) return rc;
	const bool want_v = d_viol || d_where, want_r = d_row_lo || d_row_hi || want_v;
	if (!d_lo && !d_hi && !want_r) return fail(NTG_E_BADARG, "no output asked for: pass d_lo, d_hi, d_row_lo, d_row_hi, d_viol or d_where");
	if (int rc = cert_bounds(want_v, d_lower, d_upper)) return rc;
	if (want_r && p->D.nltc == 0) return fail(NTG_E_BADARG, "the plan has no linear trajectory rows (nltc == 0)");
	if (int rc = cert_batch_size(p, batch, false)) return rc;
	if (int rc = cert_host(p)) return rc;
	for (int i = 0; want_r && i < p->D.nltc; i++) {   // every row's polygon lives on the pieces of one basis class
		const LinRowFlag R = lin_row_flag(p, i);
		if (!R.flag)
			return fail(NTG_E_UNSUPPORTED, "linear trajectory row " + std::to_string(i) + " names outputs " + std::to_string(R.first) + " and " + std::to_string(R.other) +
			                                   " of different basis classes: its envelope has no common pieces (the entry envelope d_lo / d_hi is still served)");
	}
	EnvArgs A{};
	cert_base(p, batch, d_x, d_lower, d_upper, A.g);
	cert_lin(p, A.lin);
	A.nsub = nsub; A.npc = A.g.lmax << nsub;
	if (ntg_envelope_lds(A) > NTG_ENVELOPE_LDS_MAX) return fail(NTG_E_UNSUPPORTED, "the extraction tables of this plan exceed 64 KiB of LDS");
	A.lo = d_lo; A.hi = d_hi; A.row_lo = d_row_lo; A.row_hi = d_row_hi; A.viol = d_viol; A.where = d_where;
	HIPCHK(hipSetDevice(p->device));
	HIPCHK(ntg_launch_envelope(A, plan_ncu(p), (hipStream_t)stream));
	return 0;
}

extern "C" int ntg_batch_envelope_sos(const ntg_plan *p, int batch, const double *d_x, int nsub, const double *d_lower, const double *d_upper,
                                      double *d_q_lo, double *d_q_hi, double *d_viol, int *d_where, void *stream)
{
	if (!p) return fail(NTG_E_BADARG, "null plan");
	if (int rc = cert_nsub(nsub)) return rc;
	if (int rc = cert_batch(batch, d_x)) return rc > 0 ? 0 : rc;
	const bool want_v = d_viol || d_where;
	if (!d_q_lo && !d_q_hi && !want_v) return fail(NTG_E_BADARG, "no output asked for: pass d_q_lo, d_q_hi, d_viol or d_where");
	if (int rc = cert_bounds(want_v, d_lower, d_upper)) return rc;
	if (int rc = cert_host(p)) return rc;
	if (p->D.nnltc == 0) return fail(NTG_E_BADARG, "the plan has no nonlinear trajectory rows (nnltc == 0)");
	if (int rc = cert_batch_size(p, batch, true)) return rc;
	const NtgFamily *f = ntg_family(p->D.family);
	SosArgs A{};
	const SosCount n = cert_sos(p, f, A.sos);
	if (n.ncert == 0)
		return fail(NTG_E_UNSUPPORTED, std::string("no nonlinear trajectory row of this plan is certified: the family ") + (f ? f->name : "?") +
		                                   " declares none of them as a sum of squares (or the entries they name have no common pieces)");
	if (int rc = cert_sos_fits(p)) return rc;
	if (want_v && n.first0 >= 0)
		return fail(NTG_E_UNSUPPORTED, "nonlinear trajectory row " + std::to_string(n.first0) + " is not certified (ntg_plan_sos_rows): d_viol / d_where would be a partial "
		                                   "certificate; d_q_lo / d_q_hi are still served");
	if (int rc = cert_sos_prm(p, n)) return rc;
	cert_base(p, batch, d_x, d_lower, d_upper, A.g);
	A.nsub = nsub; A.npc = A.g.lmax << nsub;
	if (ntg_envelope_sos_lds(A) > NTG_ENVELOPE_LDS_MAX) return fail(NTG_E_UNSUPPORTED, "the extraction and product tables of this plan exceed 64 KiB of LDS");
	A.q_lo = d_q_lo; A.q_hi = d_q_hi; A.viol = d_viol; A.where = d_where;
	HIPCHK(hipSetDevice(p->device));
	HIPCHK(ntg_launch_envelope_sos(A, plan_ncu(p), (hipStream_t)stream));
	return 0;
}

extern "C" int ntg_batch_extrema(const ntg_plan *p, int batch, const double *d_x, double tol, int max_depth, int sides, const double *d_lower, const double *d_upper,
                                 double *d_ext, double *d_when, int *d_status, int *d_npieces, double *d_viol, int *d_where, void *stream)
{
	if (!p) return fail(NTG_E_BADARG, "null plan");
	if (int rc = cert_levels(tol, max_depth)) return rc;
	if (int rc = cert_sides(sides)) return rc;
	if (int rc = cert_batch(batch, d_x)) return rc > 0 ? 0 : rc;
	const bool want_v = d_viol || d_where;
	if (!d_ext && !d_when && !d_status && !d_npieces && !want_v)
		return fail(NTG_E_BADARG, "no output asked for: pass d_ext, d_when, d_status, d_npieces, d_viol or d_where");
	if (int rc = cert_bounds(want_v, d_lower, d_upper)) return rc;
	if (int rc = cert_host(p)) return rc;
	const NtgDims &D = p->D;
	if (D.nltc + D.nnltc == 0) return fail(NTG_E_BADARG, "the plan has no trajectory rows (nltc + nnltc == 0)");
	if (int rc = cert_batch_size(p, batch, true)) return rc;
	const NtgFamily *f = ntg_family(D.family);
	ExtArgs A{};
	SosCount n = cert_sos(p, f, A.sos);
	int first_lin = -1;   // the linear rows come first
	for (int i = 0; i < D.nltc; i++) {
		const int fl = lin_row_flag(p, i).flag;
		n.ncert += fl;
		if (!fl && first_lin < 0) first_lin = i;
	}
	n.first0 = first_lin >= 0 ? first_lin : n.first0 >= 0 ? D.nltc + n.first0 : -1;
	if (n.ncert == 0)
		return fail(NTG_E_UNSUPPORTED, std::string("no trajectory row of this plan is certified (ntg_plan_extrema_rows): the family ") + (f ? f->name : "?") +
		                                   " declares no nonlinear row as a sum of squares, and no linear row names outputs of one basis class");
	if (int rc = cert_sos_fits(p)) return rc;
	if (want_v && n.first0 >= 0)
		return fail(NTG_E_UNSUPPORTED, "trajectory row " + std::to_string(n.first0) + " is not certified (ntg_plan_extrema_rows): d_viol / d_where would be a partial "
		                                   "certificate; the other outputs are still served");
	if (int rc = cert_sos_prm(p, n)) return rc;
	cert_base(p, batch, d_x, d_lower, d_upper, A.g, A.q.koff, &A.q.nk);
	cert_lin(p, A.lin);
	cert_bisect(A.q, tol, max_depth, sides, d_ext, d_when, d_status, d_npieces, d_viol, d_where);
	if (A.g.kmax > NTG_MAX_ORDER || ntg_extrema_lds(A) > NTG_EXTREMA_LDS_MAX)
		return fail(NTG_E_UNSUPPORTED, "the tables and work lists of this plan exceed " + std::to_string(NTG_EXTREMA_LDS_MAX / 1024) + " KiB of LDS");
	HIPCHK(hipSetDevice(p->device));
	HIPCHK(ntg_launch_extrema(A, plan_ncu(p), (hipStream_t)stream));
	return 0;
}

extern "C" int ntg_batch_separation(const ntg_plan *p, int batch, const double *d_x, int nbody, int ndim, const int *body_outs, int deriv, int npairs, const int *d_pairs,
                                    const double *d_sep, double tol, int max_depth, double *d_min, double *d_when, int *d_status, int *d_npieces, double *d_viol, void *stream)
{
	if (!p) return fail(NTG_E_BADARG, "null plan");
	if (!d_x || !body_outs || !d_pairs) return fail(NTG_E_BADARG, "null argument");
	if (ndim < 1 || ndim > NTG_SEP_MAXDIM) return fail(NTG_E_BADARG, "ndim must lie in 1 .. " + std::to_string(NTG_SEP_MAXDIM));
	if (nbody < 1 || nbody > NTG_MAX_OUT) return fail(NTG_E_BADARG, "nbody must lie in 1 .. " + std::to_string(NTG_MAX_OUT));
	if (int rc = cert_levels(tol, max_depth)) return rc;
	const NtgDims &D = p->D;
	for (int i = 0; i < nbody * ndim; i++) {
		const int o = body_outs[i];
		if (o < 0 || o >= D.nout) return fail(NTG_E_BADARG, "body " + std::to_string(i / ndim) + " names output " + std::to_string(o) + ": the plan has outputs 0 .. " + std::to_string(D.nout - 1));
		if (deriv < 0 || deriv >= D.d[o]) return fail(NTG_E_BADARG, "deriv must lie in 0 .. maxderiv - 1 of every output named (output " + std::to_string(o) + ": " + std::to_string(D.d[o]) + ")");
	}
	if (!d_min && !d_when && !d_status && !d_npieces && !d_viol) return fail(NTG_E_BADARG, "no output asked for: pass d_min, d_when, d_status, d_npieces or d_viol");
	if (d_viol && !d_sep) return fail(NTG_E_BADARG, "d_viol needs the required distances d_sep");
	if (npairs <= 0 || batch <= 0) return 0;
	if (int rc = cert_host(p)) return rc;
	for (int i = 1; i < nbody * ndim; i++)   // one polygon per knot interval needs common knot intervals
		if (D.cls[body_outs[i]] != D.cls[body_outs[0]])
			return fail(NTG_E_UNSUPPORTED, "outputs " + std::to_string(body_outs[0]) + " and " + std::to_string(body_outs[i]) + " of the bodies belong to different basis classes: their "
			                                   "difference has no common pieces");
	if (p->grid_batch)
		return fail(NTG_E_UNSUPPORTED, "the plan carries per-problem grids: two problems then have no common knot intervals (ntg_batch_separation takes plans on their own grid only)");
	SepArgs A{};
	cert_base(p, batch, d_x, nullptr, nullptr, A.g);
	cert_products(A.sos);
	{   // the one class of the bodies, alone in the tables
		const int cl = D.cls[body_outs[0]];
		const EnvClass C = A.g.c[cl];
		A.g.nclass = 1; A.g.c[0] = EnvClass{C.k, C.m, C.l, 0, C.l * C.k * C.k}; A.g.ne = C.l * (C.k * C.k + 1);
		A.g.lmax = C.l; A.g.kmax = C.k; A.g.knots[0] = A.g.knots[cl];
		A.n = C.l * (C.k - C.m) + C.m;
		A.sos.nrow = 1;
		A.sos.row[0] = SosRow{ndim, 0, 2 * std::max(C.k - 1 - deriv, 0), 1};
		for (int t = 0; t < ndim; t++) A.sos.term[0][t] = SosTerm{t * A.n, deriv, -1, 0, 0.0};
	}
	for (int g = 0; g < nbody; g++)
		for (int t = 0; t < ndim; t++) A.biC[g][t] = D.iC[body_outs[g * ndim + t]];
	A.npairs = npairs; A.nbody = nbody; A.ndim = ndim; A.max_depth = max_depth; A.tol = tol;
	if (A.g.kmax > NTG_MAX_ORDER || ntg_separation_lds(A) > NTG_EXTREMA_LDS_MAX)
		return fail(NTG_E_UNSUPPORTED, "the tables and work lists of this call exceed " + std::to_string(NTG_EXTREMA_LDS_MAX / 1024) + " KiB of LDS");
	A.pairs = d_pairs; A.sep = d_sep;
	A.min = d_min; A.when = d_when; A.status = d_status; A.npieces = d_npieces; A.viol = d_viol;
	HIPCHK(hipSetDevice(p->device));
	HIPCHK(ntg_launch_separation(A, plan_ncu(p), (hipStream_t)stream));
	return 0;
}

// ---------------- forms declared at the call (ntg_batch_forms, ntg_batch_ratios, ntg_batch_minmax) ----------------
namespace {
// the first form that names two basis classes, and two outputs that show it
struct FormCross { int form = -1, a = -1, b = -1; };
// where a declaration goes: rows [maxforms], and the terms either [maxforms][NTG_FORM_MAXTERMS] (flat = false: FormArgs) or one table of
// maxterms for all forms, row.t0 the form's first (flat = true: MinmaxArgs)
struct FormSink { FormRow *row; FormTerm *term; int maxforms, maxterms; bool flat; };
// the arguments that declare the forms, checked in ntg_batch_forms' order, and the forms in the kernels' form (S.row, S.term)
int forms_declare(const ntg_plan *p, const double *d_x, int nform, const int *form_nterms, const ntg_form_term *terms, int nfp, const double *d_fprm,
                  double tol, int max_depth, int sides, const FormSink &S, FormCross &X)
{
	if (!p) return fail(NTG_E_BADARG, "null plan");
	if (!d_x || !form_nterms || !terms) return fail(NTG_E_BADARG, "null argument");
	if (nform < 0 || nform > S.maxforms) return fail(NTG_E_BADARG, "nform must lie in 0 .. " + std::to_string(S.maxforms));
	if (nfp < 0) return fail(NTG_E_BADARG, "nfp must be >= 0");
	if (int rc = cert_levels(tol, max_depth)) return rc;
	if (int rc = cert_sides(sides)) return rc;
	const NtgDims &D = p->D;
	const ntg_form_term *q = terms;
	for (int f = 0; f < nform; f++) {
		const int nt = form_nterms[f];
		const std::string fname = "form " + std::to_string(f);
		if (nt < 1 || nt > NTG_FORM_MAXTERMS) return fail(NTG_E_BADARG, fname + " has " + std::to_string(nt) + " terms: 1 .. " + std::to_string(NTG_FORM_MAXTERMS) + " are taken");
		FormRow &R = S.row[f];
		const int t0 = (int)(q - terms);
		if (S.flat && t0 + nt > S.maxterms)
			return fail(NTG_E_BADARG, fname + " brings the terms of all forms to " + std::to_string(t0 + nt) + ": " + std::to_string(S.maxterms) + " are taken at one call");
		R.t0 = S.flat ? t0 : 0;
		int first = -1;
		for (int t = 0; t < nt; t++, q++) {
			const std::string tname = fname + ", term " + std::to_string(t);
			const bool lin = q->v == -1;
			if (q->u < 0 || q->u >= D.nz) return fail(NTG_E_BADARG, tname + ": u = " + std::to_string(q->u) + " is no flag entry of the plan (0 .. " + std::to_string(D.nz - 1) + ")");
			if (q->v < -1 || q->v >= D.nz) return fail(NTG_E_BADARG, tname + ": v = " + std::to_string(q->v) + " is neither -1 nor a flag entry of the plan (0 .. " + std::to_string(D.nz - 1) + ")");
			if (q->pu < -1 || q->pu >= nfp || (!lin && (q->pv < -1 || q->pv >= nfp)))
				return fail(NTG_E_BADARG, tname + ": pu and pv must lie in -1 .. nfp - 1 = " + std::to_string(nfp - 1));
			if ((q->pu >= 0 || (!lin && q->pv >= 0)) && !d_fprm) return fail(NTG_E_BADARG, tname + " names a parameter, but d_fprm is null");
			if (!std::isfinite(q->w) || !std::isfinite(q->su) || (!lin && !std::isfinite(q->sv))) return fail(NTG_E_BADARG, tname + ": w, su and sv must be finite");
			const FlagEntry eu = flag_entry(D, q->u), ev = lin ? eu : flag_entry(D, q->v);
			if (first < 0) { first = eu.o; R.cl = D.cls[eu.o]; }
			for (const int o : {eu.o, ev.o})
				if (D.cls[o] != R.cl && X.form < 0) { X.form = f; X.a = first; X.b = o; }
			const int du = std::max(D.order[eu.o] - 1 - eu.r, 0), dv = lin ? 0 : std::max(D.order[ev.o] - 1 - ev.r, 0);
			R.D = std::max(R.D, du + dv);
			FormTerm &T = S.term[S.flat ? t0 + t : f * NTG_FORM_MAXTERMS + t];
			T.iCu = D.iC[eu.o]; T.ru = (short)eu.r; T.pu = q->pu; T.su = q->su; T.w = q->w;
			T.iCv = lin ? 0 : D.iC[ev.o]; T.rv = (short)(lin ? 0 : ev.r); T.pv = lin ? -1 : q->pv; T.sv = lin ? 0.0 : q->sv;
			T.kind = lin ? NTG_FORM_LIN : (q->v == q->u && q->pu == q->pv && std::memcmp(&q->su, &q->sv, sizeof(double)) == 0) ? NTG_FORM_SQUARE : NTG_FORM_PROD;
		}
		R.nt = nt;
	}
	return 0;
}
// the outputs: one of them, and both bounds (named lo and hi in the message) where a violation is asked for
int forms_outputs(const double *d_lo, const double *d_hi, const char *lo, const char *hi, double *d_ext, double *d_when, int *d_status, int *d_npieces, double *d_viol, int *d_where)
{
	const bool want_v = d_viol || d_where;
	if (!d_ext && !d_when && !d_status && !d_npieces && !want_v)
		return fail(NTG_E_BADARG, "no output asked for: pass d_ext, d_when, d_status, d_npieces, d_viol or d_where");
	if (want_v && (!d_lo || !d_hi)) return fail(NTG_E_BADARG, std::string("d_viol / d_where need the bounds ") + lo + " and " + hi);
	return 0;
}
// what a non-empty call refuses about the plan and the forms
int forms_refuse(const ntg_plan *p, int batch, const FormCross &X)
{
	if (int rc = cert_batch_size(p, batch, false)) return rc;
	if (int rc = cert_host(p)) return rc;
	if (X.form >= 0)
		return fail(NTG_E_UNSUPPORTED, "form " + std::to_string(X.form) + " names outputs " + std::to_string(X.a) + " and " + std::to_string(X.b) +
		                                   " of different basis classes: it has no common pieces");
	return 0;
}
// the tables of ntg_batch_forms and ntg_batch_ratios as a sink
FormSink forms_sink(FormArgs &A) { return FormSink{A.row, &A.term[0][0], NTG_FORM_MAXFORMS, NTG_FORM_MAXFORMS * NTG_FORM_MAXTERMS, false}; }
// the kernels' arguments but the launch figures, the forms' parameters and the bounds
void forms_args(const ntg_plan *p, int batch, const double *d_x, int nform, int nfp, FormArgs &A)
{
	cert_base(p, batch, d_x, nullptr, nullptr, A.g, A.q.koff, &A.q.nk);
	A.nform = nform; A.nfp = nfp;
}
}   // namespace

extern "C" int ntg_batch_forms(const ntg_plan *p, int batch, const double *d_x, int nform, const int *form_nterms, const ntg_form_term *terms, int nfp, const double *d_fprm,
                               double tol, int max_depth, int sides, const double *d_flo, const double *d_fhi,
                               double *d_ext, double *d_when, int *d_status, int *d_npieces, double *d_viol, int *d_where, void *stream)
{
	FormArgs A{};
	FormCross X;
	if (int rc = forms_declare(p, d_x, nform, form_nterms, terms, nfp, d_fprm, tol, max_depth, sides, forms_sink(A), X)) return rc;
	if (int rc = forms_outputs(d_flo, d_fhi, "d_flo", "d_fhi", d_ext, d_when, d_status, d_npieces, d_viol, d_where)) return rc;
	if (batch <= 0 || nform == 0) return 0;
	if (int rc = forms_refuse(p, batch, X)) return rc;
	forms_args(p, batch, d_x, nform, nfp, A);
	cert_bisect(A.q, tol, max_depth, sides, d_ext, d_when, d_status, d_npieces, d_viol, d_where);
	if (A.g.kmax > NTG_MAX_ORDER || ntg_forms_lds(A) > NTG_EXTREMA_LDS_MAX)
		return fail(NTG_E_UNSUPPORTED, "the tables and work lists of this call exceed " + std::to_string(NTG_EXTREMA_LDS_MAX / 1024) + " KiB of LDS");
	A.fprm = d_fprm; A.flo = d_flo; A.fhi = d_fhi;
	HIPCHK(hipSetDevice(p->device));
	HIPCHK(ntg_launch_forms(A, plan_ncu(p), (hipStream_t)stream));
	return 0;
}

extern "C" int ntg_batch_ratios(const ntg_plan *p, int batch, const double *d_x, int nform, const int *form_nterms, const ntg_form_term *terms, int nfp, const double *d_fprm,
                                int nratio, const ntg_ratio *ratios, double tol, int max_depth, int sides, const double *d_rlo, const double *d_rhi,
                                double *d_ext, double *d_when, int *d_status, int *d_npieces, double *d_viol, int *d_where, void *stream)
{
	RatioArgs A{};
	FormCross X;
	if (int rc = forms_declare(p, d_x, nform, form_nterms, terms, nfp, d_fprm, tol, max_depth, sides, forms_sink(A.f), X)) return rc;
	if (nratio < 0 || nratio > NTG_RATIO_MAXRATIOS) return fail(NTG_E_BADARG, "nratio must lie in 0 .. " + std::to_string(NTG_RATIO_MAXRATIOS));
	if (nratio > 0 && !ratios) return fail(NTG_E_BADARG, "null argument");
	for (int r = 0; r < nratio; r++) {
		const ntg_ratio &Q = ratios[r];
		const std::string rname = "ratio " + std::to_string(r);
		if (Q.nnum < 0 || Q.nnum > NTG_RATIO_MAXFACTORS || Q.nden < 0 || Q.nden > NTG_RATIO_MAXFACTORS)
			return fail(NTG_E_BADARG, rname + ": nnum and nden must lie in 0 .. " + std::to_string(NTG_RATIO_MAXFACTORS));
		if (Q.nnum + Q.nden == 0) return fail(NTG_E_BADARG, rname + " has both sides empty");
		for (int a = 0; a < Q.nnum + Q.nden; a++) {
			const int f = a < Q.nnum ? Q.num[a] : Q.den[a - Q.nnum];
			if (f < 0 || f >= nform)
				return fail(NTG_E_BADARG, rname + " names form " + std::to_string(f) + ": the call declares forms 0 .. " + std::to_string(nform - 1));
		}
	}
	if (int rc = forms_outputs(d_rlo, d_rhi, "d_rlo", "d_rhi", d_ext, d_when, d_status, d_npieces, d_viol, d_where)) return rc;
	if (batch <= 0 || nratio == 0) return 0;
	if (int rc = forms_refuse(p, batch, X)) return rc;
	int dmax = 0;
	for (int r = 0; r < nratio; r++) {   // the sides' degrees, the one class, and the product tables the chains use
		const ntg_ratio &Q = ratios[r];
		RatioRow &R = A.r[r];
		const std::string rname = "ratio " + std::to_string(r);
		int deg[2] = {0, 0}, first = -1;
		for (int side = 0; side < 2; side++) {
			const int nf = side ? Q.nden : Q.nnum;
			for (int a = 0; a < nf; a++) {
				const int f = side ? Q.den[a] : Q.num[a];
				(side ? R.den : R.num)[a] = (unsigned char)f;
				if (first < 0) first = f;
				else if (A.f.row[f].cl != A.f.row[first].cl)
					return fail(NTG_E_UNSUPPORTED, rname + " names forms " + std::to_string(first) + " and " + std::to_string(f) + " of different basis classes: it has no common pieces");
				deg[side] += A.f.row[f].D;
			}
			if (deg[side] > NTG_RATIO_MAXDEG)
				return fail(NTG_E_UNSUPPORTED, rname + ": its " + (side ? "denominator" : "numerator") + " has degree " + std::to_string(deg[side]) + ", above " + std::to_string(NTG_RATIO_MAXDEG));
		}
		for (int side = 0; side < 2; side++) {
			const int nf = side ? Q.nden : Q.nnum;
			int d = 0;
			for (int a = 0; a < nf; a++) {
				const int e = A.f.row[side ? Q.den[a] : Q.num[a]].D;
				if (a > 0) {
					int q = 0;
					while (q < A.npair && (A.pd[q] != d || A.pe[q] != e)) q++;
					if (q == A.npair) { A.pd[q] = (unsigned char)d; A.pe[q] = (unsigned char)e; A.poff[q] = A.npw; A.npw = (unsigned short)(A.npw + (d + 1) * (e + 1)); A.npair++; }
					(side ? R.pd : R.pn)[a - 1] = (unsigned char)q;
				}
				d += e;
			}
		}
		R.nnum = (unsigned char)Q.nnum; R.nden = (unsigned char)Q.nden; R.cl = (unsigned char)A.f.row[first].cl;
		R.dN = (unsigned char)deg[0]; R.dD = (unsigned char)deg[1]; R.DR = (unsigned char)std::max(deg[0], deg[1]);
		dmax = std::max(dmax, (int)R.DR);
	}
	forms_args(p, batch, d_x, nform, nfp, A.f);
	cert_bisect(A.f.q, tol, max_depth, sides, d_ext, d_when, d_status, d_npieces, d_viol, d_where);
	A.nratio = (unsigned char)nratio;
	A.kr = (unsigned char)(dmax <= 12 && A.f.g.kmax <= 6 ? 13 : 25);
	A.nw = (unsigned char)(ntg_ratios_lds(A, 4) <= NTG_EXTREMA_LDS_MAX ? 4 : 2);
	if (A.f.g.kmax > NTG_MAX_ORDER || ntg_ratios_lds(A, A.nw) > NTG_EXTREMA_LDS_MAX)
		return fail(NTG_E_UNSUPPORTED, "the tables and work lists of this call exceed " + std::to_string(NTG_EXTREMA_LDS_MAX / 1024) + " KiB of LDS");
	A.f.fprm = d_fprm; A.f.flo = d_rlo; A.f.fhi = d_rhi;
	HIPCHK(hipSetDevice(p->device));
	HIPCHK(ntg_launch_ratios(A, plan_ncu(p), (hipStream_t)stream));
	return 0;
}

// ---------------- sines and cosines declared at the call (ntg_batch_trig) ----------------
extern "C" int ntg_batch_trig(const ntg_plan *p, int batch, const double *d_x, int nform, const int *form_nterms, const ntg_trig_term *terms, int nfp, const double *d_fprm,
                              double tol, int max_depth, int sides, const double *d_flo, const double *d_fhi,
                              double *d_ext, double *d_when, int *d_status, int *d_npieces, double *d_viol, int *d_where, void *stream)
{
	if (!p) return fail(NTG_E_BADARG, "null plan");
	if (!d_x || !form_nterms || !terms) return fail(NTG_E_BADARG, "null argument");
	if (nform < 0 || nform > NTG_TRIG_MAXFORMS) return fail(NTG_E_BADARG, "nform must lie in 0 .. " + std::to_string(NTG_TRIG_MAXFORMS));
	if (nfp < 0) return fail(NTG_E_BADARG, "nfp must be >= 0");
	if (int rc = cert_levels(tol, max_depth)) return rc;
	if (int rc = cert_sides(sides)) return rc;
	const NtgDims &D = p->D;
	TrigArgs A{};
	FormCross X;
	const ntg_trig_term *q = terms;
	for (int f = 0; f < nform; f++) {
		const int nt = form_nterms[f];
		const std::string fname = "form " + std::to_string(f);
		if (nt < 1 || nt > NTG_TRIG_MAXTERMS) return fail(NTG_E_BADARG, fname + " has " + std::to_string(nt) + " terms: 1 .. " + std::to_string(NTG_TRIG_MAXTERMS) + " are taken");
		TrigRow &R = A.row[f];
		TrigTerm lin[NTG_TRIG_MAXTERMS];   // the LIN terms go behind the SIN and COS terms, both in declared order
		int first = -1;
		for (int t = 0; t < nt; t++, q++) {
			const std::string tname = fname + ", term " + std::to_string(t);
			if (q->kind < NTG_TRIG_SIN || q->kind > NTG_TRIG_LIN) return fail(NTG_E_BADARG, tname + ": kind = " + std::to_string(q->kind) + " is none of NTG_TRIG_SIN, _COS, _LIN (0 .. 2)");
			if (q->nent < 1 || q->nent > NTG_TRIG_MAXENT) return fail(NTG_E_BADARG, tname + ": nent = " + std::to_string(q->nent) + " must lie in 1 .. " + std::to_string(NTG_TRIG_MAXENT));
			for (int i = 0; i < q->nent; i++)
				if (q->ent[i] < 0 || q->ent[i] >= D.nz)
					return fail(NTG_E_BADARG, tname + ": ent[" + std::to_string(i) + "] = " + std::to_string(q->ent[i]) + " is no flag entry of the plan (0 .. " + std::to_string(D.nz - 1) + ")");
			if (q->pp < -1 || q->pp >= nfp) return fail(NTG_E_BADARG, tname + ": pp must lie in -1 .. nfp - 1 = " + std::to_string(nfp - 1));
			if (q->pp >= 0 && !d_fprm) return fail(NTG_E_BADARG, tname + " names a parameter, but d_fprm is null");
			bool finite = std::isfinite(q->w) && std::isfinite(q->phase);
			for (int i = 0; i < q->nent; i++) finite = finite && std::isfinite(q->coef[i]);
			if (!finite) return fail(NTG_E_BADARG, tname + ": coef, phase and w must be finite");
			TrigTerm T{};
			for (int i = 0; i < q->nent; i++) {
				const FlagEntry e = flag_entry(D, q->ent[i]);
				if (first < 0) { first = e.o; R.cl = D.cls[e.o]; }
				if (D.cls[e.o] != R.cl && X.form < 0) { X.form = f; X.a = first; X.b = e.o; }
				T.iC[i] = D.iC[e.o]; T.r[i] = (short)e.r; T.coef[i] = q->coef[i];
				T.dt = std::max(T.dt, (short)std::max(D.order[e.o] - 1 - e.r, 0));
			}
			T.kind = (short)q->kind; T.nent = (short)q->nent; T.pp = q->pp; T.phase = q->phase; T.w = q->w;
			R.D = std::max(R.D, (int)T.dt);
			R.W += std::fabs(q->w);
			if (q->kind == NTG_TRIG_LIN) lin[R.nlin++] = T;
			else A.term[f][R.ntrig++] = T;
		}
		for (int t = 0; t < R.nlin; t++) A.term[f][R.ntrig + t] = lin[t];
	}
	if (int rc = forms_outputs(d_flo, d_fhi, "d_flo", "d_fhi", d_ext, d_when, d_status, d_npieces, d_viol, d_where)) return rc;
	if (batch <= 0 || nform == 0) return 0;
	if (int rc = forms_refuse(p, batch, X)) return rc;
	cert_base(p, batch, d_x, nullptr, nullptr, A.g, A.q.koff, &A.q.nk);
	A.q.nk += (A.g.ne + A.q.nk) & 1;   // the work lists start at 16 bytes: the lanes read their pieces in 16-byte words
	A.nform = nform; A.nfp = nfp; A.nprm = nfp + ((A.g.nC + nfp) & 1);
	cert_bisect(A.q, tol, max_depth, sides, d_ext, d_when, d_status, d_npieces, d_viol, d_where);
	A.nw = ntg_trig_lds(A, 4) <= NTG_EXTREMA_LDS_MAX ? 4 : 2;
	if (A.g.kmax > NTG_MAX_ORDER || ntg_trig_lds(A, A.nw) > NTG_EXTREMA_LDS_MAX)
		return fail(NTG_E_UNSUPPORTED, "the tables and work lists of this call exceed " + std::to_string(NTG_EXTREMA_LDS_MAX / 1024) + " KiB of LDS: the class tables, and per wavefront nC + nfp + " +
		                                   std::to_string(NTG_EXTREMA_CAP) + " (4 KM + 3) doubles, KM = 6 or 10");
	A.fprm = d_fprm; A.flo = d_flo; A.fhi = d_fhi;
	HIPCHK(hipSetDevice(p->device));
	HIPCHK(ntg_launch_trig(A, plan_ncu(p), (hipStream_t)stream));
	return 0;
}

// ---------------- min / max expressions over forms declared at the call (ntg_batch_minmax) ----------------
extern "C" int ntg_batch_minmax(const ntg_plan *p, int batch, const double *d_x, int nform, const int *form_nterms, const ntg_form_term *terms, int nfp, const double *d_fprm,
                                int ngroup, const ntg_minmax_group *groups, const ntg_minmax_member *members, double tol, int max_depth, int sides,
                                const double *d_glo, const double *d_ghi, double *d_ext, double *d_when, int *d_which, int *d_status, int *d_npieces,
                                double *d_viol, int *d_where, void *stream)
{
	MinmaxArgs A{};
	FormCross X;
	if (int rc = forms_declare(p, d_x, nform, form_nterms, terms, nfp, d_fprm, tol, max_depth, sides, FormSink{A.row, A.term, NTG_MINMAX_MAXFORMS, NTG_MINMAX_MAXTERMS, true}, X)) return rc;
	if (ngroup < 0 || ngroup > NTG_MINMAX_MAXGROUPS) return fail(NTG_E_BADARG, "ngroup must lie in 0 .. " + std::to_string(NTG_MINMAX_MAXGROUPS));
	if (ngroup > 0 && (!groups || !members)) return fail(NTG_E_BADARG, "null argument: groups and members");
	int mtot = 0, mmax = 0;
	for (int g = 0; g < ngroup; g++) {
		const ntg_minmax_group &Q = groups[g];
		const std::string gname = "group " + std::to_string(g);
		MinmaxGroup &G = A.grp[g];
		if (Q.outer < NTG_MINMAX_MIN || Q.outer > NTG_MINMAX_MAX || Q.inner < NTG_MINMAX_MIN || Q.inner > NTG_MINMAX_MAX)
			return fail(NTG_E_BADARG, gname + ": outer and inner must be NTG_MINMAX_MIN (0) or NTG_MINMAX_MAX (1)");
		if (Q.nclause < 1 || Q.nclause > NTG_MINMAX_MAXCLAUSES) return fail(NTG_E_BADARG, gname + ": nclause = " + std::to_string(Q.nclause) + " must lie in 1 .. " + std::to_string(NTG_MINMAX_MAXCLAUSES));
		G.outer = Q.outer; G.inner = Q.inner; G.m0 = mtot;
		for (int k = 0; k < Q.nclause; k++) {
			const std::string cname = gname + ", clause " + std::to_string(k);
			const int n = Q.nmem[k];
			if (n < 1) return fail(NTG_E_BADARG, cname + " has " + std::to_string(n) + " members: a clause needs at least one");
			if (n > NTG_MINMAX_MAXMEMBERS || G.nm + n > NTG_MINMAX_MAXMEMBERS)
				return fail(NTG_E_BADARG, cname + " brings the group to " + std::to_string(G.nm + n) + " members: at most " + std::to_string(NTG_MINMAX_MAXMEMBERS) + " are taken");
			if (mtot + n > NTG_MINMAX_MAXMEMTOT)
				return fail(NTG_E_BADARG, cname + " brings the members of all groups to " + std::to_string(mtot + n) + ": at most " + std::to_string(NTG_MINMAX_MAXMEMTOT) + " are taken");
			for (int j = 0; j < n; j++) {
				const ntg_minmax_member &m = members[mtot + j];
				const std::string mname = cname + ", member " + std::to_string(j);
				if (m.form < 0 || m.form >= nform) return fail(NTG_E_BADARG, mname + " names form " + std::to_string(m.form) + ": the call declares forms 0 .. " + std::to_string(nform - 1));
				if (m.pc < -1 || m.pc >= nfp) return fail(NTG_E_BADARG, mname + ": pc must lie in -1 .. nfp - 1 = " + std::to_string(nfp - 1));
				if (m.pc >= 0 && !d_fprm) return fail(NTG_E_BADARG, mname + " names a parameter, but d_fprm is null");
				if (!std::isfinite(m.c)) return fail(NTG_E_BADARG, mname + ": c must be finite");
				A.mem[mtot + j] = MinmaxMem{m.form, m.pc, m.c};
			}
			mtot += n; G.nm += n;
			G.clast |= 1u << (G.nm - 1);
		}
		mmax = std::max(mmax, G.nm);
	}
	const bool want_v = d_viol || d_where;
	if (!d_ext && !d_when && !d_which && !d_status && !d_npieces && !want_v)
		return fail(NTG_E_BADARG, "no output asked for: pass d_ext, d_when, d_which, d_status, d_npieces, d_viol or d_where");
	if (want_v && (!d_glo || !d_ghi)) return fail(NTG_E_BADARG, "d_viol / d_where need the bounds d_glo and d_ghi");
	if (batch <= 0 || ngroup == 0) return 0;
	if (int rc = forms_refuse(p, batch, X)) return rc;
	const NtgDims &D = p->D;
	int dmax = 0;
	for (int g = 0; g < ngroup; g++) {   // the one class and the degree of every group
		MinmaxGroup &G = A.grp[g];
		const int f0 = A.mem[G.m0].form;
		G.cl = A.row[f0].cl;
		for (int m = G.m0; m < G.m0 + G.nm; m++) {
			const FormRow &R = A.row[A.mem[m].form];
			if (R.cl != G.cl) {   // two outputs that show it: the first entry of each form
				const auto out_of = [&](int f) { const int u = terms[A.row[f].t0].u; return flag_entry(D, u).o; };
				return fail(NTG_E_UNSUPPORTED, "group " + std::to_string(g) + " names forms " + std::to_string(f0) + " and " + std::to_string(A.mem[m].form) + " on outputs " +
				                                   std::to_string(out_of(f0)) + " and " + std::to_string(out_of(A.mem[m].form)) + " of different basis classes: it has no common pieces");
			}
			G.D = std::max(G.D, R.D);
		}
		dmax = std::max(dmax, G.D);
	}
	cert_base(p, batch, d_x, nullptr, nullptr, A.g, A.q.koff, &A.q.nk);
	A.nform = nform; A.nfp = nfp; A.ngroup = ngroup;
	cert_bisect(A.q, tol, max_depth, sides, d_ext, d_when, d_status, d_npieces, d_viol, d_where);
	A.mcap = mmax <= 8 ? 8 : NTG_MINMAX_MAXMEMBERS;
	A.pw = ntg_minmax_points(A.g, dmax) | 1;
	A.nw = ntg_minmax_lds(A, 4) <= NTG_EXTREMA_LDS_MAX ? 4 : ntg_minmax_lds(A, 2) <= NTG_EXTREMA_LDS_MAX ? 2 : 1;
	if (A.g.kmax > NTG_MAX_ORDER || ntg_minmax_lds(A, A.nw) > NTG_EXTREMA_LDS_MAX)
		return fail(NTG_E_UNSUPPORTED, "the tables and work lists of this call exceed " + std::to_string(NTG_EXTREMA_LDS_MAX / 1024) + " KiB of LDS even with one wavefront: the product and class tables, and per wavefront nC + nfp + " +
		                                   std::to_string(NTG_EXTREMA_CAP) + " (" + std::to_string(A.mcap) + " * " + std::to_string(A.pw) + " + 1) doubles");
	A.fprm = d_fprm; A.glo = d_glo; A.ghi = d_ghi; A.which = d_which;
	HIPCHK(hipSetDevice(p->device));
	HIPCHK(ntg_launch_minmax(A, plan_ncu(p), (hipStream_t)stream));
	return 0;
}
