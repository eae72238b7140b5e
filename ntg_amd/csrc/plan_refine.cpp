// plan_refine.cpp -- ntg_batch_refine behind include/ntg_amd.h: which pairs of plans it takes, the conditions under which the spline space
// of `to` contains that of `from` (checked here from the host mirrors on shared grids, by the kernel on per-problem grids), and the launch.
// The arithmetic is in refine.hpp.
#include <cstdio>
#include "plan_priv.hpp"

static std::string out_name(int o) { return "output " + std::to_string(o); }

// shared grids: every break of `from` needs its own partner among `to`'s, the ends theirs (the rule refine_pp_kernel applies per problem)
static int check_breaks(const std::vector<double> &fb, const std::vector<double> &tb, int o)
{
	const int lf = (int)fb.size() - 1, lt = (int)tb.size() - 1;
	const double tol = NTG_REFINE_TOL * (tb[lt] - tb[0]);
	auto text = [](double v) { char s[64]; snprintf(s, sizeof s, "%.17g", v); return std::string(s); };
	std::vector<int> pi(lf + 1);
	for (int i = 0; i <= lf; i++) pi[i] = refine_partner(tb.data(), lt, fb[i]);
	auto apart = [&](int i) { return !(std::fabs(tb[pi[i]] - fb[i]) <= tol); };
	for (int i : {0, lf})   // the ends first, then the interior breaks in order
		if (apart(i) || pi[i] != (i == 0 ? 0 : lt))
			return fail(NTG_E_BADARG, out_name(o) + ": the " + (i == 0 ? "first" : "last") + " breaks of the two plans do not agree (break " + std::to_string(i) + " of `from` at " + text(fb[i]) + ", of `to` at " + text(tb[i == 0 ? 0 : lt]) + ")");
	for (int i = 1; i <= lf; i++) {
		if (i < lf && apart(i)) return fail(NTG_E_BADARG, out_name(o) + ": break " + std::to_string(i) + " of `from` (at " + text(fb[i]) + ") has no partner among the breaks of `to`");
		if (pi[i] <= pi[i - 1]) return fail(NTG_E_BADARG, out_name(o) + ": break " + std::to_string(i) + " of `from` (at " + text(fb[i]) + ") shares its partner among the breaks of `to` with the break before it");
	}
	return 0;
}

extern "C" int ntg_batch_refine(const ntg_plan *from, const ntg_plan *to, int batch, const double *d_x_from, double *d_x_to, void *stream)
{
	if (!from || !to) return fail(NTG_E_BADARG, "null plan");
	if (batch <= 0) return 0;
	const NtgDims &F = from->D, &T = to->D;
	if (F.family == NTG_FAM_HOST || T.family == NTG_FAM_HOST) return fail(NTG_E_UNSUPPORTED, "host-callback plans are not taken by the batch calls");
	if (!d_x_from || !d_x_to) return fail(NTG_E_BADARG, "null argument");
	if (F.nout != T.nout) return fail(NTG_E_BADARG, "the plans differ in nout (" + std::to_string(F.nout) + " and " + std::to_string(T.nout) + ")");
	if (from->device != to->device) return fail(NTG_E_BADARG, "the plans live on different devices");
	for (int o = 0; o < F.nout; o++) {
		if (F.order[o] != T.order[o])
			return fail(NTG_E_BADARG, out_name(o) + ": the plans differ in order (" + std::to_string(F.order[o]) + " and " + std::to_string(T.order[o]) + ")");
		if (T.mult[o] > F.mult[o])
			return fail(NTG_E_BADARG, out_name(o) + ": `to` asks for more smoothness than `from` has (mult " + std::to_string(T.mult[o]) + " > " + std::to_string(F.mult[o]) + ")");
	}
	const int pp = from->grid_batch ? 1 : 0;
	if ((to->grid_batch ? 1 : 0) != pp) return fail(NTG_E_UNSUPPORTED, "one plan is on its own grid and the other on per-problem grids: refine takes two of a kind");
	if (pp && (batch != from->grid_batch || batch != to->grid_batch)) return fail(NTG_E_BADARG, "the plans carry per-problem grids for another batch size");
	if (pp && (F.nclass != 1 || T.nclass != 1)) return fail(NTG_E_UNSUPPORTED, "per-problem grids need one basis class in each plan");
	const char *a0 = (const char *)d_x_from, *a1 = a0 + (size_t)batch * F.nC * 8, *b0 = (const char *)d_x_to, *b1 = b0 + (size_t)batch * T.nC * 8;
	if (a0 < b1 && b0 < a1) return fail(NTG_E_BADARG, "d_x_from and d_x_to overlap");

	RefineArgs A{};
	A.nout = F.nout; A.batch = batch; A.nCf = F.nC; A.nCt = T.nC; A.xf = d_x_from; A.xt = d_x_to;
	for (int o = 0; o < F.nout; o++) {
		RefineOut &R = A.o[o];
		R.k = F.order[o]; R.mf = F.mult[o]; R.mt = T.mult[o]; R.lf = F.ninterv[o]; R.lt = T.ninterv[o];
		R.nf = F.ncoef[o]; R.nt = T.ncoef[o]; R.icf = F.iC[o]; R.ict = T.iC[o]; R.rep = o;
		A.lmax_f = std::max(A.lmax_f, R.lf); A.lmax_t = std::max(A.lmax_t, R.lt);
		// outputs with the same two spline spaces share one band of weights: same basis class in both plans
		for (int r = 0; r < o; r++)
			if (F.cls[r] == F.cls[o] && T.cls[r] == T.cls[o]) { R.rep = A.o[r].rep; break; }
		if (R.rep == o) { R.aoff = A.na; A.na += R.nt * R.k; } else R.aoff = A.o[R.rep].aoff;
		if (pp) { A.bf[o] = from->d_grid_knots; A.bt[o] = to->d_grid_knots; }
		else { A.bf[o] = from->d_knots[F.cls[o]]; A.bt[o] = to->d_knots[T.cls[o]]; }
	}
	if (!pp)
		for (int o = 0; o < F.nout; o++)
			if (A.o[o].rep == o)
				if (int rc = check_breaks(from->h_knots[o], to->h_knots[o], o)) return rc;
	if (ntg_refine_lds(A, pp) > NTG_REFINE_LDS_MAX) return fail(NTG_E_UNSUPPORTED, "the refinement tables of this pair of plans exceed 64 KiB of LDS");

	HIPCHK(hipSetDevice(from->device));
	hipStream_t st = (hipStream_t)stream;
	if (!pp) {
		HIPCHK(ntg_launch_refine(A, 0, plan_ncu(to), st));
		return 0;
	}
	// per-problem grids: the kernel checks every problem's two break sequences; the call waits for its error word
	StreamScratch scratch(st);
	hipError_t e = scratch.alloc(&A.err, 1);
	if (e == hipSuccess) e = hipMemsetAsync(A.err, 0xff, 8, st);
	if (e == hipSuccess) e = ntg_launch_refine(A, 1, plan_ncu(to), st);
	unsigned long long herr = ~0ull;
	if (e == hipSuccess) e = hipMemcpyAsync(&herr, A.err, 8, hipMemcpyDeviceToHost, st);
	const hipError_t es = hipStreamSynchronize(st);
	HIPCHK(e);
	HIPCHK(es);
	if (herr != ~0ull) {
		const int b = (int)(herr >> 32), code = (int)((herr >> 24) & 0xff), i = (int)(herr & 0xffffff);
		const std::string where = "problem " + std::to_string(b) + ": ";
		if (code == NTG_REFINE_E_ENDS) return fail(NTG_E_BADARG, where + "the " + (i == 0 ? "first" : "last") + " breaks of the two grids do not agree (break " + std::to_string(i) + " of `from`)");
		if (code == NTG_REFINE_E_PARTNER) return fail(NTG_E_BADARG, where + "break " + std::to_string(i) + " of `from` has no partner among the breaks of `to`");
		return fail(NTG_E_BADARG, where + "break " + std::to_string(i) + " of `from` shares its partner among the breaks of `to` with the break before it");
	}
	return 0;
}
