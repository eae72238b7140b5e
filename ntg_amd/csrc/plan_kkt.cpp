// plan_kkt.cpp -- ntg_batch_kkt: first-order optimality residuals of a batch of points, whoever produced them (kkt.hpp).
// The batch goes through in chunks of problems: per chunk the evaluation ntg_batch_eval runs for mode 2 without the dense Jacobian
// (values, gradient, residuals, banded Jacobian rows), the expanded bounds of ntg_batch_bounds, then kkt_kernel.  Scratch, stream ordered,
// one allocation (StreamScratch releases it on every path), per problem of a chunk:
//   f [1]  g [nC]  c [ncnln]  jband [ncnln][sumk]  bl, bu [nC + nclin + ncnln]
// (f is not used: with it the evaluation is the instance ntg_batch_eval launches for the same request).  A chunk holds as many problems
// as stay under the scratch cap, at least one.
#include "plan_priv.hpp"

#define NTG_KKT_SCRATCH_CAP (256ll << 20)

static long long kkt_scratch_doubles(const NtgDims &D) { return 1ll + D.nC + (long long)D.ncnln * (1 + D.sumk) + 2ll * (D.nC + D.nclin + D.ncnln); }

// the tables as problem b0 of the batch sees them at index 0: a launch over the problems [b0, b0 + nb) reads its per-problem values
// (grids, family parameters) by the problem's index within the launch
static NtgTables tables_from(const NtgTables &T0, int b0)
{
	NtgTables T = T0;
	const size_t b = (size_t)b0;
	if (T.pp_rowv) T.rowv += b * T.pp_rowv;
	if (T.pp_bps) T.bps += b * T.pp_bps;
	if (T.pp_lin) { T.csr_val += b * T.pp_lin; T.csc_val += b * T.pp_lin; }
	if (T.pp_sinv) T.sinv_val += b * T.pp_sinv;
	if (T.pp_q) T.q_val += b * T.pp_q;
	if (T.pp_n0b) T.n0b += b * T.pp_n0b;
	if (T.pp_blk) T.blk += b * T.pp_blk;
	if (T.pp_k0) T.nwt_k0 += b * T.pp_k0;
	if (T.pp_lf) T.nwt_lf += b * T.pp_lf;
	if (T.pp_ilin) { T.icsr_val += b * T.pp_ilin; T.icsc_val += b * T.pp_ilin; }
	if (T.pp_prm) T.prm += b * T.pp_prm;
	return T;
}

static int batch_kkt(const ntg_plan *p, int batch, const double *d_x, const double *d_lower, const double *d_upper, const double *d_clambda,
                     double *d_res, double *d_r, void *stream, long long scratch_cap)
{
	if (!p) return fail(NTG_E_BADARG, "null plan");
	if (batch <= 0) return 0;
	const NtgDims &D = p->D;
	if (D.family == NTG_FAM_HOST) return fail(NTG_E_UNSUPPORTED, "host-callback plans have no device evaluation to audit: ntg() returns clambda itself");
	if (!d_x || !d_lower || !d_upper || !d_clambda) return fail(NTG_E_BADARG, "null argument");
	if (!d_res && !d_r) return fail(NTG_E_BADARG, "no output asked for: pass d_res or d_r");
	if (p->grid_batch && batch != p->grid_batch) return fail(NTG_E_BADARG, "the plan carries per-problem grids for another batch size");
	if (int rc = check_params(p, batch)) return rc;
	if (scratch_cap <= 0) return fail(NTG_E_BADARG, "scratch cap must be positive");
	if (ntg_kkt_lds(D) > NTG_KKT_LDS_MAX) return fail(NTG_E_UNSUPPORTED, "residual, coefficients and offset table of one problem exceed 160 KiB of LDS");
	HIPCHK(hipSetDevice(p->device));
	hipStream_t st = (hipStream_t)stream;
	const long long per = kkt_scratch_doubles(D) * 8;   // bytes of one problem
	const int chunk = (int)std::max<long long>(1, std::min<long long>(batch, scratch_cap / per));
	const int ntot = D.nC + D.nclin + D.ncnln;
	EvalShape es;
	if (int rc = eval_shape(p, chunk, &es)) return rc;
	StreamScratch scratch(st);
	double *d_s = nullptr;
	hipError_t e = scratch.alloc(&d_s, (size_t)chunk * kkt_scratch_doubles(D));
	if (e != hipSuccess) return fail(NTG_E_HIP, hipGetErrorString(e));
	double *d_f = d_s, *d_g = d_f + chunk, *d_c = d_g + (size_t)chunk * D.nC, *d_jb = d_c + (size_t)chunk * D.ncnln;
	double *d_bl = d_jb + (size_t)chunk * D.ncnln * D.sumk, *d_bu = d_bl + (size_t)chunk * ntot;
	const int ncu = plan_ncu(p);
	// persistent workgroups: what is resident at once (LDS-limited, at most 8 workgroups of 4 waves per CU)
	const int wg_per_cu = (int)std::max<size_t>(1, std::min<size_t>(8, (160 * 1024) / (ntg_kkt_lds(D) + 256)));
	int rc = 0;
	for (int b0 = 0; b0 < batch && e == hipSuccess && !rc; b0 += chunk) {
		const int nb = std::min(chunk, batch - b0);
		if (nb != chunk) rc = eval_shape(p, nb, &es);   // (the last chunk: the grid follows the number of problems)
		if (rc) break;
		const NtgTables Tc = tables_from(p->T, b0);
		EvalArgs ea{es.nt, es.grid, ncu, nb, 2, d_x + (size_t)b0 * D.nC, d_f, d_g, D.ncnln ? d_c : nullptr, D.ncnln ? d_jb : nullptr, nullptr, st};
		e = ntg_launch_eval(D, Tc, es.L, ea);
		if (e == hipSuccess) e = ntg_launch_bounds(D, nb, d_lower + (size_t)b0 * D.nbounds, d_upper + (size_t)b0 * D.nbounds, d_bl, d_bu, st);
		KktArgs ka{b0, nb, std::min(nb, ncu * wg_per_cu), d_x, d_clambda, d_g, d_c, d_jb, d_bl, d_bu, d_res, d_r, st};
		if (e == hipSuccess) e = ntg_launch_kkt(D, p->T, ka);
	}
	if (rc) return rc;
	if (e != hipSuccess) return fail(NTG_E_HIP, hipGetErrorString(e));
	return 0;
}

extern "C" int ntg_batch_kkt(const ntg_plan *p, int batch, const double *d_x, const double *d_lower, const double *d_upper,
                             const double *d_clambda, double *d_res, double *d_r, void *stream)
{
	return batch_kkt(p, batch, d_x, d_lower, d_upper, d_clambda, d_res, d_r, stream, NTG_KKT_SCRATCH_CAP);
}
// diagnostic: the same with the scratch cap stated by the caller (tests force several chunks with it); one problem takes
// 8 (1 + nC + ncnln (1 + sumk) + 2 (nC + nclin + ncnln)) bytes
extern "C" int ntg_debug_batch_kkt(const ntg_plan *p, int batch, const double *d_x, const double *d_lower, const double *d_upper,
                                   const double *d_clambda, double *d_res, double *d_r, void *stream, long long scratch_cap)
{
	return batch_kkt(p, batch, d_x, d_lower, d_upper, d_clambda, d_res, d_r, stream, scratch_cap);
}
