// plan.cpp -- error handling, the device queries, and the entry points behind include/ntg_amd.h that are one launch each: evaluation
// (with its launch shape, which ntg_batch_kkt shares), bounds, the kinematic car's flat-to-state map, the basis of many grids.  The
// solve is in plan_solve.cpp, the calls that sample a trajectory at times in plan_times.cpp; plan_priv.hpp lists the other units.  No
// numerical fallback lives on the host: evaluation and the SQP all run in the kernels.
#include <cstdlib>
#include "plan_priv.hpp"
#include "family_module.hpp"

static thread_local std::string g_err;
int ntg_fail(int code, const std::string &msg) { g_err = msg; return code; }

extern "C" const char *ntg_last_error(void) { return g_err.c_str(); }
extern "C" int ntg_device_count(void)
{
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess) return 0;
	return n;
}
extern "C" void ntg_default_opts(ntg_solve_opts *o)
{
	o->itlim = 0; o->opttol = 0.0; o->steplimit = 2.0; o->ls_mu = 1e-4; o->ls_eta = 0.9;
	o->ls_maxfev = 20; o->hessian = 0; o->fixed_iters = 0; o->block_threads = 0; o->qn_memory = 0; o->warm_start = 0;
}

int plan_ncu(const ntg_plan *p)
{
	if (p->ncu <= 0) {
		hipDeviceProp_t prop;
		p->ncu = (hipGetDeviceProperties(&prop, p->device) == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 256;
	}
	return p->ncu;
}

// launch shape of the evaluation of `batch` problems (ntg_batch_eval, and ntg_batch_kkt for each of its chunks)
int eval_shape(const ntg_plan *p, int batch, EvalShape *s)
{
	const NtgDims &D = p->D;
	int nt = auto_threads(D);
	SmemLayout L = ntg_make_layout(D, nt, 0, 1);
	if (nt == 256 && L.total > 80 * 1024) { nt = 512; L = ntg_make_layout(D, nt, 0, 1); }   // one workgroup per CU anyway: give it more waves
	if (L.total > 160 * 1024) return fail(NTG_E_UNSUPPORTED, "problem tables exceed 160 KiB of LDS");
	// persistent grid = what is resident at once: LDS-limited workgroups per CU, capped by the waves a
	// CU holds (32) and by the register budget the kernel was compiled for (NTG_EVAL_WAVES per SIMD is a
	// lower bound; 8 workgroups of 128 threads = 4 waves per SIMD is the most that can ever be resident)
	const int ncu = plan_ncu(p);
	const int wg_per_cu = std::max(1, std::min(std::min(8, 32 / (nt / 64)), (160 * 1024) / std::max(L.total, 1)));
	int grid = std::min(batch, ncu * wg_per_cu);
	if (const char *eg = getenv("NTG_AMD_EVAL_GRID")) grid = std::max(1, std::min(grid, atoi(eg)));   // experiments only
	s->nt = nt; s->grid = grid; s->L = L;
	return 0;
}

extern "C" int ntg_batch_bounds(const ntg_plan *p, int batch, const double *d_lower, const double *d_upper,
                                double *d_bl, double *d_bu, void *stream)
{
	if (!p) return fail(NTG_E_BADARG, "null plan");
	HIPCHK(hipSetDevice(p->device));
	HIPCHK(ntg_launch_bounds(p->D, batch, d_lower, d_upper, d_bl, d_bu, (hipStream_t)stream));
	return 0;
}

extern "C" int ntg_batch_eval(const ntg_plan *p, int batch, const double *d_x, int mode, double *d_f, double *d_g,
                              double *d_c, double *d_jband, double *d_cjac, void *stream)
{
	if (!p) return fail(NTG_E_BADARG, "null plan");
	if (batch <= 0) return 0;
	if (!d_x) return fail(NTG_E_BADARG, "null x");
	if (mode < 0 || mode > 2) return fail(NTG_E_BADARG, "mode must be 0, 1 or 2");
	if (p->D.family == NTG_FAM_HOST) return fail(NTG_E_UNSUPPORTED, "host-callback plans evaluate through npsolCostFunction");
	if (p->grid_batch && batch != p->grid_batch) return fail(NTG_E_BADARG, "the plan carries per-problem grids for another batch size");
	if (int rc = check_params(p, batch)) return rc;
	HIPCHK(hipSetDevice(p->device));
	const NtgDims &D = p->D;
	EvalShape es;
	if (int rc = eval_shape(p, batch, &es)) return rc;
	hipStream_t st = (hipStream_t)stream;
	if (d_cjac && D.ncnln) HIPCHK(hipMemsetAsync(d_cjac, 0, (size_t)batch * D.ncnln * D.nC * 8, st)); // GcJac starts zeroed (ntg.c:217)
	EvalArgs ea{es.nt, es.grid, plan_ncu(p), batch, mode, d_x, d_f, d_g, d_c, d_jband, d_cjac, st};
	HIPCHK(ntg_launch_eval(D, p->T, es.L, ea));
	return 0;
}

extern "C" int ntg_batch_kincar_reverse(const ntg_plan *p, int batch, int ntimes, const double *d_z, double wheelbase, int reverse_gear,
                                        double *d_state, void *stream)
{
	if (!p) return fail(NTG_E_BADARG, "null plan");
	if (batch <= 0 || ntimes <= 0) return 0;
	if (!d_z || !d_state) return fail(NTG_E_BADARG, "null argument");
	const NtgDims &D = p->D;
	const NtgFamily *f = ntg_family(D.family);
	if (!f || !f->kincar_flag || D.nout % 2 || D.nz != 3 * D.nout)
		return fail(NTG_E_UNSUPPORTED, "kincar_flat_reverse needs a kincar-family plan (two outputs per car, three flag entries per output)");
	if (!(wheelbase > 0.0)) return fail(NTG_E_BADARG, "wheelbase must be positive");
	HIPCHK(hipSetDevice(p->device));
	HIPCHK(ntg_launch_kincar_reverse((long long)batch * ntimes, D.nz, D.nout / 2, wheelbase, reverse_gear, d_z, d_state, (hipStream_t)stream));
	return 0;
}

extern "C" int ntg_basis_batch(int ngrids, int ninterv, int order, int mult, int maxderiv, int nbps, const double *d_knots,
                               const double *d_bps, double *d_blk, int *d_off, void *stream)
{
	if (order < 1 || order > NTG_MAX_ORDER || mult < 0 || mult >= order || maxderiv < 1 || maxderiv > order || ninterv < 1 || nbps < 1)
		return fail(NTG_E_BADARG, "bad spline spec");
	if (ngrids <= 0) return 0;
	if (ngrids > 65535) return fail(NTG_E_BADARG, "at most 65535 grids per call");
	HIPCHK(ntg_launch_basis(ngrids, ninterv, order, mult, maxderiv, nbps, d_knots, d_bps, ninterv + 1, nbps, d_blk, d_off,
	                        (hipStream_t)stream));
	return 0;
}
