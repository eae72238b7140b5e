// plan_cost.cpp -- ntg_batch_cost: the running cost of a batch of trajectories at arbitrary times, summed under the caller's quadrature
// weights (cost.hpp).  The walk over the batch is ntg_batch_check's (time_tile_walk, plan_times.cpp): the basis at the times in stream-ordered
// scratch, per-problem grids in chunks of problems under the scratch cap.  Scratch of its own: one partial sum per problem and tile of
// NTG_CHECK_NT times, added in tile order by cost_final_kernel.  Its owner (StreamScratch) releases it on every path.
#include "plan_priv.hpp"
#include "family_module.hpp"

static int batch_cost(const ntg_plan *p, int batch, const double *d_x, int ntimes, const double *d_times, const double *d_weights,
                      long long times_stride, double *d_cost, double *d_vals, void *stream, long long scratch_cap)
{
	if (!p) return fail(NTG_E_BADARG, "null plan");
	if (batch <= 0 || ntimes <= 0) return 0;
	const NtgDims &D = p->D;
	if (D.family == NTG_FAM_HOST) return fail(NTG_E_UNSUPPORTED, "host-callback plans have no device cost function to evaluate");
	if (const NtgFamily *f = ntg_family(D.family))
		if (f->nparam_bp > 0) return fail(NTG_E_UNSUPPORTED, "the plan's family reads parameters per breakpoint: they exist at the breakpoints only, not at the times between them");
	if (D.nucf == 0) return fail(NTG_E_BADARG, "the plan has no running cost (nucf = 0)");
	if (!d_x || !d_times) return fail(NTG_E_BADARG, "null argument");
	if (!d_cost && !d_vals) return fail(NTG_E_BADARG, "no output asked for: pass d_cost or d_vals");
	if (d_cost && !d_weights) return fail(NTG_E_BADARG, "the sum needs the quadrature weights (d_weights)");
	if (scratch_cap <= 0) return fail(NTG_E_BADARG, "scratch cap must be positive");
	if (int rc = time_args_check(p, batch, ntimes, times_stride)) return rc;
	HIPCHK(hipSetDevice(p->device));
	hipStream_t st = (hipStream_t)stream;
	const int ntiles = (ntimes + NTG_CHECK_NT - 1) / NTG_CHECK_NT;
	CostArgs ca{};
	ca.t.x = d_x; ca.t.st = st;
	ca.weights = d_cost ? d_weights : nullptr; ca.vals = d_vals;
	StreamScratch scratch(st);
	hipError_t e = hipSuccess;
	if (d_cost) e = scratch.alloc(&ca.pcost, (size_t)batch * ntiles);
	return time_tile_run(p, "cost", e, batch, ntimes, d_times, times_stride, scratch_cap, ca.t, [&] { return ntg_launch_cost(D, p->T, ca); },
	                     [&] { return d_cost ? ntg_launch_cost_final(batch, ntiles, ca.pcost, d_cost, st) : hipSuccess; });
}

extern "C" int ntg_batch_cost(const ntg_plan *p, int batch, const double *d_x, int ntimes, const double *d_times, const double *d_weights,
                              long long times_stride, double *d_cost, double *d_vals, void *stream)
{
	return batch_cost(p, batch, d_x, ntimes, d_times, d_weights, times_stride, d_cost, d_vals, stream, NTG_TIME_SCRATCH_CAP);
}
// diagnostic: the same with the scratch cap of the per-problem time tables stated by the caller (tests force several chunks with it)
extern "C" int ntg_debug_batch_cost(const ntg_plan *p, int batch, const double *d_x, int ntimes, const double *d_times, const double *d_weights,
                                    long long times_stride, double *d_cost, double *d_vals, void *stream, long long scratch_cap)
{
	return batch_cost(p, batch, d_x, ntimes, d_times, d_weights, times_stride, d_cost, d_vals, stream, scratch_cap);
}
