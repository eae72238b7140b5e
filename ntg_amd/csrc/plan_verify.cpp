// plan_verify.cpp -- ntg_batch_verify: the analytic derivatives of the plan's family against central differences, at the breakpoints
// (verify.hpp).  The walk over the batch is ntg_batch_check's (time_tile_walk, plan_times.cpp) with the breakpoints as the times -- the plan's,
// or after ntg_plan_set_grids every problem's own: the basis at them in stream-ordered scratch, per-problem grids in chunks of problems
// under the scratch cap.  Scratch of its own: one (value, key) pair per problem, tile of NTG_CHECK_NT breakpoints, slot and kind, which
// verify_final_kernel scans in tile order.  Its owner (StreamScratch) releases it on every path.
#include "plan_priv.hpp"
#include "family_module.hpp"

static int batch_verify(const ntg_plan *p, int batch, const double *d_x, double *d_err, int *d_where, double *d_leak, int *d_leak_where,
                        void *stream, long long scratch_cap)
{
	if (!p) return fail(NTG_E_BADARG, "null plan");
	if (batch <= 0) return 0;
	const NtgDims &D = p->D;
	if (D.family == NTG_FAM_HOST) return fail(NTG_E_UNSUPPORTED, "host-callback plans have no device callbacks to verify");
	if (!d_x) return fail(NTG_E_BADARG, "null argument");
	if (!d_err && !d_where && !d_leak && !d_leak_where) return fail(NTG_E_BADARG, "no output asked for: pass d_err, d_where, d_leak or d_leak_where");
	if (scratch_cap <= 0) return fail(NTG_E_BADARG, "scratch cap must be positive");
	// the breakpoints are the times: one vector for the batch, or every problem's own row of the per-problem grids
	const int P = D.P;
	const long long stride = p->grid_batch ? p->T.pp_bps : 0;
	if (int rc = time_args_check(p, batch, P, stride)) return rc;
	// (time_args_check has refused tables above 160 KiB less check_kernel's 64 static bytes, with the same words; verify_kernel's static part
	// -- the waves' maxima and keys of six slots -- is 512 bytes, so this covers the 448 bytes between the two limits)
	if (ntg_check_lds(D) > NTG_VERIFY_LDS_MAX) return fail(NTG_E_UNSUPPORTED, "basis tables of one breakpoint tile exceed 160 KiB of LDS");
	HIPCHK(hipSetDevice(p->device));
	hipStream_t st = (hipStream_t)stream;
	const int ntiles = (P + NTG_CHECK_NT - 1) / NTG_CHECK_NT;
	const size_t npart = (size_t)batch * ntiles * 2 * NTG_VERIFY_NSLOT;
	VerifyArgs va{};
	va.t.x = d_x; va.t.st = st;
	StreamScratch scratch(st);
	hipError_t e = scratch.alloc(&va.pval, npart);
	if (e == hipSuccess) e = scratch.alloc(&va.pkey, npart);
	return time_tile_run(p, "verify", e, batch, P, p->T.bps, stride, scratch_cap, va.t, [&] { return ntg_launch_verify(D, p->T, va); },
	                     [&] { return ntg_launch_verify_final(batch, ntiles, P, D.nz, va.pval, va.pkey, d_err, d_where, d_leak, d_leak_where, st); });
}

extern "C" int ntg_batch_verify(const ntg_plan *p, int batch, const double *d_x, double *d_err, int *d_where, double *d_leak, int *d_leak_where,
                                void *stream)
{
	return batch_verify(p, batch, d_x, d_err, d_where, d_leak, d_leak_where, stream, NTG_TIME_SCRATCH_CAP);
}
// diagnostic: the same with the scratch cap of the per-problem time tables stated by the caller (tests force several chunks with it)
extern "C" int ntg_debug_batch_verify(const ntg_plan *p, int batch, const double *d_x, double *d_err, int *d_where, double *d_leak,
                                      int *d_leak_where, void *stream, long long scratch_cap)
{
	return batch_verify(p, batch, d_x, d_err, d_where, d_leak, d_leak_where, stream, scratch_cap);
}
