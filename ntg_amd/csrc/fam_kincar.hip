// fam_kincar.hip -- eval_kernel / sqp_kernel instances of one problem family (own translation unit: the
// families compile in parallel).  Tuned instances fix nout and the spline order at compile time.
#include "solve_impl.hpp"
#include "check.hpp"
#include "cost.hpp"
#include "verify.hpp"

// fam_kincar_chm.hip: 2 or 6 outputs of order 6 whose cost active variables are the second derivative of every output
hipError_t ntg_launch_eval_kincar_chm(const NtgDims &D, const NtgTables &T, const SmemLayout &L, const EvalArgs &a);
hipError_t ntg_launch_sqp_kincar_chm(const NtgDims &D, const NtgTables &T, const SmemLayout &L, const SolveParams &sp, const SqpArgs &a);

static hipError_t fam_launch_eval(const NtgDims &D, const NtgTables &T, const SmemLayout &L, const EvalArgs &a)
{
	const bool small = (a.nt == 128 || a.nt == 256) && ntg_all_d(D, 3);
	const int ku = ntg_uniform_order(D, a.nt, 4);
	const bool chm = ntg_chm_match(D, 4, 3);
	(void)ku;
	// channel-mask instances: the cost's active variables are the second derivative of every output (kincar.c:133-137)
	if (small && chm && ku == 6 && (D.nout == 2 || D.nout == 4 || D.nout == 6)) return ntg_launch_eval_kincar_chm(D, T, L, a);
	if (small && D.nout == 2 && ku == 6) return launch_eval_small<NTG_FAM_KINCAR, 2, 6>(D, T, L, a);
	if (small && D.nout == 6 && ku == 6) return launch_eval_small<NTG_FAM_KINCAR, 6, 6>(D, T, L, a);
	if (small && D.nout == 2 && ku == 5) return launch_eval_small<NTG_FAM_KINCAR, 2, 5>(D, T, L, a);
	return launch_eval_generic<NTG_FAM_KINCAR>(D, T, L, a);
}

static hipError_t fam_launch_sqp(const NtgDims &D, const NtgTables &T, const SmemLayout &L, const SolveParams &sp, const SqpArgs &a)
{
	const bool small = (a.nt == 128 || a.nt == 256) && ntg_all_d(D, 3);
	const int ku = ntg_uniform_order(D, a.nt, 4);
	const bool chm = ntg_chm_match(D, 4, 3);
	(void)ku;
	if (small && !a.big && chm && ku == 6 && (D.nout == 2 || D.nout == 4 || D.nout == 6)) return ntg_launch_sqp_kincar_chm(D, T, L, sp, a);
	if (small && !a.big && D.nout == 2 && ku == 6) return launch_sqp_small<NTG_FAM_KINCAR, 2, 6>(D, T, L, sp, a);
	if (small && !a.big && D.nout == 6 && ku == 6) return launch_sqp_small<NTG_FAM_KINCAR, 6, 6>(D, T, L, sp, a);
	if (small && !a.big && D.nout == 2 && ku == 5) return launch_sqp_small<NTG_FAM_KINCAR, 2, 5>(D, T, L, sp, a);
	return launch_sqp_generic<NTG_FAM_KINCAR>(D, T, L, sp, a);
}

// the time-tile kernels (check.hpp, cost.hpp, verify.hpp): instances by flag size, the same for the three.  In both passes: the
// device pass instantiates the kernels from this line.
static constexpr TileLaunchers fam_tile = tile_launchers<NTG_FAM_KINCAR, 6, 18, NTG_MAX_NZ>();

// the family on the host (family_module.hpp): its shape rule, and its descriptor from Family<>'s constants.  Host pass only: the device
// pass would emit the constant object into the device code as well.
#ifndef __HIP_DEVICE_COMPILE__
static const char *shape_rule(const ntg_spec &s)
{
	return s.nnlic + s.nnltc * s.nbps + s.nnlfc > 0 ? "family has no nonlinear constraints" : nullptr;
}
extern const NtgFamily ntg_fam_kincar = ntg_builtin_family<NTG_FAM_KINCAR>("kincar", 0, shape_rule, fam_launch_eval, fam_launch_sqp, fam_tile, true);
#endif
