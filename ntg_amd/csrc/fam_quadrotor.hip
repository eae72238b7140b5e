// fam_quadrotor.hip -- eval_kernel / sqp_kernel instances of one problem family (own translation unit: the
// families compile in parallel).  Tuned instances fix nout and the spline order at compile time.
#include "solve_impl.hpp"
#include "check.hpp"
#include "cost.hpp"
#include "verify.hpp"

// config D: 4 outputs, order 8, maxderiv 5 (656 coefficients, 201 breakpoints): 256 lanes, three coefficients per lane
static hipError_t fam_launch_eval(const NtgDims &D, const NtgTables &T, const SmemLayout &L, const EvalArgs &a)
{
	if (a.nt == 256 && ntg_all_d(D, 5) && D.nout == 4 && ntg_uniform_order(D, 256, 4) == 8)
		return launch_eval_one<NTG_FAM_QUADROTOR, 4, 8, 256, 4>(D, T, L, a);
	if (a.nt == 512 && ntg_all_d(D, 5) && D.nout == 4 && ntg_uniform_order(D, 512, 4) == 8)
		return launch_eval_one<NTG_FAM_QUADROTOR, 4, 8, 512, 4>(D, T, L, a);   // one workgroup per CU: more waves per workgroup
	return launch_eval_generic<NTG_FAM_QUADROTOR>(D, T, L, a);
}

static hipError_t fam_launch_sqp(const NtgDims &D, const NtgTables &T, const SmemLayout &L, const SolveParams &sp, const SqpArgs &a)
{
	if (a.nt == 256 && ntg_all_d(D, 5) && D.nout == 4 && ntg_uniform_order(D, 256, 4) == 8) {
		if (sp.hessian == 3) {   // QP-based SQP step on the band model (qpdual.hpp)
			if (!a.big) return launch_sqp_one<NTG_FAM_QUADROTOR, 4, 8, 256, 4, false, true, 0, true, true>(D, T, L, sp, a);
			return launch_sqp_generic<NTG_FAM_QUADROTOR>(D, T, L, sp, a);
		}
		if (sp.hessian == 2) {   // structured Newton mode (newton.hpp)
			if (a.big) return launch_sqp_one<NTG_FAM_QUADROTOR, 4, 8, 256, 4, true, true, 0, true>(D, T, L, sp, a);
			return launch_sqp_one<NTG_FAM_QUADROTOR, 4, 8, 256, 4, false, true, 0, true>(D, T, L, sp, a);
		}
		if (a.big) return launch_sqp_one<NTG_FAM_QUADROTOR, 4, 8, 256, 4, true>(D, T, L, sp, a);
		return launch_sqp_one<NTG_FAM_QUADROTOR, 4, 8, 256, 4, false>(D, T, L, sp, a);
	}
	return launch_sqp_generic<NTG_FAM_QUADROTOR>(D, T, L, sp, a);
}

// the time-tile kernels (check.hpp, cost.hpp, verify.hpp): instances by flag size, the same for the three.  In both passes: the
// device pass instantiates the kernels from this line.
static constexpr TileLaunchers fam_tile = tile_launchers<NTG_FAM_QUADROTOR, 20, NTG_MAX_NZ>();

// the family on the host (family_module.hpp): its shape rule, and its descriptor from Family<>'s constants.  (x, y, z) couple through thrust and
// speed; the yaw output appears in no row: the one family whose plans have a free output (free_outputs_ok).  Host pass only: the device
// pass would emit the constant object into the device code as well.
#ifndef __HIP_DEVICE_COMPILE__
static const char *shape_rule(const ntg_spec &s)
{
	return s.nout != 4 || s.nnlic || s.nnlfc || s.nnltc > 2 ? "quadrotor family: 4 outputs, at most two trajectory constraints" : nullptr;
}
// row 0 = x''^2 + y''^2 + (z'' + g)^2, row 1 = x'^2 + y'^2 + z'^2: sums of squares (ntg_batch_envelope_sos)
static int sos_rows(int row, int, NtgSosTerm *t)
{
	if (row == 0) { t[0] = {2, 0.0, -1}; t[1] = {7, 0.0, -1}; t[2] = {12, -Family<NTG_FAM_QUADROTOR>::G, -1}; return 3; }
	if (row == 1) { t[0] = {1, 0.0, -1}; t[1] = {6, 0.0, -1}; t[2] = {11, 0.0, -1}; return 3; }
	return 0;
}
extern const NtgFamily ntg_fam_quadrotor =
	ntg_family_sos(ntg_builtin_family<NTG_FAM_QUADROTOR>("quadrotor", 4, shape_rule, fam_launch_eval, fam_launch_sqp, fam_tile, false, true), sos_rows);
#endif
