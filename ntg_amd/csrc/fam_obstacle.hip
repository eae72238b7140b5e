// fam_obstacle.hip -- eval_kernel / sqp_kernel instances of one problem family (own translation unit: the
// families compile in parallel); the selection among them is obstacle_launch.hpp's.
#include "obstacle_launch.hpp"

static hipError_t fam_launch_eval(const NtgDims &D, const NtgTables &T, const SmemLayout &L, const EvalArgs &a) { return obstacle_launch_eval<NTG_FAM_OBSTACLE>(D, T, L, a); }
static hipError_t fam_launch_sqp(const NtgDims &D, const NtgTables &T, const SmemLayout &L, const SolveParams &sp, const SqpArgs &a) { return obstacle_launch_sqp<NTG_FAM_OBSTACLE>(D, T, L, sp, a); }
// (in both passes: the device pass instantiates the time-tile kernels from this line)
static constexpr TileLaunchers fam_tile = obstacle_tile<NTG_FAM_OBSTACLE>();

// the family on the host (family_module.hpp): its shape rule, and its descriptor from Family<>'s constants.  Host pass only: the device
// pass would emit the constant object into the device code as well.
#ifndef __HIP_DEVICE_COMPILE__
static const char *shape_rule(const ntg_spec &s)
{
	return s.nout != 2 || s.nnlic || s.nnlfc || s.nnltc > 1 ? "obstacle family: 2 outputs, at most one trajectory constraint" : nullptr;
}
// row 0 = (x - 20)^2 + (y - 0.5)^2, a sum of squares (ntg_batch_envelope_sos)
static int sos_rows(int row, int, NtgSosTerm *t)
{
	if (row != 0) return 0;
	t[0] = {0, 20.0, -1}; t[1] = {3, 0.5, -1};
	return 2;
}
extern const NtgFamily ntg_fam_obstacle = ntg_family_sos(ntg_builtin_family<NTG_FAM_OBSTACLE>("obstacle", 2, shape_rule, fam_launch_eval, fam_launch_sqp, fam_tile, true), sos_rows);
#endif
