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
extern const NtgFamily ntg_fam_obstacle = ntg_builtin_family<NTG_FAM_OBSTACLE>("obstacle", 2, shape_rule, fam_launch_eval, fam_launch_sqp, fam_tile, true);
#endif
