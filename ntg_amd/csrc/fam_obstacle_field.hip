// fam_obstacle_field.hip -- eval_kernel / sqp_kernel instances of the obstacle-field family (per-problem obstacle centres, families.hpp,
// obstacle_field.hpp); the same instances as fam_obstacle.hip, by the same selection (obstacle_launch.hpp).
#include "obstacle_launch.hpp"

static hipError_t fam_launch_eval(const NtgDims &D, const NtgTables &T, const SmemLayout &L, const EvalArgs &a) { return obstacle_launch_eval<NTG_FAM_OBSTACLE_FIELD>(D, T, L, a); }
static hipError_t fam_launch_sqp(const NtgDims &D, const NtgTables &T, const SmemLayout &L, const SolveParams &sp, const SqpArgs &a) { return obstacle_launch_sqp<NTG_FAM_OBSTACLE_FIELD>(D, T, L, sp, a); }
// (in both passes: the device pass instantiates the time-tile kernels from this line)
static constexpr TileLaunchers fam_tile = obstacle_tile<NTG_FAM_OBSTACLE_FIELD>();

// the family on the host (family_module.hpp): its shape rule, and its descriptor from Family<>'s constants.  Host pass only: the device
// pass would emit the constant object into the device code as well.
#ifndef __HIP_DEVICE_COMPILE__
static const char *shape_rule(const ntg_spec &s)
{
	return s.nout != 2 || s.nnlic || s.nnlfc || s.nnltc < 1 || s.nnltc > Family<NTG_FAM_OBSTACLE_FIELD>::NNLTC
	           ? "obstacle-field family: 2 outputs, 1 to 8 trajectory constraints (one per obstacle), no initial or final rows" : nullptr;
}
static_assert(Family<NTG_FAM_OBSTACLE_FIELD>::NNLTC == 8, "the shape rule's text says 8");
// every row j = (x - cx_j)^2 + (y - cy_j)^2, the centre from the row's parameter block: a sum of squares (ntg_batch_envelope_sos)
static int sos_rows(int, int, NtgSosTerm *t)
{
	t[0] = {0, 0.0, 0}; t[1] = {3, 0.0, 1};
	return 2;
}
static_assert(Family<NTG_FAM_OBSTACLE_FIELD>::NPARAM_ROW == 2, "sos_rows reads cx_j, cy_j");
extern const NtgFamily ntg_fam_obstacle_field =
	ntg_family_sos(ntg_builtin_family<NTG_FAM_OBSTACLE_FIELD>("obstacle_field", 2, shape_rule, fam_launch_eval, fam_launch_sqp, fam_tile, true), sos_rows);
#endif
