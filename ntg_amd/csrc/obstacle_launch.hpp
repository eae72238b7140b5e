// obstacle_launch.hpp -- instance selection shared by the two obstacle families (fam_obstacle.hip, fam_obstacle_field.hip): both are
// the kincar cost on two outputs with trajectory rows on (x, y), so each unit instantiates the same shapes for its own family.
// Tuned instances fix nout and the spline order at compile time.
#pragma once
#include "solve_impl.hpp"
#include "check.hpp"
#include "cost.hpp"
#include "verify.hpp"

template <int FAM>
static hipError_t obstacle_launch_eval(const NtgDims &D, const NtgTables &T, const SmemLayout &L, const EvalArgs &a)
{
	const bool small = (a.nt == 128 || a.nt == 256) && ntg_all_d(D, 3);
	const int ku = ntg_uniform_order(D, a.nt, 4);
	(void)ku;
	if (small && D.nout == 2 && ku == 6) return launch_eval_small<FAM, 2, 6>(D, T, L, a);
	return launch_eval_generic<FAM>(D, T, L, a);
}

template <int FAM>
static hipError_t obstacle_launch_sqp(const NtgDims &D, const NtgTables &T, const SmemLayout &L, const SolveParams &sp, const SqpArgs &a)
{
	const bool small = (a.nt == 128 || a.nt == 256) && ntg_all_d(D, 3);
	const int ku = ntg_uniform_order(D, a.nt, 4);
	(void)ku;
	if (small && !a.big && D.nout == 2 && ku == 6 && sp.hessian == 3) {   // QP-based SQP step on the band model (qpdual.hpp)
		if (a.nt == 128) return launch_sqp_one<FAM, 2, 6, 128, 4, false, true, 0, true, true>(D, T, L, sp, a);
		return launch_sqp_one<FAM, 2, 6, 256, 4, false, true, 0, true, true>(D, T, L, sp, a);
	}
	if (small && !a.big && D.nout == 2 && ku == 6 && sp.hessian == 2) {   // structured Newton mode (newton.hpp)
		if (a.nt == 128) return launch_sqp_one<FAM, 2, 6, 128, 4, false, true, 0, true>(D, T, L, sp, a);
		return launch_sqp_one<FAM, 2, 6, 256, 4, false, true, 0, true>(D, T, L, sp, a);
	}
	if (small && !a.big && D.nout == 2 && ku == 6) return launch_sqp_small<FAM, 2, 6>(D, T, L, sp, a);
	return launch_sqp_generic<FAM>(D, T, L, sp, a);
}

// the time-tile kernels (check.hpp, cost.hpp, verify.hpp): the families have two outputs, a flag of 6
template <int FAM>
constexpr TileLaunchers obstacle_tile() { return tile_launchers<FAM, 6>(); }
