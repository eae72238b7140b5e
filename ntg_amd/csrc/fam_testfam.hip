// fam_testfam.hip -- eval_kernel / sqp_kernel instances of one problem family (own translation unit: the
// families compile in parallel).  Tuned instances fix nout and the spline order at compile time.
#include "solve_impl.hpp"
#include "check.hpp"
#include "cost.hpp"
#include "verify.hpp"

static hipError_t fam_launch_eval(const NtgDims &D, const NtgTables &T, const SmemLayout &L, const EvalArgs &a)
{
	const bool small = (a.nt == 128 || a.nt == 256) && ntg_all_d(D, 3);
	const int ku = ntg_uniform_order(D, a.nt, 4);
	(void)ku;
	if (small && D.nout == 3 && D.nC <= 4 * a.nt && D.nI == 0) return launch_eval_small<NTG_FAM_TESTFAM, 3, 0>(D, T, L, a);
	return launch_eval_generic<NTG_FAM_TESTFAM>(D, T, L, a);
}

static hipError_t fam_launch_sqp(const NtgDims &D, const NtgTables &T, const SmemLayout &L, const SolveParams &sp, const SqpArgs &a)
{
	const bool small = (a.nt == 128 || a.nt == 256) && ntg_all_d(D, 3);
	const int ku = ntg_uniform_order(D, a.nt, 4);
	(void)ku;
	if (small && !a.big && D.nout == 3 && D.nC <= 4 * a.nt && D.nI == 0) return launch_sqp_small<NTG_FAM_TESTFAM, 3, 0>(D, T, L, sp, a);
	return launch_sqp_generic<NTG_FAM_TESTFAM>(D, T, L, sp, a);
}

// the time-tile kernels (check.hpp, cost.hpp, verify.hpp): instances by flag size, the same for the three.  In both passes: the
// device pass instantiates the kernels from this line.
static constexpr TileLaunchers fam_tile = tile_launchers<NTG_FAM_TESTFAM, 9, NTG_MAX_NZ>();

// the family on the host (family_module.hpp): its shape rule, and its descriptor from Family<>'s constants.  Host pass only: the device
// pass would emit the constant object into the device code as well.
#ifndef __HIP_DEVICE_COMPILE__
static const char *shape_rule(const ntg_spec &s)
{
	return s.nnlic > 1 || s.nnltc > 2 || s.nnlfc > 1 ? "testfam has 1/2/1 nonlinear constraints" : nullptr;
}
// row 0 = z_0^2 + z_L^2 (L the last output) is a sum of squares (ntg_batch_envelope_sos); row 1 has a cosine and is not declared
static int sos_rows(int row, int nout, NtgSosTerm *t)
{
	if (row != 0) return 0;
	t[0] = {0, 0.0, -1}; t[1] = {3 * (nout - 1), 0.0, -1};
	return 2;
}
extern const NtgFamily ntg_fam_testfam = ntg_family_sos(ntg_builtin_family<NTG_FAM_TESTFAM>("testfam", 0, shape_rule, fam_launch_eval, fam_launch_sqp, fam_tile), sos_rows);
#endif
