// solve_launch.hpp -- host launchers of eval_kernel and sqp_kernel: one (family, nout, order) instance at the workgroup
// size the host picked, and the ladders over the sizes for the small and the generic instances.  Included by
// solve_impl.hpp only; the per-family dispatchers (fam_*.hip) call them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include "ntg_dev.hpp"
#include "families.hpp"
#include "eval.hpp"
#include "sqp_kernel.hpp"

// ------------------------------------------------------------------------------------------
// launchers: one (family, nout, order) instance at the workgroup size the host picked
// ------------------------------------------------------------------------------------------
template <int FAM, int NOUT, int K, int NT, int EPT, int CHM = 0>
static hipError_t launch_eval_one(const NtgDims &D, const NtgTables &T, const SmemLayout &L, const EvalArgs &a)
{
	if (NOUT > 0 && D.ncnln > 0 && a.mode == 2 && !a.cj && a.f && a.g && a.c && a.jb && !getenv("NTG_AMD_NO_BANDONLY")) {
		auto kfb = eval_kernel<FAM, NOUT, K, NT, EPT, CHM, (NOUT > 0)>;
		if (L.total > 64 * 1024) (void)hipFuncSetAttribute((const void *)kfb, hipFuncAttributeMaxDynamicSharedMemorySize, L.total);
		hipLaunchKernelGGL(kfb, dim3(a.grid), dim3(NT), L.total, a.st, D, T, L, a.batch, a.mode, a.x, a.f, a.g, a.c, a.jb, a.cj);
		return hipGetLastError();
	}
	auto kfn = eval_kernel<FAM, NOUT, K, NT, EPT, CHM>;
	if (L.total > 64 * 1024) (void)hipFuncSetAttribute((const void *)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, L.total);
	hipLaunchKernelGGL(kfn, dim3(a.grid), dim3(NT), L.total, a.st, D, T, L, a.batch, a.mode, a.x, a.f, a.g, a.c, a.jb, a.cj);
	return hipGetLastError();
}
template <int FAM, int NOUT, int K, int NT, int EPT, bool BIG, bool HESS = true, int CHM = 0, bool NWT = false, bool QPM = false>
static hipError_t launch_sqp_one(const NtgDims &D, const NtgTables &T, const SmemLayout &L, const SolveParams &sp, const SqpArgs &a)
{
	auto kfn = sqp_kernel<FAM, NOUT, K, NT, EPT, BIG, HESS, CHM, NWT, QPM>;
	if (QPM != (sp.hessian == 3)) return hipErrorInvalidValue;
	if (NWT && (!D.nwt_on || !a.nwtw || D.nwt_cg != Family<FAM>::CG || D.nwt_go != Family<FAM>::COUPLE || ((D.nwt_tw ? 2 : 1) * D.nwt_ngrp + D.nwt_nfo) * 64 > NT)) return hipErrorInvalidValue;
	if (L.total > 64 * 1024) (void)hipFuncSetAttribute((const void *)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, L.total);
	hipLaunchKernelGGL(kfn, dim3(a.batch), dim3(NT), L.total, a.st, D, T, L, sp, a.batch, a.lo, a.up, a.x, a.obj, a.inf, a.it, a.nf,
	                   a.cl, a.hist, a.alw, a.vecw, a.nwtw);
	return hipGetLastError();
}
// the small-problem instances: 128 or 256 lanes, all vectors in LDS
template <int FAM, int NOUT, int K, int CHM = 0>
static hipError_t launch_eval_small(const NtgDims &D, const NtgTables &T, const SmemLayout &L, const EvalArgs &a)
{
	if (a.nt == 128) return launch_eval_one<FAM, NOUT, K, 128, 4, CHM>(D, T, L, a);
	if (a.nt == 256) return launch_eval_one<FAM, NOUT, K, 256, 4, CHM>(D, T, L, a);
	return hipErrorInvalidValue;
}
template <int FAM, int NOUT, int K, int CHM = 0>
static hipError_t launch_sqp_small(const NtgDims &D, const NtgTables &T, const SmemLayout &L, const SolveParams &sp, const SqpArgs &a)
{
	if (a.big) return hipErrorInvalidValue;
	if (sp.hessian != 1) {   // identity cold start: the instance without any preconditioner code
		if (a.nt == 128) return launch_sqp_one<FAM, NOUT, K, 128, 4, false, false, CHM>(D, T, L, sp, a);
		if (a.nt == 256) return launch_sqp_one<FAM, NOUT, K, 256, 4, false, false, CHM>(D, T, L, sp, a);
		return hipErrorInvalidValue;
	}
	if (a.nt == 128) return launch_sqp_one<FAM, NOUT, K, 128, 4, false, true, CHM>(D, T, L, sp, a);
	if (a.nt == 256) return launch_sqp_one<FAM, NOUT, K, 256, 4, false, true, CHM>(D, T, L, sp, a);
	return hipErrorInvalidValue;
}
// the generic instance of a family (run-time nout / order) at every workgroup size, LDS-resident or BIG
template <int FAM>
static hipError_t launch_eval_generic(const NtgDims &D, const NtgTables &T, const SmemLayout &L, const EvalArgs &a)
{
	if (a.nt == 128) return launch_eval_one<FAM, 0, 0, 128, 4>(D, T, L, a);
	if (a.nt == 256) return launch_eval_one<FAM, 0, 0, 256, 4>(D, T, L, a);
	if (a.nt == 512) return launch_eval_one<FAM, 0, 0, 512, 4>(D, T, L, a);
	return hipErrorInvalidValue;
}
// structured Newton mode, generic instances (families that offer it: Family::COUPLE > 0)
template <int FAM>
static hipError_t launch_sqp_newton_generic(const NtgDims &D, const NtgTables &T, const SmemLayout &L, const SolveParams &sp, const SqpArgs &a)
{
	if constexpr (Family<FAM>::COUPLE > 0) {
		if (sp.hessian == 3) {   // QP-based SQP step: generic instances
			if (a.big) {
				if (a.nt == 512) return launch_sqp_one<FAM, 0, 0, 512, 4, true, true, 0, true, true>(D, T, L, sp, a);
				return hipErrorInvalidValue;
			}
			if (a.nt == 128) return launch_sqp_one<FAM, 0, 0, 128, 4, false, true, 0, true, true>(D, T, L, sp, a);
			if (a.nt == 256) return launch_sqp_one<FAM, 0, 0, 256, 4, false, true, 0, true, true>(D, T, L, sp, a);
			if (a.nt == 512) return launch_sqp_one<FAM, 0, 0, 512, 4, false, true, 0, true, true>(D, T, L, sp, a);
			return hipErrorInvalidValue;
		}
		if (a.big) {
			if (a.nt == 256) return launch_sqp_one<FAM, 0, 0, 256, 4, true, true, 0, true>(D, T, L, sp, a);
			if (a.nt == 512) return launch_sqp_one<FAM, 0, 0, 512, 4, true, true, 0, true>(D, T, L, sp, a);
			return hipErrorInvalidValue;
		}
		if (a.nt == 128) return launch_sqp_one<FAM, 0, 0, 128, 4, false, true, 0, true>(D, T, L, sp, a);
		if (a.nt == 256) return launch_sqp_one<FAM, 0, 0, 256, 4, false, true, 0, true>(D, T, L, sp, a);
		if (a.nt == 512) return launch_sqp_one<FAM, 0, 0, 512, 4, false, true, 0, true>(D, T, L, sp, a);
	}
	return hipErrorInvalidValue;
}
template <int FAM>
static hipError_t launch_sqp_generic(const NtgDims &D, const NtgTables &T, const SmemLayout &L, const SolveParams &sp, const SqpArgs &a)
{
	if (sp.hessian == 2 || sp.hessian == 3) return launch_sqp_newton_generic<FAM>(D, T, L, sp, a);
	if (a.big) {
		if (a.nt == 256) return launch_sqp_one<FAM, 0, 0, 256, 4, true>(D, T, L, sp, a);
		if (a.nt == 512) return launch_sqp_one<FAM, 0, 0, 512, 4, true>(D, T, L, sp, a);
		return hipErrorInvalidValue;
	}
	if (a.nt == 128) return launch_sqp_one<FAM, 0, 0, 128, 4, false>(D, T, L, sp, a);
	if (a.nt == 256) return launch_sqp_one<FAM, 0, 0, 256, 4, false>(D, T, L, sp, a);
	if (a.nt == 512) return launch_sqp_one<FAM, 0, 0, 512, 4, false>(D, T, L, sp, a);
	return hipErrorInvalidValue;
}
