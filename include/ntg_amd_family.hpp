// include/ntg_amd_family.hpp -- write your own problem family and build it into a loadable module.
//
// A family is a struct of static callbacks, the device counterpart of the six callbacks of ntg() (ntg.h:81-83,90-92):
//
//   ucf(nout, i, z, f, df)     running cost at breakpoint i                       (required)
//   icf(nout, z, f, df)        initial cost                                       (default: 0)
//   fcf(nout, z, f, df)        final cost                                         (default: 0)
//   nlicf(nout, z, c, dc)      initial nonlinear constraint rows, NNLIC of them   (default: none)
//   nltcf(nout, i, z, c, dc)   trajectory nonlinear constraint rows, NNLTC        (default: none)
//   nlfcf(nout, z, c, dc)      final nonlinear constraint rows, NNLFC             (default: none)
//
// The contract (the same the built-in families of ntg_amd/csrc/families.hpp keep):
//   - z is the flat flag of ONE point: output o, derivative r is z[iz[o] + r] with iz[o] = DM * o (== the reference's zp[o][r],
//     colloc.c:425-447).  Every output of a plan that uses the family has maxderiv == DM; nz = DM * nout.
//   - gradients are over the full stacked flag: df[0 .. nz) is written in full (zeros where the function does not depend on an
//     entry), as the reference's callbacks do (cost.c:107-108, constraints.c:146-151).
//   - dc is row-major [ncon][nz] (== the reference's dc[constraint][variable]); c[ncon].
//   - the active-variable lists of the plan (ntg_spec icav/tcav/fcav, icostav/tcostav/fcostav) must cover every flag entry a
//     callback reads: the kernels only materialise the entries some list names.
//   - callbacks are device code: no allocation, no host calls, no recursion; keep them __forceinline__ (NTG_AMD_HD below does).
//
// Per-problem parameters (ntg_plan_set_params): a family that reads data besides the flat flag -- obstacle positions, a
// reference to track -- declares NPARAM (doubles per problem) and / or NPARAM_BP (doubles per breakpoint); a plan of the family then needs
// NPARAM + NPARAM_BP * nbps doubles per problem, laid out [NPARAM fixed | NPARAM_BP for breakpoint 0 | ... ].  Such a family writes EVERY
// callback with one more trailing argument, const double *prm, the problem's row (the same for all breakpoints; ucf / nltcf get the
// breakpoint index i, so breakpoint data is prm[NPARAM + NPARAM_BP * i + k]):
//   ucf(nout, i, z, f, df, prm)   icf(nout, z, f, df, prm)   nltcf(nout, i, z, c, dc, prm)   ... (the defaults come in both forms)
// The row is read only; it is the same for every lane that works on the problem.
//
// Derive from ntg_amd::FamilyDefaults<YourFamily> and write only the callbacks your problem has.  The defaults are: no nonlinear
// rows of any kind (NNLIC = NNLTC = NNLFC = 0), zero initial and final cost, DM = 3, the trajectory rows' two-step form
// (nltc_val / nltc_vjp) through the dense nltcf, and no second-order blocks.  Then, in one .hip file:
//
//   #include "ntg_amd_family.hpp"
//   struct MyFamily : ntg_amd::FamilyDefaults<MyFamily> { static constexpr int NNLTC = 1; static NTG_AMD_HD void ucf(...) {...} ... };
//   NTG_AMD_FAMILY_MODULE(MyFamily, "my_family", 0)        // 0: any number of outputs, else the one a plan must have
//
// build it with ntg_amd.family.build_module("my_family.hip") and load it with ntg_family_load() / ntg_amd.api.load_family(); the id
// it returns goes into ntg_spec.family.  What a module family does not get: the tuned fixed-shape and
// wave-kernel instances, the structured Newton / QP steps (hessian = 2 / 3 act as 1, as for every family without them), the ntg()
// drop-in path.
//
// Without a HIP compiler this header only defines NTG_AMD_HD and the callback defaults, so that a plain C++ build (a host-side test
// shim, a CPU reference) can compile the SAME family header the module is built from.
#pragma once

#if defined(__HIP__) || defined(__HIPCC__)
#ifndef NTG_AMD_ABI
#error "build family modules with ntg_amd.family.build_module(): it passes the header stamp (-DNTG_AMD_ABI) the library checks at load"
#endif
#define NTG_AMD_FAMILY_DEVICE 1
#define NTG_AMD_HD __host__ __device__ __forceinline__
#include "../ntg_amd/csrc/solve_impl.hpp"
#include "../ntg_amd/csrc/check.hpp"
#include "../ntg_amd/csrc/cost.hpp"
#include "../ntg_amd/csrc/verify.hpp"
#include "../ntg_amd/csrc/family_module.hpp"
#else
#define NTG_AMD_FAMILY_DEVICE 0
#define NTG_AMD_HD inline
#endif

namespace ntg_amd {

// F: the family that derives from these defaults (its own members hide the ones here)
template <class F>
struct FamilyDefaults {
	static constexpr int DM = 3;                        // maxderiv of every output
	static constexpr int NNLIC = 0, NNLTC = 0, NNLFC = 0;
	static constexpr int TAPE = 1;                      // doubles nltc_val keeps for nltc_vjp
	static constexpr unsigned long long TCON_VARS = ~0ull;   // flag entries a trajectory row can depend on (all: not declared)
	static constexpr bool PER_OUTPUT_COST = false;      // only the tuned built-in instances use this
	static constexpr int COUPLE = 0, CG = 1;            // no second-order blocks (modules do not offer them)
	static constexpr unsigned long long GROUP_VARS = 0; // flag entries of one coupling group (none: COUPLE = 0)
	static constexpr int NPARAM = 0, NPARAM_BP = 0;     // per-problem parameters: doubles per problem, doubles per breakpoint
	static NTG_AMD_HD int row_group(int) { return 0; }
	static NTG_AMD_HD void icf(int nout, const double *, double &f, double *df)
	{
		f = 0.0;
		for (int v = 0; v < F::DM * nout; v++) df[v] = 0.0;
	}
	static NTG_AMD_HD void fcf(int nout, const double *, double &f, double *df)
	{
		f = 0.0;
		for (int v = 0; v < F::DM * nout; v++) df[v] = 0.0;
	}
	static NTG_AMD_HD void nlicf(int, const double *, double *, double *) {}
	static NTG_AMD_HD void nltcf(int, int, const double *, double *, double *) {}
	static NTG_AMD_HD void nlfcf(int, const double *, double *, double *) {}
	// ... and the same defaults in the form a family with parameters is called in (trailing prm)
	static NTG_AMD_HD void icf(int nout, const double *z, double &f, double *df, const double *) { icf(nout, z, f, df); }
	static NTG_AMD_HD void fcf(int nout, const double *z, double &f, double *df, const double *) { fcf(nout, z, f, df); }
	static NTG_AMD_HD void nlicf(int, const double *, double *, double *, const double *) {}
	static NTG_AMD_HD void nltcf(int, int, const double *, double *, double *, const double *) {}
	static NTG_AMD_HD void nlfcf(int, const double *, double *, double *, const double *) {}
#if NTG_AMD_FAMILY_DEVICE
	// the trajectory rows in the augmented-Lagrangian evaluation's two-step form: values, then df += J' t, both through nltcf
	template <int NZMAX> static __device__ __forceinline__ void nltc_val(int nout, int i, const double *z, double *c, double *) { DenseTraj<F, NZMAX>::val(nout, i, z, c); }
	template <int NZMAX> static __device__ __forceinline__ void nltc_vjp(int nout, int nz, int i, const double *z, const double *t, double *df, const double *) { DenseTraj<F, NZMAX>::vjp(nout, nz, i, z, t, df); }
	template <int NZMAX> static __device__ __forceinline__ void nltc_block(int, int, const double *, const double *, double, bool, double *) {}
	template <int NZMAX> static __device__ __forceinline__ void nltc_val(int nout, int i, const double *z, double *c, double *, const double *prm) { DenseTraj<F, NZMAX>::val(nout, i, z, c, prm); }
	template <int NZMAX> static __device__ __forceinline__ void nltc_vjp(int nout, int nz, int i, const double *z, const double *t, double *df, const double *, const double *prm)
	{
		DenseTraj<F, NZMAX>::vjp(nout, nz, i, z, t, df, prm);
	}
	template <int NZMAX> static __device__ __forceinline__ void nltc_block(int, int, const double *, const double *, double, bool, double *, const double *) {}
#endif
};

}  // namespace ntg_amd

#if NTG_AMD_FAMILY_DEVICE
// FAMILY: the family struct; NAME: a string literal; NOUT_REQUIRED: the number of outputs a plan must have, 0 = any.
// Instantiates the generic kernels (run-time nout and spline order) for FAMILY -- evaluation at 128 / 256 / 512 threads, solve at
// 128 / 256 / 512 threads plus the HBM-resident (BIG) form at 256 / 512, the between-breakpoints check (check.hpp), the running cost
// under a quadrature (cost.hpp) and the derivative audit at the breakpoints (verify.hpp) -- and exports one
// symbol, the entry point ntg_family_module_v1, which returns the descriptor the library checks at load (family_module.hpp).  Use it
// once per module.
// A module is built from two compilations of the same source (ntg_amd/family.py does both): NTG_AMD_MODULE_PART = 1, the evaluation
// and solve instances, the descriptor and the entry point; NTG_AMD_MODULE_PART = 2, the check, cost and verify instances and their launchers alone.  Each
// part keeps its own device assembly.  NTG_AMD_MODULE_PART = 0 (the default) is the whole module in one compilation.
#ifndef NTG_AMD_MODULE_PART
#define NTG_AMD_MODULE_PART 0
#endif
#define NTG_AMD_MODULE_FAMILY_(FAMILY)                                                                                                     \
	static_assert(FAMILY::COUPLE == 0, "module families have no second-order (Newton / QP) blocks");                                       \
	static_assert(FAMILY::DM >= 1 && FAMILY::NNLIC >= 0 && FAMILY::NNLTC >= 0 && FAMILY::NNLFC >= 0, "bad family constants");           \
	static_assert(FamPrmCounts<FAMILY>::n >= 0 && FamPrmCounts<FAMILY>::bp >= 0 && FamPrmRow<FAMILY>::value == 0, "bad parameter counts");  \
	template <> struct Family<NTG_FAM_MODULE_SLOT> : FAMILY {};
// the check, cost and verify launchers: hidden like everything but the entry point, with names of their own so that the two parts can refer to them
#define NTG_AMD_MODULE_CHECK_DECL_                                                                                                         \
	hipError_t ntg_module_launch_check(const NtgDims &D, const NtgTables &T, const CheckArgs &a);                                         \
	hipError_t ntg_module_launch_cost(const NtgDims &D, const NtgTables &T, const CostArgs &a);                                            \
	hipError_t ntg_module_launch_verify(const NtgDims &D, const NtgTables &T, const VerifyArgs &a)
// (their bodies: the one launcher of time_tile.hpp; a module has the widest flag's instances only)
#define NTG_AMD_MODULE_CHECK_                                                                                                              \
	static constexpr TileLaunchers ntg_module_tile = tile_launchers<NTG_FAM_MODULE_SLOT, NTG_MAX_NZ>();                                    \
	hipError_t ntg_module_launch_check(const NtgDims &D, const NtgTables &T, const CheckArgs &a) { return ntg_module_tile.check(D, T, a); } \
	hipError_t ntg_module_launch_cost(const NtgDims &D, const NtgTables &T, const CostArgs &a) { return ntg_module_tile.cost(D, T, a); }   \
	hipError_t ntg_module_launch_verify(const NtgDims &D, const NtgTables &T, const VerifyArgs &a) { return ntg_module_tile.verify(D, T, a); }
#define NTG_AMD_MODULE_MAIN_(FAMILY, NAME, NOUT_REQUIRED)                                                                                  \
	namespace {                                                                                                                            \
	hipError_t ntg_module_launch_eval(const NtgDims &D, const NtgTables &T, const SmemLayout &L, const EvalArgs &a)                      \
	{                                                                                                                                      \
		return launch_eval_generic<NTG_FAM_MODULE_SLOT>(D, T, L, a);                                                                       \
	}                                                                                                                                      \
	hipError_t ntg_module_launch_sqp(const NtgDims &D, const NtgTables &T, const SmemLayout &L, const SolveParams &sp, const SqpArgs &a) \
	{                                                                                                                                      \
		return launch_sqp_generic<NTG_FAM_MODULE_SLOT>(D, T, L, sp, a);                                                                    \
	}                                                                                                                                      \
	const ntg_family_module_desc ntg_module_desc = {                                                                                       \
		NTG_AMD_ABI, (int)sizeof(NtgDims), (int)sizeof(NtgTables), (int)sizeof(SmemLayout), (int)sizeof(SolveParams),                     \
		(int)sizeof(EvalArgs), (int)sizeof(SqpArgs), NAME, FAMILY::DM, FAMILY::NNLIC, FAMILY::NNLTC, FAMILY::NNLFC, (NOUT_REQUIRED),        \
		&ntg_module_launch_eval, &ntg_module_launch_sqp, FamPrmCounts<FAMILY>::n, FamPrmCounts<FAMILY>::bp, (int)sizeof(CheckArgs),     \
		&ntg_module_launch_check, (int)sizeof(CostArgs), &ntg_module_launch_cost, (int)sizeof(VerifyArgs), &ntg_module_launch_verify};                                                                                                  \
	}                                                                                                                                      \
	extern "C" __attribute__((visibility("default"))) const ntg_family_module_desc *ntg_family_module_v1(void) { return &ntg_module_desc; }
#if NTG_AMD_MODULE_PART == 0
#define NTG_AMD_FAMILY_MODULE(FAMILY, NAME, NOUT_REQUIRED) \
	NTG_AMD_MODULE_FAMILY_(FAMILY) NTG_AMD_MODULE_CHECK_ NTG_AMD_MODULE_MAIN_(FAMILY, NAME, NOUT_REQUIRED)
#elif NTG_AMD_MODULE_PART == 1
#define NTG_AMD_FAMILY_MODULE(FAMILY, NAME, NOUT_REQUIRED) \
	NTG_AMD_MODULE_FAMILY_(FAMILY) NTG_AMD_MODULE_CHECK_DECL_; NTG_AMD_MODULE_MAIN_(FAMILY, NAME, NOUT_REQUIRED)
#else
#define NTG_AMD_FAMILY_MODULE(FAMILY, NAME, NOUT_REQUIRED) NTG_AMD_MODULE_FAMILY_(FAMILY) NTG_AMD_MODULE_CHECK_
#endif
#endif
