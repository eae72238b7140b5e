// family_module.hpp -- what the host knows about a problem family: NtgFamily, the descriptor every reader on the host gets from
// ntg_family(id), and ntg_family_module_desc, the descriptor a loadable family module exports (include/ntg_amd_family.hpp fills it in,
// family_registry.cpp checks it and wraps it into an NtgFamily).  Kept out of include/ntg_amd.h: that header declares plain C functions only.
#pragma once
#include "ntg_dev.hpp"

// stamp of the library's headers (ntg_amd/build.py hashes its HEADERS list and passes -DNTG_AMD_ABI=... to the library and to every
// module): a module compiled against other headers than the library it is loaded into is refused
#ifndef NTG_AMD_ABI
#define NTG_AMD_ABI 0ull
#endif

// the Family<> slot a module's kernels are instantiated for.  Every module uses the same slot, so two modules hold kernels with the
// same mangled names: the module's hidden visibility and dlopen(RTLD_LOCAL) keep each launch inside its own shared object.  At run
// time a module family has the id ntg_family_load() returned (>= NTG_FAM_MODULE_BASE), the kernels never read it.
#define NTG_FAM_MODULE_SLOT 1000
#define NTG_FAMILY_MODULE_ENTRY "ntg_family_module_v1"

typedef hipError_t (*ntg_module_eval_fn)(const NtgDims &, const NtgTables &, const SmemLayout &, const EvalArgs &);
typedef hipError_t (*ntg_module_sqp_fn)(const NtgDims &, const NtgTables &, const SmemLayout &, const SolveParams &, const SqpArgs &);
typedef hipError_t (*ntg_module_check_fn)(const NtgDims &, const NtgTables &, const CheckArgs &);
typedef hipError_t (*ntg_module_cost_fn)(const NtgDims &, const NtgTables &, const CostArgs &);
typedef hipError_t (*ntg_module_verify_fn)(const NtgDims &, const NtgTables &, const VerifyArgs &);
// the launchers of a family's time-tile kernels, made from its one list of flag sizes (tile_launchers, time_tile.hpp)
struct TileLaunchers { ntg_module_check_fn check; ntg_module_cost_fn cost; ntg_module_verify_fn verify; };

struct ntg_family_module_desc {
	unsigned long long abi;   // NTG_AMD_ABI the module was compiled with (first member in every version of the descriptor)
	int sizeof_dims, sizeof_tables, sizeof_layout, sizeof_params, sizeof_eval_args, sizeof_sqp_args;
	const char *name;
	int dm;                   // maxderiv of every output
	int nnlic, nnltc, nnlfc;  // the most nonlinear rows of each kind a plan may use
	int nout;                 // outputs a plan must have (0: any)
	ntg_module_eval_fn launch_eval;
	ntg_module_sqp_fn launch_sqp;
	int nparam, nparam_bp;    // per-problem parameters: doubles per problem, doubles per breakpoint (ntg_plan_param_count)
	int sizeof_check_args;
	ntg_module_check_fn launch_check;   // the module's check_kernel instance (ntg_batch_check)
	int sizeof_cost_args;
	ntg_module_cost_fn launch_cost;     // the module's cost_kernel instance (ntg_batch_cost)
	int sizeof_verify_args;
	ntg_module_verify_fn launch_verify; // the module's verify_kernel instance (ntg_batch_verify)
};
typedef const ntg_family_module_desc *(*ntg_family_module_entry_fn)(void);

// A nonlinear trajectory row declared as a sum of squares of shifted flag entries (ntg_batch_envelope_sos):
//   c_j(z) = sum_{t < nt_j} (z[v_t] - s_t)^2,   s_t = shift_t + (pidx_t >= 0 ? prm_row_j[pidx_t] : 0)
// v: flag entry; prm_row_j: the problem's parameter block of row j (params + j * nparam_row).  Squares only: no weights, no bilinear terms.
struct NtgSosTerm { int v; double shift; int pidx; };
// the declaration of row j for a plan with nout outputs: fills t[0 .. NTG_SOS_MAXTERMS) and returns nt_j, 0: the row is not declared
typedef int (*ntg_sos_decl_fn)(int row, int nout, NtgSosTerm *t);

// One problem family as the host sees it.  A built-in family defines its descriptor in its own fam_*.hip, from Family<FAM>'s constants
// (ntg_builtin_family, families.hpp); a loaded module's is filled from its ntg_family_module_desc at load.
struct NtgFamily {
	const char *name;
	int dm;                    // maxderiv of every output
	int nnlic, nnltc, nnlfc;   // the most nonlinear rows of each kind a plan may use
	int nout;                  // outputs a plan must have (0: any)
	// structured Newton / QP modes (newton.hpp): outputs per coupling group (0: the family has no second-order blocks), size of a group's
	// block, the flag entries of ONE group its rows depend on (relative to the group's first entry), and whether outputs left over
	// after the groups -- outputs that appear in no row -- are allowed
	int couple, cg; u64 group_mask; bool free_outputs_ok;
	int nparam, nparam_bp, nparam_row;   // per-problem parameters: doubles per problem, per breakpoint, per trajectory row function
	bool kincar_flag;          // every pair of outputs is the flat flag of examples/kincar.c (ntg_batch_kincar_reverse)
	// the family's own rule for a plan's shape: the text of the refusal, nullptr if the spec passes.  A module has none: the limits
	// above are its rule
	const char *(*shape)(const ntg_spec &);
	ntg_module_eval_fn launch_eval;
	ntg_module_sqp_fn launch_sqp;
	ntg_module_check_fn launch_check;
	ntg_module_cost_fn launch_cost;
	ntg_module_verify_fn launch_verify;
	// which of the family's trajectory rows are sums of squares (nullptr: none).  A built-in family sets it next to its
	// ntg_builtin_family(...) call (ntg_family_sos); a loaded module declares nothing: ntg_family_module_desc has no field for it
	ntg_sos_decl_fn sos;
};
constexpr NtgFamily ntg_family_sos(NtgFamily f, ntg_sos_decl_fn sos) { f.sos = sos; return f; }

// the registry (family_registry.cpp): ids 0 .. of the built-in families, ids >= NTG_FAM_MODULE_BASE of loaded modules; nullptr for any
// other id (NTG_FAM_HOST included: the host-callback path is not a device family)
const NtgFamily *ntg_family(int family);
