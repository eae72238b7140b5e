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
};

// the registry (family_registry.cpp): ids 0 .. of the built-in families, ids >= NTG_FAM_MODULE_BASE of loaded modules; nullptr for any
// other id (NTG_FAM_HOST included: the host-callback path is not a device family)
const NtgFamily *ntg_family(int family);
