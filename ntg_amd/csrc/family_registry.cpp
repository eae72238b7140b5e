// family_registry.cpp -- the one table of problem families: the built-in ones by id, and user families loaded at run time
// (ntg_family_load / ntg_family_info of include/ntg_amd.h).  Every reader on the host -- plan construction, the launch dispatch
// below -- asks ntg_family(id) and gets the family's descriptor (NtgFamily, family_module.hpp).
//
// A module is a shared object built from include/ntg_amd_family.hpp (ntg_amd/family.py: build_module): the generic eval_kernel /
// sqp_kernel instances of one family and one exported entry point that returns its descriptor (family_module.hpp).  Loading is a
// dlopen(RTLD_NOW | RTLD_LOCAL) and a check of that descriptor against this library's build -- no HIP call, so it works without a GPU.
// Module ids are NTG_FAM_MODULE_BASE + the order of loading; the same file loaded twice keeps its id; modules are never unloaded
// (their launchers may sit in a captured hipGraph of any plan).
#include <dlfcn.h>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <mutex>
#include <string>
#include "family_module.hpp"
#include "plan.hpp"

#define NTG_FAM_MODULE_MAX 64   // modules one process may load

// the built-in families, each defined in its own fam_*.hip from Family<FAM>'s constants; indexed by family id
extern const NtgFamily ntg_fam_kincar, ntg_fam_vanderpol, ntg_fam_testfam, ntg_fam_obstacle, ntg_fam_quadrotor, ntg_fam_manip, ntg_fam_obstacle_field;
static const NtgFamily *const g_builtin[] = {&ntg_fam_kincar, &ntg_fam_vanderpol, &ntg_fam_testfam, &ntg_fam_obstacle, &ntg_fam_quadrotor, &ntg_fam_manip, &ntg_fam_obstacle_field};
static_assert(NTG_FAM_KINCAR == 0 && NTG_FAM_VANDERPOL == 1 && NTG_FAM_TESTFAM == 2 && NTG_FAM_OBSTACLE == 3 && NTG_FAM_QUADROTOR == 4 && NTG_FAM_MANIP == 5 &&
                  NTG_FAM_OBSTACLE_FIELD == 6 && sizeof(g_builtin) / sizeof(g_builtin[0]) == 7, "g_builtin is indexed by family id");

static std::mutex g_mutex;   // serialises loading; lookups read the published descriptors without it
static NtgFamily g_wrapped[NTG_FAM_MODULE_MAX];   // a loaded module's descriptor as an NtgFamily, filled once before it is published
static std::atomic<const NtgFamily *> g_module[NTG_FAM_MODULE_MAX];
static std::string g_path[NTG_FAM_MODULE_MAX];   // resolved path of every loaded module (guarded by g_mutex)
static int g_count = 0;

static const NtgFamily *module_family(int family)
{
	const int j = family - NTG_FAM_MODULE_BASE;
	if (j < 0 || j >= NTG_FAM_MODULE_MAX) return nullptr;
	return g_module[j].load(std::memory_order_acquire);
}

const NtgFamily *ntg_family(int family)
{
	if (family >= 0 && family < (int)(sizeof(g_builtin) / sizeof(g_builtin[0]))) return g_builtin[family];
	return module_family(family);
}

// family dispatch: every family, built in (its translation unit fam_*.hip picks between its tuned -- compile-time nout / order -- instances
// and the generic one) or loaded from a module, launches its eval_kernel, sqp_kernel, check_kernel, cost_kernel and verify_kernel
// instances through its descriptor
template <class Call> static hipError_t via_family(const NtgDims &D, Call call)
{
	const NtgFamily *f = ntg_family(D.family);
	return f ? call(*f) : hipErrorInvalidValue;
}
hipError_t ntg_launch_eval(const NtgDims &D, const NtgTables &T, const SmemLayout &L, const EvalArgs &a) { return via_family(D, [&](const NtgFamily &f) { return f.launch_eval(D, T, L, a); }); }
hipError_t ntg_launch_sqp(const NtgDims &D, const NtgTables &T, const SmemLayout &L, const SolveParams &sp, const SqpArgs &a) { return via_family(D, [&](const NtgFamily &f) { return f.launch_sqp(D, T, L, sp, a); }); }
hipError_t ntg_launch_check(const NtgDims &D, const NtgTables &T, const CheckArgs &a) { return via_family(D, [&](const NtgFamily &f) { return f.launch_check(D, T, a); }); }
hipError_t ntg_launch_cost(const NtgDims &D, const NtgTables &T, const CostArgs &a) { return via_family(D, [&](const NtgFamily &f) { return f.launch_cost(D, T, a); }); }
hipError_t ntg_launch_verify(const NtgDims &D, const NtgTables &T, const VerifyArgs &a) { return via_family(D, [&](const NtgFamily &f) { return f.launch_verify(D, T, a); }); }

static std::string hex64(unsigned long long v)
{
	char b[32];
	std::snprintf(b, sizeof b, "%016llx", v);
	return b;
}

static int size_mismatch(const std::string &path, const char *what, int mod, int lib)
{
	return ntg_fail(NTG_E_BADARG, "family module " + path + ": sizeof(" + what + ") is " + std::to_string(mod) + " in the module, " +
	                                  std::to_string(lib) + " in the library: rebuild the module against this library's headers");
}

extern "C" int ntg_family_load(const char *path, int *family)
{
	if (!path || !family) return ntg_fail(NTG_E_BADARG, "null argument");
	char buf[PATH_MAX];
	if (!realpath(path, buf)) return ntg_fail(NTG_E_BADARG, std::string("family module not found: ") + path);
	const std::string rp(buf);
	std::lock_guard<std::mutex> lk(g_mutex);
	for (int j = 0; j < g_count; j++)
		if (g_path[j] == rp) { *family = NTG_FAM_MODULE_BASE + j; return 0; }
	if (g_count >= NTG_FAM_MODULE_MAX) return ntg_fail(NTG_E_BADARG, "too many family modules loaded (" + std::to_string(NTG_FAM_MODULE_MAX) + ")");
	// (a refused module is not closed again either: its HIP registration ran when it was opened)
	void *h = dlopen(rp.c_str(), RTLD_NOW | RTLD_LOCAL);
	if (!h) { const char *e = dlerror(); return ntg_fail(NTG_E_BADARG, "cannot open family module " + rp + ": " + (e ? e : "?")); }
	auto entry = (ntg_family_module_entry_fn)dlsym(h, NTG_FAMILY_MODULE_ENTRY);
	if (!entry) return ntg_fail(NTG_E_BADARG, "family module " + rp + " has no entry point " NTG_FAMILY_MODULE_ENTRY " (built without NTG_AMD_FAMILY_MODULE?)");
	const ntg_family_module_desc *d = entry();
	if (!d) return ntg_fail(NTG_E_BADARG, "family module " + rp + ": null descriptor");
	if (d->abi != (unsigned long long)NTG_AMD_ABI)
		return ntg_fail(NTG_E_BADARG, "family module " + rp + " was built against headers with ABI stamp " + hex64(d->abi) + ", this library has " +
		                                  hex64((unsigned long long)NTG_AMD_ABI) + ": rebuild the module (ntg_amd.family.build_module)");
	if (d->sizeof_dims != (int)sizeof(NtgDims)) return size_mismatch(rp, "NtgDims", d->sizeof_dims, (int)sizeof(NtgDims));
	if (d->sizeof_tables != (int)sizeof(NtgTables)) return size_mismatch(rp, "NtgTables", d->sizeof_tables, (int)sizeof(NtgTables));
	if (d->sizeof_layout != (int)sizeof(SmemLayout)) return size_mismatch(rp, "SmemLayout", d->sizeof_layout, (int)sizeof(SmemLayout));
	if (d->sizeof_params != (int)sizeof(SolveParams)) return size_mismatch(rp, "SolveParams", d->sizeof_params, (int)sizeof(SolveParams));
	if (d->sizeof_eval_args != (int)sizeof(EvalArgs)) return size_mismatch(rp, "EvalArgs", d->sizeof_eval_args, (int)sizeof(EvalArgs));
	if (d->sizeof_sqp_args != (int)sizeof(SqpArgs)) return size_mismatch(rp, "SqpArgs", d->sizeof_sqp_args, (int)sizeof(SqpArgs));
	if (d->sizeof_check_args != (int)sizeof(CheckArgs)) return size_mismatch(rp, "CheckArgs", d->sizeof_check_args, (int)sizeof(CheckArgs));
	if (d->sizeof_cost_args != (int)sizeof(CostArgs)) return size_mismatch(rp, "CostArgs", d->sizeof_cost_args, (int)sizeof(CostArgs));
	if (d->sizeof_verify_args != (int)sizeof(VerifyArgs)) return size_mismatch(rp, "VerifyArgs", d->sizeof_verify_args, (int)sizeof(VerifyArgs));
	if (!d->name || !d->launch_eval || !d->launch_sqp || !d->launch_check || !d->launch_cost || !d->launch_verify || d->dm < 1 || d->dm > NTG_MAX_ORDER || d->nnlic < 0 || d->nnltc < 0 || d->nnlfc < 0 ||
	    d->nout < 0 || d->nout > NTG_MAX_OUT || d->nparam < 0 || d->nparam_bp < 0)
		return ntg_fail(NTG_E_BADARG, "family module " + rp + ": malformed descriptor");
	NtgFamily &f = g_wrapped[g_count];
	f = NtgFamily{};   // no coupling blocks, no shape rule of its own, no kincar flag
	f.name = d->name; f.dm = d->dm; f.nnlic = d->nnlic; f.nnltc = d->nnltc; f.nnlfc = d->nnlfc; f.nout = d->nout; f.cg = 1;
	f.nparam = d->nparam; f.nparam_bp = d->nparam_bp;
	f.launch_eval = d->launch_eval; f.launch_sqp = d->launch_sqp; f.launch_check = d->launch_check; f.launch_cost = d->launch_cost; f.launch_verify = d->launch_verify;
	g_path[g_count] = rp;
	g_module[g_count].store(&f, std::memory_order_release);
	*family = NTG_FAM_MODULE_BASE + g_count++;
	return 0;
}

extern "C" int ntg_family_info(int family, char *name, int name_len, int *maxderiv, int *nnlic, int *nnltc, int *nnlfc, int *nout)
{
	const NtgFamily *d = module_family(family);   // (built-in ids are refused: the call describes what ntg_family_load returned)
	if (!d) return ntg_fail(NTG_E_BADARG, "not a loaded family module: " + std::to_string(family));
	if (name && name_len > 0) { std::strncpy(name, d->name, (size_t)name_len - 1); name[name_len - 1] = '\0'; }
	if (maxderiv) *maxderiv = d->dm;
	if (nnlic) *nnlic = d->nnlic;
	if (nnltc) *nnltc = d->nnltc;
	if (nnlfc) *nnlfc = d->nnlfc;
	if (nout) *nout = d->nout;
	return 0;
}
