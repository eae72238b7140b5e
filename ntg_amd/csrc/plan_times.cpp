// plan_times.cpp -- the calls that sample a trajectory at the caller's times, and what they share on the host: the layout refusals of a
// time vector, and the one builder of "basis_kernel's output at the times, in stream-ordered scratch" (time_tables_walk).  Its users:
// ntg_batch_interp here, which writes the flat flag, and the walk of the kernels with times on the lanes (time_tile.hpp) --
// ntg_batch_check here, ntg_batch_cost in plan_cost.cpp, ntg_batch_verify in plan_verify.cpp.  Nothing here waits for the stream or
// copies from host memory: every call can sit in a captured stream.
#include "plan_priv.hpp"
#include "family_module.hpp"

// What a call with a time vector refuses about its layout, in the order the calls document; 0: go on.
static int time_layout_check(const ntg_plan *p, int batch, int ntimes, long long times_stride)
{
	if (p->grid_batch && batch != p->grid_batch) return fail(NTG_E_BADARG, "the plan carries per-problem grids for another batch size");
	if (times_stride != 0 && times_stride < ntimes) return fail(NTG_E_BADARG, "times_stride must be 0 (one time vector for the batch) or >= ntimes");
	if (times_stride != 0 && !p->grid_batch) return fail(NTG_E_BADARG, "per-problem times need per-problem grids (ntg_plan_set_grids); pass times_stride = 0");
	return 0;
}

// ... and what the calls on time tiles refuse besides: the parameters and the LDS
int time_args_check(const ntg_plan *p, int batch, int ntimes, long long times_stride)
{
	if (int rc = time_layout_check(p, batch, ntimes, times_stride)) return rc;
	if (int rc = check_params(p, batch)) return rc;
	if (ntg_check_lds(p->D) > NTG_CHECK_LDS_MAX) return fail(NTG_E_UNSUPPORTED, "basis tables of one time tile exceed 160 KiB of LDS");
	return 0;
}

// The builder: the basis of every class at the times (the same kernel that builds the collocation tables) in scratch it owns, stream
// ordered and released when it returns, handed to use() one chunk of problems at a time.
// On the shared grid the tables do not depend on the batch: one set, one chunk.  On per-problem grids every problem is on its own knots
// (one basis class), at its own times or, times_stride == 0, all at the same; its tables are as large as its flags would be, so the batch
// goes through in chunks of problems whose tables stay under scratch_cap bytes (at least one problem per chunk).
hipError_t time_tables_walk(const ntg_plan *p, int batch, int ntimes, const double *d_times, long long times_stride, long long scratch_cap,
                            hipStream_t st, const std::function<hipError_t(const TimeTables &)> &use)
{
	const NtgDims &D = p->D;
	TimeTables t{};
	t.pp = p->grid_batch ? 1 : 0;
	size_t tot = 0;   // doubles of one set of time tables: every class on the shared grid, the one class of a problem on per-problem grids
	for (int c = 0; c < D.nclass; c++) { t.gbase[c] = (int)tot; tot += (size_t)ntimes * D.cls_k[c] * D.cls_d[c]; }
	t.pp_tab = (long long)tot;
	const size_t per_tab = tot * 8 + (size_t)(t.pp ? 1 : D.nclass) * ntimes * 4;   // bytes of one set
	const int chunk = t.pp ? (int)std::max<long long>(1, std::min<long long>(batch, scratch_cap / (long long)per_tab)) : batch;
	const int ntab = t.pp ? chunk : 1;
	StreamScratch scratch(st);
	double *d_tblk = nullptr; int *d_toff = nullptr;
	hipError_t e = scratch.alloc(&d_tblk, (size_t)ntab * tot);
	if (e == hipSuccess) e = scratch.alloc(&d_toff, (size_t)ntab * (t.pp ? 1 : D.nclass) * ntimes);
	t.tblk = d_tblk; t.toff = d_toff;
	const int l = D.cls_l[0];
	for (int b0 = 0; b0 < batch && e == hipSuccess; b0 += chunk) {
		t.b0 = b0; t.nb = std::min(chunk, batch - b0);
		for (int c = 0; !t.pp && c < D.nclass && e == hipSuccess; c++)
			e = ntg_launch_basis(1, D.cls_l[c], D.cls_k[c], D.cls_m[c], D.cls_d[c], ntimes, p->d_knots[c], d_times, 0, 0, d_tblk + t.gbase[c], d_toff + (size_t)c * ntimes, st);
		for (int g0 = 0; t.pp && g0 < t.nb && e == hipSuccess; g0 += 65535)   // (basis_kernel takes at most 65535 grids per launch)
			e = ntg_launch_basis(std::min(65535, t.nb - g0), l, D.cls_k[0], D.cls_m[0], D.cls_d[0], ntimes, p->d_grid_knots + (size_t)(b0 + g0) * (l + 1),
			                     d_times + (size_t)(b0 + g0) * times_stride, l + 1, times_stride, d_tblk + (size_t)g0 * tot, d_toff + (size_t)g0 * ntimes, st);
		if (e == hipSuccess) e = use(t);
	}
	return e;
}

// ---- ntg_batch_interp: the flat flag at the times (interp_kernel, times.hip) ----
static int batch_interp(const ntg_plan *p, int batch, const double *d_x, int ntimes, const double *d_times, long long times_stride, double *d_z,
                        void *stream, long long scratch_cap)
{
	if (!p) return fail(NTG_E_BADARG, "null plan");
	if (batch <= 0 || ntimes <= 0) return 0;
	if (!d_x || !d_times || !d_z) return fail(NTG_E_BADARG, "null argument");
	if (scratch_cap <= 0) return fail(NTG_E_BADARG, "scratch cap must be positive");
	if (int rc = time_layout_check(p, batch, ntimes, times_stride)) return rc;
	HIPCHK(hipSetDevice(p->device));
	hipStream_t st = (hipStream_t)stream;
	InterpArgs a{};
	a.ntimes = ntimes; a.x = d_x; a.z = d_z;
	const hipError_t e = time_tables_walk(p, batch, ntimes, d_times, times_stride, scratch_cap, st, [&](const TimeTables &t) { a.t = t; return ntg_launch_interp(p->D, a, st); });
	if (e != hipSuccess) return fail(NTG_E_HIP, hipGetErrorString(e));
	return 0;
}

extern "C" int ntg_batch_interp_strided(const ntg_plan *p, int batch, const double *d_x, int ntimes, const double *d_times,
                                        long long times_stride, double *d_z, void *stream)
{
	return batch_interp(p, batch, d_x, ntimes, d_times, times_stride, d_z, stream, NTG_TIME_SCRATCH_CAP);
}
extern "C" int ntg_batch_interp(const ntg_plan *p, int batch, const double *d_x, int ntimes, const double *d_times, double *d_z,
                                void *stream)
{
	// documented layout of d_times: [ntimes] on the plan's grid, [batch][ntimes] with per-problem grids
	return ntg_batch_interp_strided(p, batch, d_x, ntimes, d_times, (p && p->grid_batch) ? (long long)ntimes : 0, d_z, stream);
}
// diagnostic: the same with the scratch cap of the per-problem time tables stated by the caller (tests force several chunks with it)
extern "C" int ntg_debug_batch_interp_strided(const ntg_plan *p, int batch, const double *d_x, int ntimes, const double *d_times,
                                              long long times_stride, double *d_z, void *stream, long long scratch_cap)
{
	return batch_interp(p, batch, d_x, ntimes, d_times, times_stride, d_z, stream, scratch_cap);
}

// ---- the kernels with times on the lanes (time_tile.hpp): ntg_batch_check here, ntg_batch_cost in plan_cost.cpp, ntg_batch_verify in
// plan_verify.cpp ----
// The walk over the batch: fills the tile fields of `a` (the caller set x, st and its own fields) from the builder's chunks and calls
// launch() for every one.
hipError_t time_tile_walk(const ntg_plan *p, int batch, int ntimes, const double *d_times, long long times_stride, long long scratch_cap,
                          CheckArgs &a, const std::function<hipError_t()> &launch)
{
	const NtgDims &D = p->D;
	a.ntimes = ntimes; a.ntiles = (ntimes + NTG_CHECK_NT - 1) / NTG_CHECK_NT;
	a.times_stride = times_stride; a.times = d_times; a.sumkd = 0;
	for (int c = 0; c < D.nclass; c++) { a.lbase[c] = a.sumkd; a.sumkd += D.cls_k[c] * D.cls_d[c]; }
	// workgroups: (time tile, group of problems); a group's problems share the staged tile on the shared grid, so no more groups than
	// fill the device a few times over
	const int want_groups = std::max(1, (8 * plan_ncu(p) + a.ntiles - 1) / a.ntiles);
	return time_tables_walk(p, batch, ntimes, d_times, times_stride, scratch_cap, a.st, [&](const TimeTables &t) {
		a.b0 = t.b0; a.nb = t.nb; a.pp = t.pp; a.pp_tab = t.pp_tab; a.tblk = t.tblk; a.toff = t.toff;
		std::copy(t.gbase, t.gbase + NTG_MAX_OUT, a.gbase);
		a.ngroups = std::min(std::min(t.nb, want_groups), 65535);
		return launch();
	});
}

// ---- ntg_batch_check: the trajectory rows of solved problems between the breakpoints (check.hpp) ----
// Scratch besides the walk's: one (violation, key) pair per problem and tile of NTG_CHECK_NT times.
static int batch_check(const ntg_plan *p, int batch, const double *d_x, const double *d_lower, const double *d_upper, int ntimes,
                       const double *d_times, long long times_stride, double *d_viol, int *d_where, double *d_rows, void *stream,
                       long long scratch_cap)
{
	if (!p) return fail(NTG_E_BADARG, "null plan");
	if (batch <= 0 || ntimes <= 0) return 0;
	const NtgDims &D = p->D;
	if (D.family == NTG_FAM_HOST) return fail(NTG_E_UNSUPPORTED, "host-callback plans have no device row functions to check");
	if (const NtgFamily *f = ntg_family(D.family))
		if (f->nparam_bp > 0) return fail(NTG_E_UNSUPPORTED, "the plan's family reads parameters per breakpoint: they exist at the breakpoints only, not at the times between them");
	if (D.nltc + D.nnltc == 0) return fail(NTG_E_BADARG, "no trajectory rows to check");
	if (!d_x || !d_times) return fail(NTG_E_BADARG, "null argument");
	if (!d_viol && !d_where && !d_rows) return fail(NTG_E_BADARG, "no output asked for: pass d_viol, d_where or d_rows");
	if ((d_viol || d_where) && (!d_lower || !d_upper)) return fail(NTG_E_BADARG, "violations need the bounds (d_lower, d_upper)");
	if (scratch_cap <= 0) return fail(NTG_E_BADARG, "scratch cap must be positive");
	if (int rc = time_args_check(p, batch, ntimes, times_stride)) return rc;
	HIPCHK(hipSetDevice(p->device));
	hipStream_t st = (hipStream_t)stream;
	const bool want_max = d_viol || d_where;
	const int ntiles = (ntimes + NTG_CHECK_NT - 1) / NTG_CHECK_NT;
	CheckArgs a{};
	a.x = d_x; a.lo = want_max ? d_lower : nullptr; a.up = want_max ? d_upper : nullptr;
	a.ltc = p->d_ltc; a.rows = d_rows; a.st = st;
	StreamScratch scratch(st);
	hipError_t e = hipSuccess;
	if (want_max) e = scratch.alloc(&a.pviol, (size_t)batch * ntiles);
	if (e == hipSuccess && want_max) e = scratch.alloc(&a.pkey, (size_t)batch * ntiles);
	return time_tile_run(p, "check", e, batch, ntimes, d_times, times_stride, scratch_cap, a, [&] { return ntg_launch_check(D, p->T, a); },
	                     [&] { return want_max ? ntg_launch_check_final(batch, ntiles, ntimes, a.pviol, a.pkey, d_viol, d_where, st) : hipSuccess; });
}

extern "C" int ntg_batch_check(const ntg_plan *p, int batch, const double *d_x, const double *d_lower, const double *d_upper, int ntimes,
                               const double *d_times, long long times_stride, double *d_viol, int *d_where, double *d_rows, void *stream)
{
	return batch_check(p, batch, d_x, d_lower, d_upper, ntimes, d_times, times_stride, d_viol, d_where, d_rows, stream, NTG_TIME_SCRATCH_CAP);
}
// diagnostic: the same with the scratch cap of the per-problem time tables stated by the caller (tests force several chunks with it)
extern "C" int ntg_debug_batch_check(const ntg_plan *p, int batch, const double *d_x, const double *d_lower, const double *d_upper, int ntimes,
                                     const double *d_times, long long times_stride, double *d_viol, int *d_where, double *d_rows, void *stream,
                                     long long scratch_cap)
{
	return batch_check(p, batch, d_x, d_lower, d_upper, ntimes, d_times, times_stride, d_viol, d_where, d_rows, stream, scratch_cap);
}
