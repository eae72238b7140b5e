// plan_solve.cpp -- ntg_batch_solve and the receding-horizon calls around it (ntg_batch_mpc_shift, _shift_multipliers, _run), and the
// solve setup they share with the sizing calls: which kernel takes a solve, with what workgroup size and LDS layout, and where its
// buffers lie in the caller's workspace (solve_setup below: the one place that decides it, for sizing and for the launch alike).
#include <cfloat>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include "plan_priv.hpp"
#include "nwt_map.hpp"

extern "C" const char *ntg_solve_kernel_name(void) { return "sqp_kernel"; }
extern "C" const char *ntg_batch_solve_kernel(const ntg_plan *p, int batch, const ntg_solve_opts *o);
// diagnostic: LDS bytes and block size the solve / eval launches of this plan use
extern "C" int ntg_debug_layout(const ntg_plan *p, const ntg_solve_opts *o, int *lds_solve, int *lds_eval, int *nt_solve);

static int resolve_params(const ntg_plan *p, const ntg_solve_opts *o, SolveParams *sp, int *nt)
{
	const NtgDims &D = p->D;
	ntg_solve_opts def; ntg_default_opts(&def);
	if (!o) o = &def;
	sp->itlim = o->itlim > 0 ? o->itlim : std::max(50, 3 * (D.nC + D.nclin) + 10 * D.ncnln);
	sp->memcap = std::min(sp->itlim, o->qn_memory > 0 ? o->qn_memory : 256);
	sp->ls_maxfev = o->ls_maxfev > 0 ? o->ls_maxfev : 20;
	sp->hessian = o->hessian; sp->fixed_iters = o->fixed_iters; sp->warm = o->warm_start ? 1 : 0;
	// the structured Newton mode does not apply (or: per-problem grids -- its cost model and maps belong to the plan's grid): collocation
	// preconditioner.  Decided HERE, once: workspace size, layout and launch all see the same mode (a switch after the workspace was sized
	// for hessian = 2 -- no quasi-Newton history -- would let the quasi-Newton mode write its history past the end of the workspace).
	if (sp->hessian < 0 || sp->hessian > 3) sp->hessian = 0;
	// the QP-based SQP step (hessian = 3) rides on the structured Newton mode's band model: where that does not apply it does not either
	if (sp->hessian >= 2 && (!D.nwt_on || (p->grid_batch && !p->T.pp_k0))) sp->hessian = 1;
	sp->stamps = getenv("NTG_AMD_STAMPS") ? std::max(1, atoi(getenv("NTG_AMD_STAMPS"))) : 0;
	const double r = o->opttol > 0 ? o->opttol : std::pow(DBL_EPSILON, 0.8);
	sp->sr = std::sqrt(r);
	sp->steplimit = o->steplimit > 0 ? o->steplimit : 2.0;
	sp->ls_mu = o->ls_mu > 0 ? o->ls_mu : 1e-4; sp->ls_eta = o->ls_eta > 0 ? o->ls_eta : 0.9;
	int t = o->block_threads;
	if (t != 128 && t != 256 && t != 512) t = auto_threads(D);
	// the structured Newton mode runs one wavefront per coupling group: a workgroup too small for the plan's groups grows to hold them, and a
	// plan with more groups than the largest workgroup has waves takes the collocation preconditioner (decided here, once: workspace, layout
	// and launch all see the same mode)
	if (sp->hessian >= 2) {
		const int nwv = (D.nwt_tw ? 2 : 1) * D.nwt_ngrp + D.nwt_nfo;   // two waves per group with the two-sided factorisation
		while (t < 512 && nwv * 64 > t) t *= 2;
		if (nwv * 64 > t) sp->hessian = 1;
	}
	*nt = t;
	return 0;
}

// does the solve keep all its vectors in LDS, or only the two that are read across lanes (sqp_kernel, BIG)?
static int solve_layout(const NtgDims &D, int nt, SmemLayout *L, int *big, const SolveParams *sp = nullptr)
{
	// a short quasi-Newton memory keeps its pair scalars in LDS -- unless those bytes would cost a resident workgroup
	const int hrc = (sp && sp->hessian < 2 && sp->memcap < NTG_HRC_LDS) ? sp->memcap + 1 : 0;   // + 1: the one-vector-per-major form wants a slot more than pairs
	auto resident = [](int total) { return (160 * 1024) / std::max(total, 1); };
	*big = 0;
	const int qp = (sp && sp->hessian == 3) ? 1 : 0;   // the QP-based SQP step keeps its slots behind the Newton mode's solve vectors
	*L = ntg_make_layout(D, nt, 5, 1, hrc, qp);
	if (hrc && resident(L->total) < resident(L->total - 16 * hrc)) *L = ntg_make_layout(D, nt, 5, 1, 0, qp);
	if (L->total <= 160 * 1024) return 0;
	*big = 1;
	*L = ntg_make_layout(D, nt, 1, 0, hrc, qp);
	if (hrc && L->total > 160 * 1024) *L = ntg_make_layout(D, nt, 1, 0, 0, qp);
	return L->total <= 160 * 1024 ? 0 : -1;
}
static size_t hist_doubles(const NtgDims &D, int batch, const SolveParams &sp)
{
	if (sp.hessian >= 2) return 0;   // the structured Newton mode keeps no quasi-Newton pairs
	return (size_t)batch * sp.memcap * (2 * D.nC + 2);
}
static size_t al_doubles(const NtgDims &D, int batch) { return (size_t)batch * 2 * (D.ncnln + D.nI); }
// structured Newton mode / QP-based SQP step: the per-problem workspace of nwt_map.hpp
static size_t nwt_doubles(const NtgDims &D, int batch, const SolveParams &sp, int nt)
{
	if (sp.hessian < 2 || !D.nwt_on) return 0;
	return (size_t)batch * nwt_map(D, nt, sp.hessian == 3, D.nwt_cg).total;
}

// ---- The solve setup: everything the host decides about one solve of (plan, batch, options) ----
// Two questions are asked of it.
//   sizing  (ntg_batch_workspace_bytes, ntg_batch_solve_kernel): asked before the first hessian = 1 solve, so the preconditioner may not
//           exist yet.  While it does not, the kernel named is the one that runs if the preconditioner comes out in its block form
//           (assume_block = true).
//   launch  (ntg_batch_solve, ntg_batch_mpc_shift_multipliers): ntg_batch_solve asks after build_precond; a hessian = 1 solve whose
//           preconditioner is not there cannot go to the wave kernel (assume_block = false).
// Both see the same parameters (resolve_params), the singular downgrade (hessian 1 -> 0) as soon as the preconditioner is known to be
// singular, the same layout and the same workspace.  The workspace does not depend on the question: its size covers sqp_kernel's areas
// for the resolved mode and the wave kernel's HBM chain tier for BOTH wave instances (hessian 0 and 1; the block form assumed while the
// preconditioner is not built), so a downgrade after sizing never outgrows it.  Workspace, from its start:
//   [0, al_off)         quasi-Newton history of sqp_kernel, or the wave kernel's chain tier          (doubles)
//   [al_off, vec_off)   [batch][2][ncnln + nI] multipliers, estimates
//   [vec_off, nwt_off)  [batch][5][npad] x, gp, gp+, d, g (BIG only)
//   [nwt_off, ...)      structured Newton mode: bands and blocks
//   counter_off         (bytes) problem queue counter of the wave kernel, inside the 256 bytes that end the workspace
struct SolveSetup {
	SolveParams sp; int nt = 0;
	SmemLayout L; int big = 0; bool fits = false;   // fits: the layout stays within 160 KiB of LDS
	bool wave = false; NtgWavePlan wp;              // the wave kernel takes the solve, and its launch shape
	bool precond_seen = false;                      // the preconditioner existed when this was computed
	size_t al_off = 0, vec_off = 0, nwt_off = 0; long long counter_off = 0, bytes = 0;
};

// ntg_wave_plan for this plan; assume_block: as if the preconditioner were there in its block form (one dense block per output)
static bool wave_plan_for(const ntg_plan *p, const SolveParams &sp, int batch, bool assume_block, NtgWavePlan *w)
{
	if (!assume_block) return ntg_wave_plan(p->D, p->T, sp, batch, plan_ncu(p), w);
	static const double unbuilt = 0.0;   // stands for the blocks: the shape test looks at the pointer and the block size only
	NtgTables T2 = p->T; T2.n0b = &unbuilt; T2.n0b_n = p->D.ncoef[0];
	return ntg_wave_plan(p->D, T2, sp, batch, plan_ncu(p), w);
}

static SolveSetup solve_setup(const ntg_plan *p, int batch, const ntg_solve_opts *o, bool assume_block)
{
	const NtgDims &D = p->D;
	SolveSetup s;
	resolve_params(p, o, &s.sp, &s.nt);
	s.precond_seen = p->precond_ready;
	if (s.sp.hessian == 1 && p->precond_ready && p->precond_singular) s.sp.hessian = 0;
	s.fits = solve_layout(D, s.nt, &s.L, &s.big, &s.sp) == 0;
	// (hessian = 3 on a BIG layout with 256 threads: the fix -- raise nt to 512 and lay out again -- goes here)
	s.al_off = hist_doubles(D, batch, s.sp);
	s.vec_off = s.al_off + al_doubles(D, batch);
	s.nwt_off = s.vec_off + (s.big ? (size_t)batch * 5 * ((D.nC + 1) & ~1) : 0);
	size_t dbl = s.nwt_off + nwt_doubles(D, batch, s.sp, s.nt);
	// the wave kernel's HBM tier of the direction chains (per resident wave, not per problem); sized for both of its instances
	for (int h = 0; h < 2; h++) {
		SolveParams s2 = s.sp; s2.hessian = h;
		NtgWavePlan w;
		if (wave_plan_for(p, s2, batch, false, &w) || (h == 1 && !p->grid_batch && !p->precond_ready && wave_plan_for(p, s2, batch, true, &w)))
			dbl = std::max(dbl, w.hist_doubles);
	}
	s.bytes = (long long)(dbl * 8 + 256);
	s.counter_off = (s.bytes - 256) & ~(long long)7;
	// which solve kernel takes the batch: the wave kernel (one wavefront per problem) for the plans it covers, else sqp_kernel
	const bool unbuilt = s.sp.hessian == 1 && !p->precond_ready;   // the preconditioner's block form is part of the wave kernel's test
	s.wave = unbuilt ? (assume_block && wave_plan_for(p, s.sp, batch, true, &s.wp)) : wave_plan_for(p, s.sp, batch, false, &s.wp);
	return s;
}

// name of the kernel ntg_batch_solve will launch for (plan, batch, options): "sqp_wave_kernel" (one wavefront per problem) or "sqp_kernel"
extern "C" const char *ntg_batch_solve_kernel(const ntg_plan *p, int batch, const ntg_solve_opts *o)
{
	if (!p) return "";
	return solve_setup(p, batch, o, true).wave ? "sqp_wave_kernel" : "sqp_kernel";
}

extern "C" long long ntg_batch_workspace_bytes(const ntg_plan *p, int batch, const ntg_solve_opts *o)
{
	if (!p) return 0;
	return solve_setup(p, batch, o, true).bytes;
}

extern "C" int ntg_batch_solve(const ntg_plan *pc, int batch, const double *d_lower, const double *d_upper, double *d_x,
                               const ntg_solve_opts *o, double *d_objective, int *d_inform, int *d_iters, int *d_nfev,
                               double *d_clambda, void *d_work, long long work_bytes, void *stream)
{
	ntg_plan *p = const_cast<ntg_plan *>(pc);
	if (!p) return fail(NTG_E_BADARG, "null plan");
	if (batch <= 0) return 0;
	if (!d_x || !d_lower || !d_upper) return fail(NTG_E_BADARG, "null argument");
	if (p->D.family == NTG_FAM_HOST) return fail(NTG_E_UNSUPPORTED, "host-callback plans are solved by ntg()");
	if (p->grid_batch && batch != p->grid_batch) return fail(NTG_E_BADARG, "the plan carries per-problem grids for another batch size");
	if (int rc = check_params(p, batch)) return rc;
	if (!p->lin_ok) return fail(NTG_E_BADARG, "linear constraint rows are rank deficient");
	HIPCHK(hipSetDevice(p->device));
	SolveSetup s = solve_setup(p, batch, o, false);
	if (work_bytes < s.bytes || !d_work) return fail(NTG_E_BADARG, "workspace too small");
	if (p->grid_batch && s.sp.hessian == 1 && !p->T.pp_n0b) return fail(NTG_E_BADARG, "per-problem grids were set without the preconditioner (with_precond = 0): solve with hessian = 0");
	if (s.sp.hessian == 1) {   // built on first use, once: two threads or streams may first-solve the same plan
		std::lock_guard<std::mutex> lk(p->precond_mutex);
		if (!p->precond_ready) { int rc = build_precond(p); if (rc) return rc; }
		if (!s.precond_seen) s = solve_setup(p, batch, o, false);   // a plan's first hessian = 1 solve: asked again now that the preconditioner is known
	}
	if (!s.fits) return fail(NTG_E_UNSUPPORTED, "problem state exceeds 160 KiB of LDS");
	double *work = (double *)d_work;
	SqpArgs sa{s.nt, s.big, batch, d_lower, d_upper, d_x, d_objective, d_inform, d_iters, d_nfev, d_clambda, work, work + s.al_off,
	           s.big ? work + s.vec_off : nullptr, s.sp.hessian >= 2 ? work + s.nwt_off : nullptr, (hipStream_t)stream,
	           (unsigned int *)((char *)d_work + s.counter_off)};
	if (s.wave) HIPCHK(ntg_launch_sqp_wave(p->D, p->T, s.sp, sa, s.wp));   // one wavefront per problem
	else HIPCHK(ntg_launch_sqp(p->D, p->T, s.L, s.sp, sa));
	return 0;
}

// The multipliers' share of the receding-horizon step (see ntg_amd.h): the estimates of the trajectory rows in the workspace move shift_bp
// breakpoints towards the start of the horizon.
extern "C" int ntg_batch_mpc_shift_multipliers(const ntg_plan *p, int batch, int shift_bp, const ntg_solve_opts *o, void *d_work, long long work_bytes,
                                               void *stream)
{
	if (!p) return fail(NTG_E_BADARG, "null plan");
	if (batch <= 0) return 0;
	const NtgDims &D = p->D;
	if (D.ncnln + D.nI == 0 || D.nnltc == 0 || shift_bp == 0) return 0;
	if (shift_bp < 0 || shift_bp >= D.P) return fail(NTG_E_BADARG, "shift out of range");
	const SolveSetup s = solve_setup(p, batch, o, false);
	if (!d_work || work_bytes < s.bytes) return fail(NTG_E_BADARG, "workspace too small");
	HIPCHK(hipSetDevice(p->device));
	HIPCHK(ntg_launch_mpc_shift_lambda(D, batch, shift_bp, (double *)d_work + s.al_off, (hipStream_t)stream));   // the multipliers' area, as ntg_batch_solve lays it out
	return 0;
}

// A receding-horizon run: nsteps times (solve, shift).  The first step runs directly (it may build the preconditioner);
// the (solve, count, shift) sequence of the remaining steps is captured once into a hipGraph and replayed, so that a
// step costs one graph launch instead of three kernel launches from the host loop.
extern "C" int ntg_batch_mpc_run(const ntg_plan *p, int batch, int nsteps, int shift_bp, int shift_knots, double *d_x,
                                 double *d_lower, double *d_upper, const ntg_solve_opts *o, int *d_inform, int *d_notconv,
                                 void *d_work, long long work_bytes, void *stream)
{
	if (!p) return fail(NTG_E_BADARG, "null plan");
	if (batch <= 0 || nsteps <= 0) return 0;
	if (!d_x || !d_lower || !d_upper || !d_inform) return fail(NTG_E_BADARG, "null argument");
	if (shift_bp < 0 || shift_bp >= p->D.P || shift_knots < 0) return fail(NTG_E_BADARG, "shift out of range");
	if (p->grid_batch && batch != p->grid_batch) return fail(NTG_E_BADARG, "the plan carries per-problem grids for another batch size");
	if (int rc = check_params(p, batch)) return rc;
	HIPCHK(hipSetDevice(p->device));
	hipStream_t st = (hipStream_t)stream, own = nullptr;
	if (!st) { HIPCHK(hipStreamCreateWithFlags(&own, hipStreamNonBlocking)); st = own; }   // the legacy default stream cannot be captured
	// The FIRST solve is cold whatever the caller's options say: a warm start reads the multiplier estimates of the previous solve from
	// d_work (sqp_kernel.hpp: `if (sp.warm) al_lam[j] = al_t[j]`), and before the first solve the workspace holds nothing of the kind.
	// The estimates it leaves are shifted with the horizon, so the captured / replayed steps start warm as asked.
	ntg_solve_opts cold;
	if (o) { cold = *o; cold.warm_start = 0; }
	auto step = [&](const ntg_solve_opts *so) -> int {
		int rc = ntg_batch_solve(p, batch, d_lower, d_upper, d_x, so, nullptr, d_inform, nullptr, nullptr, nullptr, d_work, work_bytes, st);
		if (rc) return rc;
		if (d_notconv) { hipError_t e = ntg_launch_count_notconv(batch, d_inform, d_notconv, st); if (e != hipSuccess) return fail(NTG_E_HIP, hipGetErrorString(e)); }
		rc = ntg_batch_mpc_shift(p, batch, shift_bp, shift_knots, d_x, d_lower, d_upper, st);
		if (rc) return rc;
		if (o && o->warm_start) rc = ntg_batch_mpc_shift_multipliers(p, batch, shift_bp, o, d_work, work_bytes, st);   // the multipliers travel with the horizon
		return rc;
	};
	int rc = 0;
	if (own) rc = hipDeviceSynchronize() == hipSuccess ? 0 : NTG_E_HIP;   // order after work queued on the default stream
	if (!rc) rc = step(o ? &cold : nullptr);
	if (!rc && nsteps > 1) {
		hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr;
		hipError_t e = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal);
		if (e == hipSuccess) {
			rc = step(o);
			hipError_t e2 = hipStreamEndCapture(st, &graph);
			if (!rc && e2 != hipSuccess) rc = fail(NTG_E_HIP, hipGetErrorString(e2));
			if (!rc && hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) != hipSuccess) rc = fail(NTG_E_HIP, "hipGraphInstantiate failed");
			for (int s = 1; !rc && s < nsteps; s++) if (hipGraphLaunch(exec, st) != hipSuccess) rc = fail(NTG_E_HIP, "hipGraphLaunch failed");
			if (exec) (void)hipGraphExecDestroy(exec);
			if (graph) (void)hipGraphDestroy(graph);
		} else {
			for (int s = 1; !rc && s < nsteps; s++) rc = step(o);   // capture unavailable: plain launches
		}
	}
	if (own) { if (hipStreamSynchronize(own) != hipSuccess && !rc) rc = NTG_E_HIP; (void)hipStreamDestroy(own); }
	return rc;
}

extern "C" int ntg_batch_mpc_shift(const ntg_plan *p, int batch, int shift_bp, int shift_knots, double *d_x,
                                   double *d_lower, double *d_upper, void *stream)
{
	if (!p) return fail(NTG_E_BADARG, "null plan");
	if (batch <= 0) return 0;
	if (!d_x || !d_lower || !d_upper) return fail(NTG_E_BADARG, "null argument");
	if (shift_bp < 0 || shift_bp >= p->D.P || shift_knots < 0) return fail(NTG_E_BADARG, "shift out of range");
	// the shift re-pins the initial bounds with the basis blocks of the grid in force (T.blk: the plan's, or every problem's own after
	// ntg_plan_set_grids, which keeps them for this)
	if (p->grid_batch && batch != p->grid_batch) return fail(NTG_E_BADARG, "the plan carries per-problem grids for another batch size");
	HIPCHK(hipSetDevice(p->device));
	HIPCHK(ntg_launch_mpc_shift(p->D, p->T, batch, shift_bp, shift_knots, p->d_lic, d_x, d_lower, d_upper, (hipStream_t)stream));
	return 0;
}

extern "C" int ntg_debug_layout(const ntg_plan *p, const ntg_solve_opts *o, int *lds_solve, int *lds_eval, int *nt_solve)
{
	if (!p) return NTG_E_BADARG;
	const SolveSetup s = solve_setup(p, 1, o, true);
	const SmemLayout &L = s.L;
	const int big = s.big;
	if (getenv("NTG_AMD_DEBUG"))
		fprintf(stderr, "solve layout (big %d): rowv %d colp %d chrow %d off %d bps %d wts %d x %d dfz %d fvals %d red %d dfi %d vecs %d lam %d rho %d oinfo %d ls %d tI %d q_idx %d q_col %d q_val %d csr_ptr %d sinv_val %d total %d | row_total %d col_total %d ntav %d q_nt %d q_w %d lin_nnz %d sinv_nnz %d lin_lds %d\n",
		        big, L.rowv, L.colp, L.chrow, L.off, L.bps, L.wts, L.x, L.dfz, L.fvals, L.red, L.dfi, L.vecs, L.lam, L.rho, L.oinfo, L.ls, L.tI, L.q_idx, L.q_col, L.q_val, L.csr_ptr, L.sinv_val, L.total,
		        p->D.row_total, p->D.col_total, p->D.ntav, p->D.q_nt, p->D.q_w, p->D.lin_nnz, p->D.sinv_nnz, p->D.lin_lds);
	if (lds_solve) *lds_solve = big ? -L.total : L.total;   // negative: only the cross-lane vectors are in LDS
	if (lds_eval) *lds_eval = ntg_make_layout(p->D, auto_threads(p->D), 0, 1).total;
	if (nt_solve) *nt_solve = s.nt;
	return 0;
}
