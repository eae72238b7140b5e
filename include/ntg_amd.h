/*
 * include/ntg_amd.h -- C ABI of the MI355X-native batched NTG engine (libntg_amd.so).
 *
 * Plain pointers and sizes only.  Pointers named d_* are DEVICE pointers (HBM of the GPU the
 * plan was created on); everything else is host memory.  `stream` is a hipStream_t passed as
 * void* (NULL = default stream).  All entry points return 0 on success, a negative NTG_E_*
 * code otherwise; ntg_last_error() returns a message.  Nothing here falls back to the CPU:
 * without a usable gfx950 device every call fails with NTG_E_NODEVICE.
 *
 * Which reference interface each entry point replaces (files under /root/reference/src):
 *   ntg_plan_create      ntg.c:114-229   ConcatCollocMatrix + LinearConstraintsMatrix + the
 *                                        argument stash into file-scope globals (ntg.c:119-152)
 *                        colloc.c:57-117 CollocMatrix: knots_/interv_/bsplvd_ at every breakpoint
 *   ntg_plan_tables      colloc.h:42-71  read-back of Block.matrix / Block.offset / A
 *   ntg_basis_batch      colloc.c:92-111 the same basis evaluation for many grids at once
 *   ntg_plan_set_grids   ntg.c:114-229 per problem: own knots and breakpoints for every problem of a batch
 *   ntg_plan_grid_tables the read-back of ntg_plan_tables for one problem's grid
 *   ntg_plan_set_params  the file-scope parameter globals of the examples (kincar.c:43 default_params), one row per problem
 *   ntg_batch_eval       ntg.c:274-371   NPfunobj + NPfuncon (cost.c, constraints.c, integrator.c)
 *   ntg_batch_bounds     constraints.c:5-33 bounds()
 *   ntg_batch_solve      ntg.c:237-253   the npsol_() call, for `batch` problems at once
 *   npsolCostFunction / npsolConstraintFunction
 *                        ntg.c:274-280 / ntg.c:337-346  (static NPfunobj / NPfuncon; exported
 *                        under the names BASELINE.json uses, same Fortran-style signature)
 *   ntg_batch_interp     colloc.c:449-484 SplineInterp, for a batch
 *   ntg_batch_check      SplineInterp + the trajectory rows of NPfuncon (constraints.c:119-160) at arbitrary times + bounds, fused
 *   ntg_batch_cost       SplineInterp + the integrand of IntegratedCost (cost.c with integrator.c, reached through NPfunobj, ntg.c:274-280) at
 *                        arbitrary nodes under the caller's quadrature weights, fused; the reference integrates by the trapezoid rule on the breakpoints only
 *   ntg_batch_verify     NPSOL's derivative verification behind npsol_() (ntg.c:249-253: "derivative level = 3" is declared and the verification
 *                        left on), for a batch: the family's analytic derivatives against central differences, plus the active-variable lists
 *   ntg_batch_refine     nothing in the reference carries a spline to other knots; the nearest is SplineInterp (colloc.c:449-484), which the
 *                        result reproduces: the refined coefficients describe the same function
 *   ntg_batch_envelope   nothing in the reference bounds a trajectory between samples; its only dense output is SplineInterp (colloc.c:449-484),
 *                        point by point, which the result encloses: bounds of every flag entry and linear trajectory row over whole pieces of time
 *   ntg_batch_envelope_sos  nothing in the reference bounds a row between samples; constraints.c:119-160 evaluates the trajectory rows at the
 *                        breakpoints only: bounds of the sum-of-squares rows (obstacle clearance, thrust^2, speed^2) over whole pieces of time
 *   ntg_batch_extrema    nothing in the reference looks for a row's extremum between samples; constraints.c:119-160 evaluates the trajectory rows
 *                        at the breakpoints only: the minimum and maximum of every certifiable row over the horizon, enclosed to a tolerance, with their times
 *   ntg_batch_separation nothing in the reference compares two trajectories; its only dense output is SplineInterp (colloc.c:449-484), point by
 *                        point: the closest approach of pairs of planned bodies over the horizon, enclosed to a tolerance, with its time
 *   ntg_batch_forms      nothing in the reference bounds a function of the flag between samples: the minimum and maximum over the horizon of quadratic
 *                        forms of the flag declared at the call (speed^2, the turning numerator, weighted thrust, ellipses, rows of a module)
 *   ntg_batch_ratios     nothing in the reference bounds the steering angle between samples; examples/kincar.c:68-92 kincar_flat_reverse computes it
 *                        per sample: the minimum and maximum over the horizon of ratios of products of such forms (curvature^2, lateral acceleration^2)
 *   ntg_batch_trig       nothing in the reference bounds a row between samples; constraints.c:119-160 evaluates the manipulator's rows at the
 *                        breakpoints only: the minimum and maximum over the horizon of sums of sines and cosines of the flag (a tip's height and reach)
 *   ntg_batch_minmax     nothing in the reference bounds a row between samples; constraints.c:119-160 evaluates the trajectory rows at the
 *                        breakpoints only: the minimum and maximum over the horizon of min / max expressions over such forms (polygons, boxes, corridors)
 *   ntg_batch_kincar_reverse  examples/kincar.c:68-92 kincar_flat_reverse (the example's flat-to-state map), for a batch
 *   ntg(), npsoloption(), linspace(), SplineInterp(), matrix helpers: see include/ntg.h
 */
#ifndef NTG_AMD_H
#define NTG_AMD_H

#ifdef __cplusplus
extern "C" {
#endif

#define NTG_MAX_OUT 16     /* outputs per problem */
#define NTG_MAX_ORDER 10   /* spline order k */
#define NTG_MAX_NZ 64      /* sum of maxderiv (active-variable masks are 64-bit) */

#define NTG_E_NODEVICE (-1)
#define NTG_E_BADARG   (-2)
#define NTG_E_HIP      (-3)
#define NTG_E_UNSUPPORTED (-4)

#define NTG_INF_BOUND 1e20   /* NPSOL's "infinite bound": use for one-sided constraints */

/* problem families = device functors for the user callbacks of ntg.h:81-83,90-92 */
#define NTG_FAM_KINCAR 0     /* examples/kincar.c:105-117 generalised to nout outputs */
#define NTG_FAM_VANDERPOL 1  /* examples/vanderpol.c:206-241 */
#define NTG_FAM_TESTFAM 2    /* synthetic, all six callback slots */
#define NTG_FAM_OBSTACLE 3   /* kincar cost + circular-obstacle trajectory constraint (x-20)^2+(y-0.5)^2 >= r^2 */
#define NTG_FAM_QUADROTOR 4  /* 4 outputs x,y,z,yaw, maxderiv 5: snap^2 + yaw''^2; rows: thrust^2 = x''^2+y''^2+(z''+g)^2, speed^2 */
#define NTG_FAM_MANIP 5      /* 3 joints per planar arm, maxderiv 3: sum q''^2; one tip-height row sin(qa)+sin(qa+qb)+sin(qa+qb+qc) per arm */
#define NTG_FAM_OBSTACLE_FIELD 6  /* kincar cost (2 outputs) + m = nnltc <= 8 rows (x-cx_j)^2+(y-cy_j)^2 >= r_j^2: the centres are per-problem
                                     parameters [cx_0, cy_0, ..., cx_{m-1}, cy_{m-1}] (ntg_plan_set_params), the radii come through the bounds */
#define NTG_FAM_HOST (-1)    /* host function pointers (ntg() drop-in path only) */
#define NTG_FAM_MODULE_BASE 64  /* ids of families loaded from modules (ntg_family_load) start here */

typedef struct { int output; int deriv; } ntg_av; /* == AV of av.h:22-26 */

/* Everything ntg() takes that is common to a batch (ntg.h:72-99). lic/ltc/lfc are row-major
 * [n][nz] with nz = sum(maxderiv) (the examples' DoubleMatrix layout). */
typedef struct {
	int nout, nbps;
	const double *bps;
	const int *kninterv;
	const double *const *knots;
	const int *order, *mult, *maxderiv;
	int family;
	int nlic, nltc, nlfc;
	const double *lic, *ltc, *lfc;
	int nnlic, nnltc, nnlfc;
	int nicav, ntcav, nfcav;
	const ntg_av *icav, *tcav, *fcav;
	int nicf, nucf, nfcf;
	int nicostav, ntcostav, nfcostav;
	const ntg_av *icostav, *tcostav, *fcostav;
	/* optional, may be NULL: [nlic+nltc+nlfc] flags, non-zero = this linear row is an INEQUALITY row (lower <= row <= upper)
	 * for every problem of the batch.  Rows not flagged must have lower == upper in every problem (they are kept satisfied
	 * by projection); a problem that breaks this returns inform 9.  ntg() itself needs no flags: it reads the bounds. */
	const int *lin_ineq;
} ntg_spec;

typedef struct {
	int itlim;          /* major iteration limit; <=0: max(50, 3(n+nclin)+10 ncnln) (NPSOL default) */
	double opttol;      /* optimality tolerance r; <=0: eps^0.8 */
	double steplimit;   /* NPSOL "step limit", 2.0 */
	double ls_mu, ls_eta; /* 1e-4, 0.9 (NPSOL "line search tolerance") */
	int ls_maxfev;      /* 20 */
	int hessian;        /* 0 identity cold start (NPSOL), 1 collocation preconditioner (ignored when the cost model is
	                     * singular on the null space of the equality rows, e.g. a plan without equality rows),
	                     * 2 structured Newton step for nonlinear trajectory rows: band model of the augmented Lagrangian's Hessian,
	                     *   assembled and factored on the matrix cores at every major (families with second-order blocks: obstacle,
	                     *   quadrotor, manipulator; acts as 1 where it does not apply, e.g. more coupling groups than a
	                     *   workgroup has wavefronts) -- the robust mode for BASELINE's configs D and E,
	                     * 3 QP-based SQP step on the same band model: per major iteration the inequality QP on the linearised rows (what NPSOL does with the
	                     *   Jacobian ntg() hands it, ntg.c:217-220,250-253), solved through its dual by an active-set method on at most 16 (32: single-group plans
	                     *   on large workgroups) rows per coupling group, l1 merit function; a problem whose working set does not fit continues in mode 2 by itself.  Config E:
	                     *   17 majors instead of 60, 2.9 x mode 2's rate.  With warm_start the QP's first working set is the rows the carried-over
	                     *   multipliers name (no pass on the objective alone).  Acts as 1 where the band model does not apply. */
	int fixed_iters;    /* 1: exactly itlim majors, no convergence exit */
	int block_threads;  /* 0 = auto (128/256/512) */
	int qn_memory;      /* quasi-Newton updates kept before the approximation restarts from W0; <= 0: 256 */
	int warm_start;     /* plans with nonlinear / inequality rows: 1 = start the augmented-Lagrangian loop from the multiplier estimates the
	                     * previous ntg_batch_solve of the same batch left in d_work (the use NPSOL's clambda was meant for, ntg.h:64-68:
	                     * receding-horizon re-solves; ntg_batch_mpc_run shifts them with the horizon), 0 = multipliers start at 0.
	                     * The structured Newton mode then skips its pass on the objective alone. */
} ntg_solve_opts;

typedef struct ntg_plan ntg_plan;

int ntg_device_count(void);
const char *ntg_last_error(void);
void ntg_default_opts(ntg_solve_opts *o);

/* User problem families (include/ntg_amd_family.hpp, INTEGRATION.md "Your own problem family"): load a module built from that
 * header and get its family id (>= NTG_FAM_MODULE_BASE) for ntg_spec.family.  No HIP call: works without a device.  The same
 * file loaded again returns the same id; modules stay loaded for the life of the process.  NTG_E_BADARG (with the reason in
 * ntg_last_error) for a missing file, a shared object without the module entry point, or a module built against other
 * headers than this library (ABI stamp or structure sizes differ). */
int ntg_family_load(const char *path, int *family);
/* what a loaded module declares: name (NUL-terminated, truncated to name_len), maxderiv of every output, the most nonlinear
 * rows of each kind a plan may use, the outputs a plan must have (0 = any).  Any output pointer may be NULL. */
int ntg_family_info(int family, char *name, int name_len, int *maxderiv, int *nnlic, int *nnltc, int *nnlfc, int *nout);

/* Build the device-resident, batch-shared part of a problem: basis blocks and offsets (HIP
 * basis kernel), banded linear-constraint rows A, (A A')^-1, optional preconditioner. */
int ntg_plan_create(const ntg_spec *spec, int device, ntg_plan **out);
void ntg_plan_destroy(ntg_plan *p);

/* sizes: nC, nz, nclin, ncnln, nbounds, sumk, njrows (banded Jacobian rows), nblk (doubles in blk) */
int ntg_plan_dims(const ntg_plan *p, int *nC, int *nz, int *nclin, int *ncnln, int *nbounds,
                  int *sumk, int *nblk);
/* read the setup tables back to the host (any pointer may be NULL):
 *   blk  outputs concatenated, per output [bp][q][r]         (reference block[bp].matrix->elements[q][r])
 *   off  [nout][nbps]                                         (reference block[bp].offset)
 *   A    dense column-major nclin x nC, ld = nclin            (what ntg.c:206 hands to NPSOL) */
int ntg_plan_tables(const ntg_plan *p, double *blk, int *off, double *A);
/* workspace (bytes) ntg_batch_solve needs for `batch` problems with these options */
long long ntg_batch_workspace_bytes(const ntg_plan *p, int batch, const ntg_solve_opts *o);

/* bounds(): d_lower/d_upper [batch][nbounds] -> d_bl/d_bu [batch][nC+nclin+ncnln] */
int ntg_batch_bounds(const ntg_plan *p, int batch, const double *d_lower, const double *d_upper,
                     double *d_bl, double *d_bu, void *stream);

/* funobj+funcon for `batch` coefficient vectors d_x [batch][nC], mode as in NPSOL (0 values,
 * 1 gradients, 2 both).  Outputs (any may be NULL): d_f [batch], d_g [batch][nC],
 * d_c [batch][ncnln] (rows: initial; trajectory constraint-major x breakpoint; final),
 * d_jband [batch][ncnln][sumk] banded Jacobian rows (for output o the entries
 * koff[o]..koff[o]+k_o-1 sit in columns iC[o]+off[o][bp(row)]+q),
 * d_cjac [batch][nC][ncnln] = dense column-major (ld = ncnln) Jacobian as NPSOL sees it. */
int ntg_batch_eval(const ntg_plan *p, int batch, const double *d_x, int mode,
                   double *d_f, double *d_g, double *d_c, double *d_jband, double *d_cjac,
                   void *stream);

/* Solve `batch` problems: d_x [batch][nC] in/out (initial guess -> solution, ntg.c:109),
 * d_lower/d_upper [batch][nbounds].  Outputs (may be NULL): d_objective, d_inform, d_iters,
 * d_nfev [batch]; d_clambda [batch][nC+nclin+ncnln].  d_work: ntg_batch_workspace_bytes(). */
int ntg_batch_solve(const ntg_plan *p, int batch, const double *d_lower, const double *d_upper,
                    double *d_x, const ntg_solve_opts *o,
                    double *d_objective, int *d_inform, int *d_iters, int *d_nfev,
                    double *d_clambda, void *d_work, long long work_bytes, void *stream);
/* name of the solve kernel, for bench/roofline bookkeeping: the general one, and the one ntg_batch_solve launches for (plan, batch,
 * options) -- "sqp_wave_kernel" (one wavefront per problem: the kincar class of BASELINE's configs B, C, M) or "sqp_kernel" */
const char *ntg_solve_kernel_name(void);
const char *ntg_batch_solve_kernel(const ntg_plan *p, int batch, const ntg_solve_opts *o);

/* bsplvd at every collocation point for `ngrids` different grids of one spline spec
 * (per-problem horizons): d_knots [ngrids][ninterv+1], d_bps [ngrids][nbps] ->
 * d_blk [ngrids][nbps][order][maxderiv], d_off [ngrids][nbps]. */
int ntg_basis_batch(int ngrids, int ninterv, int order, int mult, int maxderiv, int nbps,
                    const double *d_knots, const double *d_bps, double *d_blk, int *d_off,
                    void *stream);

/* Per-problem grids (free final time / per-problem horizons): every problem of a batch gets its own break sequence and breakpoints --
 * the setup phase of ntg() (ntg.c:114-229: CollocMatrix per output, colloc.c:57-117; LinearConstraintsMatrix, constraints.c:198-261)
 * run per problem, as the reference runs it per call.  d_knots [batch][ninterv+1], d_bps [batch][nbps] (device).  The combinatorial
 * structure must be the plan's: one basis class, and every breakpoint in the same knot interval as in the plan's grid (checked;
 * NTG_E_BADARG otherwise) -- the index tables stay shared, the VALUES (basis blocks, trapezoid weights, linear-constraint rows,
 * (A A')^-1, projector, with_precond != 0: the preconditioner blocks) become per problem.  Nonlinear rows are allowed (free final time
 * with obstacle / thrust / speed rows: their evaluation and the augmented-Lagrangian solve read the same per-problem tables), and so are
 * linear rows declared as inequalities (ntg_spec.lin_ineq: a corridor ceiling, an end-state window; also when every linear row is one):
 * their values on the plan's sparsity pattern are computed for every grid.  A grid that puts weight (above 1e-10 x the row's largest
 * entry) where the plan's pattern of a linear row, equality or inequality, has an exact zero is refused with NTG_E_UNSUPPORTED; the
 * message names the problem and the row.  Plans with inequality rows are solved by the general kernel (sqp_kernel), hessian = 2 / 3
 * acting as 1, on per-problem grids as on the plan's own.
 * Afterwards ntg_batch_eval / ntg_batch_solve / ntg_batch_interp of exactly `batch` problems use these grids (hessian = 2 / 3 included: the band model's cost part is built per grid;
 * ntg_batch_interp then takes d_times as [batch][ntimes]: every problem at its own times; ntg_batch_mpc_shift and ntg_batch_mpc_run
 * re-pin with every problem's own basis blocks) until ntg_plan_clear_grids(). */
int ntg_plan_set_grids(ntg_plan *p, int batch, const double *d_knots, const double *d_bps, int with_precond, void *stream);
void ntg_plan_clear_grids(ntg_plan *p);
/* ntg_plan_tables for one problem of the per-problem grids in force: blk that problem's basis blocks, off the plan's (the grids share
 * it), A dense column-major nclin x nC with every linear row, equality and inequality, in the plan's row order -- the values the solver
 * reads for that problem.  Synchronous.  NTG_E_BADARG without per-problem grids or with problem outside [0, batch). */
int ntg_plan_grid_tables(const ntg_plan *p, int problem, double *blk, int *off, double *A);

/* Per-problem family parameters: the data a family's callbacks read besides the flat flag (obstacle centres, a reference to track),
 * one row of doubles per problem -- what the reference's examples keep in file-scope globals (kincar.c:43) while ntg() solves one
 * problem at a time.
 * ntg_plan_param_count: the doubles every problem needs for this plan's family (0 for the families without parameters; 2 nnltc for
 * NTG_FAM_OBSTACLE_FIELD; NPARAM + NPARAM_BP * nbps for a family module, include/ntg_amd_family.hpp).
 * ntg_plan_set_params: d_params [batch][nparam] (device) is copied, ordered on `stream`, into a buffer the plan owns (the caller's
 * pointer is not kept; setting them again with the same batch * nparam reuses the buffer at the same address).  NTG_E_BADARG if nparam
 * is not ntg_plan_param_count or the family takes none; NTG_E_UNSUPPORTED for host-callback plans.
 * Afterwards ntg_batch_eval / ntg_batch_solve / ntg_batch_mpc_run of exactly `batch` problems read problem b's row (NTG_E_BADARG for
 * any other batch); ntg_batch_mpc_run reads the buffer at every step, so new parameters set between two runs take effect.
 * ntg_batch_mpc_shift / ntg_batch_bounds / ntg_batch_interp call no family callback and ignore them.  A family that needs parameters
 * refuses eval / solve / mpc_run (NTG_E_BADARG) while none are set.  Independent of per-problem grids: both can be in force.
 * ntg_plan_clear_params drops them. */
int ntg_plan_param_count(const ntg_plan *p, int *nparam);
int ntg_plan_set_params(ntg_plan *p, int batch, int nparam, const double *d_params, void *stream);
void ntg_plan_clear_params(ntg_plan *p);

/* SplineInterp (colloc.c:449-484) for a whole batch: the flat flag of every problem at ntimes points in time shared by
 * the batch (d_times [ntimes], inside the knot range of every output) -> d_z [batch][ntimes][nz], entry iz[o]+r =
 * D^r z_o(t).  This is the input of a flat-to-state map such as kincar_flat_reverse (kincar.c:68-92).  The call is stream ordered: it
 * never waits for the stream and reads no host memory after it returns, so it may sit in a captured stream.  Scratch (the basis at the
 * times) is stream ordered, released on every path and does not grow with batch * ntimes * nz (per-problem grids: the batch goes through
 * in chunks). */
int ntg_batch_interp(const ntg_plan *p, int batch, const double *d_x, int ntimes, const double *d_times, double *d_z,
                     void *stream);
/* The same with the layout of d_times stated by the caller instead of implied by the plan's state: problem b reads its ntimes points at
 * d_times + b * times_stride.  times_stride = 0: one time vector shared by the batch (allowed with and without per-problem grids);
 * times_stride >= ntimes: per-problem times, only with per-problem grids (NTG_E_BADARG otherwise).  ntg_batch_interp() is this call with
 * times_stride = 0 on the plan's grid and = ntimes after ntg_plan_set_grids(). */
int ntg_batch_interp_strided(const ntg_plan *p, int batch, const double *d_x, int ntimes, const double *d_times,
                             long long times_stride, double *d_z, void *stream);

/* Check solved trajectories BETWEEN the breakpoints.  The solvers enforce the trajectory rows at the collocation breakpoints only; this
 * call evaluates them at any times, fused on the device: for every problem b and every time t of its time vector the flat flag z(t) of
 * d_x[b] (SplineInterp's arithmetic, colloc.c:476-481), the nltc linear trajectory rows ltc . z, the nnltc nonlinear trajectory rows
 * (the family's row functions, with the problem's parameter row), each compared with that row function's bounds in d_lower / d_upper
 * ([batch][nbounds], the order lic, ltc, lfc, nlic, nltc, nlfc of ntg_batch_bounds; a bound with |.| >= NTG_INF_BOUND is absent).  The
 * violation of a row at a time is max(l - c, c - u, 0).  No flag is written to memory.
 * Outputs (any may be NULL, not all three):
 *   d_viol  [batch]     the largest violation over all rows and times, 0 if there is none
 *   d_where [batch][2]  {row, time index} of that maximum: row in [0, nltc + nnltc), linear rows first; on equal violations the smallest
 *                       row * ntimes + time index; {-1, -1} where d_viol is 0
 *   d_rows  [batch][nltc + nnltc][ntimes]  every row value
 * d_times / times_stride as for ntg_batch_interp_strided: 0 = one [ntimes] vector for the batch (with or without per-problem grids),
 * >= ntimes = per-problem times (only with per-problem grids; the basis then comes from that problem's knots).  Times must lie inside
 * the knot range.  The breakpoint index a family callback receives is that of the last breakpoint (the plan's, or the problem's own) at
 * or before t; the built-in families ignore it.  Results are bit-identical from call to call and do not depend on the batch around a
 * problem.  Scratch is stream ordered and does not grow with batch * ntimes * nz (per-problem grids: the batch goes through in chunks).
 * NTG_E_UNSUPPORTED for host-callback plans, for module families with per-breakpoint parameters (NPARAM_BP > 0: their data exists
 * at breakpoints only), for a plan whose basis tables of one tile of 128 times exceed the LDS (sum over basis classes of order x
 * maxderiv above about 150) and for a plan shape the family has no check instance for (none among the plans ntg_plan_create accepts); NTG_E_BADARG for a plan without trajectory rows, parameters not set, a batch other than the grids' or the
 * parameters', a bad times_stride.  batch <= 0 or ntimes <= 0 returns 0. */
int ntg_batch_check(const ntg_plan *p, int batch, const double *d_x, const double *d_lower, const double *d_upper,
                    int ntimes, const double *d_times, long long times_stride,
                    double *d_viol, int *d_where, double *d_rows, void *stream);

/* Audit the running cost BETWEEN the breakpoints.  The solvers minimise the trapezoid sum of the running cost on the collocation
 * breakpoints (IntegratedCost, cost.c with integrator.c); this call evaluates the same integrand at any times and sums it under any
 * quadrature, fused on the device: for every problem b and every time t_i of its time vector the flat flag z(t_i) of d_x[b] (SplineInterp's
 * arithmetic, colloc.c:476-481, exactly as ntg_batch_check computes it) and the family's running cost L_i = ucf(z(t_i)), with the problem's
 * parameter row.  No flag and no gradient is written to memory.
 * Outputs (either may be NULL, not both):
 *   d_cost [batch]          sum_i w_i L_i
 *   d_vals [batch][ntimes]  the unweighted L_i; d_vals[b][i] does not depend on ntimes or on the other times
 * The initial and final cost functions are NOT part of the result: f of ntg_batch_eval minus d_cost at the plan's own trapezoid nodes and
 * weights is what they contribute.
 * d_times and d_weights share one layout, stated by times_stride as for ntg_batch_check: 0 = one [ntimes] vector pair for the batch (with
 * or without per-problem grids), >= ntimes = per-problem vectors (only with per-problem grids; the basis then comes from that problem's
 * knots).  d_weights may be NULL only if d_cost is NULL.  Times must lie inside the knot range.  The breakpoint index the callback
 * receives is that of the last breakpoint (the plan's, or the problem's own) at or before t_i; the built-in families ignore it.
 * The sum has a fixed order: within a tile of 128 times the lanes' terms w_i L_i, a fixed butterfly over the 64 lanes of a wave, the waves
 * in index order; then the tiles of a problem in tile order.  No floating-point atomics: results are bit-identical from call to call and
 * do not depend on the batch around a problem.  Scratch is stream ordered, released on every path and does not grow with batch * ntimes
 * * nz (per-problem grids: the batch goes through in chunks).
 * NTG_E_UNSUPPORTED for host-callback plans, for module families with per-breakpoint parameters (NPARAM_BP > 0: their data exists at
 * breakpoints only) and for a plan whose basis tables of one tile of 128 times exceed the LDS (ntg_batch_check's limit); NTG_E_BADARG for
 * a plan without a running cost (nucf == 0), null d_x or d_times, both outputs null, d_cost without d_weights, parameters not set, a batch
 * other than the grids' or the parameters', a bad times_stride.  batch <= 0 or ntimes <= 0 returns 0. */
int ntg_batch_cost(const ntg_plan *p, int batch, const double *d_x,
                   int ntimes, const double *d_times, const double *d_weights, long long times_stride,
                   double *d_cost, double *d_vals, void *stream);

/* Audit the PROBLEM DEFINITION before anybody solves: the analytic derivatives the plan's family returns against central differences, and
 * the plan's active-variable lists against what the callbacks depend on.  Every solver mode trusts both; the reference gets the first check
 * from NPSOL's derivative verification (ntg.c:249-253).  d_x [batch][nC]: any coefficients -- a random point, a guess, a solution.
 * For every problem the full flat flag z, all nz entries, is built by SplineInterp's arithmetic (colloc.c:476-481) on the plan's basis, or
 * after ntg_plan_set_grids on that problem's own.  The six callback slots, in this order everywhere below: icf, ucf, fcf, nlicf, nltcf,
 * nlfcf (NTG_VERIFY_NSLOT).  Initial slots (icf, nlicf) are audited at breakpoint 0, trajectory slots (ucf, nltcf) at every breakpoint,
 * final slots (fcf, nlfcf) at the last breakpoint; a slot the plan does not use (nicf == 0, nnltc == 0, ...) is not called at all.  The
 * callback receives the breakpoint index and the problem's parameter row exactly as in ntg_batch_eval (parameters per problem, per row
 * function and per breakpoint alike: the points are the breakpoints, so families with NPARAM_BP > 0 are audited too).
 * Definition.  For every point, every function of a slot (the cost, or constraint row j) and every flag entry v:
 *   h = 2^-17 * max(1, |z_v|),  zp = z_v + h,  zm = z_v - h,  fd = (f(zp) - f(zm)) / (zp - zm)       only entry v moves
 *   an = the analytic df[v] or dc[j][v] at the unperturbed z
 *   scale = max(1, |f(z)|, |an|, |fd|),  e = |fd - an| / scale
 * 2^-17 ~ 7.6e-6 is eps^(1/3) rounded to a power of two, the step that balances a central difference's truncation error against its
 * rounding error; the division is by the step actually taken.
 * Outputs (any may be NULL, not all four):
 *   d_err        [batch][6]     per slot the largest e over the points, functions and entries v THAT THE SLOT'S OWN ACTIVE-VARIABLE LIST
 *                               NAMES (icostav / tcostav / fcostav for the costs, icav / tcav / fcav for the rows); 0 for an unused slot
 *   d_where      [batch][6][3]  {function (0 for a cost, the row for constraints), breakpoint, flag entry} of that maximum; on equal
 *                               values the smallest (function * nbps + breakpoint) * nz + entry wins; {-1, -1, -1} where d_err is 0
 *   d_leak       [batch][6]     per slot the largest max(|an|, |fd|) / scale over the entries v the slot's list does NOT name: anything
 *                               above rounding means the callback depends on an entry the solver never gives it (the kernels only
 *                               materialise the entries some list names; a missing ntg_av entry makes the callback read a zero,
 *                               silently); 0 for an unused slot or a list that names every entry
 *   d_leak_where [batch][6][3]  as d_where, for d_leak
 * A NaN among the inputs of a maximum stays in it (ntg_batch_kkt's rule); its place is that of the first NaN in the order above.
 * There is NO threshold inside the library: the caller decides what counts as wrong.  A wrong derivative shows at the size of its relative
 * error (a sign error near 1, a factor 1 + 1/64 near 1e-2, a dependence on an unlisted entry at the size of that derivative), while the
 * arithmetic noise of a correct family sits many orders of magnitude below that (DESIGN.md 2g states the floor).
 * Stream ordered.  Scratch is stream ordered, released on every path and does not grow with batch * nbps * nz (per-problem grids: the batch
 * goes through in chunks).  Maxima with a total order on ties, no floating-point atomics: results are bit-identical from call to call and
 * do not depend on the batch around a problem.
 * NTG_E_UNSUPPORTED for host-callback plans, for a plan whose basis tables of one tile of 128 breakpoints exceed the LDS
 * (ntg_batch_check's limit) and for a plan shape the family has no instance for; NTG_E_BADARG for a null plan, null d_x, all outputs null,
 * parameters needed but not set, a batch other than the grids' or the parameters'.  batch <= 0 returns 0. */
#define NTG_VERIFY_NSLOT 6   /* icf, ucf, fcf, nlicf, nltcf, nlfcf -- in this order */
int ntg_batch_verify(const ntg_plan *p, int batch, const double *d_x,
                     double *d_err, int *d_where, double *d_leak, int *d_leak_where, void *stream);

/* Audit a batch of points: the first-order optimality (KKT) residuals of  min F(x)  s.t.  bl <= (A x, c(x)) <= bu  at d_x with the
 * multipliers d_clambda, whoever produced them -- ntg_batch_solve stopped by its own rule (inform 0), capped by itlim or run with
 * fixed_iters (inform 4 by design), a receding-horizon loop, a warm re-solve, or the caller's own estimate.  It replaces what a caller of
 * the reference does by hand with the clambda, g and cJac outputs of npsol_ (ntg.c:250-253); the reference has no such audit, and the dense
 * Jacobian it would need is never formed here: the pass runs on the banded rows of ntg_batch_eval.
 * d_x [batch][nC]; d_lower / d_upper [batch][nbounds] as for ntg_batch_solve; d_clambda [batch][nC + nclin + ncnln] as ntg_batch_solve
 * writes it: lam_A = entries nC .. nC + nclin of a problem, lam_c = the ncnln entries behind them, in ntg_batch_eval's row order.  The first
 * nC entries are NEVER READ (the coefficients are unbounded, and the diagnostic builds park counters there).  Sign convention (NPSOL's):
 * g = A' lam_A + J' lam_c; a multiplier >= 0 belongs to an active lower bound, <= 0 to an active upper bound.  (bl, bu) is the expansion
 * ntg_batch_bounds produces; a bound with |.| >= NTG_INF_BOUND is absent.  The values of A are the ones the solver reads: every linear
 * row, equality or declared inequality, on the plan's grid or, after ntg_plan_set_grids, on that problem's own.  Per-problem parameters
 * are honoured (the evaluation is ntg_batch_eval's).  Built-in families and loaded modules alike.
 * Outputs (either may be NULL, not both):
 *   d_r   [batch][nC]            r = g(x) - A' lam_A - J(x)' lam_c
 *   d_res [batch][NTG_KKT_NRES]
 *     [0] max |r|                [1] max |g|  (the usual test is res[0] / max(1, res[1]) <= tolerance)
 *     [2] largest violation max(bl - a . x, a . x - bu, 0) of a linear row       [3] the same of a nonlinear row, c(x) for a . x; 0 if ncnln = 0
 *     [4] complementarity with signs, the largest over all rows of  lam+ s_lo + lam- s_up  with lam+ = max(lam, 0), lam- = max(-lam, 0),
 *         s_lo = min(max(v - bl, 0), 1), s_up = min(max(bu - v, 0), 1) for the row value v, an absent bound giving slack 1: a multiplier
 *         on a bound that is not active counts with the slack (at most 1), one of the wrong sign at full size.  No activity tolerance.
 *     [5] max |lam| over the nclin + ncnln rows
 *   A NaN among the inputs of a maximum stays in it.
 * Stream ordered.  Scratch is stream ordered, released on every path and does not grow with the batch beyond 256 MiB (the batch goes
 * through in chunks of problems).  Results are bit-identical from call to call and do not depend on the batch around a problem.
 * NTG_E_UNSUPPORTED for host-callback plans (ntg() returns clambda itself) and for a plan with nC above about 10000 (r and x of a problem
 * stay in LDS); NTG_E_BADARG for null d_x, bounds or d_clambda, both outputs null, parameters not set, a batch other than the grids' or
 * the parameters'.  batch <= 0 returns 0. */
#define NTG_KKT_NRES 6
int ntg_batch_kkt(const ntg_plan *p, int batch, const double *d_x, const double *d_lower, const double *d_upper,
                  const double *d_clambda, double *d_res, double *d_r, void *stream);

/* Carry spline coefficients to a finer knot grid, exactly: d_x_from [batch][nC(from)] -> d_x_to [batch][nC(to)] (device pointers on the
 * plans' common device; they must not overlap).  For every problem and output, d_x_to holds the coefficients on `to`'s knots of the same
 * piecewise polynomial that d_x_from describes on `from`'s knots: knot insertion (the blossom of the coarse spline at the fine knots), no
 * fitting and no sampling -- SplineInterp (colloc.c:449-484) of d_x_to on `to` reproduces SplineInterp of d_x_from on `from`; the
 * reference itself has no such operation.  The usual use: ntg_batch_check reports a violation between breakpoints, the caller builds a
 * plan on more knot intervals and starts its solve from the refined solution; or a hand-made guess on a coarse grid.
 * Only the two spline spaces matter: family, rows, cost, breakpoints, maxderiv and parameters of the two plans may differ freely.
 * Conditions, per output (NTG_E_BADARG otherwise; the message names the output and the offending break): same nout, same device, same
 * order; mult_to <= mult_from (a fine plan may ask for less smoothness, never more); the first and last breaks of the two plans agree and
 * every interior break of `from` has a partner of its own among `to`'s breaks.  Two breaks are partners when they differ by at most 1e-12
 * x the knot range (break sequences built by accumulation, like linspace() of the reference, ntg.c:374-389, are not bit-equal where they
 * should coincide); the arithmetic uses `to`'s value for both, so the inclusion of the knot vectors is exact.  On identical spline spaces
 * d_x_to is bit-equal to d_x_from.  Results are bit-identical from call to call and do not depend on the batch around a problem.
 * Both plans on their own grids: checked on the host, the call is stream ordered.  Both plans with per-problem grids (ntg_plan_set_grids)
 * for exactly `batch` problems: every problem uses its own two break sequences, the conditions are checked on the device and THE CALL
 * WAITS FOR THE STREAM to read the result; the message names the first offending problem (its d_x_to row is not written, the rows of the
 * problems that pass are).  NTG_E_BADARG for a batch other than the grids'.  NTG_E_UNSUPPORTED: one plan on its own grid and the other
 * on per-problem grids; host-callback plans; a pair whose weight tables exceed 64 KiB of LDS.  batch <= 0 returns 0. */
int ntg_batch_refine(const ntg_plan *from, const ntg_plan *to, int batch,
                     const double *d_x_from, double *d_x_to, void *stream);

/* Certify a trajectory OVER TIME: bounds of every flag entry and of every linear trajectory row that hold at every time of the horizon,
 * not at sampled times.  ntg_batch_check tells what the rows are at the times passed in; this call makes the statement "for all t" for the
 * rows a guarantee is cheap for -- the linear rows ltc on flat outputs and their derivatives (a corridor ceiling, a velocity or acceleration
 * limit, declared as ranges through ntg_spec.lin_ineq) -- because the trajectory is a B-spline: on each knot interval every flag entry
 * D^r z_o is a polynomial, its Bezier control polygon on that interval encloses it, and halving the interval shrinks the enclosure
 * quadratically.  No family callback is involved: every built-in family and every loaded module alike, per-breakpoint-parameter families
 * included; per-problem parameters are ignored.  d_x [batch][nC]: any coefficients.
 * Pieces.  Output o has l_o = kninterv[o] knot intervals [a_j, b_j] (after ntg_plan_set_grids: those of the problem's own knots).  Each
 * interval is cut into 2^nsub equal parts in the local parameter s = (t - a_j) / (b_j - a_j); piece q = (j << nsub) + i is
 * s in [i / 2^nsub, (i + 1) / 2^nsub].  0 <= nsub <= NTG_ENVELOPE_MAX_NSUB.  npc = (max_o l_o) << nsub is the piece stride of every output.
 * Entry envelope d_lo / d_hi [batch][nz][npc], entry iz[o] + r in the layout of ntg_batch_interp.  With k = order[o]:
 *   1. On interval j, z_o is a polynomial of degree k - 1 in the k coefficients of that span.  Its Bezier control points on [a_j, b_j] are
 *      the blossom of the spline at (a_j repeated k-1-i, b_j repeated i), i = 0 .. k-1 (the de Boor triangle ntg_batch_refine uses, with
 *      these arguments).  The weights do not depend on the coefficients.
 *   2. The control points of D^r z_o on the interval come from r rounds of beta'_i = d / (b_j - a_j) * (beta_{i+1} - beta_i), d the degree
 *      before the round.
 *   3. The control points on a piece come from that polygon by de Casteljau at the dyadic ends of the piece, in the local parameter: at
 *      (i + 1) / 2^nsub keeping the left polygon, then at i / (i + 1) of what is left keeping the right one.  No knot enters this step.
 *   lo is the minimum and hi the maximum of the piece's k - r control points.  For r >= k both are 0.  For pieces q >= l_o << nsub,
 *   lo = +inf and hi = -inf, an empty set.  A NaN among the control points stays in both (ntg_batch_kkt's rule).
 * Row envelope d_row_lo / d_row_hi [batch][nltc][npc] for the linear trajectory rows: row i is sum_v ltc[i][v] z_v(t).  All outputs the row
 * names (non-zero ltc[i][v]) must belong to one basis class (same knots, order, mult, maxderiv); the row's pieces are that class's.  On a
 * piece, each named entry's polygon is degree-elevated to the largest degree among the named entries, b'_i = i/(d+1) b_{i-1} +
 * (1 - i/(d+1)) b_i, and the polygons are summed with the row's coefficients, v ascending; min and max of the summed polygon are the row's
 * bounds on that piece.  This is the row's own Bezier polygon, not interval arithmetic: a row such as x' - y' whose terms cancel gets a
 * tight bound.
 * Certified violation.  d_viol [batch]: the largest max(l - row_lo, row_hi - u, 0) over rows and pieces, with the bounds taken from
 * d_lower / d_upper [batch][nbounds] at the ltc columns exactly as ntg_batch_check reads them (|bound| >= NTG_INF_BOUND: absent).
 * d_where [batch][2] = {row, piece} of that maximum; ties go to the smallest row * npc + piece; {-1, -1} where d_viol is 0.  A NaN in a
 * row's bounds on a piece makes d_viol NaN, at the place of the first NaN in that order.  d_viol == 0 certifies, up to the rounding stated
 * next, that every linear trajectory row holds at every time of the horizon.
 * Rounding.  The enclosure is exact in exact arithmetic.  In double precision every control point is a chain of at most k + nsub convex
 * combinations and r scaled differences: with S = max_i |c_{o,i}| * (2 (k-1) / h_min)^r (h_min the shortest knot interval of the output)
 * each step loses at most a few units in the last place of S; 2^-42 * S covers the chain with a factor of ten to spare.
 * Any output pointer may be NULL, but not all six; d_lower / d_upper are required only when d_viol or d_where is asked for.
 * Stream ordered.  The call allocates no scratch at all (a problem is reduced inside one workgroup), so nothing grows with
 * batch * nz * npc and nothing is left to release on any path.  No floating-point atomics: results are bit-identical from call to call
 * and do not depend on the batch around a problem.
 * batch <= 0 returns 0.  NTG_E_BADARG for a null plan or null d_x, nsub out of range, all outputs null, violation outputs without bounds,
 * row or violation outputs on a plan with nltc == 0, a batch other than the per-problem grids'.  NTG_E_UNSUPPORTED for host-callback plans,
 * for row or violation outputs when some linear trajectory row names outputs of different basis classes (the entry envelope of such a plan
 * is still served), and for a plan whose extraction tables exceed 64 KiB of LDS (sum over basis classes of l (k^2 + 1), plus nC). */
#define NTG_ENVELOPE_MAX_NSUB 6
int ntg_batch_envelope(const ntg_plan *p, int batch, const double *d_x, int nsub,
                       const double *d_lower, const double *d_upper,
                       double *d_lo, double *d_hi,
                       double *d_row_lo, double *d_row_hi,
                       double *d_viol, int *d_where, void *stream);

/* Certify the QUADRATIC trajectory rows over time: ntg_batch_envelope's statement "for all t", for the nonlinear trajectory rows that are
 * sums of squares of shifted flag entries -- the obstacle row of NTG_FAM_OBSTACLE, every row of NTG_FAM_OBSTACLE_FIELD, thrust^2 and speed^2
 * of NTG_FAM_QUADROTOR.  The solvers enforce these rows at the breakpoints only, and ntg_batch_check tells what they are at the times
 * passed in; between two breakpoints a car can clip an obstacle.  Every flag entry is a polynomial on a knot interval, so such a row is one
 * too, and its Bezier polygon follows exactly from the polygons ntg_batch_envelope builds by a Bezier product.  No family callback runs.
 * Declaration.  A family declares row j of its nonlinear trajectory rows, on the host, as
 *   c_j(z) = sum_{t < nt_j} (z[v_t] - s_t)^2,   s_t = const_t + (pidx_t >= 0 ? prm_row_j[pidx_t] : 0)
 * with nt_j <= NTG_SOS_MAXTERMS, v_t a flag entry and prm_row_j the problem's parameter block of that row (ntg_plan_set_params).  Squares
 * only: no weights, no bilinear terms (ntg_batch_forms certifies what this excludes: the form is declared at the call).  The built-in families declare: OBSTACLE row 0; OBSTACLE_FIELD every row; QUADROTOR rows 0 and 1;
 * TESTFAM row 0 (its row 1 has a cosine).  MANIP, KINCAR and VANDERPOL declare nothing.  Loaded modules declare nothing: the module
 * descriptor has no field for it yet, so every row of a module family counts as undeclared (ntg_batch_forms certifies such a row: the
 * caller declares it at the call).
 * ntg_plan_sos_rows: flags[nnltc], 1 = row j is certified by ntg_batch_envelope_sos on this plan, 0 = no statement (the row is undeclared,
 * or it names outputs of different basis classes and has no common pieces).  No device call.
 * Pieces.  Pieces, npc and the range of nsub are exactly as in ntg_batch_envelope.  A row's pieces are those of the basis class of the
 * entries it names (a row with flag 0: of the first entry it names, or of output 0).  d_q_lo / d_q_hi are [batch][nnltc][npc].
 * Per term.  The control points beta_i, i = 0 .. d, of entry v_t on the piece come from steps 1-3 of ntg_batch_envelope, with the same
 * arithmetic.  Then p_i = beta_i - s_t.  If the entry's derivative order is >= k its polygon is the single point 0 and p_0 = -s_t.
 * Square, degree d -> 2d.  g_m = sum_{i+j=m} W_d[i][j] p_i p_j, i ascending, with W_d[i][j] = C(d,i) C(d,j) / C(2d,m) formed on the
 * host from exact integer binomials and rounded once.  This is the Bezier product of the polygon with itself, not interval arithmetic.
 * Row polygon.  Every term's polygon is degree-elevated to D = max_t 2 d_t with the formula ntg_batch_envelope states, and the polygons
 * are summed in term order.  lo / hi are the min / max of the D + 1 points; a NaN among them stays in both (the env_min / env_max rule of
 * ntg_batch_envelope).  Pieces past the class's own are lo = +inf, hi = -inf.  A row with flag 0 gives lo = -inf, hi = +inf on the live
 * pieces, which is no statement.
 * Certified violation.  d_viol [batch], d_where [batch][2] = {row, piece}: the largest max(l - lo, hi - u, 0) over certified rows and pieces,
 * the bounds read from d_lower / d_upper [batch][nbounds] at the nnltc columns, in the nlic, nltc, nlfc, nnlic, nnltc order of
 * ntg_batch_check (|bound| >= NTG_INF_BOUND: absent).  Ties go to the smallest row * npc + piece; a NaN wins over every number, the first
 * NaN in that order (the env_take rule of ntg_batch_envelope); {-1, -1} where the violation is 0.  d_viol == 0 certifies, up to the
 * rounding stated next, that every such row holds at every time of the horizon.
 * Rounding.  With S_t = max_i |c_{o,i}| (2(k-1)/h_min)^r + |s_t| for term t (o, r the output and derivative order of v_t), each factor's
 * control point carries at most 2^-42 S_t, the statement of ntg_batch_envelope with its factor of ten to spare.  So a product control point
 * carries at most 2 * 2^-42 S_t^2 plus a few units in the last place of S_t^2; elevation and the sum add a few more.  The row's slack is
 * 2^-40 * sum_t S_t^2.
 * Any output pointer may be NULL, but not all four; d_lower / d_upper are required only for d_viol / d_where.  Stream ordered.  No scratch
 * allocation and no floating-point atomics: results are bit-identical from call to call and independent of the batch around a problem.
 * Per-problem parameters are read for pidx >= 0; per-problem grids are honoured, with the batch rules of ntg_batch_envelope.
 * batch <= 0 returns 0, after the null-plan and nsub checks.  NTG_E_BADARG for a null plan or null d_x, nsub out of range, all four outputs
 * null, violation outputs without bounds, nnltc == 0, parameters needed but not set, a batch other than the grids' or the parameters'.
 * NTG_E_UNSUPPORTED for host-callback plans, for tables above NTG_ENVELOPE_LDS_MAX (64 KiB of LDS: the extraction tables of
 * ntg_batch_envelope plus 385 product weights and the parameter row), for more than 8 trajectory rows, for a plan no row of which is
 * certified (the message says the family declares none), and for d_viol / d_where when some row of the plan has flag 0 (the message names
 * the row): a partial certificate must not read as a whole one. */
#define NTG_SOS_MAXTERMS 4
/* flags[nnltc]: 1 = row j is certified by ntg_batch_envelope_sos on this plan,
 * 0 = no statement (undeclared, or names outputs of different basis classes). No device call. */
int ntg_plan_sos_rows(const ntg_plan *p, int *flags);

int ntg_batch_envelope_sos(const ntg_plan *p, int batch, const double *d_x, int nsub,
                           const double *d_lower, const double *d_upper,
                           double *d_q_lo, double *d_q_hi, double *d_viol, int *d_where, void *stream);

/* Certified row EXTREMA over time, by bisection: the global minimum and maximum of each certifiable trajectory row over the horizon, each
 * enclosed to a tolerance and each with a witness time.  ntg_batch_envelope and ntg_batch_envelope_sos cut every knot interval into the same
 * 2^nsub pieces; a row that sits on its bound at a breakpoint (the obstacle row of a solved problem) is then never certified, because the
 * polygon of the piece holding that breakpoint lies below the bound by a term of order (piece width)^2.  This call bisects only the pieces
 * that can still hold the extremum and says by how much the row is violated between breakpoints, no more than that, and WHEN.
 * Rows.  nrow = nltc + nnltc, the linear trajectory rows first: ntg_batch_check's numbering.  ntg_plan_extrema_rows: flags[nrow], no
 * device call.  A linear row has flag 1 when the outputs it names (non-zero ltc[i][v]) belong to one basis class; a row of zeros counts as
 * class 0 and has flag 1.  A nonlinear row has the flag ntg_plan_sos_rows gives it.  Loaded modules declare no sum of squares yet: their
 * linear rows are certified, their nonlinear rows are not (ntg_batch_forms certifies a quadratic one, declared at the call).
 * Outputs, any may be NULL but not all six:
 *   d_ext     [batch][nrow][4]  {min_lo, min_hi, max_lo, max_hi}
 *   d_when    [batch][nrow][2]  {t_min, t_max}
 *   d_status  [batch][nrow]     NTG_EXTREMA_OK / _DEPTH / _FULL / _NAN / _NONE
 *   d_npieces [batch][nrow]     polygons evaluated
 *   d_viol    [batch][2]        {attained, certified}
 *   d_where   [batch][2]        row of each of the two violations; ties to the smallest row; -1 where the figure is 0
 * Definition, per problem and per row with flag 1.
 * 1. Level-0 pieces.  The level-0 pieces are the l knot intervals of the row's basis class (after ntg_plan_set_grids: the problem's own
 *    intervals).  The polygon B_0 .. B_D of the row on interval j is the row polygon of ntg_batch_envelope (linear rows) or
 *    ntg_batch_envelope_sos (nonlinear rows) at nsub = 0, piece j, formed by the same sequence of operations.  So with max_depth = 0, min_lo
 *    equals the minimum over j of those calls' row_lo / q_lo and max_hi equals the maximum of their row_hi / q_hi, bit for bit.  A row of zeros
 *    has D = 0 and B_0 = 0.
 * 2. Indexing and state.  A piece at level lambda of interval j has an index i in [0, 2^lambda); its ends lie at the local parameters
 *    i / 2^lambda and (i + 1) / 2^lambda, and B_0 and B_D are the row's values at those ends.  plo and phi are the env_min / env_max of its
 *    D + 1 points.  The row keeps four quantities: U, the smallest end value seen, with its time; V, the largest end value seen, with its time;
 *    Rlo, the smallest plo of a retired piece (initially +inf); Rhi, the largest phi of a retired piece (initially -inf).  The time of an end
 *    is kn[j] + hh[j] * ((double)i / (double)(1 << lambda)) with hh[j] = kn[j + 1] - kn[j], the product and the sum rounded separately (no
 *    fused multiply-add); an end at local parameter 1 takes kn[j + 1].  On equal values the smaller time wins, so minimum and maximum do not
 *    depend on the order of the pieces.  A NaN end value is never taken.
 * 3. Level lambda.  Update U and V with both ends of every piece of the level.  Then decide each piece: a piece is open if
 *    (sides & 1) and plo < U - tol, or (sides & 2) and phi > V + tol.  Every other piece retires into Rlo / Rhi.
 *    No open piece: status OK, stop.  lambda == max_depth: status DEPTH, the open pieces retire, stop.  More than NTG_EXTREMA_CAP open
 *    pieces: status FULL, they retire, stop.  Otherwise every open piece is split at the middle by de Casteljau: each new point is
 *    0.5 * (a + b), the two end points of a polygon are carried over, not recomputed; the children form level lambda + 1.
 * 4. Result.  min_lo = Rlo, min_hi = U, max_lo = V, max_hi = Rhi; t_min and t_max are the times of U and V; npieces is the number of
 *    polygons evaluated over all levels (l at level 0, two per open piece afterwards).  Always min_lo <= min over t of the row <= min_hi, and
 *    the same for the maximum, up to the rounding below.  min_hi and max_lo are attained values.  With status OK and the side asked for,
 *    min_hi - min_lo <= tol.  A side not asked for never opens a piece, but its two numbers are kept from the pieces visited and are still valid.
 * 5. NaN.  A NaN in any plo / phi makes all four numbers and both times NaN, with status NAN.  Such a piece is never open, the levels go on
 *    without it, and npieces counts as usual.
 * 6. Rows with flag 0: (-inf, +inf, -inf, +inf), times NaN, status NONE, npieces 0.
 * 7. Violation.  Bounds d_lower / d_upper [batch][nbounds] are read as ntg_batch_check reads them (|bound| >= NTG_INF_BOUND is absent).
 *    Both figures are maxima over the rows: attained = max(l - min_hi, max_lo - u, 0) -- at d_when the row really violates by this much;
 *    certified = max(l - min_lo, max_hi - u, 0) -- no time violates by more.  certified == 0 certifies the plan's rows over the whole horizon.
 *    A NaN wins over every number (the env_take rule of ntg_batch_envelope).  Both are refused (NTG_E_UNSUPPORTED, naming the row) when some
 *    row has flag 0: the rule of ntg_batch_envelope_sos.
 * Rounding.  The level-0 polygon carries the slack of the call it comes from.  A halving adds one rounding per new point, of at most
 * 2^-53 max|B|; a point passes at most D <= 18 of them per level, over at most 30 levels: less than 2^-43 max|B|, and max|B| <= sum_t S_t^2
 * for a quadratic row.  So the slack is 2^-39 * sum_t S_t^2 for a quadratic row (S_t as in ntg_batch_envelope_sos) and twice
 * ntg_batch_envelope's row slack for a linear one.
 * Arguments.  tol is finite and >= 0; 0 <= max_depth <= NTG_EXTREMA_MAX_DEPTH; sides is one of 1 (minimum), 2 (maximum), 3 (both).
 * Stream ordered, without scratch in HBM and without floating-point atomics: a wavefront owns a problem and keeps the open pieces of one
 * row in a work list in LDS.  Results are bit-identical from call to call and independent of the batch around a problem.  Per-problem
 * parameters and per-problem grids are honoured with the batch rules of ntg_batch_envelope_sos.
 * batch <= 0 returns 0 after the null-plan and argument checks.  NTG_E_BADARG for a null plan or null d_x, an argument outside the ranges
 * above, all outputs null, violation outputs without bounds, nrow == 0, parameters needed but not set, a batch other than the grids' or the
 * parameters'.  NTG_E_UNSUPPORTED for host-callback plans, for a plan without any flagged row, for nnltc > 8, and for tables and work lists
 * above 158 KiB of LDS: 385 product weights, sum over basis classes of l (k^2 + 2) + 1, and per wavefront of four nC + the parameter row +
 * 64 (D_max + 2) doubles with D_max = 10 (largest order <= 6) or 18 -- on per-problem grids the class tables count per wavefront too. */
#define NTG_EXTREMA_MAX_DEPTH 30
#define NTG_EXTREMA_CAP 64          /* open pieces of one row at one level */
#define NTG_EXTREMA_OK 0            /* every piece closed: the tolerance is met */
#define NTG_EXTREMA_DEPTH 1         /* stopped at max_depth with pieces still open */
#define NTG_EXTREMA_FULL 2          /* stopped because more than NTG_EXTREMA_CAP pieces were open */
#define NTG_EXTREMA_NAN 3
#define NTG_EXTREMA_NONE (-1)       /* no statement for this row */

/* flags[nltc + nnltc]: 1 = ntg_batch_extrema certifies the row on this plan, 0 = no statement. No device call. */
int ntg_plan_extrema_rows(const ntg_plan *p, int *flags);

int ntg_batch_extrema(const ntg_plan *p, int batch, const double *d_x,
                      double tol, int max_depth, int sides,
                      const double *d_lower, const double *d_upper,
                      double *d_ext, double *d_when, int *d_status, int *d_npieces,
                      double *d_viol, int *d_where, void *stream);

/* Certified closest approach of PAIRS of trajectories: the smallest squared distance over the horizon between two planned bodies, enclosed to
 * a tolerance, with the time of it, and by how much a required distance is missed.  The certificates above work on one problem's own rows;
 * the distance between two vehicles is not such a row: the two may be cars of one problem or belong to different problems of the batch.  On
 * a common knot interval both trajectories are polynomials, so their difference is one too, and the squared distance is a sum of squares of
 * that difference: ntg_batch_envelope_sos's polygons and ntg_batch_extrema's bisection apply.  No family callback runs.
 * Bodies.  body_outs is a HOST array [nbody][ndim], copied by the call: row g names the ndim outputs that are the coordinates of body g (three
 * kinematic cars: {0,1}, {2,3}, {4,5}).  1 <= ndim <= NTG_SEP_MAXDIM, 1 <= nbody <= NTG_MAX_OUT.  Every output named must exist, all must
 * belong to one basis class, and 0 <= deriv < maxderiv[o].  deriv = 0 gives the distance of positions, deriv = 1 the relative speed.
 * Pairs.  d_pairs is a device array [npairs][4] of {a, b, ga, gb}: body ga of problem a against body gb of problem b; a == b is allowed (two
 * cars of one problem).  The kernel checks 0 <= a, b < batch and 0 <= ga, gb < nbody before it reads anything of the pair.  A pair that fails
 * has status NTG_SEP_BADPAIR, NaN in both entries of d_min, in d_when and in both entries of d_viol, and npieces 0; it never causes a read
 * outside d_x.
 * Required distance.  d_sep is a device array [npairs] or NULL; s2 = sep * sep, one rounding.  NULL means s2 = +inf: no threshold.
 * Outputs, any may be NULL but not all five:
 *   d_min     [npairs][2]  {min_lo, min_hi} of the squared distance
 *   d_when    [npairs]     the time of min_hi
 *   d_status  [npairs]     NTG_EXTREMA_OK / _DEPTH / _FULL / _NAN, or NTG_SEP_BADPAIR
 *   d_npieces [npairs]     polygons evaluated
 *   d_viol    [npairs][2]  {attained, certified}; requires d_sep
 * Definition, per pair.
 * 1. Difference coefficients.  The class of the named outputs has n coefficients per output.  For dimension t,
 *    delta_t[i] = x[a][iC[oa_t] + i] - x[b][iC[ob_t] + i], i = 0 .. n-1, with oa_t = body_outs[ga][t] and ob_t = body_outs[gb][t]: one IEEE
 *    subtraction per coefficient, and nothing else is rounded here.  From here on the pair is a virtual problem with ndim outputs whose
 *    coefficients are delta.
 * 2. Level-0 polygons.  The row is c(t) = sum_t (D^deriv delta_t(t))^2.  On knot interval j its polygon is formed by the sequence of
 *    operations of ntg_batch_envelope_sos: extract, deriv differences, the square by the W_d tables, the terms summed in dimension order; the
 *    terms are {dimension t, derivative deriv, shift 0, no parameter} (beta - 0.0 and beta are the same bits).  The polygon is bit-identical
 *    to that of ntg_batch_extrema at sides = 1 on a plan whose sum-of-squares row has those terms with zero shift, given delta as coefficients.
 * 3. Levels.  Steps 2 to 4 of ntg_batch_extrema's definition with sides = 1, and one addition to the opening rule: a piece is open iff
 *    plo < U - tol and not plo >= s2.  A piece that cannot come closer than the required distance retires at once, so with a threshold most
 *    pairs of a fleet end at level 0.  Statuses NTG_EXTREMA_OK / _DEPTH / _FULL / _NAN with the same meaning, the cap NTG_EXTREMA_CAP.
 * 4. Results.  min_lo = Rlo, min_hi = U (an attained value), d_when the time of U, npieces the number of polygons evaluated.  Always
 *    min_lo <= min over t of c <= min_hi, up to the rounding below.  With status OK, min_lo >= min(min_hi - tol, s2).
 * 5. Violation, in squared distance.  attained = max(s2 - min_hi, 0): the pair really comes closer than required, at d_when.
 *    certified = max(s2 - min_lo, 0): at no time does the pair come closer than required by more than this.  certified == 0 certifies the
 *    separation over the whole horizon.  A NaN s2 makes both figures NaN; the bisection then runs as without a threshold.
 * 6. NaN.  A NaN in any plo is handled as in ntg_batch_extrema's rule 5: both numbers and the time are NaN, the status is NAN.
 * Rounding.  ntg_batch_extrema's slack for a quadratic row, 2^-39 * sum_t S_t^2, with S_t = max_i (|x_a,i| + |x_b,i|) * (2 (k - 1) / h_min)^deriv:
 * the sum of magnitudes in place of max |c| covers the one rounding of delta.
 * Arguments.  tol is finite and >= 0; 0 <= max_depth <= NTG_EXTREMA_MAX_DEPTH.
 * Stream ordered, without scratch in HBM and without floating-point atomics: a wavefront owns a pair and keeps delta and the open pieces in
 * LDS.  Results are bit-identical from call to call; the result of a pair does not depend on the other pairs or on the batch.  Per-problem
 * parameters are ignored.
 * npairs <= 0 or batch <= 0 returns 0 after the null-plan and argument checks.  NTG_E_BADARG for a null plan, d_x, body_outs or d_pairs, for
 * ndim, nbody, deriv, tol or max_depth outside the ranges above, an output index out of range, all five outputs null, d_viol without d_sep.
 * NTG_E_UNSUPPORTED, with a message that says why, for host-callback plans, for named outputs of different basis classes (the message names
 * the two outputs), for a plan with per-problem grids in force (two problems then have no common knot intervals; the a == b case included),
 * and for tables above 158 KiB of LDS: 385 product weights, l (k^2 + 2) + 1 of the class, and per wavefront of four ndim n + 64 (D_max + 2)
 * doubles with D_max = 10 (order <= 6) or 18. */
#define NTG_SEP_MAXDIM 4            /* == NTG_SOS_MAXTERMS */
#define NTG_SEP_BADPAIR (-2)        /* status: a problem or body index of the pair is out of range */

int ntg_batch_separation(const ntg_plan *p, int batch, const double *d_x,
                         int nbody, int ndim, const int *body_outs, int deriv,
                         int npairs, const int *d_pairs, const double *d_sep,
                         double tol, int max_depth,
                         double *d_min, double *d_when, int *d_status, int *d_npieces,
                         double *d_viol, void *stream);

/* Certified extrema of QUADRATIC FORMS of the flat flag that the caller declares at the call: ntg_batch_extrema's statement -- the global
 * minimum and maximum over the horizon, each enclosed to a tolerance and each with a witness time -- for functions that are not rows of the
 * plan, or are rows its family cannot declare: weighted squares, bilinear terms, linear terms, on every plan (built-in families, loaded
 * modules, per-problem grids).  The speed^2 of a kinematic car, its turning numerator x' y'' - y' x'', v . a, a weighted thrust limit, an
 * elliptical keep-out zone, a nonlinear row of a module family.  On a knot interval every flag entry is a polynomial, so a quadratic form of
 * the flag is one too, and its Bezier polygon follows from the entries' polygons by the Bezier product of two polygons.
 * No family callback runs.
 * Forms.  form_nterms [nform] and terms are HOST arrays, copied by the call; terms is concatenated form after form.  Form j is
 *   q_j(z) = sum_t term_t,   term_t = w (z[u] - a)(z[v] - b) when v >= 0,   term_t = w (z[u] - a) when v == -1 (sv and pv are then ignored)
 * with the shifts a = su + (pu >= 0 ? fprm_b[pu] : 0) and b = sv + (pv >= 0 ? fprm_b[pv] : 0).  u and v are flag entries iz[o] + r in the
 * layout of ntg_batch_interp.  fprm_b is row b of d_fprm [batch][nfp]: the call's own per-problem parameters (an obstacle centre, a
 * half-plane offset), not the family's, so ntg_plan_set_params is neither needed nor read.  All entries a form names must belong to one
 * basis class; the form's pieces are that class's knot intervals, and different forms may use different classes.  A constant offset is the
 * caller's business: it moves the bounds.  1 <= terms per form <= NTG_FORM_MAXTERMS, 0 <= nform <= NTG_FORM_MAXFORMS.
 * Outputs, any may be NULL but not all six:
 *   d_ext     [batch][nform][4]  {min_lo, min_hi, max_lo, max_hi}
 *   d_when    [batch][nform][2]  {t_min, t_max}
 *   d_status  [batch][nform]     NTG_EXTREMA_OK / _DEPTH / _FULL / _NAN
 *   d_npieces [batch][nform]     polygons evaluated
 *   d_viol    [batch][2]         {attained, certified}
 *   d_where   [batch][2]         form of each of the two violations; ties to the smallest form; -1 where the figure is 0
 * Definition, per problem and per form.
 * 1. Level-0 polygon of form j on knot interval i of its class (after ntg_plan_set_grids: the problem's own intervals).  For each term, in
 *    declared order:
 *    a. Factors.  The control points beta of entry u come from steps 1-3 of ntg_batch_envelope at nsub = 0, with the same arithmetic as
 *       ntg_batch_envelope_sos; the degree is d = k - 1 - r_u, and a derivative of order >= k is the single point 0 with d = 0.  Then
 *       p_i = beta_i - a.  For v >= 0 the degree e and the points q_j of entry v come the same way with the shift b.
 *    b. Product, degree d + e.  g_m = sum_{i + j = m} W_{d,e}[i][j] * p_i * q_j, i ascending, W_{d,e}[i][j] = C(d,i) C(e,j) / C(d+e, i+j):
 *       the numerator is an exact integer product and the division is the one rounding (the binomials are at most C(18,9), so everything
 *       is exact in double up to that division).  W_{d,d} is therefore bit-equal to the W_d of ntg_batch_envelope_sos.  A linear term has
 *       g_i = p_i.
 *    c. Squares.  A square term has v == u, pu == pv and su == sv bitwise; its product is formed exactly as ntg_batch_envelope_sos forms
 *       a square.  A form whose terms are all squares with w == 1.0 then has the same level-0 polygon, bit for bit, as the equivalent
 *       sum-of-squares row of ntg_batch_extrema.
 *    d. Sum.  The term's polygon is w * g_m with one rounding; it is elevated to the form's degree D_j = max_t deg_t with the formula
 *       ntg_batch_envelope states and added to the form's polygon, terms in declared order (the product and the sum are rounded separately).
 *       D_j <= 2 (kmax - 1) <= 18.
 * 2. Levels, results, NaN.  Steps 2 to 5 of ntg_batch_extrema's definition, unchanged: tol, max_depth, sides, NTG_EXTREMA_CAP and the
 *    statuses keep their meaning; the times come from the form's class.  Every form is certified: there is no status NONE and no
 *    partial-certificate refusal.
 * 3. Violation.  Bounds d_flo / d_fhi [batch][nform]; a bound with |bound| >= NTG_INF_BOUND is absent.  attained and certified are the
 *    maxima over the forms exactly as in rule 7 of ntg_batch_extrema; a form with both bounds absent contributes 0.  certified == 0
 *    certifies every declared form over the whole horizon.
 * Rounding.  With S_x = max_i |c_{o,i}| (2(k-1)/h_min)^r + |shift| for factor x, a factor's control point carries at most 2^-42 S_x.  The
 * slack of a form is 2^-39 * sum_t |w_t| S_u S_v, with S_v = 1 for a linear term.
 * Arguments.  tol, max_depth and sides as in ntg_batch_extrema.  Stream ordered, without scratch in HBM and without floating-point atomics:
 * a wavefront owns a problem and walks its forms.  Results are bit-identical from call to call and independent of the batch around a
 * problem.  Per-problem grids are honoured with the batch rule of ntg_batch_extrema: the batch must be the grids'.
 * batch <= 0 or nform == 0 returns 0 after the null-plan and argument checks.  NTG_E_BADARG, naming the form and term where one is at fault,
 * for a null plan, d_x, form_nterms or terms; nform outside 0 .. NTG_FORM_MAXFORMS; a form with 0 or more than NTG_FORM_MAXTERMS terms; u outside
 * [0, nz) or v outside [-1, nz); pu or pv outside [-1, nfp); nfp < 0, or a parameter named while d_fprm is null; a non-finite w, su or sv;
 * tol, max_depth or sides out of range; all six outputs null; violation outputs without both bounds; a batch other than the grids'.
 * NTG_E_UNSUPPORTED for host-callback plans, for a form that names entries of different basis classes (the message names the form and the two
 * outputs), and for tables and work lists above 158 KiB of LDS: 3025 product weights, sum over basis classes of l (k^2 + 2) + 1, and per
 * wavefront of four nC + nfp + 64 (D_max + 2) doubles with D_max = 10 (largest order <= 6) or 18 -- on per-problem grids the class tables
 * count per wavefront too. */
#define NTG_FORM_MAXFORMS 8
#define NTG_FORM_MAXTERMS 8      /* per form */
typedef struct { int u, v, pu, pv; double w, su, sv; } ntg_form_term;

int ntg_batch_forms(const ntg_plan *p, int batch, const double *d_x,
                    int nform, const int *form_nterms, const ntg_form_term *terms,
                    int nfp, const double *d_fprm,
                    double tol, int max_depth, int sides,
                    const double *d_flo, const double *d_fhi,
                    double *d_ext, double *d_when, int *d_status, int *d_npieces,
                    double *d_viol, int *d_where, void *stream);

/* Certified extrema of RATIOS of products of quadratic forms of the flat flag: ntg_batch_forms' statement for
 *   R_r(t) = prod_{a < nnum} q_{num[a]}(z(t)) / prod_{b < nden} q_{den[b]}(z(t)),
 * the quantities the physical limits of a flat system are made of.  With S = x'^2 + y'^2 and T = x' y'' - y' x'' of a kinematic car: the squared
 * curvature kappa^2 = T T / (S S S), hence the steering angle tan delta = L kappa that ntg_batch_kincar_reverse computes per sample; the squared
 * lateral acceleration T T / S; the heading slope y' / x'.  On a knot interval let N = sum n_i B_i^D and Q = sum d_i B_i^D be the Bezier polygons
 * of numerator and denominator at one degree D, with every d_i > 0.  Then N / Q = sum_i (n_i / d_i) (d_i B_i / sum_j d_j B_j) is a convex
 * combination of the quotients n_i / d_i: min_i n_i / d_i <= N / Q <= max_i n_i / d_i on the piece, and the end quotients are attained values.
 * De Casteljau halves both polygons, so ntg_batch_extrema's bisection applies to the pair.  No family callback runs.
 * Forms are declared exactly as for ntg_batch_forms (form_nterms, terms, nfp, d_fprm: same arrays, same checks, same messages); they are the
 * factors, none of them is certified by itself.  ratios [nratio] is a HOST array, copied by the call.  nnum == 0 is the numerator 1, nden == 0
 * the denominator 1 (a product of forms, S S); an index may repeat (a power).  Every form a ratio names must belong to one basis class;
 * different ratios may use different classes.  0 <= nratio <= NTG_RATIO_MAXRATIOS, 0 <= nnum, nden <= NTG_RATIO_MAXFACTORS, not both 0.
 * Outputs as for ntg_batch_forms with the ratio in the place of the form: d_ext [batch][nratio][4], d_when [batch][nratio][2], d_status and
 * d_npieces [batch][nratio], d_viol and d_where [batch][2]; any may be NULL but not all six.
 * Definition, per problem and per ratio.
 * 1. Level 0, knot interval j of the ratio's class.  The polygon F_f of every form named is step 1 of ntg_batch_forms, bit for bit.  The
 *    numerator is the chain G = F_{num[0]}; G = G (x) F_{num[a]}, a ascending, with (x) the product rule 1b of ntg_batch_forms between the chain
 *    so far (degree d) and the form (degree e): g_m = sum_{i + j = m} W_{d,e}[i][j] * G_i * F_j, i ascending, every product and every sum
 *    rounded; W = C(d,i) C(e,j) / C(d+e,i+j), the numerator an exact integer (below 2^53: at most C(24,12)^2), the division its one rounding.
 *    The denominator likewise.  An empty side is the single point 1.0.  The degrees are dN = sum D_f and dD = sum D_f; the lower side is
 *    elevated to DR = max(dN, dD) with the formula ntg_batch_envelope states (a side of ones stays ones, bit for bit).
 * 2. Piece.  A piece carries both polygons n_0 .. n_DR and d_0 .. d_DR.  A NaN in either marks the ratio as rule 5 of ntg_batch_extrema does
 *    (status NTG_EXTREMA_NAN), before anything else.  Otherwise, if every d_i > 0: rho_i = n_i / d_i by one IEEE division, plo = min rho_i,
 *    phi = max rho_i.  Otherwise plo = -inf and phi = +inf: the piece is open on every side asked for.
 * 3. Ends.  An end with d > 0 contributes rho to U / V, with its time exactly as in rule 2 of ntg_batch_extrema.  An end with d <= 0 is never
 *    taken and marks the ratio POLE: after the end-taking of the level that marked it the loop stops with status NTG_RATIO_POLE, ext =
 *    (-inf, +inf, -inf, +inf), NaN times, and npieces the pairs formed so far.  NAN takes precedence over POLE.
 * 4. Levels, results, statuses.  Rules 2 to 5 of ntg_batch_extrema otherwise: tol (absolute, in units of the ratio), max_depth, sides,
 *    NTG_EXTREMA_CAP, the statuses OK / DEPTH / FULL.  Both polygons of an open piece are halved with 0.5 * (a + b).  npieces counts pairs.
 *    A ratio {nnum = 1, nden = 0} therefore returns what ntg_batch_forms returns for its form, bit for bit, and S / S returns 1.0 four times.
 * 5. Violation.  Rule 7 of ntg_batch_extrema with d_rlo / d_rhi [batch][nratio], the formulas as they stand: a POLE ratio with a bound present
 *    gives certified = +inf and attained = 0.
 * Rounding.  With M_f = sum_t |w_t| S_u S_v, a point of form f carries at most delta_f = 2^-39 M_f (ntg_batch_forms).  Let m_f = delta_f + the
 * largest |point| of the level-0 polygons of form f over the problem's knot intervals.  (x) is a convex combination of products (the weights of
 * a point sum to 1), elevation and halving are convex combinations, so the points of a side stay within prod m_f, the factors' errors reach a
 * side as prod m_f * sum_f delta_f / m_f, and the roundings of at most 3 products (22 each), 24 elevations (3 each) and 30 halvings (24 each)
 * add less than 2^-43 prod m_f:
 *   eps_side = prod_f m_f * (sum_f delta_f / m_f + 2^-43)      (an empty side: 2^-43)
 * and a quotient rho carries at most (eps_N + |rho| eps_D) / (d_min - eps_D), where d_min is the smallest denominator point of the pieces that
 * produced the figure (the division's own rounding, 2^-53 |rho|, is inside: eps_D >= 2^-43 d_min).  A certificate is claimed only where d_min >
 * eps_D.  The a-priori figure 2^-36 prod M_f per side is also true but of no use for a ratio: M_f bounds a derivative by its coefficients,
 * 40 times the speed of the test cars, and kappa^2 has ten factors.
 * Arguments.  tol, max_depth and sides as in ntg_batch_extrema.  Stream ordered, without scratch in HBM and without floating-point atomics: a
 * wavefront owns a problem and walks its ratios, lane p owns pair p.  Results are bit-identical from call to call and independent of the batch
 * around a problem.  Per-problem grids are honoured: the batch must be the grids'.
 * batch <= 0 or nratio == 0 returns 0 after the checks.  The refusals of ntg_batch_forms apply unchanged.  NTG_E_BADARG, naming the ratio, for
 * nratio outside 0 .. NTG_RATIO_MAXRATIOS, nnum or nden outside 0 .. NTG_RATIO_MAXFACTORS, both sides empty, a form index outside [0, nform).
 * NTG_E_UNSUPPORTED, naming the ratio, for a side of degree above NTG_RATIO_MAXDEG (the message names the degree), for forms of different basis
 * classes in one ratio (it names the two forms), and for tables and work lists above 158 KiB of LDS: 3025 product weights of the forms, the
 * tables (d + 1)(e + 1) of the distinct pairs of degrees the chains use, the class tables of ntg_batch_forms, and per wavefront nC + nfp +
 * 64 (2 KR + 1) doubles, KR = 13 where every DR <= 12 and the largest order is <= 6, else 25; four wavefronts, two where four do not fit. */
#define NTG_RATIO_MAXRATIOS  4
#define NTG_RATIO_MAXFACTORS 4      /* per side; repeat an index for a power */
#define NTG_RATIO_MAXDEG     24     /* Bezier degree of either side: kappa^2 of an order-6 car is 24 */
#define NTG_RATIO_POLE       4      /* status: the denominator was <= 0 at a time the bisection visited */
typedef struct { int nnum, nden; int num[NTG_RATIO_MAXFACTORS], den[NTG_RATIO_MAXFACTORS]; } ntg_ratio;

int ntg_batch_ratios(const ntg_plan *p, int batch, const double *d_x,
                     int nform, const int *form_nterms, const ntg_form_term *terms, int nfp, const double *d_fprm,
                     int nratio, const ntg_ratio *ratios,
                     double tol, int max_depth, int sides,
                     const double *d_rlo, const double *d_rhi,
                     double *d_ext, double *d_when, int *d_status, int *d_npieces,
                     double *d_viol, int *d_where, void *stream);

/* Certified extrema of SINES AND COSINES of the flat flag, declared at the call: ntg_batch_forms' statement -- the global minimum and maximum
 * over the horizon, each enclosed to a tolerance and each with a witness time -- for
 *   h_j(z) = sum_t w_t g_t(theta_t(z)),   theta_t = sum_i coef[i] * z[ent[i]] + phase + (pp >= 0 ? fprm_b[pp] : 0),
 * g_t = sin, cos or the identity by kind.  The tip height sin qa + sin(qa + qb) + sin(qa + qb + qc) of a manipulator, its x-coordinate (cosines),
 * a wall in front of the arm n . tip <= d (sines with a phase), a heading angle.  These are no polynomials in the flag, so none of the other
 * certificates takes them.  On a piece of a knot interval the angle theta_t is a polynomial with a Bezier polygon Theta_t; about the centre c of
 * that polygon sin(theta) = sin c + cos c (theta - c) + R with |R| <= rho^2 / 2, rho the polygon's radius: the linear part is a polygon again,
 * and the remainder is of the same order in the piece width as the gap between a polygon and its function, so ntg_batch_extrema's bisection
 * converges as it does for polynomial rows.  No family callback runs: every plan is served (built-in families, loaded modules, per-problem grids).
 * Forms.  form_nterms [nform] and terms are HOST arrays, copied by the call; terms is concatenated form after form.  Entries ent[i] are flag
 * entries iz[o] + r in the layout of ntg_batch_interp; 1 <= nent <= NTG_TRIG_MAXENT.  fprm_b is row b of d_fprm [batch][nfp], the call's own
 * per-problem parameters.  Every entry of a form belongs to one basis class; different forms may use different classes.
 * 1 <= terms per form <= NTG_TRIG_MAXTERMS, 0 <= nform <= NTG_TRIG_MAXFORMS.
 * Outputs as for ntg_batch_forms, any may be NULL but not all six: d_ext [batch][nform][4] = {min_lo, min_hi, max_lo, max_hi}, d_when
 * [batch][nform][2], d_status [batch][nform] (NTG_EXTREMA_OK / _DEPTH / _FULL / _NAN), d_npieces [batch][nform], d_viol [batch][2] =
 * {attained, certified} and d_where [batch][2] against d_flo / d_fhi [batch][nform].
 * Definition, per problem and per form.  Every product and every sum below is rounded separately (no fused multiply-add).
 * 1. Level-0 angle polygons, knot interval j of the form's class.  The control points of each entry come from steps 1-3 of ntg_batch_envelope at
 *    nsub = 0 with ntg_batch_forms' arithmetic (rule 1a there, shift 0): degree k - 1 - r, a derivative of order >= k is the single point 0.
 *    Each entry polygon is multiplied by its coef (one rounding), elevated with the formula ntg_batch_envelope states, and the entry polygons
 *    are summed in declared order; then phase + fprm_b[pp] is added to every point.  A SIN or COS term is elevated to D_j, the largest entry
 *    degree of the whole form (D_j <= 9).  A LIN term is elevated to the largest entry degree of the term, multiplied by w_t (one rounding),
 *    elevated to D_j and added to the form's linear polygon Lambda, LIN terms in declared order: rule 1d of ntg_batch_forms.  A piece carries
 *    the angle polygons Theta_t,0..D of its SIN and COS terms and, if the form has a LIN term, Lambda: at most NTG_TRIG_MAXTERMS polygons.
 * 2. Piece enclosure.  For a SIN or COS term lo_t = min_m Theta_t,m, hi_t = max_m Theta_t,m, c_t = 0.5 * (lo_t + hi_t),
 *    rho_t = max(hi_t - c_t, c_t - lo_t), (S, C) = sincos(c_t), and T_t,m = w_t * (S + C * (Theta_t,m - c_t)) for SIN,
 *    T_t,m = w_t * (C - S * (Theta_t,m - c_t)) for COS.  P_m = 0 + sum_t T_t,m over the SIN and COS terms in declared order, + Lambda_m last;
 *    r = sum_t |w_t| * rho_t * rho_t * 0.5 over the same terms, from 0; plo = min_m P_m - r, phi = max_m P_m + r.  If the form has no LIN
 *    term, plo = max(plo, -W) and phi = min(phi, W) with W = sum_t |w_t| (a NaN stays).
 * 3. Ends.  The value at a piece end is 0 + sum_t w_t g_t(Theta_t,end) over the SIN and COS terms in declared order, + Lambda_end last;
 *    Theta_t,end is the polygon's first or last point, which de Casteljau carries over bit for bit.  These are the attained values U / V, with
 *    the times and the smaller-time tie rule of rule 2 of ntg_batch_extrema.
 * 4. Levels, results, NaN, violation.  Rules 2 to 7 of ntg_batch_extrema, unchanged.  Every polygon of an open piece is halved with
 *    0.5 * (a + b).  npieces counts pieces: l at level 0, two per open piece afterwards.  Every form is certified: there is no status NONE.
 * 5. A form whose terms are all LIN with nent = 1, coef = 1.0, phase = 0 and pp = -1 returns what ntg_batch_forms returns for the linear
 *    terms w (z[u] - 0): ext, when, status and npieces are equal under ==.  That is why the LIN terms share one polygon.
 * Rounding.  With S_i as in ntg_batch_forms for entry i, A_t = |phase_t| + |fprm_b[pp]| + sum_i |coef_i| S_i bounds the angle of term t.  A
 * point of Theta_t carries at most 2^-41 A_t: 2^-42 sum_i |coef_i| S_i from the entries, the elevations and at most 270 halvings the rest
 * (counted as for ntg_batch_forms).  The enclosure of rule 2 is exact mathematics for the polygon it is given, sin and cos have the Lipschitz
 * constant 1, the device sincos is taken at 4 ulp, and the roundings of rule 2 add less than 2^-49 (1 + A_t) per term and 2^-51 A_t^2 for the
 * remainder.  The slack of a form is
 *   slack_j = 2^-39 * sum_t |w_t| (1 + A_t)      for A_t <= 2^11; a term with a larger A_t adds 2^-51 |w_t| A_t^2     (DESIGN.md 2n).
 * Figures are returned as computed; the slack is part of the contract.
 * Arguments.  tol, max_depth and sides as in ntg_batch_extrema.  Stream ordered, without scratch in HBM and without floating-point atomics: a
 * wavefront owns a problem and walks its forms, lane p owns open piece p.  Results are bit-identical from call to call and independent of
 * the batch around a problem.  Per-problem grids are honoured: the batch must be the grids'.
 * batch <= 0 or nform == 0 returns 0 after the checks.  NTG_E_BADARG, naming the form and term where one is at fault, for a null plan, d_x,
 * form_nterms or terms; nform outside 0 .. NTG_TRIG_MAXFORMS; a form with 0 or more than NTG_TRIG_MAXTERMS terms; kind outside 0 .. 2; nent
 * outside 1 .. NTG_TRIG_MAXENT; an entry outside [0, nz); pp outside [-1, nfp); nfp < 0, or a parameter named while d_fprm is null; a
 * non-finite coef, phase or w; tol, max_depth or sides out of range; all six outputs null; violation outputs without both bounds; a batch
 * other than the grids'.  NTG_E_UNSUPPORTED for host-callback plans, for a form that names entries of different basis classes (the message
 * names the form and the two outputs), and for tables and work lists above 158 KiB of LDS: sum over basis classes of l (k^2 + 2) + 1, and
 * per wavefront nC + nfp + 64 (4 KM + 3) doubles, KM = 6 (largest order <= 6) or 10 -- on per-problem grids the class tables count per
 * wavefront too; four wavefronts, two where four do not fit. */
#define NTG_TRIG_MAXFORMS 8
#define NTG_TRIG_MAXTERMS 4      /* per form */
#define NTG_TRIG_MAXENT   4      /* flag entries per angle */
#define NTG_TRIG_SIN 0
#define NTG_TRIG_COS 1
#define NTG_TRIG_LIN 2           /* the angle itself: w * theta */
typedef struct { int kind, nent, pp, pad; int ent[NTG_TRIG_MAXENT]; double coef[NTG_TRIG_MAXENT]; double phase, w; } ntg_trig_term;

int ntg_batch_trig(const ntg_plan *p, int batch, const double *d_x,
                   int nform, const int *form_nterms, const ntg_trig_term *terms,
                   int nfp, const double *d_fprm,
                   double tol, int max_depth, int sides,
                   const double *d_flo, const double *d_fhi,
                   double *d_ext, double *d_when, int *d_status, int *d_npieces,
                   double *d_viol, int *d_where, void *stream);

/* Certified extrema of MIN / MAX EXPRESSIONS over quadratic forms of the flat flag, declared at the call: ntg_batch_forms' statement -- the
 * global minimum and maximum over the horizon, each enclosed to a tolerance and each with a witness time -- for
 *   h_g(t) = OUTER_k INNER_{j in clause k} m_kj(t),   m(t) = q_form(z(t)) + d,   OUTER and INNER each min or max,
 * the regions that several functions describe together.  A convex polygonal obstacle: the trajectory stays outside iff min over t of max_j
 * n_j . (p(t) - v_j) >= 0 (no single face says so: each goes negative far from the polygon).  A rotated box, a lane, a convex corridor: inside
 * iff max over t of max_j (...) <= 0.  A safe corridor of overlapping boxes: max over t of min_k max_j f_kj <= 0.  Coverage by beacons: max over
 * t of min_j (d_j^2 - R_j^2) <= 0.  min and max are monotone: with every member enclosed by [plo_m, phi_m] on a piece, OUTER_k INNER_j over the
 * plo and over the phi enclose h_g there, and its value at a piece end is the same expression over the members' end points, which are attained
 * values.  So ntg_batch_extrema's bisection applies to pieces that carry the polygons of all members.  No family callback runs: every plan is
 * served (built-in families, loaded modules, per-problem grids).
 * Forms are declared exactly as for ntg_batch_forms (form_nterms, terms, nfp, d_fprm: same arrays, same checks, same messages); none of them is
 * certified by itself.  0 <= nform <= NTG_MINMAX_MAXFORMS, at most NTG_FORM_MAXTERMS terms per form and NTG_MINMAX_MAXTERMS = 40 over all forms
 * (40 terms, 16 forms, 32 members and 4 groups are what fits the 4096-byte kernel argument: 3520 bytes).
 * Members and groups.  groups [ngroup] and members are HOST arrays, copied by the call; members is concatenated group after group, clause after
 * clause: group g has nclause clauses of nmem[k] members.  Member m is q_form(z(t)) + d with d = c + (pc >= 0 ? fprm_b[pc] : 0), one rounding.
 * outer and inner are NTG_MINMAX_MIN or NTG_MINMAX_MAX.  All forms named by one group belong to one basis class; different groups may use
 * different classes.  0 <= ngroup <= NTG_MINMAX_MAXGROUPS, 1 <= nclause <= NTG_MINMAX_MAXCLAUSES, nmem[k] >= 1, at most NTG_MINMAX_MAXMEMBERS
 * members per group and 32 over all groups.
 * Outputs, any may be NULL but not all seven; those of ntg_batch_forms with the group in the place of the form:
 *   d_ext     [batch][ngroup][4]  {min_lo, min_hi, max_lo, max_hi}
 *   d_when    [batch][ngroup][2]  {t_min, t_max}
 *   d_which   [batch][ngroup][2]  the member, by its index in the group's concatenated list, that decides h_g at t_min and at t_max: inside a
 *                                 clause the member that attains INNER, ties to the smallest index; among the clauses the clause that attains
 *                                 OUTER, ties to the smallest clause; -1 where the time is NaN
 *   d_status  [batch][ngroup]     NTG_EXTREMA_OK / _DEPTH / _FULL / _NAN
 *   d_npieces [batch][ngroup]     pieces evaluated
 *   d_viol    [batch][2]          {attained, certified}
 *   d_where   [batch][2]          group of each of the two violations; ties to the smallest group; -1 where the figure is 0
 * Definition, per problem and per group.  Every product and every sum is rounded separately (no fused multiply-add).
 * 1. Level 0, knot interval j of the group's class.  A member's polygon is its form's level-0 polygon by step 1 of ntg_batch_forms, bit for
 *    bit.  Then + d is added to every point, with one rounding; a member with pc = -1 and c = 0.0 adds nothing.  Then the polygon is elevated
 *    to the group's degree D_g = max of its members' form degrees, with the formula ntg_batch_envelope states.  A piece carries the polygons
 *    of all members of the group.
 * 2. Piece.  plo_m and phi_m are the smallest and the largest of member m's points.  plo = OUTER_k INNER_j plo_kj and phi = OUTER_k INNER_j
 *    phi_kj: min and max of doubles, exact and independent of the order.  A NaN in any member's figures marks the group as rule 5 of
 *    ntg_batch_extrema does (status NTG_EXTREMA_NAN), before anything else.
 * 3. Ends.  The value at a piece end is OUTER_k INNER_j of the members' first or last points.  These are the attained values U / V, with the
 *    times and the smaller-time tie rule of rule 2 of ntg_batch_extrema.  which is recorded together with the value it belongs to; of two
 *    ends with equal values and equal times the one with the smaller which is kept.
 * 4. Levels, results, NaN, violation.  Rules 2 to 7 of ntg_batch_extrema, unchanged: tol, max_depth, sides, NTG_EXTREMA_CAP and the statuses
 *    OK, DEPTH, FULL and NAN; there is no NONE.  Every polygon of an open piece is halved with 0.5 * (a + b).  npieces counts pieces, not
 *    polygons: l at level 0, two per open piece afterwards.  The bounds are d_glo / d_ghi [batch][ngroup].
 * 5. Pins.  A group of one clause with one member, c = 0.0 and pc = -1, returns what ntg_batch_forms returns for that form: ext, when, status
 *    and npieces are equal under ==.  Repeating that member, as two clauses of one or one clause of two, changes nothing.  With every w and
 *    every c negated, fprm-borne offsets negated by the caller, and MIN and MAX swapped in outer and inner, ext comes back negated with its two
 *    sides exchanged, and when, which, status and npieces with the sides exchanged, under ==: every operation above is odd-symmetric in
 *    round-to-nearest.
 * Rounding.  min and max do not amplify an error: if every member's points are within e_m of the exact polygon's, plo, phi and the end values
 *    are within max_m e_m of the exact figures.  A point of form f carries at most 2^-39 M_f with M_f = sum_t |w_t| S_u S_v (ntg_batch_forms);
 *    forming d and adding it are two roundings, below 2^-52 (M_f + |d|); the at most 18 elevation steps (3 roundings each, convex combinations)
 *    add less than 2^-47 (M_f + |d|).  The slack of a group is
 *      slack_g = max over its members of 2^-39 (M_f + |d|)      (DESIGN.md 2o).
 * Convergence.  Where the extremum sits on a smooth arc of one member, the enclosure closes quadratically in the piece width, as for a form.
 *    Where it sits at a kink -- the minimum of a MAX group generically does, where two faces cross -- it closes only linearly: U - plo is about
 *    slope * width.  Only one or two pieces stay open per level, so the cost stays small, but the depth needed is about log2(h * slope / tol),
 *    h the knot interval.  With max_depth <= 30 a tolerance far below h * slope * 2^-30 ends in status DEPTH: that is the honest answer, and the
 *    enclosure returned is still valid.
 * Arguments.  tol, max_depth and sides as in ntg_batch_extrema.  Stream ordered, without scratch in HBM and without floating-point atomics: a
 * wavefront owns a problem and walks its groups, lane p owns open piece p.  Results are bit-identical from call to call and independent of
 * the batch around a problem.  Per-problem grids are honoured: the batch must be the grids'.
 * batch <= 0 or ngroup == 0 returns 0 after the checks.  The refusals of ntg_batch_forms apply unchanged (with the caps above).  NTG_E_BADARG,
 * naming the group, clause or member at fault, for null groups or members with ngroup > 0; ngroup, nclause, nmem[k], the members of a group or
 * of all groups outside their ranges; a clause with 0 members; outer or inner outside {0, 1}; form outside [0, nform); pc outside [-1, nfp), or
 * pc named while d_fprm is null; a non-finite c; all seven outputs null; violation outputs without both bounds; a batch other than the grids'.
 * NTG_E_UNSUPPORTED for host-callback plans, for a form that names entries of different basis classes, for a group whose forms belong to
 * different basis classes (the message names the group and the two outputs), and for tables and work lists above 158 KiB of LDS even with one
 * wavefront: 3025 product weights, sum over basis classes of l (k^2 + 2) + 1, and per wavefront nC + nfp + 64 (MC * PW + 1) doubles -- MC = 8
 * where no group has more than 8 members, else 16; PW = 7 (largest order <= 6 and every group linear: polygons of 6 points), 11 (largest
 * order <= 6) or 19 -- on per-problem grids the class tables count per wavefront too.  Four wavefronts where four fit, else two, else one;
 * MC = 16 with PW = 19 does not fit even one. */
#define NTG_MINMAX_MIN 0
#define NTG_MINMAX_MAX 1
#define NTG_MINMAX_MAXFORMS   16   /* forms declared at one call */
#define NTG_MINMAX_MAXTERMS   40   /* terms of all forms together; at most NTG_FORM_MAXTERMS per form */
#define NTG_MINMAX_MAXGROUPS   4
#define NTG_MINMAX_MAXCLAUSES  8   /* per group */
#define NTG_MINMAX_MAXMEMBERS 16   /* per group; at most 32 over all groups */
typedef struct { int form, pc; double c; } ntg_minmax_member;
typedef struct { int outer, inner, nclause, pad; int nmem[NTG_MINMAX_MAXCLAUSES]; } ntg_minmax_group;

int ntg_batch_minmax(const ntg_plan *p, int batch, const double *d_x,
                     int nform, const int *form_nterms, const ntg_form_term *terms, int nfp, const double *d_fprm,
                     int ngroup, const ntg_minmax_group *groups, const ntg_minmax_member *members,
                     double tol, int max_depth, int sides,
                     const double *d_glo, const double *d_ghi,
                     double *d_ext, double *d_when, int *d_which, int *d_status, int *d_npieces,
                     double *d_viol, int *d_where, void *stream);

/* The flat-to-state map of the kinematic car for a whole ntg_batch_interp result (examples/kincar.c:68-92 kincar_flat_reverse,
 * called per sample by the example's output loop, kincar.c:392-406): d_z [batch][ntimes][nz] -> d_state [batch][ntimes][ncars][5] =
 * x, y, theta, v, delta for every car (ncars = nout / 2; outputs 2c, 2c+1 are the rear-axle position of car c).  reverse_gear != 0
 * is the reference's dir == 'r'.  kincar-family plans only. */
int ntg_batch_kincar_reverse(const ntg_plan *p, int batch, int ntimes, const double *d_z, double wheelbase, int reverse_gear,
                             double *d_state, void *stream);

/* Receding-horizon step (the warm-start use NPSOL's istate/clambda/R were meant for, ntg.h:64-68):
 * re-pin the linear initial-constraint bounds of every problem to the flat flag of its current
 * solution at breakpoint shift_bp, and shift the coefficients by shift_knots knot intervals
 * (tail = last coefficient) as the next initial guess.  d_x, d_lower, d_upper are updated in place.  After ntg_plan_set_grids: with
 * every problem's own basis blocks (the batch must be the grids'). */
int ntg_batch_mpc_shift(const ntg_plan *p, int batch, int shift_bp, int shift_knots, double *d_x,
                        double *d_lower, double *d_upper, void *stream);

/* nsteps receding-horizon steps (solve, then ntg_batch_mpc_shift) without returning to the caller in between; after the
 * first step the (solve, shift) pair is replayed as a hipGraph.  d_inform [batch] receives the last step's inform,
 * d_notconv [1] (may be NULL; zero it first) accumulates the number of problems whose re-solve did not end with inform 0.
 * With stream == NULL the run uses a private stream and returns when it has finished. */
/* The multiplier part of the receding-horizon step: the estimates of the trajectory rows kept in d_work move shift_bp breakpoints towards the
 * start of the horizon (row (j, i) <- row (j, i + shift_bp), the tail starts at 0), ready for a solve with warm_start = 1.
 * ntg_batch_mpc_run does this itself when the options ask for a warm start; callers that run their own loop call it after
 * ntg_batch_mpc_shift.  No-op for plans without such rows. */
int ntg_batch_mpc_shift_multipliers(const ntg_plan *p, int batch, int shift_bp, const ntg_solve_opts *o, void *d_work, long long work_bytes,
                                    void *stream);

int ntg_batch_mpc_run(const ntg_plan *p, int batch, int nsteps, int shift_bp, int shift_knots, double *d_x,
                      double *d_lower, double *d_upper, const ntg_solve_opts *o, int *d_inform, int *d_notconv,
                      void *d_work, long long work_bytes, void *stream);

/* ntg_open(): everything ntg() does before it calls npsol_ (ntg.c:114-229), with ntg()'s own
 * argument list minus initialguess, the bounds and the outputs; the problem stays current until
 * ntg_close().  For external SQP/IPOPT drivers (Pending:9) that iterate on their own and only need
 * the two callbacks below. */
int ntg_open(
	int nout, double *bps, int nbps, int *kninterv, double **knots, int *order, int *mult, int *max_deriv,
	int nlic, double **lic, int nltc, double **ltc, int nlfc, double **lfc,
	int nnlic, void (*nlicf)(int *, int *, double *, double **, double **),
	int nnltc, void (*nltcf)(int *, int *, int *, double *, double **, double **),
	int nnlfc, void (*nlfcf)(int *, int *, double *, double **, double **),
	int ninitialconstrav, ntg_av *initialconstrav, int ntrajectoryconstrav, ntg_av *trajectoryconstrav,
	int nfinalconstrav, ntg_av *finalconstrav,
	int nicf, void (*icf)(int *, int *, double *, double *, double **),
	int nucf, void (*ucf)(int *, int *, int *, double *, double *, double **),
	int nfcf, void (*fcf)(int *, int *, double *, double *, double **),
	int ninitialcostav, ntg_av *initialcostav, int ntrajectorycostav, ntg_av *trajectorycostav,
	int nfinalcostav, ntg_av *finalcostav);
void ntg_close(void);

/* NPSOL-facing callbacks of the single-problem drop-in (valid while ntg() is running or between
 * ntg_open() and ntg_close()).  Host pointers, Fortran conventions (scalars by pointer),
 * cJac column-major ldJ x n. */
void npsolCostFunction(int *mode, int *n, double *x, double *f, double *g, int *nstate);
void npsolConstraintFunction(int *mode, int *ncnln, int *n, int *ldJ, int *needc, double *x,
                             double *c, double *cJac, int *nstate);

#ifdef __cplusplus
}
#endif
#endif
