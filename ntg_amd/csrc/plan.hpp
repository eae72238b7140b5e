// plan.hpp -- the plan object behind include/ntg_amd.h and the launcher prototypes.
#pragma once
#include <hip/hip_runtime.h>
#include <vector>
#include <mutex>
#include <string>
#include "ntg_dev.hpp"
#include "refine.hpp"

struct ntg_plan {
	int device = 0;
	int *d_pfidx = nullptr, *d_pbinfo = nullptr; int prec_dev = -1, prec_nrmax = 0;   // device path of the per-problem preconditioner blocks: tables, applicability (-1: not decided)
	double *d_grid_knots = nullptr;   // per-problem grids: device copy of the knots [grid_batch][ninterv + 1] (ntg_batch_interp)
	mutable int ncu = 0;                        // compute units of the device (queried on first use)
	NtgDims D;
	NtgTables T;
	bool lin_ok = true;
	std::mutex precond_mutex;                   // guards the lazy build of the preconditioner
	bool precond_ready = false;                 // W0 tables (T.n0 or T.n0b) built
	bool precond_singular = false;              // the cost Hessian model is singular on null(A_E): hessian = 1 falls back to the identity
	std::vector<void *> owned;                  // device allocations
	std::vector<std::vector<double>> h_knots;   // host mirrors of the setup tables
	std::vector<double> h_bps, h_blk, h_aband, h_Adense, h_AE;   // h_Adense: all linear rows; h_AE: the equality rows
	std::vector<int> h_off, h_rbp, class_rep;
	std::vector<ntg_av> icostav, tcostav, fcostav;
	// host copies of the shared index tables (per-problem grids recompute the values behind them)
	std::vector<int> h_chrow, h_csr_ptr, h_csr_col, h_csc_ptr, h_csc_row, h_sinv_ptr, h_sinv_col, h_erow, h_qcol;
	std::vector<int> h_irow, h_icsr_ptr, h_icsr_col, h_icsc_ptr, h_icsc_row;   // ... and of the linear inequality rows (nI > 0)
	std::vector<short> h_qidx;
	std::vector<double> h_linrows;              // the user's linear rows, stacked [nlic | nltc | nlfc][nz]
	// per-problem grids (ntg_plan_set_grids): number of problems they were set for (0: shared grid), their device arrays
	int grid_batch = 0;
	std::vector<void *> grid_owned;
	NtgTables T_shared;                         // the tables of the shared grid, restored by ntg_plan_clear_grids
	double *d_lic = nullptr;                    // [nlic][nz] kept for the receding-horizon shift
	double *d_ltc = nullptr;                    // [nltc][nz] kept for ntg_batch_check
	// per-problem grids on the device (grids.hip): the user's linear rows stacked [nclin][nz], row -> coefficient map and padding mask of
	// the projector's ELL pattern, the plan's block offsets; the plan's own projector values (host) to tell padding from pattern
	double *d_linrows = nullptr; int *d_qrow2coef = nullptr, *d_planoff = nullptr, *d_erow = nullptr; unsigned char *d_qpad = nullptr;
	std::vector<double> h_qval;
	std::vector<double *> d_knots;              // break sequence of every basis class (ntg_batch_interp)
	// per-problem family parameters (ntg_plan_set_params): the plan's own buffer [prm_batch][prm_n] (prm_cap doubles allocated), the batch
	// they were set for (0: none); NtgTables::prm / pp_prm point into it (ntg_plan_clear_grids puts them back after restoring the tables)
	double *d_prm = nullptr; size_t prm_cap = 0; int prm_batch = 0, prm_n = 0;
};

void ntg_plan_dense_A(const ntg_plan *p, double *A);
// sets the message ntg_last_error() returns (this thread), returns code
int ntg_fail(int code, const std::string &msg);

// ---- layout.cpp: the LDS carve-up, tables + (with_x) the coefficient vector + nvec further vectors of nC doubles ----
//   eval_kernel   nvec 0 (the gradient is assembled into the x buffer once x is no longer needed)
//   host path     nvec 1
//   sqp_kernel    nvec 5 (xt, gp, gp+, d, g) with x -- or, BIG, nvec 1 (xt) without x: the rest lives in HBM/L2
SmemLayout ntg_make_layout(const NtgDims &D, int nthreads, int nvec, int with_x, int hrc_pairs = 0, int qp = 0);

// ---- family_registry.cpp: the family's instance of eval_kernel, sqp_kernel and the three time-tile kernels (check.hpp, cost.hpp,
// verify.hpp), through its descriptor; hipErrorInvalidValue: no such family, or no instance for this shape ----
hipError_t ntg_launch_eval(const NtgDims &D, const NtgTables &T, const SmemLayout &L, const EvalArgs &a);
hipError_t ntg_launch_sqp(const NtgDims &D, const NtgTables &T, const SmemLayout &L, const SolveParams &sp, const SqpArgs &a);
hipError_t ntg_launch_check(const NtgDims &D, const NtgTables &T, const CheckArgs &a);
hipError_t ntg_launch_cost(const NtgDims &D, const NtgTables &T, const CostArgs &a);
hipError_t ntg_launch_verify(const NtgDims &D, const NtgTables &T, const VerifyArgs &a);

// ---- fam_kincar_wave.hip: one wavefront per problem (solve_wave.hpp): does it take this solve, and its launch shape / HBM workspace ----
struct NtgWavePlan { int fat, nwv, grid, cap, hbm_slots, nlds, ppg, noagpr; size_t lds, hist_doubles; };   // ppg: per-problem grids (wave-private value tables)
bool ntg_wave_plan(const NtgDims &D, const NtgTables &T, const SolveParams &sp, int batch, int ncu, NtgWavePlan *w);
hipError_t ntg_launch_sqp_wave(const NtgDims &D, const NtgTables &T, const SolveParams &sp, const SqpArgs &a, const NtgWavePlan &w);

// ---- basis.hip: the basis at the breakpoints (or a caller's times) of ngrids grids, the banded linear rows, bounds() ----
hipError_t ntg_launch_basis(int ngrids, int l, int k, int m, int d, int P, const double *knots, const double *bps,
                            long long knots_stride, long long bps_stride, double *blk, int *off, hipStream_t st);
hipError_t ntg_launch_linrows(const NtgDims &D, const NtgTables &T, const double *lic, const double *ltc,
                              const double *lfc, double *aband, int *rbp, hipStream_t st);
hipError_t ntg_launch_bounds(const NtgDims &D, int batch, const double *lo, const double *up, double *bl, double *bu,
                             hipStream_t st);

// ---- hostpath.hip: the kernels around the host callbacks of ntg() (ntg_host.cpp) ----
hipError_t ntg_launch_hostz(const NtgDims &D, const NtgTables &T, const SmemLayout &L, const double *x, u64 mI,
                            u64 mT, u64 mF, double *Z, hipStream_t st);
hipError_t ntg_launch_hostcost(const NtgDims &D, const NtgTables &T, const SmemLayout &L, const double *fT,
                               const double *dfT, const double *fdI, const double *fdF, double *F, double *g,
                               hipStream_t st);
hipError_t ntg_launch_hostcon(const NtgDims &D, const NtgTables &T, const double *dc, double *jband, double *cjac,
                              hipStream_t st);

// ---- times.hip: the flat flag at times (one chunk of problems), the last step of each time-tile reduction over a problem's tiles, the
// kinematic car's flat-to-state map ----
hipError_t ntg_launch_interp(const NtgDims &D, const InterpArgs &a, hipStream_t st);
hipError_t ntg_launch_check_final(int batch, int ntiles, int ntimes, const double *pviol, const long long *pkey, double *viol, int *where, hipStream_t st);
hipError_t ntg_launch_cost_final(int batch, int ntiles, const double *pcost, double *cost, hipStream_t st);
hipError_t ntg_launch_verify_final(int batch, int ntiles, int nbps, int nz, const double *pval, const long long *pkey, double *err, int *where, double *leak,
                                   int *leak_where, hipStream_t st);
hipError_t ntg_launch_kincar_reverse(long long nsamp, int nz, int ncars, double wheelbase, int reverse_gear, const double *z, double *out, hipStream_t st);

// ---- mpc.hip: the receding-horizon shift of coefficients and bounds, of the multiplier estimates, and the count of unconverged problems ----
hipError_t ntg_launch_mpc_shift(const NtgDims &D, const NtgTables &T, int batch, int sbp, int sknot, const double *lic,
                                double *x, double *lower, double *upper, hipStream_t st);
hipError_t ntg_launch_mpc_shift_lambda(const NtgDims &D, int batch, int sbp, double *alw, hipStream_t st);
hipError_t ntg_launch_count_notconv(int batch, const int *inform, int *count, hipStream_t st);

// ---- certs.hip: the kernels written once for every family -- the time certificates (envelope.hpp, envelope_sos.hpp, extrema.hpp,
// separation.hpp, forms.hpp), refine (refine.hpp; pp: per-problem grids) and one chunk of kkt (kkt.hpp, after ntg_launch_eval in mode 2
// and ntg_launch_bounds filled its scratch); hipErrorInvalidValue: the tables exceed the LDS ----
hipError_t ntg_launch_envelope(const EnvArgs &A, int ncu, hipStream_t st);
hipError_t ntg_launch_envelope_sos(const SosArgs &A, int ncu, hipStream_t st);
hipError_t ntg_launch_extrema(const ExtArgs &A, int ncu, hipStream_t st);
hipError_t ntg_launch_separation(const SepArgs &A, int ncu, hipStream_t st);
hipError_t ntg_launch_forms(const FormArgs &A, int ncu, hipStream_t st);
hipError_t ntg_launch_refine(const RefineArgs &A, int pp, int ncu, hipStream_t st);
hipError_t ntg_launch_kkt(const NtgDims &D, const NtgTables &T, const KktArgs &a);

// ---- ratios.hip: minimum and maximum over the horizon of ratios of products of forms, by the certificates' bisection on pairs of
// polygons (ratios.hpp) ----
hipError_t ntg_launch_ratios(const RatioArgs &A, int ncu, hipStream_t st);

// ---- trig.hip: minimum and maximum over the horizon of sums of sines and cosines of the flag, by the certificates' bisection on pieces
// of several angle polygons (trig.hpp) ----
hipError_t ntg_launch_trig(const TrigArgs &A, int ncu, hipStream_t st);

// ---- minmax.hip: minimum and maximum over the horizon of min / max expressions over declared forms, by the certificates' bisection on
// pieces that carry the polygons of all members of a group (minmax.hpp) ----
hipError_t ntg_launch_minmax(const MinmaxArgs &A, int ncu, hipStream_t st);

// ---- grids.hip: per-problem grids, the device-side setup algebra ----
struct NtgGridLin {
	const double *blk, *linrows; const int *plan_off, *erow, *csr_ptr, *csr_col, *csc_ptr, *csc_row, *sinv_ptr, *sinv_col, *q_col, *q_row2coef;
	const unsigned char *q_pad; double *csr_val, *csc_val, *sinv_val, *q_val; int *err;
};
hipError_t ntg_launch_grid_rows(const NtgDims &D, int batch, const double *blk, const int *off, const int *plan_off, double *rowv, int *err, hipStream_t st);
hipError_t ntg_launch_grid_lin(const NtgDims &D, int batch, const NtgGridLin &g, hipStream_t st);
// the linear inequality rows' values on the plan's CSR / CSC patterns, every grid (grids.hip, grid_ilin_kernel); inz: entries of one problem
struct NtgGridILin {
	const double *blk, *linrows; const int *plan_off, *irow, *icsr_ptr, *icsr_col, *icsc_ptr, *icsc_row; double *icsr_val, *icsc_val; int *err; int inz;
};
hipError_t ntg_launch_grid_ilin(const NtgDims &D, int batch, const NtgGridILin &g, hipStream_t st);
// preconditioner blocks of every grid on the device (grids.hip, grid_prec_kernel)
struct NtgGridPrec { const double *blk, *bps; const int *plan_off, *fidx, *binfo; double *n0b; int *err; int nblk, nb, spad, n0b_sz, nrmax; };
hipError_t ntg_launch_grid_prec(const NtgDims &D, int batch, const NtgGridPrec &g, hipStream_t st);
// structured Newton mode on per-problem grids: cost model (band, every coupling group; two-sided layout where the plan uses it) and the free
// outputs' band factors of every grid, from the per-problem channel rows and breakpoints
struct NtgGridNwt { const double *rowv, *bps; const int *plan_off; const short *lo, *hi; double *k0, *lf; int *err; int k0_sz, lf_sz; };
hipError_t ntg_launch_grid_nwt(const NtgDims &D, int batch, const NtgGridNwt &g, hipStream_t st);
