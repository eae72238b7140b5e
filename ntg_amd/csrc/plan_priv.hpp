// plan_priv.hpp -- what the host translation units behind include/ntg_amd.h share and nobody else sees: error reporting, the owners
// of device allocations and of stream-ordered scratch, the small algebra used by more than one of them, and the functions one unit offers
// the others.
//   plan.cpp        error handling, device queries, and the calls that are one launch each: eval (and its launch shape), bounds,
//                   kincar_reverse, basis_batch
//   plan_solve.cpp  ntg_batch_solve and the receding-horizon calls; the solve setup (which kernel, which layout, which part of the workspace)
//   plan_times.cpp  the calls at the caller's times: the one builder of the basis tables at the times, ntg_batch_interp, the walk of the
//                   time-tile kernels, ntg_batch_check
//   plan_cost.cpp   ntg_batch_cost: the running cost of a batch at arbitrary times under a quadrature
//   plan_verify.cpp ntg_batch_verify: a family's analytic derivatives against central differences at the breakpoints
//   plan_build.cpp  ntg_plan_create: spec validation, basis classes, channel tables, linear rows; the structured-Newton tables; the
//                   preconditioner; plan queries
//   plan_grids.cpp  per-problem grids (ntg_plan_set_grids) and per-problem family parameters
//   plan_refine.cpp ntg_batch_refine: which pairs of plans it takes, the break conditions on shared grids, the launch
//   plan_kkt.cpp    ntg_batch_kkt: first-order optimality residuals of a batch
//   plan_cert.cpp   the time certificates ntg_batch_envelope, ntg_batch_envelope_sos and ntg_batch_extrema: bounds of the flag entries and
//                   of the trajectory rows that hold over the whole horizon; their common refusals, row tables and kernel arguments
// (layout.cpp and family_registry.cpp are host units too; they need plan.hpp only.)
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <functional>
#include <string>
#include <type_traits>
#include <vector>
#include "ntg_dev.hpp"
#include "plan.hpp"

static inline int fail(int code, const std::string &msg) { return ntg_fail(code, msg); }
#define HIPCHK(x)                                                                                 \
	do {                                                                                          \
		hipError_t e_ = (x);                                                                      \
		if (e_ != hipSuccess) return fail(NTG_E_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); \
	} while (0)

// Owner of device allocations: what it allocated is freed when it goes out of scope, unless handed over (to the plan's list) first.
// A function allocates through one of these, returns on any failure, and hands over on success.
class DevOwner {
	std::vector<void *> ptrs_;
public:
	DevOwner() = default;
	DevOwner(const DevOwner &) = delete;
	DevOwner &operator=(const DevOwner &) = delete;
	DevOwner(DevOwner &&o) noexcept : ptrs_(std::move(o.ptrs_)) { o.ptrs_.clear(); }
	~DevOwner() { free_all(); }
	// n elements, filled from src unless that is null; n == 0 allocates nothing and gives nullptr.  T may be const (a table's field).
	template <class T> int upload(T **dst, const typename std::remove_const<T>::type *src, size_t n)
	{
		*dst = nullptr;
		if (n == 0) return 0;
		HIPCHK(hipMalloc((void **)dst, n * sizeof(T)));
		ptrs_.push_back((void *)*dst);
		if (src) HIPCHK(hipMemcpy((void *)*dst, src, n * sizeof(T), hipMemcpyHostToDevice));
		return 0;
	}
	template <class T> int alloc(T **dst, size_t n) { return upload(dst, nullptr, n); }
	void free_one(const void *q)   // a temporary that is no longer needed
	{
		auto it = std::find(ptrs_.begin(), ptrs_.end(), q);
		if (it != ptrs_.end()) { (void)hipFree(*it); ptrs_.erase(it); }
	}
	void free_all() { for (void *q : ptrs_) (void)hipFree(q); ptrs_.clear(); }
	void release_into(std::vector<void *> &dst) { dst.insert(dst.end(), ptrs_.begin(), ptrs_.end()); ptrs_.clear(); }   // in allocation order
};

// Owner of stream-ordered scratch, DevOwner's counterpart for hipMallocAsync: what it allocated is freed on its stream (hipFreeAsync,
// in allocation order) when it goes out of scope, on every path.  The frees are ordered behind the work already on the stream; a user
// that has to wait for that work (the host reads a result, or the work reads host memory) synchronises the stream itself.
class StreamScratch {
	static constexpr int CAP = 4;   // buffers of one owner (the most a user has: 3); a fixed array: no heap allocation per call
	hipStream_t st_;
	void *ptrs_[CAP];
	int n_ = 0;
public:
	explicit StreamScratch(hipStream_t st) : st_(st) {}
	StreamScratch(const StreamScratch &) = delete;
	StreamScratch &operator=(const StreamScratch &) = delete;
	~StreamScratch() { for (int i = 0; i < n_; i++) (void)hipFreeAsync(ptrs_[i], st_); }
	// n elements; on failure *dst is null and nothing is owned
	template <class T> hipError_t alloc(T **dst, size_t n)
	{
		const hipError_t e = n_ < CAP ? hipMallocAsync((void **)dst, n * sizeof(T), st_) : hipErrorOutOfMemory;
		if (e == hipSuccess) ptrs_[n_++] = (void *)*dst; else *dst = nullptr;
		return e;
	}
};

// ---------------- small algebra with more than one user ----------------
bool chol_lower(std::vector<double> &a, int n);                      // row-major, in place; false: not positive definite
void chol_solve(const std::vector<double> &L, int n, double *b);

// Compressed rows of a dense row-major matrix with nc columns, exact zeros dropped.  Row i is row sel[i] of A (sel null: row i).  By
// rows (CSR: idx = column) or by columns (CSC: idx = position of the row in sel).  nnz counts the entries; an empty pattern gets one
// dummy entry (index 0, value 0.0) behind it so that the device arrays exist.
struct Sparse { std::vector<int> ptr, idx; std::vector<double> val; int nnz = 0; };
Sparse dense_to_csr(const double *A, int nr, int nc, const int *sel = nullptr);
Sparse dense_to_csc(const double *A, int nr, int nc, const int *sel = nullptr);

// linear row r of the stacked rows [nlic | nltc x P | nlfc] (ntg.c:156): the user's row slot (0 .. nlic + nltc + nlfc) and its breakpoint
struct LinRow { int slot, bp; };
static inline LinRow lin_row(const NtgDims &D, int r)
{
	if (r < D.nlic) return {r, 0};
	if (r < D.nlic + D.nltc * D.P) return {D.nlic + (r - D.nlic) / D.P, (r - D.nlic) % D.P};
	return {D.nlic + D.nltc + (r - D.nlic - D.nltc * D.P), D.P - 1};
}

// trapezoid weight of breakpoint i
static inline double trap_weight(const double *bps, int i, int P)
{
	double w = 0.0;
	if (i > 0) w += (bps[i] - bps[i - 1]) / 2;
	if (i < P - 1) w += (bps[i + 1] - bps[i]) / 2;
	return w;
}

// The cost terms a Hessian model sums over: add(active variables, breakpoint, weight) for the running cost at every breakpoint
// (scale x trapezoid weight), the initial cost and the final cost (scale), in this order.
template <class F> static inline void for_cost_terms(const ntg_plan *p, const double *bps, double scale, F add)
{
	const NtgDims &D = p->D;
	for (int i = 0; i < D.P; i++) { const double w = trap_weight(bps, i, D.P); if (D.nucf) add(p->tcostav, i, scale * w); }
	if (D.nicf) add(p->icostav, 0, scale);
	if (D.nfcf) add(p->fcostav, D.P - 1, scale);
}

// H0 += w m m' for derivative r of one output at one breakpoint: b = its [k][d] basis block, base = index of the block's first coefficient in H0
static inline void h0_add(std::vector<double> &H0, int nb, int base, const double *b, int k, int d, int r, double w)
{
	for (int q1 = 0; q1 < k; q1++) for (int q2 = 0; q2 < k; q2++) H0[(size_t)(base + q1) * nb + base + q2] += w * b[q1 * d + r] * b[q2 * d + r];
}

// first output that uses preconditioner block q (NtgDims::n0_blk), -1: none
static inline int block_output(const NtgDims &D, int q)
{
	for (int o = 0; o < D.nout; o++) if (D.n0_blk[o] == q) return o;
	return -1;
}

// ---------------- between the units ----------------
// W0 = Z (Z' H0 Z)^-1 Z' of one block; 0, an error code, or 1: H0 is singular on null(A)  (plan_build.cpp)
int precond_block(const std::vector<double> &H0, const std::vector<double> &A, int m, int n, std::vector<double> &W0);
int build_precond(ntg_plan *p);   // the caller holds ntg_plan::precond_mutex
int plan_ncu(const ntg_plan *p);   // compute units of the plan's device (plan.cpp)
// workgroup size of the evaluation, and of the solve unless the options or the structured Newton mode ask for another: breakpoints and
// coefficients are spread over the lanes
static inline int auto_threads(const NtgDims &D) { return (D.P <= 128 && D.nC <= 512) ? 128 : (D.nC <= 1024 ? 256 : 512); }
// per-problem family parameters (plan_grids.cpp): doubles per problem the plan's family needs; are they set, for this batch?
int param_count(const ntg_plan *p);
int check_params(const ntg_plan *p, int batch);
// launch shape of the evaluation of `batch` problems: workgroup size, persistent grid, LDS layout; 0 or an error code  (plan.cpp)
struct EvalShape { int nt, grid; SmemLayout L; };
int eval_shape(const ntg_plan *p, int batch, EvalShape *s);
// ---- the calls at the caller's times (plan_times.cpp) ----
// The builder of the time tables: basis_kernel's output at the times in stream-ordered scratch that it owns and releases when it returns;
// use() once per chunk of problems with the chunk's tables by value (TimeTables, ntg_dev.hpp).  Shared grid: one set of tables, one
// chunk.  Per-problem grids: chunks whose tables stay under scratch_cap bytes, at least one problem each.  The one cap of every call:
#define NTG_TIME_SCRATCH_CAP (64ll << 20)
hipError_t time_tables_walk(const ntg_plan *p, int batch, int ntimes, const double *d_times, long long times_stride, long long scratch_cap,
                            hipStream_t st, const std::function<hipError_t(const TimeTables &)> &use);
// The calls on time tiles (ntg_batch_check, ntg_batch_cost, ntg_batch_verify): what they refuse about the batch, the stride, the
// parameters and the LDS; the walk over the builder's chunks, launch() once per chunk; and their common tail: the walk, the final
// kernel behind it (the walk's tables are released before it is enqueued), and what the call returns.
//   a     the tile fields of the call's arguments: the caller set x and st, the walk fills the rest before every launch
//   what  the call's name in the refusal of a shape without an instance
//   e     the outcome of the caller's own allocations: a failure skips the walk and is reported like one of its own
int time_args_check(const ntg_plan *p, int batch, int ntimes, long long times_stride);
hipError_t time_tile_walk(const ntg_plan *p, int batch, int ntimes, const double *d_times, long long times_stride, long long scratch_cap,
                          CheckArgs &a, const std::function<hipError_t()> &launch);
template <class Launch, class Finish>
static inline int time_tile_run(const ntg_plan *p, const char *what, hipError_t e, int batch, int ntimes, const double *d_times, long long times_stride,
                                long long scratch_cap, CheckArgs &a, Launch launch, Finish finish)
{
	if (e == hipSuccess) e = time_tile_walk(p, batch, ntimes, d_times, times_stride, scratch_cap, a, launch);
	if (e == hipSuccess) e = finish();
	if (e == hipErrorInvalidValue) return fail(NTG_E_UNSUPPORTED, std::string("the plan's family has no ") + what + " instance for this shape");
	if (e != hipSuccess) return fail(NTG_E_HIP, hipGetErrorString(e));
	return 0;
}
