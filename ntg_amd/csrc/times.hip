// times.hip -- the small kernels of the calls that sample a trajectory at times (plan_times.cpp, plan_cost.cpp, plan_verify.cpp) and
// their launchers: interp_kernel (ntg_batch_interp), the last steps of the three time-tile reductions -- check_final_kernel,
// cost_final_kernel, verify_final_kernel, whose kernels are instantiated per family from check.hpp, cost.hpp and verify.hpp -- and
// kincar_reverse_kernel, the flat-to-state map applied to an interp result.
#include <hip/hip_runtime.h>
#include <math.h>
#include "ntg_dev.hpp"
#include "plan.hpp"
#include "verify.hpp"

// SplineInterp (colloc.c:449-484) for a batch: the flat flag of problems [b0, b0 + nb) at ntimes points in time each.  The tables of a.t
// come from basis_kernel run on the times instead of the breakpoints (TimeTables, ntg_dev.hpp): indexed by the problem within the chunk,
// x and z by the problem of the batch.  One thread per (problem, time, flag entry), consecutive threads = consecutive flag entries of
// one time.
__global__ void interp_kernel(NtgDims D, InterpArgs a)
{
	const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	const int ntimes = a.ntimes;
	if (idx >= (long long)a.t.nb * ntimes * D.nz) return;
	const int v = (int)(idx % D.nz), t = (int)((idx / D.nz) % ntimes), bl = (int)(idx / ((long long)D.nz * ntimes)), b = a.t.b0 + bl;
	int o = 0;
	while (o + 1 < D.nout && D.iz[o + 1] <= v) o++;
	const int r = v - D.iz[o], c = D.cls[o], kk = D.order[o], d = D.d[o];
	const double *blk = a.t.tblk + (a.t.pp ? (size_t)bl * a.t.pp_tab : (size_t)a.t.gbase[c]) + ((size_t)t * kk) * d;
	const double *cx = a.x + (size_t)b * D.nC + D.iC[o] + a.t.toff[(a.t.pp ? (size_t)bl : (size_t)c) * ntimes + t];
	double acc = 0.0;
	for (int q = 0; q < kk; q++) acc += blk[q * d + r] * cx[q];   // colloc.c:476-481
	a.z[((size_t)b * ntimes + t) * D.nz + v] = acc;
}

hipError_t ntg_launch_interp(const NtgDims &D, const InterpArgs &a, hipStream_t st)
{
	const long long total = (long long)a.t.nb * a.ntimes * D.nz;
	if (total == 0) return hipSuccess;
	hipLaunchKernelGGL(interp_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, D, a);
	return hipGetLastError();
}

// ntg_batch_check, last step: the maximum over a problem's time tiles (check_kernel left one (violation, key) pair per tile; key = row *
// ntimes + time index, -1: none).  Equal violations: the smaller key.  One thread per problem, tiles in order.
__global__ void check_final_kernel(int batch, int ntiles, int ntimes, const double *__restrict__ pviol, const long long *__restrict__ pkey,
                                   double *__restrict__ viol, int *__restrict__ where)
{
	const int b = blockIdx.x * blockDim.x + threadIdx.x;
	if (b >= batch) return;
	double bv = 0.0; long long bk = -1;
	for (int i = 0; i < ntiles; i++) {
		const double v = pviol[(size_t)b * ntiles + i]; const long long k = pkey[(size_t)b * ntiles + i];
		if (v > bv || (v == bv && k >= 0 && (bk < 0 || k < bk))) { bv = v; bk = k; }
	}
	if (viol) viol[b] = bv;
	if (where) { where[2 * b] = bk < 0 ? -1 : (int)(bk / ntimes); where[2 * b + 1] = bk < 0 ? -1 : (int)(bk % ntimes); }
}
hipError_t ntg_launch_check_final(int batch, int ntiles, int ntimes, const double *pviol, const long long *pkey, double *viol, int *where, hipStream_t st)
{
	hipLaunchKernelGGL(check_final_kernel, dim3((batch + 127) / 128), dim3(128), 0, st, batch, ntiles, ntimes, pviol, pkey, viol, where);
	return hipGetLastError();
}

// ntg_batch_cost, last step: the sum over a problem's time tiles (cost_kernel left one weighted partial sum per tile).  One thread per
// problem, tiles in order.
__global__ void cost_final_kernel(int batch, int ntiles, const double *__restrict__ pcost, double *__restrict__ cost)
{
	const int b = blockIdx.x * blockDim.x + threadIdx.x;
	if (b >= batch) return;
	double s = pcost[(size_t)b * ntiles];
	for (int i = 1; i < ntiles; i++) s += pcost[(size_t)b * ntiles + i];
	cost[b] = s;
}
hipError_t ntg_launch_cost_final(int batch, int ntiles, const double *pcost, double *cost, hipStream_t st)
{
	hipLaunchKernelGGL(cost_final_kernel, dim3((batch + 127) / 128), dim3(128), 0, st, batch, ntiles, pcost, cost);
	return hipGetLastError();
}

// ntg_batch_verify, last step: the maximum over a problem's breakpoint tiles (verify_kernel left one (value, key) pair per tile, slot and kind),
// tiles in order under verify_take's total order, and the key taken apart into {function, breakpoint, flag entry}.  One thread per problem
// and (slot, kind); kind 0 goes to err / where, kind 1 to leak / leak_where, each of which may be null.
__global__ void verify_final_kernel(int batch, int ntiles, int nbps, int nz, const double *__restrict__ pval, const long long *__restrict__ pkey,
                                    double *__restrict__ err, int *__restrict__ where, double *__restrict__ leak, int *__restrict__ leak_where)
{
	constexpr int NQ = 2 * NTG_VERIFY_NSLOT;
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= batch * NQ) return;
	const int b = i / NQ, q = i - b * NQ, slot = q >> 1, kind = q & 1;
	double bv = pval[(size_t)b * ntiles * NQ + q]; long long bk = pkey[(size_t)b * ntiles * NQ + q];
	for (int t = 1; t < ntiles; t++) verify_take(bv, bk, pval[((size_t)b * ntiles + t) * NQ + q], pkey[((size_t)b * ntiles + t) * NQ + q]);
	double *ov = kind ? leak : err; int *ow = kind ? leak_where : where;
	const size_t o = (size_t)b * NTG_VERIFY_NSLOT + slot;
	if (ov) ov[o] = bv;
	if (ow) {
		const long long pt = bk >= 0 ? bk / nz : -1;
		ow[3 * o] = bk >= 0 ? (int)(pt / nbps) : -1; ow[3 * o + 1] = bk >= 0 ? (int)(pt % nbps) : -1; ow[3 * o + 2] = bk >= 0 ? (int)(bk % nz) : -1;
	}
}
hipError_t ntg_launch_verify_final(int batch, int ntiles, int nbps, int nz, const double *pval, const long long *pkey, double *err, int *where, double *leak,
                                   int *leak_where, hipStream_t st)
{
	const long long n = (long long)batch * 2 * NTG_VERIFY_NSLOT;
	hipLaunchKernelGGL(verify_final_kernel, dim3((unsigned)((n + 127) / 128)), dim3(128), 0, st, batch, ntiles, nbps, nz, pval, pkey, err, where, leak, leak_where);
	return hipGetLastError();
}

// Flat flag -> state and input of the kinematic car, the map of examples/kincar.c:68-92 (kincar_flat_reverse), for every car
// of every problem at every time of an ntg_batch_interp result: z [n][nz] with the flag of car c at entries 6 c .. 6 c + 5
// (x, x', x'', y, y', y'') -> out [n][ncars][5] = x, y, theta, v, delta.  One thread per (sample, car).
__global__ void kincar_reverse_kernel(long long nsamp, int nz, int ncars, double wheelbase, int reverse_gear,
                                      const double *__restrict__ z, double *__restrict__ out)
{
	const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (idx >= nsamp * ncars) return;
	const long long smp = idx / ncars; const int c = (int)(idx - smp * ncars);
	const double *f = z + smp * nz + 6 * c;
	const double xd = f[1], xdd = f[2], yd = f[4], ydd = f[5];
	const double th = reverse_gear ? atan2(-yd, -xd) : atan2(yd, xd);   // kincar.c:78-86
	double sn, cs;
	sincos(th, &sn, &cs);
	const double thdot_v = ydd * cs - xdd * sn, v = xd * cs + yd * sn;   // kincar.c:89-90
	double *o = out + idx * 5;
	o[0] = f[0]; o[1] = f[3]; o[2] = th; o[3] = v; o[4] = atan2(thdot_v, v * v / wheelbase);   // kincar.c:91 (pow(u[0], 2.0) / b)
}
hipError_t ntg_launch_kincar_reverse(long long nsamp, int nz, int ncars, double wheelbase, int reverse_gear, const double *z, double *out, hipStream_t st)
{
	const long long total = nsamp * ncars;
	if (total == 0) return hipSuccess;
	hipLaunchKernelGGL(kincar_reverse_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, nsamp, nz, ncars, wheelbase, reverse_gear, z, out);
	return hipGetLastError();
}
