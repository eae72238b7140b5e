// hostpath.hip -- the kernels behind ntg_host.cpp, the evaluation of host-callback plans: Z = M C (hostz_kernel: compute_z,
// lds_tables.hpp) and the banded gradient / quadrature pass (hostcost_kernel: cost_phase2, eval.hpp; hostcon_kernel) around functors
// run on the host.
#include <hip/hip_runtime.h>
#include "ntg_dev.hpp"
#include "plan.hpp"
#include "wave_ops.hpp"
#include "lds_tables.hpp"
#include "eval.hpp"

// ------------------------------------------------------------------------------------------
// host-callback path of the ntg() drop-in: the user's C function pointers run on the host
// between two kernels -- updateZ (colloc.c:344-367) and the banded assembly + quadrature.
// ------------------------------------------------------------------------------------------
// Z in the reference layout Z[iZ[o] + d_o*bp + r], iZ[o] = iz[o]*P (colloc.c:328-331); only the
// declared active variables are written (the buffer persists like GZ, ntg.c:119)
template <int NT>
__global__ void __launch_bounds__(NT)
hostz_kernel(NtgDims D, NtgTables T, SmemLayout L, const double *__restrict__ x, u64 maskI, u64 maskT,
             u64 maskF, double *__restrict__ Z)
{
	extern __shared__ __attribute__((aligned(16))) char smem_raw[];
	Smem S(smem_raw, L, D, T);
	stage_tables<NT>(D, T, S, smem_raw, L);
	for (int i = threadIdx.x; i < D.nC; i += NT) S.x[i] = x[i];
	lds_sync();
	for (int i = threadIdx.x; i < D.P; i += NT) {
		const u64 mask = maskT | (i == 0 ? maskI : 0ull) | (i == D.P - 1 ? maskF : 0ull);
		if (!mask) continue;
		double z[NTG_MAX_NZ];
		compute_z<0, 0, 3>(D, S, S.x, i, mask, z);
		for (int o = 0; o < D.nout; o++)
			for (int r = 0; r < D.d[o]; r++)
				if ((mask >> (D.iz[o] + r)) & 1ull) Z[(size_t)D.iz[o] * D.P + (size_t)D.d[o] * i + r] = z[D.iz[o] + r];
	}
}

// fT [P], dfT [P][nz] = what ucf returned at each breakpoint; fdI/fdF [nz+1] = (df, f) of icf/fcf
template <int NT>
__global__ void __launch_bounds__(NT)
hostcost_kernel(NtgDims D, NtgTables T, SmemLayout L, const double *__restrict__ fT,
                const double *__restrict__ dfT, const double *__restrict__ fdI,
                const double *__restrict__ fdF, double *__restrict__ F, double *__restrict__ g)
{
	extern __shared__ __attribute__((aligned(16))) char smem_raw[];
	Smem S(smem_raw, L, D, T);
	stage_tables<NT>(D, T, S, smem_raw, L);
	const int P = D.P, nz = D.nz;
	for (int i = threadIdx.x; i < P; i += NT) S.fvals[i] = D.nucf ? fT[i] : 0.0;
	lds_sync();
	for (int e = threadIdx.x; e < P * nz; e += NT) { const int i = e / nz, v = e % nz; if (D.tav_row[v] >= 0) S.dfz[D.tav_row[v] * (P + 1) + i] = D.nucf ? S.wts[i] * dfT[e] : 0.0; }
	for (int v = threadIdx.x; v <= nz; v += NT) { S.dfi[v] = D.nicf ? fdI[v] : 0.0; S.dff[v] = D.nfcf ? fdF[v] : 0.0; }
	double gn2;
	const double val = cost_phase2<0, 0, NT, 3, 4>(D, S, S.vecs, &gn2, CoefMap<4>(), D.nicf != 0, D.nfcf != 0, 0.0, 0.0, nullptr, nullptr);
	if (threadIdx.x == 0) *F = val;
	for (int i = threadIdx.x; i < D.nC; i += NT) g[i] = S.vecs[i];
}

// dc [ncnln][nz]: row r holds the user's dc[constraint][variable] for constraint row r
// (rows: initial; trajectory constraint-major x breakpoint; final).  One lane per row.
__global__ void hostcon_kernel(NtgDims D, NtgTables T, const double *__restrict__ dc,
                               double *__restrict__ jband, double *__restrict__ cjac)
{
	const int row = blockIdx.x * blockDim.x + threadIdx.x;
	if (row >= D.ncnln) return;
	int bp;
	if (row < D.nnlic) bp = 0;
	else if (row < D.nnlic + D.nnltc * D.P) bp = (row - D.nnlic) % D.P;
	else bp = D.P - 1;
	const double *dcrow = dc + (size_t)row * D.nz;
	for (int o = 0; o < D.nout; o++) {
		const int k = D.order[o], cc = D.cls[o], d = D.d[o];
		const int col0 = D.iC[o] + T.off[cc * D.P + bp];
		for (int q = 0; q < k; q++) {
			double a = 0.0;
			for (int r = 0; r < d; r++) {
				const int chr = T.chrow[cc * NTG_MAX_ORDER + r];
				if (chr >= 0) a += dcrow[D.iz[o] + r] * T.rowv[chr + q * D.P + bp];
			}
			if (jband) jband[(size_t)row * D.sumk + D.koff[o] + q] = a;
			if (cjac) cjac[(size_t)(col0 + q) * D.ncnln + row] = a;
		}
	}
}

hipError_t ntg_launch_hostz(const NtgDims &D, const NtgTables &T, const SmemLayout &L, const double *x, u64 mI,
                            u64 mT, u64 mF, double *Z, hipStream_t st)
{
	auto kfn = hostz_kernel<128>;
	if (L.total > 64 * 1024) (void)hipFuncSetAttribute((const void *)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, L.total);
	hipLaunchKernelGGL(kfn, dim3(1), dim3(128), L.total, st, D, T, L, x, mI, mT, mF, Z);
	return hipGetLastError();
}
hipError_t ntg_launch_hostcost(const NtgDims &D, const NtgTables &T, const SmemLayout &L, const double *fT,
                               const double *dfT, const double *fdI, const double *fdF, double *F, double *g,
                               hipStream_t st)
{
	auto kfn = hostcost_kernel<128>;
	if (L.total > 64 * 1024) (void)hipFuncSetAttribute((const void *)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, L.total);
	hipLaunchKernelGGL(kfn, dim3(1), dim3(128), L.total, st, D, T, L, fT, dfT, fdI, fdF, F, g);
	return hipGetLastError();
}
hipError_t ntg_launch_hostcon(const NtgDims &D, const NtgTables &T, const double *dc, double *jband, double *cjac,
                              hipStream_t st)
{
	if (D.ncnln == 0) return hipSuccess;
	hipLaunchKernelGGL(hostcon_kernel, dim3((D.ncnln + 63) / 64), dim3(64), 0, st, D, T, dc, jband, cjac);
	return hipGetLastError();
}
