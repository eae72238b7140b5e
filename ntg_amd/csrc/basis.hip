// basis.hip -- the setup kernels of a plan and their launchers:
//   basis_kernel    PGS knots/interv/bsplvb/bsplvd at every collocation point (reference call sites colloc.c:92-111; the Fortran is
//                   absent from the reference tree, algorithm from de Boor's PGS).  The same kernel gives the basis at a caller's
//                   times (plan_times.cpp) and at the breakpoints of many grids (ntg_basis_batch, plan_grids.cpp).
//   linrows_kernel  banded rows of the linear-constraint matrix (constraints.c:198-261)
//   bounds_kernel   bounds() (constraints.c:5-33)
#include <hip/hip_runtime.h>
#include "ntg_dev.hpp"
#include "plan.hpp"

// ------------------------------------------------------------------------------------------
// PGS on the device.  The augmented knot vector is never materialised: t(idx) is read through
// the break sequence (knots(): first/last break k times, interior breaks k-m times).
// ------------------------------------------------------------------------------------------
struct AugKnots {
	const double *brk; int l, k, m;
	__device__ __forceinline__ double operator()(int idx1) const // 1-based like the Fortran
	{
		const int idx = idx1 - 1, n = l * (k - m) + m;
		if (idx < k) return brk[0];
		if (idx >= n) return brk[l];
		return brk[1 + (idx - k) / (k - m)];
	}
};

// interv on the break sequence (2nd-edition rule at the right end), 1-based interval index
__device__ __forceinline__ int interv_breaks(const double *brk, int l, double x)
{
	const int lxt = l + 1;
	if (x < brk[0]) return 1;
	if (x >= brk[lxt - 1]) {
		for (int i = lxt - 1; i >= 1; i--)
			if (brk[i - 1] < brk[lxt - 1]) return i;
		return 1;
	}
	int lo = 1, hi = lxt;
	while (hi - lo > 1) {
		const int mid = (lo + hi) >> 1;
		if (x >= brk[mid - 1]) lo = mid; else hi = mid;
	}
	return lo;
}

// bsplvb/bsplvd (PGS).  db is [nderiv][k] (m-major) == Fortran dbiatx(k,nderiv) column-major.
__device__ void bsplvd_dev(const AugKnots &t, int k, double x, int left, int nderiv, double *db)
{
	double a[NTG_MAX_ORDER * NTG_MAX_ORDER];
	double deltal[NTG_MAX_ORDER], deltar[NTG_MAX_ORDER];
	int j = 1;
	const int mhigh = max(min(nderiv, k), 1), kp1 = k + 1;
#define DB(r, c) db[((c) - 1) * k + ((r) - 1)]
#define A_(r, c) a[((c) - 1) * k + ((r) - 1)]
	auto raise = [&](int jhigh, double *biatx) {
		while (j < jhigh) {
			const int jp1 = j + 1;
			deltar[j - 1] = t(left + j) - x;
			deltal[j - 1] = x - t(left + 1 - j);
			double saved = 0.0;
			for (int i = 1; i <= j; i++) {
				const double term = biatx[i - 1] / (deltar[i - 1] + deltal[jp1 - i - 1]);
				biatx[i - 1] = saved + deltar[i - 1] * term;
				saved = deltal[jp1 - i - 1] * term;
			}
			biatx[jp1 - 1] = saved;
			j = jp1;
		}
	};
	db[0] = 1.0;
	raise(kp1 - mhigh, db);
	if (mhigh == 1) return;
	int ideriv = mhigh;
	for (int m = 2; m <= mhigh; m++) {
		int jp1mid = 1;
		for (int jj = ideriv; jj <= k; jj++) { DB(jj, ideriv) = DB(jp1mid, 1); jp1mid++; }
		ideriv--;
		raise(kp1 - ideriv, db);
	}
	int jlow = 1;
	for (int i = 1; i <= k; i++) {
		for (int jj = jlow; jj <= k; jj++) A_(jj, i) = 0.0;
		jlow = i;
		A_(i, i) = 1.0;
	}
	for (int m = 2; m <= mhigh; m++) {
		const int kp1mm = kp1 - m;
		const double fkp1mm = (double)kp1mm;
		int il = left, i = k;
		for (int ld = 1; ld <= kp1mm; ld++) {
			const double factor = fkp1mm / (t(il + kp1mm) - t(il));
			for (int jj = 1; jj <= i; jj++) A_(i, jj) = (A_(i, jj) - A_(i - 1, jj)) * factor;
			il--; i--;
		}
		for (i = 1; i <= k; i++) {
			double sum = 0.0;
			const int jl = i > m ? i : m;
			for (int jj = jl; jj <= k; jj++) sum = A_(jj, i) * DB(jj, m) + sum;
			DB(i, m) = sum;
		}
	}
#undef DB
#undef A_
}

// one thread per (grid, breakpoint); the grid's break sequence is staged in LDS
__global__ void basis_kernel(int ngrids, int l, int k, int m, int d, int P,
                             const double *__restrict__ knots, const double *__restrict__ bps,
                             long long knots_stride, long long bps_stride,
                             double *__restrict__ blk, int *__restrict__ off)
{
	extern __shared__ __attribute__((aligned(16))) char smem_raw[];
	double *sbrk = reinterpret_cast<double *>(smem_raw);
	const int g = blockIdx.y;
	if (g >= ngrids) return;
	for (int i = threadIdx.x; i <= l; i += blockDim.x) sbrk[i] = knots[g * knots_stride + i];
	__syncthreads();
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= P) return;
	const double x = bps[g * bps_stride + i];
	const int ivl = interv_breaks(sbrk, l, x);        // colloc.c:107 on the un-augmented knots
	const int left = k + (ivl - 1) * (k - m);         // == interv_ on the augmented knots (colloc.c:98)
	AugKnots t{sbrk, l, k, m};
	double db[NTG_MAX_ORDER * NTG_MAX_ORDER];
	bsplvd_dev(t, k, x, left, d, db);
	double *o = blk + ((size_t)g * P + i) * k * d;
	for (int q = 0; q < k; q++)
		for (int r = 0; r < d; r++) o[q * d + r] = db[r * k + q];   // FTranspose (colloc.c:100-101)
	off[(size_t)g * P + i] = (ivl - 1) * (k - m);                   // colloc.c:108
}

// ------------------------------------------------------------------------------------------
// linear-constraint rows (constraints.c:198-261 through colloc.c:243-316, band entries only)
// row order [lic; ltc constraint-major x breakpoint; lfc]; one thread per (row, band column)
// ------------------------------------------------------------------------------------------
__global__ void linrows_kernel(NtgDims D, NtgTables T, const double *__restrict__ lic,
                               const double *__restrict__ ltc, const double *__restrict__ lfc,
                               double *__restrict__ aband, int *__restrict__ rbp)
{
	const int idx = blockIdx.x * blockDim.x + threadIdx.x;
	if (idx >= D.nclin * D.sumk) return;
	const int r = idx / D.sumk, kc = idx % D.sumk;
	int o = 0;
	while (o + 1 < D.nout && D.koff[o + 1] <= kc) o++;
	const int q = kc - D.koff[o];
	const double *row; int bp;
	if (r < D.nlic) { row = lic + (size_t)r * D.nz; bp = 0; }
	else if (r < D.nlic + D.nltc * D.P) { const int rr = r - D.nlic; row = ltc + (size_t)(rr / D.P) * D.nz; bp = rr % D.P; }
	else { row = lfc + (size_t)(r - D.nlic - D.nltc * D.P) * D.nz; bp = D.P - 1; }
	const int c = D.cls[o], k = D.order[o], d = D.d[o];
	const double *b = T.blk + D.cls_blk[c] + ((size_t)bp * k + q) * d;
	double acc = 0.0;
	for (int l = 0; l < d; l++) acc += row[D.iz[o] + l] * b[l];
	aband[idx] = acc;
	if (kc == 0) rbp[r] = bp;
}

// bounds(): constraints.c:5-33
__global__ void bounds_kernel(NtgDims D, int batch, const double *__restrict__ lower,
                              const double *__restrict__ upper, double *__restrict__ bl,
                              double *__restrict__ bu, double big)
{
	const int ntot = D.nC + D.nclin + D.ncnln;
	const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (idx >= (long long)batch * ntot) return;
	const int b = idx / ntot, e = idx % ntot;
	double lo, up;
	if (e < D.nC) { lo = -big; up = big; }
	else {
		int r = e - D.nC, s;
		if (r < D.nlic) s = r;
		else if ((r -= D.nlic) < D.nltc * D.P) s = D.nlic + r / D.P;
		else if ((r -= D.nltc * D.P) < D.nlfc) s = D.nlic + D.nltc + r;
		else if ((r -= D.nlfc) < D.nnlic) s = D.nlic + D.nltc + D.nlfc + r;
		else if ((r -= D.nnlic) < D.nnltc * D.P) s = D.nlic + D.nltc + D.nlfc + D.nnlic + r / D.P;
		else { r -= D.nnltc * D.P; s = D.nlic + D.nltc + D.nlfc + D.nnlic + D.nnltc + r; }
		lo = lower[(size_t)b * D.nbounds + s]; up = upper[(size_t)b * D.nbounds + s];
	}
	bl[idx] = lo; bu[idx] = up;
}

hipError_t ntg_launch_basis(int ngrids, int l, int k, int m, int d, int P, const double *knots, const double *bps,
                            long long knots_stride, long long bps_stride, double *blk, int *off, hipStream_t st)
{
	const int nt = 64;
	dim3 grid((P + nt - 1) / nt, ngrids);
	hipLaunchKernelGGL(basis_kernel, grid, dim3(nt), (size_t)(l + 1) * 8, st, ngrids, l, k, m, d, P, knots, bps,
	                   knots_stride, bps_stride, blk, off);
	return hipGetLastError();
}

hipError_t ntg_launch_linrows(const NtgDims &D, const NtgTables &T, const double *lic, const double *ltc,
                              const double *lfc, double *aband, int *rbp, hipStream_t st)
{
	const int total = D.nclin * D.sumk;
	if (total == 0) return hipSuccess;
	hipLaunchKernelGGL(linrows_kernel, dim3((total + 127) / 128), dim3(128), 0, st, D, T, lic, ltc, lfc, aband, rbp);
	return hipGetLastError();
}

hipError_t ntg_launch_bounds(const NtgDims &D, int batch, const double *lo, const double *up, double *bl, double *bu,
                             hipStream_t st)
{
	const long long total = (long long)batch * (D.nC + D.nclin + D.ncnln);
	if (total == 0) return hipSuccess;
	hipLaunchKernelGGL(bounds_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, D, batch, lo, up, bl, bu,
	                   1.7976931348623157e308);
	return hipGetLastError();
}
