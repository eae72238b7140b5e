// time_tile.hpp -- the steps of a kernel that puts TIMES on the lanes, as functions (cost_kernel, cost.hpp): a workgroup owns one tile of
// NTG_CHECK_NT times and walks over the problems of its group.  The basis values of the tile -- the [t][q][r] table basis_kernel wrote --
// are read coalesced and kept TRANSPOSED in LDS ([class][q][r][lane], rows padded by one double), the problem's coefficient row is
// staged next to them, and the flat flag of a lane's time is built in registers (SplineInterp, colloc.c:476-481).  The tile fields of
// CheckArgs (ntg_dev.hpp) describe the tables; every function here is inlined into its caller.
// check_kernel (check.hpp) has the same steps written out in its body, statement for statement: called from there, these functions
// compile to other code for its shipped instances (the 64-entry instances go from 171 to 243 vector registers, the others move by up
// to 4 % in instructions), so it keeps its text and its code.  A change to the staging, the offsets or the flag belongs in both places.
// On the host every such kernel, check_kernel included, is launched by tile_launch below; a family names its instances once (tile_launchers).
#pragma once
#include <hip/hip_runtime.h>
#include "ntg_dev.hpp"
#include "families.hpp"

// the dynamic LDS of a time-tile kernel (ntg_check_lds): table [sumkd][NT + 1], coefficient row [npad], offsets [nclass][NT]
struct TileLds { double *tab, *x; int *off; };
__device__ __forceinline__ TileLds tile_lds(char *smem_raw, const NtgDims &D, const CheckArgs &a)
{
	TileLds s;
	s.tab = reinterpret_cast<double *>(smem_raw);
	s.x = s.tab + (size_t)a.sumkd * (NTG_CHECK_NT + 1);
	s.off = reinterpret_cast<int *>(s.x + ((D.nC + 1) & ~1));
	return s;
}

// Problem bl of the launch (b of the batch) enters the workgroup: the tile's table and offsets (once per workgroup on the shared grid,
// per problem on per-problem grids), the coefficient row, the family's parameter row.  nval: times of the tile, t: this lane's time
// index.  Ends with a barrier; begins with one when the workgroup has had a problem before (its readers are done).
template <int FAM>
__device__ __forceinline__ void tile_stage(const NtgDims &D, const NtgTables &T, const CheckArgs &a, const TileLds &s, int bl, int b, int tile0, int nval, int t)
{
	constexpr int NT = NTG_CHECK_NT, LD = NT + 1;
	const int tid = threadIdx.x, ntimes = a.ntimes;
	if (bl != (int)blockIdx.y) __syncthreads();   // the previous problem's readers are done
	if (a.pp || bl == (int)blockIdx.y) {
		for (int c = 0; c < D.nclass; c++) {
			const int kd = D.cls_k[c] * D.cls_d[c], n = nval * kd;
			const double *src = a.tblk + (a.pp ? (size_t)bl * a.pp_tab : (size_t)a.gbase[c]) + (size_t)tile0 * kd;
			double *dst = s.tab + (size_t)a.lbase[c] * LD;
			// (e / kd without an integer divide per element: e < 128 k d <= 12800 and k d <= 100, so the float quotient of e + 0.5 is
			// exact to 1e-5 of a value that stays 0.005 away from every integer)
#ifndef NTG_CHECK_DIRECT
			const float rkd = 1.0f / (float)kd;
			for (int e = tid; e < n; e += NT) { const int te = (int)(((float)e + 0.5f) * rkd), qr = e - te * kd; dst[qr * LD + te] = src[e]; }
#else
			(void)n; (void)src; (void)dst;
#endif
			s.off[c * NT + tid] = a.toff[(size_t)(a.pp ? bl : c) * ntimes + t];
		}
	}
	for (int i = tid; i < D.nC; i += NT) s.x[i] = a.x[(size_t)b * D.nC + i];
	ntg_prm_publish<FAM>(T, b);
	__syncthreads();
}

// flat flag of this lane's time (tl: its index in the tile): z[iz[o] + r] = sum_q D^r B_{off+q}(t) C[iC[o] + off + q]   (colloc.c:476-481,
// q ascending); every output has maxderiv DM, z is NZMAX registers
template <int DM, int NZMAX>
__device__ __forceinline__ void tile_flag(const NtgDims &D, const CheckArgs &a, const TileLds &s, int bl, int t, int tl, double *z)
{
	constexpr int NT = NTG_CHECK_NT, LD = NT + 1, NOUTMAX = NZMAX / DM;
	const int nout = D.nout;
#pragma unroll
	for (int v = 0; v < NZMAX; v++) z[v] = 0.0;
#pragma unroll
	for (int o = 0; o < NOUTMAX; o++) {
		if (o < nout) {
			const int c = D.cls[o], k = D.order[o];
#ifndef NTG_CHECK_DIRECT
			constexpr int TS = LD;
			const double *tb = s.tab + (size_t)a.lbase[c] * LD + tl;
			(void)bl; (void)t;
#else   // tuning builds only (-DNTG_CHECK_DIRECT): no LDS copy, every lane reads its time's [q][r] block from the table
			constexpr int TS = 1;
			const double *tb = a.tblk + (a.pp ? (size_t)bl * a.pp_tab : (size_t)a.gbase[c]) + (size_t)t * k * DM;
#endif
			const double *cx = s.x + D.iC[o] + s.off[c * NT + tl];
			for (int q = 0; q < k; q++) {
				const double cq = cx[q];
#pragma unroll
				for (int r = 0; r < DM; r++) z[DM * o + r] += tb[(q * DM + r) * TS] * cq;
			}
		}
	}
}

// breakpoint index a family callback receives for time index t of problem b: the last breakpoint of the problem's grid at or before it
__device__ __forceinline__ int tile_bp_index(const NtgDims &D, const NtgTables &T, const CheckArgs &a, int b, int t)
{
	const double *bps = T.bps + (size_t)b * T.pp_bps;
	const double tv = a.times[(size_t)b * a.times_stride + t];
	int ilo = 0, ihi = D.P;
	while (ihi - ilo > 1) { const int mid = (ilo + ihi) >> 1; if (bps[mid] <= tv) ilo = mid; else ihi = mid; }
	return ilo;
}

// ---------------- host side: the one launcher of the time-tile kernels ----------------
// A kernel of this kind states in a struct K next to it (CheckTile, CostTile, VerifyTile) what the launcher cannot know:
//   Args                    its argument struct, and tile(args): the tile fields in it
//   kernel<FAM, NZMAX>()    its instance for a family and a flag size
//   refuses<Fam>(D)         shapes it does not take, besides the ones no time-tile kernel takes
//   LDS_MAX                 the most dynamic LDS a workgroup of it may ask for (160 KiB less its static part)
// NZ0, NZS...: the flag sizes the family has instances for, ascending; the one launched is the smallest that holds the plan's (the
// flag lives in registers).  hipErrorInvalidValue: no instance for this shape.
template <class K, int FAM, int NZ0, int... NZS>
static hipError_t tile_launch(const NtgDims &D, const NtgTables &T, const typename K::Args &ka)
{
	if constexpr (sizeof...(NZS) > 0) { if (D.nz > NZ0) return tile_launch<K, FAM, NZS...>(D, T, ka); }
	using Fam = Family<FAM>;
	const CheckArgs &a = K::tile(ka);
	if (D.nz > NZ0 || !ntg_all_d(D, Fam::DM) || D.nout > NZ0 / Fam::DM || K::template refuses<Fam>(D)) return hipErrorInvalidValue;
	if (a.nb <= 0 || a.ntimes <= 0) return hipSuccess;
	auto kfn = K::template kernel<FAM, NZ0>();
	const size_t lds = ntg_check_lds(D);
	if (lds > K::LDS_MAX) return hipErrorInvalidValue;   // (the batch call refuses such a plan before it gets here)
	if (lds > 64 * 1024) {
		const hipError_t e = hipFuncSetAttribute((const void *)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
		if (e != hipSuccess) return e;
	}
	hipLaunchKernelGGL(kfn, dim3(a.ntiles, a.ngroups), dim3(NTG_CHECK_NT), lds, a.st, D, T, ka);
	return hipGetLastError();
}

// The three launchers of a family (TileLaunchers, family_module.hpp) from its one list of flag sizes.  A unit that calls this includes
// check.hpp, cost.hpp and verify.hpp, and calls it where the device pass sees the call too: that is what instantiates the kernels.
struct CheckTile; struct CostTile; struct VerifyTile;
template <int FAM, int... NZS>
constexpr TileLaunchers tile_launchers()
{
	return TileLaunchers{tile_launch<CheckTile, FAM, NZS...>, tile_launch<CostTile, FAM, NZS...>, tile_launch<VerifyTile, FAM, NZS...>};
}
