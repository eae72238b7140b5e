// trig.hip -- the kernels of ntg_batch_trig (trig.hpp) and their launcher: a translation unit of its own, so that the instances of the
// other bisection calls (certs.hip, ratios.hip) stay what they are.
//
//   trig_shared_kernel / trig_pp_kernel <KM>   KM = 6 or NTG_MAX_ORDER: points of the angle polygons, the smallest that holds the plan's
//                                             largest order
#include <hip/hip_runtime.h>
#include <math.h>
#include <algorithm>
#include "ntg_dev.hpp"
#include "plan.hpp"
#include "trig.hpp"

template <int KM>
static hipError_t launch_trig(const TrigArgs &A, int ncu, size_t lds, hipStream_t st)
{
	const int nw = A.nw, groups = (A.g.batch + nw - 1) / nw;
	auto kfn = A.g.pp ? trig_pp_kernel<KM> : trig_shared_kernel<KM>;
	if (lds > 64 * 1024) {
		const hipError_t e = hipFuncSetAttribute((const void *)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
		if (e != hipSuccess) return e;
	}
	// shared grids: persistent workgroups, each builds its tables once, so each should stream several passes; no more than fill the device
	const int grid = A.g.pp ? std::min(groups, 8 * ncu) : std::max(1, std::min((groups + 3) / 4, 8 * ncu));
	hipLaunchKernelGGL(kfn, dim3(grid), dim3(64 * nw), lds, st, A);
	return hipGetLastError();
}

// hipErrorInvalidValue: the tables exceed the LDS or the declaration the kernels' tables (ntg_batch_trig refuses such a call before it gets here)
hipError_t ntg_launch_trig(const TrigArgs &A, int ncu, hipStream_t st)
{
	if (A.g.kmax > NTG_MAX_ORDER || A.nform > NTG_TRIG_MAXFORMS || (A.nw != 2 && A.nw != 4) || A.nprm < A.nfp) return hipErrorInvalidValue;
	const size_t lds = ntg_trig_lds(A, A.nw);
	if (lds > NTG_EXTREMA_LDS_MAX || ((A.g.ne + A.q.nk) & 1) || ((A.g.nC + A.nprm) & 1)) return hipErrorInvalidValue;   // (the work lists start at 16 bytes)
	for (int f = 0; f < A.nform; f++) {
		const TrigRow &R = A.row[f];
		if (R.ntrig < 0 || R.nlin < 0 || R.ntrig + R.nlin < 1 || R.ntrig + R.nlin > NTG_TRIG_MAXTERMS || R.D < 0 || R.D >= (A.g.kmax <= 6 ? 6 : NTG_MAX_ORDER) || R.cl < 0 || R.cl >= A.g.nclass)
			return hipErrorInvalidValue;
	}
	if (A.g.batch <= 0 || A.nform <= 0) return hipSuccess;
	return A.g.kmax <= 6 ? launch_trig<6>(A, ncu, lds, st) : launch_trig<NTG_MAX_ORDER>(A, ncu, lds, st);
}
