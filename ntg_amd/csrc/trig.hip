// trig.hip -- the kernels of ntg_batch_trig (trig.hpp) and the checks of their launch: a translation unit of its own, so that the instances
// of the other bisection calls (certs.hip, ratios.hip) stay what they are.
//
//   trig_shared_kernel / trig_pp_kernel <KM>   KM = 6 or NTG_MAX_ORDER: points of the angle polygons, the smallest that holds the plan's
//                                             largest order
#include <hip/hip_runtime.h>
#include <math.h>
#include <algorithm>
#include "ntg_dev.hpp"
#include "plan.hpp"
#include "trig.hpp"
#include "cert_launch.hpp"

// launch_cert (cert_launch.hpp) with nw waves per workgroup and a pass of nw problems as the unit of work
template <int KM>
static hipError_t launch_trig(const TrigArgs &A, int ncu, size_t lds, hipStream_t st)
{
	return launch_cert(trig_pp_kernel<KM>, trig_shared_kernel<KM>, A, A.g, 64 * A.nw, (A.g.batch + A.nw - 1) / A.nw, ncu, lds, st);
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
