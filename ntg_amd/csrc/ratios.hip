// ratios.hip -- the kernels of ntg_batch_ratios (ratios.hpp) and the checks of their launch: a translation unit of its own, because the
// instances carry polygons of 13 or 25 points for both plan sizes and would double the build time of certs.hip.
//
//   ratios_shared_kernel / ratios_pp_kernel <KM, KR>   KM = 6 or NTG_MAX_ORDER: the forms' polygons, as in forms.hpp; KR = 13 or 25: points of the
//                                                     pair's polygons, the smallest that holds the largest degree of the call's ratios
#include <hip/hip_runtime.h>
#include <math.h>
#include <algorithm>
#include "ntg_dev.hpp"
#include "plan.hpp"
#include "ratios.hpp"
#include "cert_launch.hpp"

// launch_cert (cert_launch.hpp) with nw waves per workgroup and a pass of nw problems as the unit of work
template <int KM, int KR>
static hipError_t launch_ratios(const RatioArgs &A, int ncu, size_t lds, hipStream_t st)
{
	return launch_cert(ratios_pp_kernel<KM, KR>, ratios_shared_kernel<KM, KR>, A, A.f.g, 64 * A.nw, (A.f.g.batch + A.nw - 1) / A.nw, ncu, lds, st);
}

// hipErrorInvalidValue: the tables exceed the LDS or the polygons the instances (ntg_batch_ratios refuses such a call before it gets here)
hipError_t ntg_launch_ratios(const RatioArgs &A, int ncu, hipStream_t st)
{
	const size_t lds = ntg_ratios_lds(A, A.nw);
	if (lds > NTG_EXTREMA_LDS_MAX || A.f.g.kmax > NTG_MAX_ORDER || A.nratio > NTG_RATIO_MAXRATIOS || (A.nw != 2 && A.nw != 4) || (A.kr != 13 && A.kr != 25)) return hipErrorInvalidValue;
	for (int r = 0; r < A.nratio; r++)
		if (A.r[r].DR >= A.kr) return hipErrorInvalidValue;
	if (A.f.g.kmax > 6 && A.kr != 25) return hipErrorInvalidValue;   // (a form's polygon of 19 points starts the chain)
	if (A.f.g.batch <= 0 || A.nratio <= 0) return hipSuccess;
	if (A.f.g.kmax <= 6) return A.kr == 13 ? launch_ratios<6, 13>(A, ncu, lds, st) : launch_ratios<6, 25>(A, ncu, lds, st);
	return launch_ratios<NTG_MAX_ORDER, 25>(A, ncu, lds, st);
}
