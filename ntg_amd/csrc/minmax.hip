// minmax.hip -- the kernels of ntg_batch_minmax (minmax.hpp) and the checks of their launch: a translation unit of its own, so that the
// instances of the other bisection calls (certs.hip, ratios.hip, trig.hip) stay what they are.
//
//   minmax_shared_kernel / minmax_pp_kernel <KM, KP>   KM = 6 or NTG_MAX_ORDER: points of a factor's polygon, by the plan's largest order;
//                                                     KP = 6, 11 or 19: points of a member's polygon in the level loop and the work list,
//                                                     the smallest that holds the call's largest group degree (ntg_minmax_points)
// The members a work list has room for (8 or 16) and the waves of a workgroup (4, 2 or 1) are figures of the launch, not of the instance: the
// member loops run to the group's own count.
#include <hip/hip_runtime.h>
#include <math.h>
#include <algorithm>
#include "ntg_dev.hpp"
#include "plan.hpp"
#include "minmax.hpp"
#include "cert_launch.hpp"

// launch_cert (cert_launch.hpp) with nw waves per workgroup and a pass of nw problems as the unit of work
template <int KM, int KP>
static hipError_t launch_minmax(const MinmaxArgs &A, int ncu, size_t lds, hipStream_t st)
{
	return launch_cert(minmax_pp_kernel<KM, KP>, minmax_shared_kernel<KM, KP>, A, A.g, 64 * A.nw, (A.g.batch + A.nw - 1) / A.nw, ncu, lds, st);
}

// hipErrorInvalidValue: the tables exceed the LDS or the declaration the kernels' tables (ntg_batch_minmax refuses such a call before it gets here)
hipError_t ntg_launch_minmax(const MinmaxArgs &A, int ncu, hipStream_t st)
{
	if (A.g.kmax > NTG_MAX_ORDER || A.nform < 0 || A.nform > NTG_MINMAX_MAXFORMS || A.ngroup < 0 || A.ngroup > NTG_MINMAX_MAXGROUPS || A.nfp < 0) return hipErrorInvalidValue;
	if ((A.nw != 1 && A.nw != 2 && A.nw != 4) || (A.mcap != 8 && A.mcap != NTG_MINMAX_MAXMEMBERS)) return hipErrorInvalidValue;
	int dmax = 0;
	for (int g = 0; g < A.ngroup; g++) {
		const MinmaxGroup &G = A.grp[g];
		if (G.nm < 1 || G.nm > A.mcap || G.m0 < 0 || G.m0 + G.nm > NTG_MINMAX_MAXMEMTOT || G.cl < 0 || G.cl >= A.g.nclass || G.D < 0 || !((G.clast >> (G.nm - 1)) & 1u)) return hipErrorInvalidValue;
		for (int m = G.m0; m < G.m0 + G.nm; m++) {
			const MinmaxMem &Q = A.mem[m];
			if (Q.form < 0 || Q.form >= A.nform || Q.pc < -1 || Q.pc >= A.nfp) return hipErrorInvalidValue;
			const FormRow &R = A.row[Q.form];
			if (R.nt < 1 || R.nt > NTG_FORM_MAXTERMS || R.t0 < 0 || R.t0 + R.nt > NTG_MINMAX_MAXTERMS || R.D < 0 || R.D > G.D || R.cl != G.cl) return hipErrorInvalidValue;
		}
		dmax = std::max(dmax, G.D);
	}
	const int kp = ntg_minmax_points(A.g, dmax);
	if (dmax >= kp || A.pw != (kp | 1)) return hipErrorInvalidValue;
	const size_t lds = ntg_minmax_lds(A, A.nw);
	if (lds > NTG_EXTREMA_LDS_MAX) return hipErrorInvalidValue;
	if (A.g.batch <= 0 || A.ngroup <= 0) return hipSuccess;
	if (kp == 6) return launch_minmax<6, 6>(A, ncu, lds, st);
	if (kp == 11) return launch_minmax<6, 11>(A, ncu, lds, st);
	return launch_minmax<NTG_MAX_ORDER, 2 * NTG_MAX_ORDER - 1>(A, ncu, lds, st);
}
