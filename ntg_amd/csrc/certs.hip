// certs.hip -- the launchers of the kernels that are written once for every family and instantiated here from their headers:
//   envelope_*      bounds of every flag entry and linear trajectory row over whole pieces of the knot intervals, from the Bezier
//                   control polygons (envelope.hpp)
//   envelope_sos_*  the same for the nonlinear trajectory rows declared as sums of squares, by the Bezier product of those polygons
//                   (envelope_sos.hpp)
//   extrema_*       minimum and maximum of those rows over the horizon, enclosed to a tolerance, by bisection of the same polygons
//                   from a work list in LDS (extrema.hpp)
//   forms_*         the same for quadratic forms of the flag declared at the call (forms.hpp)
//   separation_kernel  smallest squared distance of pairs of bodies over the horizon, by that bisection (separation.hpp)
//   refine_*        coefficients on a finer knot grid (refine.hpp)
//   kkt_kernel      first-order optimality residuals of a batch on the banded Jacobian (kkt.hpp)
// (ntg_batch_ratios' kernels, instances of the same bisection, have a unit of their own: ratios.hip.)  Host side: plan_cert.cpp,
// plan_refine.cpp, plan_kkt.cpp.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "ntg_dev.hpp"
#include "plan.hpp"
#include "refine.hpp"
#include "envelope.hpp"
#include "envelope_sos.hpp"
#include "extrema.hpp"
#include "separation.hpp"
#include "forms.hpp"
#include "kkt.hpp"
#include "cert_launch.hpp"

// The time certificates, through launch_cert (cert_launch.hpp): both kernels in the instance with the smallest private polygons that hold the
// plan's largest order (KM = 6 or NTG_MAX_ORDER).
#define NTG_CERT_LAUNCH(name, NT, units)                                                                                    \
	(A.g.kmax <= 6 ? launch_cert(name##_pp_kernel<NT, 6>, name##_shared_kernel<NT, 6>, A, A.g, NT, units, ncu, lds, st) \
	               : launch_cert(name##_pp_kernel<NT, NTG_MAX_ORDER>, name##_shared_kernel<NT, NTG_MAX_ORDER>, A, A.g, NT, units, ncu, lds, st))

// hipErrorInvalidValue: the tables exceed the LDS (the entry points refuse such a plan before it gets here).  On shared grids a workgroup of
// the two envelope calls takes one problem at a time ...
hipError_t ntg_launch_envelope(const EnvArgs &A, int ncu, hipStream_t st)
{
	const size_t lds = ntg_envelope_lds(A);
	if (lds > NTG_ENVELOPE_LDS_MAX || A.g.kmax > NTG_MAX_ORDER) return hipErrorInvalidValue;
	if (A.g.batch <= 0) return hipSuccess;
	return NTG_CERT_LAUNCH(envelope, NTG_ENVELOPE_NT, A.g.batch);
}
hipError_t ntg_launch_envelope_sos(const SosArgs &A, int ncu, hipStream_t st)
{
	const size_t lds = ntg_envelope_sos_lds(A);
	if (lds > NTG_ENVELOPE_LDS_MAX || A.g.kmax > NTG_MAX_ORDER || A.sos.nrow > NTG_SOS_MAXROWS) return hipErrorInvalidValue;
	if (A.g.batch <= 0) return hipSuccess;
	return NTG_CERT_LAUNCH(envelope_sos, NTG_ENVELOPE_NT, A.g.batch);
}
// ... and one of ntg_batch_extrema a pass of four problems, one per wave
hipError_t ntg_launch_extrema(const ExtArgs &A, int ncu, hipStream_t st)
{
	const size_t lds = ntg_extrema_lds(A);
	if (lds > NTG_EXTREMA_LDS_MAX || A.g.kmax > NTG_MAX_ORDER || A.sos.nrow > NTG_SOS_MAXROWS) return hipErrorInvalidValue;
	if (A.g.batch <= 0) return hipSuccess;
	return NTG_CERT_LAUNCH(extrema, NTG_EXTREMA_NT, (A.g.batch + NTG_EXTREMA_NT / 64 - 1) / (NTG_EXTREMA_NT / 64));
}
// ... and one of ntg_batch_forms likewise
hipError_t ntg_launch_forms(const FormArgs &A, int ncu, hipStream_t st)
{
	const size_t lds = ntg_forms_lds(A);
	if (lds > NTG_EXTREMA_LDS_MAX || A.g.kmax > NTG_MAX_ORDER || A.nform > NTG_FORM_MAXFORMS) return hipErrorInvalidValue;
	if (A.g.batch <= 0 || A.nform <= 0) return hipSuccess;
	return NTG_CERT_LAUNCH(forms, NTG_EXTREMA_NT, (A.g.batch + NTG_EXTREMA_NT / 64 - 1) / (NTG_EXTREMA_NT / 64));
}
#undef NTG_CERT_LAUNCH
// ... and one of ntg_batch_separation a pass of four pairs.  Shared grids only: the entry point refuses per-problem grids, so there is no kpp
hipError_t ntg_launch_separation(const SepArgs &A, int ncu, hipStream_t st)
{
	const size_t lds = ntg_separation_lds(A);
	constexpr int NT = NTG_EXTREMA_NT;
	if (lds > NTG_EXTREMA_LDS_MAX || A.g.kmax > NTG_MAX_ORDER || A.g.pp || A.g.nclass != 1) return hipErrorInvalidValue;
	if (A.npairs <= 0 || A.g.batch <= 0) return hipSuccess;
	const int units = (A.npairs + NT / 64 - 1) / (NT / 64);
	return A.g.kmax <= 6 ? launch_cert<SepArgs>(nullptr, separation_kernel<NT, 6>, A, A.g, NT, units, ncu, lds, st)
	                     : launch_cert<SepArgs>(nullptr, separation_kernel<NT, NTG_MAX_ORDER>, A, A.g, NT, units, ncu, lds, st);
}

// ntg_batch_refine (refine.hpp): coefficients on a finer knot grid.  pp != 0: per-problem grids.  hipErrorInvalidValue: the tables exceed the LDS.
hipError_t ntg_launch_refine(const RefineArgs &A, int pp, int ncu, hipStream_t st)
{
	const size_t lds = ntg_refine_lds(A, pp);
	if (lds > NTG_REFINE_LDS_MAX) return hipErrorInvalidValue;   // (ntg_batch_refine refuses such a pair before it gets here)
	if (pp) {
		const int groups = (A.batch + NTG_REFINE_NT / 64 - 1) / (NTG_REFINE_NT / 64);
		hipLaunchKernelGGL(refine_pp_kernel<NTG_REFINE_NT>, dim3(std::min(groups, 8 * ncu)), dim3(NTG_REFINE_NT), lds, st, A);
	} else {
		// persistent workgroups: each builds its weights once, so each should stream several problems; no more than fill the device
		const int grid = std::max(1, std::min((A.batch + 7) / 8, 8 * ncu));
		hipLaunchKernelGGL(refine_shared_kernel<NTG_REFINE_NT>, dim3(grid), dim3(NTG_REFINE_NT), lds, st, A);
	}
	return hipGetLastError();
}

// ntg_batch_kkt (kkt.hpp): one pass for every family, built in or loaded.  hipErrorInvalidValue: one problem's vectors exceed the LDS.
hipError_t ntg_launch_kkt(const NtgDims &D, const NtgTables &T, const KktArgs &a) { return launch_kkt(D, T, a); }
