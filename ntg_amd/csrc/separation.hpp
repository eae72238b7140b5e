// separation.hpp -- ntg_batch_separation: the smallest squared distance over the horizon of pairs of bodies, a body being ndim outputs of one
// basis class (the x and y of a car), of one problem or of two.  On a common knot interval both trajectories are polynomials, so their
// difference is one too, and the squared distance c(t) = sum_t (D^deriv delta_t(t))^2 is a sum-of-squares row of a virtual problem whose
// coefficients are the difference coefficients delta_t[i] = x[a][iC[oa_t] + i] - x[b][iC[ob_t] + i] (one subtraction each).
//
// Per pair, the definition of include/ntg_amd.h:
//   bounds    0 <= a, b < batch and 0 <= ga, gb < nbody before anything of the pair is read; otherwise status NTG_SEP_BADPAIR, NaN, 0 pieces.
//   delta     [ndim][n] into the wave's own LDS, where a coefficient row of ntg_batch_extrema would be.
//   level 0   sos_poly (envelope_sos.hpp) with the terms {dimension t, derivative deriv, shift 0, no parameter} on every knot interval: the
//             polygon ntg_batch_extrema forms for such a row, bit for bit.
//   levels    ext_levels (extrema.hpp) with sides = 1, in its threshold instance: a piece whose polygon does not reach below s2 = sep * sep
//             retires at once, so a pair that keeps its distance ends at level 0.  No copy of the level loop is made for it (the one
//             copy that exists is ratio_levels of ratios.hpp, for pairs of polygons).
// separation_kernel: persistent workgroups of four waves; the term and class tables, the unfolded product tables, the extraction weights and
// the breaks of the one class are built once into LDS; every wave then streams pairs with its own delta and work list.  After the set-up
// there is no workgroup barrier (ext_levels says why its list needs none; delta is written and read by one wave, whose LDS operations
// complete in order).  No scratch in HBM, no atomics, nothing depends on the other pairs or on the batch.  Every private array is indexed by
// unrolled loop counters only.
#pragma once
#include "extrema.hpp"

// level-0 polygons of the pair: row 0 of the staged tables on the wave's delta
template <int KM>
struct SepSrc {
	const SosTables &T; const ExtLds &M; SosRow R; EnvClass C;
	__device__ __forceinline__ EnvPoly<2 * KM - 1> operator()(int j) const { return sos_poly<KM>(T, 0, R, C, M.wl, M.tab, M.xrow, M.prow, j, 0, 0); }
};

template <int NT, int KM>
__global__ void __launch_bounds__(NT)
separation_kernel(SepArgs A)
{
	extern __shared__ __attribute__((aligned(16))) char smem_raw[];
	constexpr int NW = NT / 64, KD = 2 * KM - 1;
	__shared__ SosTables T;
	const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
	const int nd = A.ndim * A.n;
	double *wl = reinterpret_cast<double *>(smem_raw);    // the product tables, unfolded
	double *tab = wl + NTG_SOS_WFULL;                     // weights and interval lengths of the class
	double *kns = tab + A.g.ne;                           // its breaks
	double *delta = kns + A.g.lmax + 1 + (size_t)wave * (nd + NTG_EXTREMA_CAP * (KD + 1));
	double *list = delta + nd;
	const ExtLds M{wl, tab, kns, delta, nullptr, list, reinterpret_cast<long long *>(list + NTG_EXTREMA_CAP * KD)};
	sos_stage(A.sos, A.g, T, tid);
	sos_unfold(A.sos, wl, tid, NT);
	env_build_classes(A.g, tab, kns, nullptr, tid, NT);
	const EnvClass C = T.c[0];
	const SosRow R = T.row[0];
	const SepSrc<KM> src{T, M, R, C};
	for (int q0 = blockIdx.x * NW; q0 < A.npairs; q0 += gridDim.x * NW) {
		const int q = q0 + wave;
		if (q >= A.npairs) continue;
		const int *pr = A.pairs + 4 * (size_t)q;
		const int a = __builtin_amdgcn_readfirstlane(pr[0]), b = __builtin_amdgcn_readfirstlane(pr[1]);
		const int ga = __builtin_amdgcn_readfirstlane(pr[2]), gb = __builtin_amdgcn_readfirstlane(pr[3]);
		const bool bad = a < 0 || a >= A.g.batch || b < 0 || b >= A.g.batch || ga < 0 || ga >= A.nbody || gb < 0 || gb >= A.nbody;
		double s2 = INFINITY;
		if (A.sep) { const double s = A.sep[q]; s2 = s * s; }
		double res[4], tw[2];
		int status = NTG_SEP_BADPAIR, npieces = 0;
		if (bad) { res[0] = res[1] = NAN; tw[0] = NAN; }
		else {
			const double *xa = A.g.x + (size_t)a * A.g.nC, *xb = A.g.x + (size_t)b * A.g.nC;
			__builtin_amdgcn_wave_barrier();   // the pair before is done with delta
			for (int e = lane; e < nd; e += 64) {
				const int t = e / A.n, i = e - t * A.n;
				delta[e] = xa[A.biC[ga][t] + i] - xb[A.biC[gb][t] + i];
			}
			__builtin_amdgcn_wave_barrier();
			const ExtRun Q{kns, tab + C.hoff, C.l, R.D, A.max_depth, 1, A.tol, s2};
			ext_levels<KM, true>(Q, M, src, lane, res, tw, status, npieces);
		}
		if (lane == 0) {
			if (A.min) { A.min[2 * (size_t)q] = res[0]; A.min[2 * (size_t)q + 1] = res[1]; }
			if (A.when) A.when[q] = tw[0];
			if (A.status) A.status[q] = status;
			if (A.npieces) A.npieces[q] = npieces;
			if (A.viol) {   // of the attained value, of the certified one; a NaN (a bad pair, a NaN row, a NaN s2) stays
				A.viol[2 * (size_t)q] = env_max(0.0, s2 - res[1]);
				A.viol[2 * (size_t)q + 1] = env_max(0.0, s2 - res[0]);
			}
		}
	}
}
