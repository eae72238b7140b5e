// forms.hpp -- ntg_batch_forms: the minimum and maximum over the horizon of quadratic forms of the flat flag declared AT THE CALL,
//   q(z) = sum_t w_t (z[u_t] - a_t)(z[v_t] - b_t)  or  w_t (z[u_t] - a_t),   a = su + fprm_b[pu], b = sv + fprm_b[pv],
// independent of the plan's family and rows: speed^2, the turning numerator x' y'' - y' x'', weighted thrust, ellipses, rows of a module.
// On a knot interval every flag entry is a polynomial, so the form is one too, and its Bezier polygon follows from the entries' polygons by
// the Bezier PRODUCT of two polygons of degrees d and e; envelope_sos.hpp's square is the case "polygon times itself".
//
// Per (problem, form), the definition of include/ntg_amd.h:
//   level 0   form_poly on every knot interval j of the form's basis class.  Per term, in declared order: the factors' polygons as sos_poly
//             forms them (EnvPoly::extract / diff, then the shift); the product g_m = sum_{i + j = m} W_{d,e}[i][j] p_i q_j, i ascending (a
//             square term by sos_square_point on the table W_{d,d}, a linear term g = p); the term's polygon w g_m, elevated to the form's
//             degree D where it is lower, added to the form's polygon.  A term of full degree is accumulated point by point.
//   levels    ext_levels (extrema.hpp) in ntg_batch_extrema's instance: there is one level loop.
// The tables W_{d,e} of all 100 pairs of degrees (3025 doubles) are built once per workgroup into LDS from an exact integer Pascal triangle:
// the numerator is an exact integer product, the division the one rounding, so W_{d,d} is bit-equal to the host-built W_d of CertSos.
//
//   forms_shared_kernel  plans on their own grid: persistent workgroups of four waves; the product tables, the extraction weights and the
//                        breaks of every basis class are built once into LDS; every wave then streams problems with its own x row, fprm row
//                        and work list.  No workgroup barrier after the set-up.
//   forms_pp_kernel      per-problem grids: the same, with breaks and weights of the wave's own problem.
// The form and term tables are read from the kernel argument at wave-uniform indices.  No scratch in HBM, no atomics, nothing depends on the
// batch around a problem.  Every private array is indexed by unrolled loop counters only.
#pragma once
#include "extrema.hpp"

#define NTG_FORM_PASCAL (2 * NTG_MAX_ORDER - 1)   // rows of the triangle: n = 0 .. 2 (NTG_MAX_ORDER - 1)

// Pascal's triangle C(n, r), n <= 18, into pas [n][r] (exact: C(18,9) = 48620), then every product table from it: one thread per weight
__device__ __forceinline__ void form_build_products(double *wt, unsigned int *pas, int tid, int nthr)
{
	constexpr int NP = NTG_FORM_PASCAL, TRI = NTG_MAX_ORDER * (NTG_MAX_ORDER + 1) / 2;
	for (int n = 0; n < NP; n++) {
		for (int r = tid; r <= n; r += nthr) pas[n * NP + r] = (r == 0 || r == n) ? 1u : pas[(n - 1) * NP + r - 1] + pas[(n - 1) * NP + r];
		__syncthreads();
	}
	for (int q = tid; q < NTG_FORM_WALL; q += nthr) {
		int d = 0;
		while (q >= TRI * ((d + 1) * (d + 2) / 2)) d++;
		const int rem = q - TRI * (d * (d + 1) / 2);
		int e = 0;
		while (rem >= (d + 1) * ((e + 1) * (e + 2) / 2)) e++;
		const int at = rem - (d + 1) * (e * (e + 1) / 2), i = at / (e + 1), j = at - i * (e + 1);
		wt[q] = (double)(pas[d * NP + i] * pas[e * NP + j]) / (double)pas[(d + e) * NP + i + j];
	}
	__syncthreads();
}

// the shifted polygon of the flag entry with coefficient offset iC and derivative order r on knot interval j, as sos_poly forms it at
// nsub = 0: p_i = beta_i - sh.  Returns its degree (a derivative of order >= k: the single point 0 - sh)
template <int KM>
__device__ __forceinline__ int form_factor(EnvPoly<KM> &P, const EnvClass C, const double *tab, const double *xrow, int iC, int r, double sh, int j, double h)
{
	int d = C.k - 1 - r;
	if (d >= 0) {
		P.extract(tab + C.eoff + j * C.k * C.k, xrow + iC + C.k - 1 + j * (C.k - C.m), C.k);
		for (int q = 1; q <= r; q++) P.diff(C.k - q, h);
	} else {
		d = 0;
		P.b[0] = 0.0;
	}
#pragma unroll
	for (int s = 0; s < KM; s++) P.b[s] = s <= d ? P.b[s] - sh : 0.0;
	return d;
}

// point m of the product of P (degree d) and Q (degree e): W = the table of (d, e), [d + 1][e + 1]
template <int KM, int M>
__device__ __forceinline__ double form_product_point(const EnvPoly<KM> &P, const EnvPoly<KM> &Q, const double *W, int d, int e)
{
	double acc = 0.0;
#pragma unroll
	for (int a = 0; a < KM; a++) {
		const int c = M - a;
		if (c >= 0 && c < KM) { if (a <= d && c <= e) acc += W[a * (e + 1) + c] * P.b[a] * Q.b[c]; }
	}
	return acc;
}
// S (+)= w * (the term's product polygon), point by point: the product and the sum are rounded separately.  sq: a square term, P = Q
template <int KM, int M = 0>
__device__ __forceinline__ void form_term_into(EnvPoly<2 * KM - 1> &S, const EnvPoly<KM> &P, const EnvPoly<KM> &Q, const double *W, int d, int e, bool sq, double w, bool add)
{
#pragma clang fp contract(off)
	if constexpr (M < 2 * KM - 1) {
		if (M <= d + e) {
			const double g = w * (sq ? sos_square_point<KM, M>(P, W, d) : form_product_point<KM, M>(P, Q, W, d, e));
			S.b[M] = add ? S.b[M] + g : g;
		} else if (!add) S.b[M] = 0.0;
		form_term_into<KM, M + 1>(S, P, Q, W, d, e, sq, w, add);
	}
}

// what the kernels know of form f
struct FormOf {
	const FormArgs &A; int f; FormRow R; EnvClass C;
	__device__ __forceinline__ const FormTerm &term(int t) const { return A.term[f][t]; }
};

// Polygon (degree R.D) of a form on knot interval j: its terms' polygons, elevated to R.D where they are lower, summed in declared order.
// FO: what the caller knows of the form -- its row R, its class C and its terms term(t) (FormOf here, MinmaxFormOf in minmax.hpp)
template <int KM, class FO>
__device__ __forceinline__ EnvPoly<2 * KM - 1> form_poly(const FO &F, const ExtLds &M, int j)
{
#pragma clang fp contract(off)
	constexpr int KD = 2 * KM - 1;
	const EnvClass C = F.C;
	const int D = F.R.D;
	const double h = M.tab[C.hoff + j];
	EnvPoly<KD> S;
#pragma unroll
	for (int s = 0; s < KD; s++) S.b[s] = 0.0;
	for (int t = 0; t < F.R.nt; t++) {
		const FormTerm &Q = F.term(t);
		const int kind = Q.kind;
		const double w = Q.w;
		EnvPoly<KM> P, V;
		const int d = form_factor<KM>(P, C, M.tab, M.xrow, Q.iCu, Q.ru, Q.su + (Q.pu >= 0 ? M.prow[Q.pu] : 0.0), j, h);
		if (kind == NTG_FORM_LIN) {
			if (d == D) {
#pragma unroll
				for (int s = 0; s < KM; s++) { if (s <= D) S.b[s] += w * P.b[s]; }
			} else {
				EnvPoly<KD> G;
#pragma unroll
				for (int s = 0; s < KD; s++) G.b[s] = 0.0;
#pragma unroll
				for (int s = 0; s < KM; s++) G.b[s] = w * P.b[s];
				for (int u = d; u < D; u++) G.elevate(u);
#pragma unroll
				for (int s = 0; s < KD; s++) { if (s <= D) S.b[s] += G.b[s]; }
			}
			continue;
		}
		const bool sq = kind == NTG_FORM_SQUARE;
		int e = d;
		if (sq) V = P;
		else e = form_factor<KM>(V, C, M.tab, M.xrow, Q.iCv, Q.rv, Q.sv + (Q.pv >= 0 ? M.prow[Q.pv] : 0.0), j, h);
		const double *W = M.wl + ntg_form_woff(d, e);
		if (d + e == D) form_term_into<KM>(S, P, V, W, d, e, sq, w, true);
		else {   // a term of lower degree than the form: its polygon whole, elevated, then added
			EnvPoly<KD> G;
			form_term_into<KM>(G, P, V, W, d, e, sq, w, false);
			for (int u = d + e; u < D; u++) G.elevate(u);
#pragma unroll
			for (int s = 0; s < KD; s++) { if (s <= D) S.b[s] += G.b[s]; }
		}
	}
	return S;
}

// level-0 polygons of a form, for ext_levels
template <int KM>
struct FormSrc {
	const FormOf &F; const ExtLds &M;
	__device__ __forceinline__ EnvPoly<2 * KM - 1> operator()(int j) const { return form_poly<KM>(F, M, j); }
};

// every form of problem b, by one wave whose x row and fprm row are in M
template <int KM>
__device__ __forceinline__ void form_problem(const FormArgs &A, const ExtLds &M, int b, int lane)
{
	const int nform = A.nform;
	ExtOut O{A.q, lane};
	for (int f = 0; f < nform; f++) {
		const FormRow R = A.row[f];
		const EnvClass C = A.g.c[R.cl];
		const FormOf F{A, f, R, C};
		const ExtRun Q{M.kns + A.q.koff[R.cl], M.tab + C.hoff, C.l, R.D, A.q.max_depth, A.q.sides, A.q.tol, INFINITY};
		const FormSrc<KM> src{F, M};
		double res[4], tw[2];
		int status, npieces;
		ext_levels<KM, false>(Q, M, src, lane, res, tw, status, npieces);
		const size_t at = (size_t)b * nform + f;
		O.row(at, res, tw, status, npieces);
		if (O.want_v()) O.fold(A.flo[at], A.fhi[at], res, f);
	}
	O.problem(b);
}

template <int NT, int KM>
__global__ void __launch_bounds__(NT)
forms_shared_kernel(FormArgs A)
{
	extern __shared__ __attribute__((aligned(16))) char smem_raw[];
	constexpr int NW = NT / 64;
	__shared__ unsigned int pas[NTG_FORM_PASCAL * NTG_FORM_PASCAL];
	const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
	const ExtStage S = ntg_forms_layout(A, 2 * KM - 1).wave(reinterpret_cast<double *>(smem_raw), wave);
	const ExtLds M = S.view();   // (the kernel stages through S; everything below reads through M)
	form_build_products(S.wl, pas, tid, NT);
	env_build_classes(A.g, S.tab, S.kns, A.q.koff, tid, NT);
	for (int b0 = blockIdx.x * NW; b0 < A.g.batch; b0 += gridDim.x * NW) {
		const int b = b0 + wave;
		if (b >= A.g.batch) continue;
		__builtin_amdgcn_wave_barrier();   // the problem before is done with the rows
		env_stage_rows(A.g, nullptr, b, S.xrow, nullptr, lane, 64);
		cert_stage_fprm(A.fprm, A.nfp, b, S.prow, lane);
		__builtin_amdgcn_wave_barrier();
		form_problem<KM>(A, M, b, lane);
	}
}

// per-problem grids: one basis class; every wave builds the weights of its own problem
template <int NT, int KM>
__global__ void __launch_bounds__(NT)
forms_pp_kernel(FormArgs A)
{
	extern __shared__ __attribute__((aligned(16))) char smem_raw[];
	constexpr int NW = NT / 64;
	__shared__ unsigned int pas[NTG_FORM_PASCAL * NTG_FORM_PASCAL];
	const EnvClass C = A.g.c[0];
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const ExtStage S = ntg_forms_layout(A, 2 * KM - 1).wave(reinterpret_cast<double *>(smem_raw), wave);
	const ExtLds M = S.view();   // (the kernel stages through S; everything below reads through M)
	form_build_products(S.wl, pas, threadIdx.x, NT);
	const int per_pass = gridDim.x * NW;
	for (int b0 = 0; b0 < A.g.batch; b0 += per_pass) {   // (the same trip count for every wave of the grid: the barriers below are uniform)
		const int b = b0 + blockIdx.x * NW + wave;
		const bool on = b < A.g.batch;
		__syncthreads();
		if (on) { env_stage_pp(A.g, nullptr, b, S.kns, S.xrow, nullptr, lane); cert_stage_fprm(A.fprm, A.nfp, b, S.prow, lane); }
		__syncthreads();
		if (on) env_build(S.kns, C, S.tab + C.eoff, S.tab + C.hoff, lane, 64);
		__syncthreads();
		if (on) form_problem<KM>(A, M, b, lane);
	}
}
