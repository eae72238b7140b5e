// envelope_sos.hpp -- ntg_batch_envelope_sos: bounds, at EVERY time of a piece of a knot interval, of the nonlinear trajectory rows a family
// declares as sums of squares of shifted flag entries, c(z) = sum_t (z[v_t] - s_t)^2 (NtgFamily::sos, family_module.hpp).  On a knot interval
// every flag entry is a polynomial, so the row is one too, and its Bezier control polygon encloses it like envelope.hpp's enclose the linear rows.
//
// Per (row, piece), with the polygons of envelope.hpp (EnvPoly::extract / diff / piece, the same arithmetic as ntg_batch_envelope's entries):
//   1. factor of term t: the control points beta_i, i = 0 .. d, of entry v_t on the piece, shifted: p_i = beta_i - s_t (a derivative of
//      order >= k is the zero polynomial: d = 0, p_0 = -s_t).
//   2. its square, degree 2 d: g_m = sum_{i + j = m} W_d[i][j] p_i p_j, i ascending, W_d[i][j] = C(d,i) C(d,j) / C(2d,m) -- the Bezier
//      product of the polygon with itself.  The tables come from the host (exact integer binomials, one rounding each).
//   3. the row's polygon: every term's polygon elevated to D = max_t 2 d_t (EnvPoly::elevate) and the polygons summed in term order.
//   lo / hi = min / max of its D + 1 points (env_min / env_max: a NaN stays in both).
// The certified violation of a problem is the largest max(l - lo, hi - u, 0) over certified rows and pieces, key row * npc + piece, with
// env_take's order.
//
//   envelope_sos_shared_kernel  plans on their own grid: persistent workgroups; the row, term and class tables, the product tables and the
//                               extraction weights of every basis class are built once into LDS, then per problem the x row and the parameter row are staged in LDS and one
//                               thread takes one (row, piece), pieces fastest; the maximum by the wave butterfly, then the waves in index order.
//   envelope_sos_pp_kernel      per-problem grids: one wavefront per problem with its own breaks, weights, x row and parameter row in LDS.
// A problem is owned by one workgroup (one wave), every number by one thread: no scratch in HBM, no atomics, nothing depends on the batch
// around a problem.  A thread holds the row's polygon (2 KM - 1 doubles) and one factor polygon (KM doubles); the points of a square are
// formed one at a time and added to the row's polygon as they come.  Only a term of lower degree than its row -- no built-in declaration has
// one -- is formed whole first, because it has to be elevated.  Every private array is indexed by unrolled loop counters only.
#pragma once
#include "envelope.hpp"

// point m of the square of P (degree d): W = the unfolded table of degree d, [d + 1][d + 1]
template <int KM, int M>
__device__ __forceinline__ double sos_square_point(const EnvPoly<KM> &P, const double *W, int d)
{
	double acc = 0.0;
#pragma unroll
	for (int a = 0; a < KM; a++) {
		const int c = M - a;
		if (c >= 0 && c < KM) { if (a <= d && c <= d) acc += W[a * (d + 1) + c] * P.b[a] * P.b[c]; }
	}
	return acc;
}
template <int KM, int M = 0>
__device__ __forceinline__ void sos_square_into(EnvPoly<2 * KM - 1> &S, const EnvPoly<KM> &P, const double *W, int d, bool add)
{
	if constexpr (M < 2 * KM - 1) {
		if (M <= 2 * d) { const double g = sos_square_point<KM, M>(P, W, d); S.b[M] = add ? S.b[M] + g : g; }
		else if (!add) S.b[M] = 0.0;
		sos_square_into<KM, M + 1>(S, P, W, d, add);
	}
}

// the product tables of every degree, unfolded from the triangles of the kernel argument: one thread per weight
__device__ __forceinline__ void sos_unfold(const CertSos &A, double *wl, int tid, int nthr)
{
	for (int e = tid; e < NTG_SOS_WFULL; e += nthr) {
		int d = 0;
		while (e >= ntg_sos_wfull(d + 1)) d++;
		const int rem = e - ntg_sos_wfull(d), i = rem / (d + 1), j = rem - i * (d + 1), a = min(i, j), c = max(i, j);
		wl[e] = A.w[ntg_sos_wtri(d) + a * (d + 1) - a * (a - 1) / 2 + (c - a)];
	}
}

// the row, term and class tables a thread looks up by its own row: copied from the kernel argument into LDS, every copy at a uniform index
struct SosTables { SosRow row[NTG_SOS_MAXROWS]; SosTerm term[NTG_SOS_MAXROWS][NTG_SOS_MAXTERMS]; EnvClass c[NTG_MAX_OUT]; };
__device__ __forceinline__ void sos_stage(const CertSos &A, const CertBase &G, SosTables &T, int tid)
{
	for (int j = 0; j < A.nrow; j++) {
		if (tid == 0) T.row[j] = A.row[j];
		for (int t = 0; t < NTG_SOS_MAXTERMS; t++) { if (tid == 0) T.term[j][t] = A.term[j][t]; }
	}
	for (int c = 0; c < G.nclass; c++) { if (tid == 0) T.c[c] = G.c[c]; }
}

// Polygon (degree R.D) of sum-of-squares row `row` = R of class C on piece [i, i + 1] / (msk + 1) of knot interval j: the squares of its
// terms' shifted polygons, elevated to R.D where they are lower, summed in term order
template <int KM>
__device__ __forceinline__ EnvPoly<2 * KM - 1> sos_poly(const SosTables &T, int row, const SosRow R, const EnvClass C, const double *wl, const double *tab, const double *xrow,
                                                        const double *prow, int j, int i, int msk)
{
	constexpr int KD = 2 * KM - 1;
	const double h = tab[C.hoff + j];
	EnvPoly<KD> S;
#pragma unroll
	for (int s = 0; s < KD; s++) S.b[s] = 0.0;
	for (int t = 0; t < R.nt; t++) {
		const SosTerm Q = T.term[row][t];
		const double sh = Q.s0 + (Q.poff >= 0 ? prow[Q.poff] : 0.0);
		EnvPoly<KM> P;
		int d = C.k - 1 - Q.r;
		if (d >= 0) {
			P.extract(tab + C.eoff + j * C.k * C.k, xrow + Q.iC + C.k - 1 + j * (C.k - C.m), C.k);
			for (int r = 1; r <= Q.r; r++) P.diff(C.k - r, h);
			P.piece(d, i, msk);
		} else {   // a derivative of order >= k: the zero polynomial
			d = 0;
			P.b[0] = 0.0;
		}
#pragma unroll
		for (int s = 0; s < KM; s++) P.b[s] = s <= d ? P.b[s] - sh : 0.0;
		const double *W = wl + ntg_sos_wfull(d);
		if (2 * d == R.D) sos_square_into<KM>(S, P, W, d, true);
		else {   // a term of lower degree than the row: its polygon whole, elevated, then added
			EnvPoly<KD> G;
			sos_square_into<KM>(G, P, W, d, false);
			for (int u = 2 * d; u < R.D; u++) G.elevate(u);
#pragma unroll
			for (int s = 0; s < KD; s++) { if (s <= R.D) S.b[s] += G.b[s]; }
		}
	}
	return S;
}

// row envelope of problem b and its largest certified violation (bv, bk): one thread per (row, piece), pieces fastest
template <int KM>
__device__ __forceinline__ void sos_rows(const SosArgs &A, const SosTables &T, const double *wl, const double *tab, const double *xrow, const double *prow, int b, int tid, int nthr,
                                         double &bv, long long &bk)
{
	const int nrow = A.sos.nrow, npc = A.npc, nsub = A.nsub, msk = (1 << nsub) - 1;
	const bool want_v = A.viol || A.where;
	for (int e = tid; e < nrow * npc; e += nthr) {
		const int row = e / npc, q = e - row * npc;
		const SosRow R = T.row[row];
		const EnvClass C = T.c[R.cl];
		const bool live = q < (C.l << nsub);
		double lo = INFINITY, hi = -INFINITY;   // past the class's own pieces: the empty set
		if (live && !R.flag) { lo = -INFINITY; hi = INFINITY; }   // no statement
		else if (live) {
			const EnvPoly<2 * KM - 1> S = sos_poly<KM>(T, row, R, C, wl, tab, xrow, prow, q >> nsub, q & msk, msk);
			S.range(R.D, lo, hi);
		}
		const size_t at = ((size_t)b * nrow + row) * npc + q;
		if (A.q_lo) A.q_lo[at] = lo;
		if (A.q_hi) A.q_hi[at] = hi;
		if (want_v && live && R.flag) {
			const double v = env_viol(A.g.lower[(size_t)b * A.g.nbounds + A.sos.slot0 + row], A.g.upper[(size_t)b * A.g.nbounds + A.sos.slot0 + row], lo, hi);
			env_take(bv, bk, v, (v > 0.0 || v != v) ? (long long)e : -1ll);
		}
	}
}

template <int NT, int KM>
__global__ void __launch_bounds__(NT)
envelope_sos_shared_kernel(SosArgs A)
{
	extern __shared__ __attribute__((aligned(16))) char smem_raw[];
	__shared__ double r_v[NT / 64];
	__shared__ long long r_k[NT / 64];
	__shared__ SosTables T;
	double *wl = reinterpret_cast<double *>(smem_raw);    // the product tables, unfolded
	double *tab = wl + NTG_SOS_WFULL;                     // weights and interval lengths of every basis class
	double *xrow = tab + A.g.ne;                          // [nC]
	double *prow = xrow + A.g.nC;                         // [np]
	double *kn = prow + A.sos.np;                         // breaks of the class being set up
	const int tid = threadIdx.x;
	sos_stage(A.sos, A.g, T, tid);
	sos_unfold(A.sos, wl, tid, NT);
	env_build_classes(A.g, tab, kn, nullptr, tid, NT);
	const bool want_v = A.viol || A.where;
	for (int b = blockIdx.x; b < A.g.batch; b += gridDim.x) {
		env_stage_rows(A.g, &A.sos, b, xrow, prow, tid, NT);
		__syncthreads();
		double bv = 0.0; long long bk = -1;
		sos_rows<KM>(A, T, wl, tab, xrow, prow, b, tid, NT, bv, bk);
		if (want_v) {
			env_group_max<NT>(bv, bk, r_v, r_k, tid);
			if (tid == 0) env_store_max(A.viol, A.where, A.npc, b, bv, bk);
		}
		__syncthreads();   // xrow, prow and the waves' slots are free again
	}
}

// per-problem grids: one basis class, so every row has the pieces of class 0
template <int NT, int KM>
__global__ void __launch_bounds__(NT)
envelope_sos_pp_kernel(SosArgs A)
{
	extern __shared__ __attribute__((aligned(16))) char smem_raw[];
	constexpr int NW = NT / 64;
	__shared__ SosTables T;
	const EnvClass C = A.g.c[0];
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	double *wl = reinterpret_cast<double *>(smem_raw);
	double *tab = wl + NTG_SOS_WFULL + (size_t)wave * (A.g.ne + A.g.nC + A.sos.np + C.l + 1);
	double *xrow = tab + A.g.ne, *prow = xrow + A.g.nC, *kn = prow + A.sos.np;
	const bool want_v = A.viol || A.where;
	sos_stage(A.sos, A.g, T, threadIdx.x);
	sos_unfold(A.sos, wl, threadIdx.x, NT);
	const int per_pass = gridDim.x * NW;
	for (int b0 = 0; b0 < A.g.batch; b0 += per_pass) {   // (the same trip count for every wave of the grid: the barriers below are uniform)
		const int b = b0 + blockIdx.x * NW + wave;
		const bool on = b < A.g.batch;
		__syncthreads();
		if (on) env_stage_pp(A.g, &A.sos, b, kn, xrow, prow, lane);
		__syncthreads();
		if (on) env_build(kn, C, tab + C.eoff, tab + C.hoff, lane, 64);
		__syncthreads();
		if (on) {
			double bv = 0.0; long long bk = -1;
			sos_rows<KM>(A, T, wl, tab, xrow, prow, b, lane, 64, bv, bk);
			if (want_v) {
				env_wave_max(bv, bk);
				if (lane == 0) env_store_max(A.viol, A.where, A.npc, b, bv, bk);
			}
		}
	}
}
