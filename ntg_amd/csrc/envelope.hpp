// envelope.hpp -- ntg_batch_envelope: bounds of every flag entry D^r z_o and of every linear trajectory row that hold at EVERY time of a
// piece of a knot interval, not at sampled times: the trajectory is a B-spline, so on a knot interval every entry is a polynomial and its
// Bezier control polygon encloses it (convex hull property); halving the piece shrinks the enclosure quadratically.
//
// Per output and knot interval j = [a, b] (span mu = k - 1 + j (k - m) of the augmented knots):
//   1. interval polygon: beta_i = blossom of the spline at (a x (k-1-i), b x i), i = 0 .. k-1 -- the de Boor triangle of refine.hpp (RefTri)
//      with these arguments.  Its weights do not depend on the coefficients: E[j][i][q] = weight of c[mu - q], the triangle run on the k
//      unit vectors, built once (env_build).  A thread forms beta_i = c[mu] + sum_{q >= 1} E[j][i][q] (c[mu - q] - c[mu]): the weights of a
//      control point sum to 1, and in this form a constant spline gives its constant back bit for bit.
//   2. derivative r: r rounds of beta'_i = d / (b - a) (beta_{i+1} - beta_i), d the degree before the round.
//   3. piece i of the 2^nsub equal parts of the interval, local parameter [s0, s1] = [i, i + 1] / 2^nsub: de Casteljau at s1 keeping the
//      left polygon (skipped for the last piece), then at s0 / s1 keeping the right one (skipped for the first piece).  No knot enters.
//   lo / hi = min / max of the piece's k - r control points; a NaN among them stays in both (the rule of kkt.hpp).
// A linear trajectory row sum_v ltc[v] z_v names entries of one basis class; on a piece every named entry's polygon is degree-elevated to
// the largest degree among them and the polygons are summed with the row's coefficients, v ascending: the row's own Bezier polygon, so
// terms that cancel do cancel.  The certified violation of a problem is the largest max(l - row_lo, row_hi - u, 0) over rows and pieces,
// with the key row * npc + piece; ties go to the smallest key, a NaN wins over every number (the first NaN by key).
//
//   envelope_shared_kernel  plans on their own grid.  A workgroup builds the weights of every basis class once (one thread per weight)
//                           into LDS, then streams problems from a persistent loop: coalesced read of the x row into LDS, one thread per
//                           (output, piece) -- pieces are the fast index, so a wave's stores of one entry are consecutive words of the
//                           [nz][npc] plane -- then one thread per (row, piece); the maximum over the workgroup by the wave butterfly and
//                           the waves in index order (check.hpp's scheme).  Pieces past an output's own count are written as the empty set.
//   envelope_pp_kernel      per-problem grids: one wavefront per problem (four problems per workgroup pass) with its own breaks, x row
//                           and weights in LDS.
// A problem is owned by one workgroup (one wave), every number by one thread: no scratch in HBM, no atomics, nothing depends on the batch
// around a problem.  Every private array is indexed by unrolled loop counters only (KM bounds them: the smallest instance that holds the
// plan's largest order), so nothing goes to the private segment.
#pragma once
#include <cmath>
#include "ntg_dev.hpp"
#include "wave_ops.hpp"
#include "refine.hpp"

// the smaller / larger of the two; a NaN, once in, stays
__device__ __forceinline__ double env_min(double a, double b) { return (b < a || b != b) ? b : a; }
__device__ __forceinline__ double env_max(double a, double b) { return (b > a || b != b) ? b : a; }

// the (violation, key) maximum of two candidates; key < 0: nothing seen.  Larger wins, a NaN over every number, ties and NaNs by the smaller key.
__device__ __forceinline__ void env_take(double &bv, long long &bk, double ov, long long ok)
{
	if (ok < 0) return;
	const bool bn = bv != bv, on = ov != ov;
	bool take;
	if (bk < 0) take = true;
	else if (bn || on) take = on && (!bn || ok < bk);
	else take = ov > bv || (ov == bv && ok < bk);
	if (take) { bv = ov; bk = ok; }
}
template <int BIT>
__device__ __forceinline__ void env_xchg_step(double &bv, long long &bk)
{
	const double ov = lane_xchg<BIT>(bv);
	const long long ok = __double_as_longlong(lane_xchg<BIT>(__longlong_as_double(bk)));   // (moved as two 32-bit halves: no arithmetic on it)
	env_take(bv, bk, ov, ok);
}

// Extraction weights and interval lengths of one basis class from its breaks kn[0 .. l]: E[(j k + i) k + q], hh[j].  One thread per weight.
__device__ __forceinline__ void env_build(const double *kn, const EnvClass C, double *E, double *hh, int tid, int nthr)
{
	const int k = C.k, kk = k * k;
	const RefKnots tau{kn, nullptr, C.l, k, C.m, C.l * (k - C.m) + C.m};
	for (int e = tid; e < C.l * kk; e += nthr) {
		const int j = e / kk, iq = e - j * kk, i = iq / k, q = iq - i * k;
		const int mu = k - 1 + j * (k - C.m);
		const double a = kn[j], b = kn[j + 1];
		RefTri tri;
#pragma unroll
		for (int s = 0; s < NTG_MAX_ORDER - 1; s++) {
			const bool on = s < k - 1;
			tri.tl[s] = on ? tau(mu - s) : 0.0; tri.tr[s] = on ? tau(mu + 1 + s) : 1.0; tri.tx[s] = on ? (s < k - 1 - i ? a : b) : 0.0;
		}
		double d[NTG_MAX_ORDER];
#pragma unroll
		for (int s = 0; s < NTG_MAX_ORDER; s++) d[s] = s == q ? 1.0 : 0.0;
		E[e] = tri.run(k, d);
	}
	for (int j = tid; j < C.l; j += nthr) hh[j] = kn[j + 1] - kn[j];
}

// A Bezier polygon of degree d <= KM - 1 in registers; every loop is unrolled, the degree only masks.
template <int KM>
struct EnvPoly {
	double b[KM];
	// interval polygon of z_o: E = the interval's [k][k] weights, c -> c[mu]
	__device__ __forceinline__ void extract(const double *E, const double *c, int k)
	{
		const double c0 = c[0];
		double dc[KM];
#pragma unroll
		for (int q = 1; q < KM; q++) dc[q] = q < k ? c[-q] - c0 : 0.0;
#pragma unroll
		for (int i = 0; i < KM; i++) {
			double acc = c0;
			if (i < k) {
#pragma unroll
				for (int q = 1; q < KM; q++) { if (q < k) acc += E[i * k + q] * dc[q]; }
			}
			b[i] = acc;
		}
	}
	// one difference round on an interval of length h: degree d -> d - 1
	__device__ __forceinline__ void diff(int d, double h)
	{
		const double f = (double)d / h;
#pragma unroll
		for (int i = 0; i < KM - 1; i++) { if (i < d) b[i] = f * (b[i + 1] - b[i]); }
	}
	// de Casteljau at s, the polygon on [0, s] stays
	__device__ __forceinline__ void cut_left(int d, double s)
	{
#pragma unroll
		for (int lev = 1; lev < KM; lev++) {
			if (lev <= d) {
#pragma unroll
				for (int i = KM - 1; i >= lev; i--) { if (i <= d) b[i] = b[i - 1] + s * (b[i] - b[i - 1]); }
			}
		}
	}
	// de Casteljau at s, the polygon on [s, 1] stays
	__device__ __forceinline__ void cut_right(int d, double s)
	{
#pragma unroll
		for (int lev = 1; lev < KM; lev++) {
			if (lev <= d) {
#pragma unroll
				for (int i = 0; i < KM - lev; i++) { if (i <= d - lev) b[i] = b[i] + s * (b[i + 1] - b[i]); }
			}
		}
	}
	// piece [i, i + 1] / (msk + 1) of the interval
	__device__ __forceinline__ void piece(int d, int i, int msk)
	{
		if (i < msk) cut_left(d, (double)(i + 1) / (double)(msk + 1));
		if (i > 0) cut_right(d, (double)i / (double)(i + 1));
	}
	// degree d -> d + 1 (d + 1 <= KM - 1): b'_i = i / (d + 1) b_{i-1} + (1 - i / (d + 1)) b_i
	__device__ __forceinline__ void elevate(int d)
	{
#pragma unroll
		for (int i = KM - 1; i >= 1; i--) {
			if (i == d + 1) b[i] = b[i - 1];
			else if (i <= d) { const double a = (double)i / (double)(d + 1); b[i] = a * b[i - 1] + (1.0 - a) * b[i]; }
		}
	}
	__device__ __forceinline__ void range(int d, double &lo, double &hi) const
	{
		lo = hi = b[0];
#pragma unroll
		for (int i = 1; i < KM; i++) { if (i <= d) { lo = env_min(lo, b[i]); hi = env_max(hi, b[i]); } }
	}
};

// entry envelope of problem b: one thread per (output, piece), pieces fastest
template <int KM>
__device__ __forceinline__ void env_entries(const EnvArgs &A, const double *tab, const double *xrow, int b, int tid, int nthr)
{
	const CertLin &L = A.lin;
	const int npc = A.npc, nsub = A.nsub, msk = (1 << nsub) - 1;
	for (int e = tid; e < L.nout * npc; e += nthr) {
		const int o = e / npc, q = e - o * npc, dm = L.d[o];
		const EnvClass C = A.g.c[L.cls[o]];
		const size_t base = ((size_t)b * L.nz + L.iz[o]) * npc + q;
		if (q >= (C.l << nsub)) {   // past the output's own pieces: the empty set
			for (int r = 0; r < dm; r++) {
				if (A.lo) A.lo[base + (size_t)r * npc] = INFINITY;
				if (A.hi) A.hi[base + (size_t)r * npc] = -INFINITY;
			}
			continue;
		}
		const int j = q >> nsub, i = q & msk;
		EnvPoly<KM> P;
		P.extract(tab + C.eoff + j * C.k * C.k, xrow + L.iC[o] + C.k - 1 + j * (C.k - C.m), C.k);
		const double h = tab[C.hoff + j];
		for (int r = 0; r < dm; r++) {
			const int d = C.k - 1 - r;
			double lo = 0.0, hi = 0.0;   // r >= k: the zero polynomial
			if (d >= 0) {
				if (r > 0) P.diff(d + 1, h);
				EnvPoly<KM> Q = P;
				Q.piece(d, i, msk);
				Q.range(d, lo, hi);
			}
			if (A.lo) A.lo[base + (size_t)r * npc] = lo;
			if (A.hi) A.hi[base + (size_t)r * npc] = hi;
		}
	}
}

// Shape of linear row lr: the basis class cl of the first entry it names (class of output 0 for a row of zeros), the largest degree D among
// the entries it names (0 for a row of zeros: the zero polynomial, one point), and flag = 1 when every entry named belongs to one class.
// c: the class table (a kernel's argument or its copy in LDS)
struct EnvRowShape { int cl, D, flag; };
__device__ __forceinline__ EnvRowShape env_row_shape(const CertLin &L, const EnvClass *c, const double *lr)
{
	EnvRowShape R{-1, 0, 1};
	int first = -1;
	for (int o = 0; o < L.nout; o++) {
		const int k = c[L.cls[o]].k;
		for (int r = 0; r < L.d[o]; r++) {
			if (lr[L.iz[o] + r] == 0.0) continue;
			if (first < 0) first = o;
			else if (L.cls[o] != L.cls[first]) R.flag = 0;
			if (r < k) { if (R.cl < 0) R.cl = L.cls[o]; R.D = max(R.D, k - 1 - r); }
		}
	}
	if (R.cl < 0) R.cl = L.cls[0];
	return R;
}

// Polygon (degree D) of linear row lr of class cl = C on piece [i, i + 1] / (msk + 1) of knot interval j: every named entry's polygon
// elevated to D, the polygons summed with the row's coefficients, v ascending
template <int KM>
__device__ __forceinline__ EnvPoly<KM> env_poly_lin(const CertLin &L, const double *lr, int cl, int D, const EnvClass C, const double *tab, const double *xrow, int j, int i, int msk)
{
	const double h = tab[C.hoff + j];
	EnvPoly<KM> S;
#pragma unroll
	for (int s = 0; s < KM; s++) S.b[s] = 0.0;
	for (int o = 0; o < L.nout; o++) {
		if (L.cls[o] != cl) continue;   // (a row that names another class has flag 0: the host refuses it, or no statement is made)
		const double *lo_r = lr + L.iz[o];
		bool any = false;
		for (int r = 0; r < L.d[o] && r < C.k; r++) any = any || lo_r[r] != 0.0;
		if (!any) continue;
		EnvPoly<KM> P;
		P.extract(tab + C.eoff + j * C.k * C.k, xrow + L.iC[o] + C.k - 1 + j * (C.k - C.m), C.k);
		for (int r = 0; r < L.d[o] && r < C.k; r++) {
			const int d = C.k - 1 - r;
			if (r > 0) P.diff(d + 1, h);
			const double w = lo_r[r];
			if (w != 0.0) {
				EnvPoly<KM> Q = P;
				Q.piece(d, i, msk);
				for (int t = d; t < D; t++) Q.elevate(t);
#pragma unroll
				for (int s = 0; s < KM; s++) { if (s <= D) S.b[s] += w * Q.b[s]; }
			}
		}
	}
	return S;
}

// violation of the bounds [l, u] by a row enclosed in [lo, hi]: max(l - lo, hi - u, 0), an infinite bound is none
__device__ __forceinline__ double env_viol(double l, double u, double lo, double hi)
{
	double v = 0.0;
	if (fabs(l) < NTG_INF_BOUND) v = env_max(v, l - lo);
	if (fabs(u) < NTG_INF_BOUND) v = env_max(v, hi - u);
	return v;
}

// row envelope of problem b and its largest certified violation (bv, bk): one thread per (row, piece), pieces fastest
template <int KM>
__device__ __forceinline__ void env_rows(const EnvArgs &A, const double *tab, const double *xrow, int b, int tid, int nthr, double &bv, long long &bk)
{
	const CertLin &L = A.lin;
	const int npc = A.npc, nsub = A.nsub, msk = (1 << nsub) - 1;
	const bool want_v = A.viol || A.where;
	for (int e = tid; e < L.nltc * npc; e += nthr) {
		const int row = e / npc, q = e - row * npc;
		const double *lr = L.ltc + (size_t)row * L.nz;
		const EnvRowShape R = env_row_shape(L, A.g.c, lr);
		const EnvClass C = A.g.c[R.cl];
		const bool live = q < (C.l << nsub);
		double lo = INFINITY, hi = -INFINITY;
		if (live) {
			const EnvPoly<KM> S = env_poly_lin<KM>(L, lr, R.cl, R.D, C, tab, xrow, q >> nsub, q & msk, msk);
			S.range(R.D, lo, hi);
		}
		const size_t at = ((size_t)b * L.nltc + row) * npc + q;
		if (A.row_lo) A.row_lo[at] = lo;
		if (A.row_hi) A.row_hi[at] = hi;
		if (want_v && live) {
			const double v = env_viol(A.g.lower[(size_t)b * A.g.nbounds + L.slot0 + row], A.g.upper[(size_t)b * A.g.nbounds + L.slot0 + row], lo, hi);
			env_take(bv, bk, v, (v > 0.0 || v != v) ? (long long)e : -1ll);
		}
	}
}

__device__ __forceinline__ void env_wave_max(double &bv, long long &bk)
{
	env_xchg_step<1>(bv, bk); env_xchg_step<2>(bv, bk); env_xchg_step<4>(bv, bk);
	env_xchg_step<8>(bv, bk); env_xchg_step<16>(bv, bk); env_xchg_step<32>(bv, bk);
}
// the workgroup's maximum, into thread 0: the wave butterfly, then the waves' slots r_v / r_k [NT / 64] in index order
template <int NT>
__device__ __forceinline__ void env_group_max(double &bv, long long &bk, double *r_v, long long *r_k, int tid)
{
	env_wave_max(bv, bk);
	if ((tid & 63) == 0) { r_v[tid >> 6] = bv; r_k[tid >> 6] = bk; }
	__syncthreads();
	if (tid == 0) { for (int w = 1; w < NT / 64; w++) env_take(bv, bk, r_v[w], r_k[w]); }
}
// problem b's violation and its key as (row, piece)
__device__ __forceinline__ void env_store_max(double *viol, int *where, int npc, int b, double bv, long long bk)
{
	if (viol) viol[b] = bk < 0 ? 0.0 : bv;
	if (where) { where[2 * (size_t)b] = bk < 0 ? -1 : (int)(bk / npc); where[2 * (size_t)b + 1] = bk < 0 ? -1 : (int)(bk % npc); }
}

// Shared grids, once per workgroup: weights and interval lengths of every basis class into tab.  kns: room for the breaks -- of every class
// at koff[c], where they are needed afterwards, or (koff null) of one class at a time
__device__ __forceinline__ void env_build_classes(const CertBase &G, double *tab, double *kns, const int *koff, int tid, int nthr)
{
	for (int c = 0; c < G.nclass; c++) {
		const EnvClass C = G.c[c];
		double *kn = kns + (koff ? koff[c] : 0);
		__syncthreads();   // the class before is done with kn
		for (int i = tid; i <= C.l; i += nthr) kn[i] = G.knots[c][i];
		__syncthreads();
		env_build(kn, C, tab + C.eoff, tab + C.hoff, tid, nthr);
	}
	__syncthreads();
}
// the x row of problem b and, for sum-of-squares rows that read one (S and S->np non-zero), its parameter row into LDS
__device__ __forceinline__ void env_stage_rows(const CertBase &G, const CertSos *S, int b, double *xrow, double *prow, int tid, int nthr)
{
	const double *src = G.x + (size_t)b * G.nC;
	for (int i = tid; i < G.nC; i += nthr) xrow[i] = src[i];
	if (S) { for (int i = tid; i < S->np; i += nthr) prow[i] = S->prm[(size_t)b * S->pp_prm + i]; }
}
// per-problem grids, by the wave that owns problem b: its breaks (one class), then its rows
__device__ __forceinline__ void env_stage_pp(const CertBase &G, const CertSos *S, int b, double *kn, double *xrow, double *prow, int lane)
{
	const int l = G.c[0].l;
	const double *kt = G.knots[0] + (size_t)b * (l + 1);
	for (int i = lane; i <= l; i += 64) kn[i] = kt[i];
	env_stage_rows(G, S, b, xrow, prow, lane, 64);
}

template <int NT, int KM>
__global__ void __launch_bounds__(NT)
envelope_shared_kernel(EnvArgs A)
{
	extern __shared__ __attribute__((aligned(16))) char smem_raw[];
	__shared__ double r_v[NT / 64];
	__shared__ long long r_k[NT / 64];
	double *tab = reinterpret_cast<double *>(smem_raw);   // weights and interval lengths of every basis class
	double *xrow = tab + A.g.ne;                          // [nC]
	double *kn = xrow + A.g.nC;                           // breaks of the class being set up
	const int tid = threadIdx.x;
	env_build_classes(A.g, tab, kn, nullptr, tid, NT);
	const bool want_e = A.lo || A.hi, want_v = A.viol || A.where, want_r = A.row_lo || A.row_hi || want_v;
	for (int b = blockIdx.x; b < A.g.batch; b += gridDim.x) {
		env_stage_rows(A.g, nullptr, b, xrow, nullptr, tid, NT);
		__syncthreads();
		if (want_e) env_entries<KM>(A, tab, xrow, b, tid, NT);
		if (want_r) {
			double bv = 0.0; long long bk = -1;
			env_rows<KM>(A, tab, xrow, b, tid, NT, bv, bk);
			if (want_v) {
				env_group_max<NT>(bv, bk, r_v, r_k, tid);
				if (tid == 0) env_store_max(A.viol, A.where, A.npc, b, bv, bk);
			}
		}
		__syncthreads();   // xrow and the waves' slots are free again
	}
}

// per-problem grids: one basis class, so every output has the shape of class 0
template <int NT, int KM>
__global__ void __launch_bounds__(NT)
envelope_pp_kernel(EnvArgs A)
{
	extern __shared__ __attribute__((aligned(16))) char smem_raw[];
	constexpr int NW = NT / 64;
	const EnvClass C = A.g.c[0];
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	double *tab = reinterpret_cast<double *>(smem_raw) + (size_t)wave * (A.g.ne + A.g.nC + C.l + 1);
	double *xrow = tab + A.g.ne, *kn = xrow + A.g.nC;
	const bool want_e = A.lo || A.hi, want_v = A.viol || A.where, want_r = A.row_lo || A.row_hi || want_v;
	const int per_pass = gridDim.x * NW;
	for (int b0 = 0; b0 < A.g.batch; b0 += per_pass) {   // (the same trip count for every wave of the grid: the barriers below are uniform)
		const int b = b0 + blockIdx.x * NW + wave;
		const bool on = b < A.g.batch;
		__syncthreads();
		if (on) env_stage_pp(A.g, nullptr, b, kn, xrow, nullptr, lane);
		__syncthreads();
		if (on) env_build(kn, C, tab + C.eoff, tab + C.hoff, lane, 64);
		__syncthreads();
		if (on) {
			if (want_e) env_entries<KM>(A, tab, xrow, b, lane, 64);
			if (want_r) {
				double bv = 0.0; long long bk = -1;
				env_rows<KM>(A, tab, xrow, b, lane, 64, bv, bk);
				if (want_v) {
					env_wave_max(bv, bk);
					if (lane == 0) env_store_max(A.viol, A.where, A.npc, b, bv, bk);
				}
			}
		}
	}
}
