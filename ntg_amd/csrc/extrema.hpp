// extrema.hpp -- ntg_batch_extrema: the global minimum and maximum over the horizon of every certifiable trajectory row, each enclosed to a
// tolerance and each with the time of the attained value, by adaptive bisection of the row's Bezier polygons.  The fixed subdivision of
// envelope.hpp / envelope_sos.hpp spends 2^nsub polygons on every knot interval; here only the pieces that can still hold the extremum are
// halved, so the work follows the data: a per-row work list in LDS, compacted at every level.
//
// Per (problem, row), the definition of include/ntg_amd.h:
//   level 0   the row's polygon on every knot interval j of its basis class: env_rows' sequence of operations for a linear row, sos_rows' for
//             a sum-of-squares row, both at nsub = 0: the same builders (env_poly_lin, sos_poly) on piece 0 of 1.
//   level L   U / V = smallest / largest end value seen, with its time (smaller time on equal values): every lane folds in the ends of its
//             pieces, the wave reduces by the butterfly.  A piece is open if its polygon reaches below U - tol (above V + tol); the others
//             retire into Rlo / Rhi.  An open piece is split in the middle by de Casteljau (0.5 * (a + b) per new point, the ends carried over).
//   The loop ends when no piece is open (OK), at max_depth (DEPTH) or with more than NTG_EXTREMA_CAP open pieces (FULL).
// A wavefront owns a problem and walks its rows one after the other.  Level 0 is a strided loop over the intervals; afterwards lane p takes
// parent p of the work list, splits it in registers and evaluates both children.  Open children go back into the list at the position the
// ballots of the wave give them: parent order first, left child first.  The list is updated in place: every lane has its parent in
// registers before any lane stores a child (the loads of a level precede its stores in program order, and LDS operations of one wave complete
// in order), so there is no workgroup barrier inside the level loop and nothing waits on data: the level loop runs at most max_depth + 1 times.
//
//   extrema_shared_kernel  plans on their own grid: persistent workgroups of four waves; the row, term and class tables, the product tables,
//                          the extraction weights and the breaks of every basis class are built once into LDS; every wave then streams problems
//                          with its own x row, parameter row and work list.
//   extrema_pp_kernel      per-problem grids: the same, with breaks and weights of the wave's own problem.
// No scratch in HBM, no atomics, nothing depends on the batch around a problem.  Every private array is indexed by unrolled loop counters only.
// The levels themselves (ext_levels) take the row as a source of level-0 polygons and a threshold flag: ext_row hands them a row of the plan,
// forms.hpp a declared form, separation.hpp the squared difference of two trajectories, with its "not plo >= s2" in the opening rule.
// ratio_levels (ratios.hpp) is its twin on pairs of polygons, kept in step by hand: whoever edits ext_levels edits that one too -- and
// trig_levels (trig.hpp, pieces of up to four angle polygons) and, the third loop on polygons proper, minmax_levels (minmax.hpp: pieces of
// up to 16 member polygons, which do not fit the registers, so that loop sweeps the members twice per level over a member-major list).  By
// hand, but held in step by the tests: tests/bisect_oracle.py is the one written sequence all of them are tested against.  One loop
// templated over the piece gives the same bits (tests/golden holds both to recorded results) and no worse registers, but it cost the extrema
// and separation kernels 1 to 2 % of their rate, more than their run-to-run spread: DESIGN.md has the figures.  The two loops share the
// de Casteljau split (ext_split) and the epilogue (ExtOut: a row's outputs, and the violation of a problem folded over its rows).
// extrema_*_kernel and separation_kernel carve their dynamic LDS by hand, in the order of BisectLds (ntg_dev.hpp), which sizes their launch:
// formed from that description the pointers cost separation_kernel 3 to 5 us a call.  Whoever moves a table here moves it there.
#pragma once
#include "wave_ops.hpp"
#include "envelope_sos.hpp"

// a declared-form call's own parameter row of problem b (forms, ratios, trig; minmax.hpp writes the loop out), by one wave
__device__ __forceinline__ void cert_stage_fprm(const double *fprm, int nfp, int b, double *row, int lane)
{
	for (int i = lane; i < nfp; i += 64) row[i] = fprm[(size_t)b * nfp + i];
}

// (value, time) minimum / maximum: on equal values the smaller time; a NaN is never taken
__device__ __forceinline__ void ext_take_min(double &v, double &t, double ov, double ot) { if (ov < v || (ov == v && ot < t)) { v = ov; t = ot; } }
__device__ __forceinline__ void ext_take_max(double &v, double &t, double ov, double ot) { if (ov > v || (ov == v && ot < t)) { v = ov; t = ot; } }
template <int BIT>
__device__ __forceinline__ void ext_xchg_step(double &u, double &tu, double &v, double &tv)
{
	const double ou = lane_xchg<BIT>(u), otu = lane_xchg<BIT>(tu), ov = lane_xchg<BIT>(v), otv = lane_xchg<BIT>(tv);
	ext_take_min(u, tu, ou, otu); ext_take_max(v, tv, ov, otv);
}
// every lane gets the wave's (U, tU), (V, tV)
__device__ __forceinline__ void ext_wave_ends(double &u, double &tu, double &v, double &tv)
{
	ext_xchg_step<1>(u, tu, v, tv); ext_xchg_step<2>(u, tu, v, tv); ext_xchg_step<4>(u, tu, v, tv);
	ext_xchg_step<8>(u, tu, v, tv); ext_xchg_step<16>(u, tu, v, tv); ext_xchg_step<32>(u, tu, v, tv);
}
template <int BIT>
__device__ __forceinline__ void ext_range_step(double &lo, double &hi)
{
	const double ol = lane_xchg<BIT>(lo), oh = lane_xchg<BIT>(hi);
	if (ol < lo) lo = ol;
	if (oh > hi) hi = oh;
}
__device__ __forceinline__ void ext_wave_range(double &lo, double &hi)
{
	ext_range_step<1>(lo, hi); ext_range_step<2>(lo, hi); ext_range_step<4>(lo, hi);
	ext_range_step<8>(lo, hi); ext_range_step<16>(lo, hi); ext_range_step<32>(lo, hi);
}

// time of end i / 2^lam of interval j (inv = 2^-lam): product and sum rounded separately, the interval's own end at local parameter 1
__device__ __forceinline__ double ext_time(const double *kn, const double *hh, int j, int i, int lam, double inv)
{
#pragma clang fp contract(off)
	const double f = hh[j] * ((double)i * inv);
	return i == (1 << lam) ? kn[j + 1] : kn[j] + f;
}

// point D of a polygon, by unrolled counters
template <int KD>
__device__ __forceinline__ double ext_last(const EnvPoly<KD> &P, int D)
{
	long long v = 0;   // (bits of the one point taken, zeros of the others: a chain of "if (s == D) v = P.b[s]" is compiled into an indexed load, which puts P in scratch)
#pragma unroll
	for (int s = 0; s < KD; s++) v |= s == D ? __double_as_longlong(P.b[s]) : 0ll;
	return __longlong_as_double(v);
}

// split in the middle by de Casteljau: Rp becomes the right child, Lp the left one
template <int KD>
__device__ __forceinline__ void ext_split(EnvPoly<KD> &Lp, EnvPoly<KD> &Rp, int Dl)
{
#pragma unroll
	for (int s = 0; s < KD; s++) Lp.b[s] = 0.0;
	Lp.b[0] = Rp.b[0];
#pragma unroll
	for (int r = 1; r < KD; r++) {
		if (r <= Dl) {
#pragma unroll
			for (int s = 0; s < KD - r; s++) { if (s <= Dl - r) Rp.b[s] = 0.5 * (Rp.b[s] + Rp.b[s + 1]); }
			Lp.b[r] = Rp.b[0];
		}
	}
}

// what the levels need of a row: the breaks and interval lengths of its basis class, the number l of its knot intervals, the degree D of its
// polygon, and the call's figures.  s2 (THR instances only): a piece whose polygon does not reach below s2 retires at once
struct ExtRun { const double *kn, *hh; int l, D, max_depth, sides; double tol, s2; };

// The definition's levels for one row, by one wave: src(j) is the row's level-0 polygon on knot interval j.  res = {min_lo, min_hi, max_lo,
// max_hi}, tw = {t_min, t_max}; every lane returns the same figures.  THR = false is ntg_batch_extrema's opening rule; THR = true adds
// ntg_batch_separation's "and not plo >= s2" to the lower side
template <int KM, bool THR, class Src>
__device__ __forceinline__ void ext_levels(const ExtRun &Q, const ExtLds &M, const Src &src, int lane, double (&res)[4], double (&tw)[2], int &status, int &npieces)
{
	constexpr int KD = 2 * KM - 1;
	const int D = Q.D;
	const double *kn = Q.kn, *hh = Q.hh;
	const double tol = Q.tol;
	const bool s_lo = Q.sides & 1, s_hi = Q.sides & 2;
	const unsigned long long below = (1ull << lane) - 1ull;
	double U = INFINITY, tU = INFINITY, V = -INFINITY, tV = INFINITY;   // the same in every lane after a level's butterfly
	double Rlo = INFINITY, Rhi = -INFINITY;   // retired pieces, this lane's
	double Olo = INFINITY, Ohi = -INFINITY;   // open pieces of the current level, this lane's: they retire when the loop stops on them
	bool nan = false;
	int nopen = 0;

	// level 0: lane + 64 t takes interval j.  Two rounds over the intervals: the ends first, then the decisions, which need U and V of the whole
	// level.  One polygon per lane (l <= 64) stays in registers between the rounds; otherwise the second round forms it again, the same way.
	const int npass = (Q.l + 63) >> 6;
	EnvPoly<KD> P;
#pragma unroll
	for (int s = 0; s < KD; s++) P.b[s] = 0.0;
	for (int it = 0; it < 2 * npass; it++) {
		const bool second = it >= npass;
		const int j = lane + 64 * (second ? it - npass : it);
		const bool on = j < Q.l;
		if (on && (!second || npass > 1)) P = src(j);
		if (!second) {
			if (on) {
				const double e0 = P.b[0], e1 = ext_last<KD>(P, D);
				ext_take_min(U, tU, e0, kn[j]); ext_take_min(U, tU, e1, kn[j + 1]);
				ext_take_max(V, tV, e0, kn[j]); ext_take_max(V, tV, e1, kn[j + 1]);
			}
			if (it == npass - 1) ext_wave_ends(U, tU, V, tV);
		} else {
			double plo = 0.0, phi = 0.0;
			bool open = false;
			if (on) {
				P.range(D, plo, phi);
				nan = nan || plo != plo || phi != phi;
				open = (s_lo && plo < U - tol && !(THR && plo >= Q.s2)) || (s_hi && phi > V + tol);
			}
			const unsigned long long m = __ballot(open);
			const int pos = nopen + __popcll(m & below);
			if (open) {
				if (plo < Olo) Olo = plo;
				if (phi > Ohi) Ohi = phi;
				if (pos < NTG_EXTREMA_CAP) {
#pragma unroll
					for (int s = 0; s < KD; s++) { if (s <= D) M.list[pos * KD + s] = P.b[s]; }
					M.keys[pos] = (long long)j << 32;
				}
			} else if (on) {
				if (plo < Rlo) Rlo = plo;
				if (phi > Rhi) Rhi = phi;
			}
			nopen += __popcll(m);
		}
	}
	npieces = Q.l;

	// levels: the open pieces of level lam are in the list; their children form level lam + 1
	status = NTG_EXTREMA_OK;
	for (int lam = 0; lam <= Q.max_depth; lam++) {
		if (nopen == 0) break;
		if (lam == Q.max_depth || nopen > NTG_EXTREMA_CAP) {
			status = lam == Q.max_depth ? NTG_EXTREMA_DEPTH : NTG_EXTREMA_FULL;
			if (Olo < Rlo) Rlo = Olo;
			if (Ohi > Rhi) Rhi = Ohi;
			break;
		}
		Olo = INFINITY; Ohi = -INFINITY;
		const bool on = lane < nopen;
		int Dl = D;
		asm volatile("" : "+s"(Dl));   // the degree's masks are formed where they are used, level by level: hoisted out of the loop they fill the scalar registers
		const double inv = 1.0 / (double)(1 << (lam + 1));
		EnvPoly<KD> Lp, Rp;
		long long key = 0;
		__builtin_amdgcn_wave_barrier();   // the list of level lam is whole
		if (on) {
#pragma unroll
			for (int s = 0; s < KD; s++) Rp.b[s] = s <= Dl ? M.list[lane * KD + s] : 0.0;
			key = M.keys[lane];
		} else {
#pragma unroll
			for (int s = 0; s < KD; s++) Rp.b[s] = 0.0;
		}
		__builtin_amdgcn_wave_barrier();   // every parent is in registers before a child is stored
		const int j = (int)(key >> 32), i = (int)(key & 0xffffffffll);
		ext_split<KD>(Lp, Rp, Dl);   // Rp becomes the right child, Lp the left one
		double llo = 0.0, lhi = 0.0, rlo = 0.0, rhi = 0.0;
		if (on) {
			const double e0 = Lp.b[0], em = Rp.b[0], e1 = ext_last<KD>(Rp, Dl);
			const double t0 = ext_time(kn, hh, j, 2 * i, lam + 1, inv), tm = ext_time(kn, hh, j, 2 * i + 1, lam + 1, inv), t1 = ext_time(kn, hh, j, 2 * i + 2, lam + 1, inv);
			ext_take_min(U, tU, e0, t0); ext_take_min(U, tU, em, tm); ext_take_min(U, tU, e1, t1);
			ext_take_max(V, tV, e0, t0); ext_take_max(V, tV, em, tm); ext_take_max(V, tV, e1, t1);
			Lp.range(Dl, llo, lhi); Rp.range(Dl, rlo, rhi);
			nan = nan || llo != llo || lhi != lhi || rlo != rlo || rhi != rhi;
		}
		ext_wave_ends(U, tU, V, tV);
		const bool openL = on && ((s_lo && llo < U - tol && !(THR && llo >= Q.s2)) || (s_hi && lhi > V + tol));
		const bool openR = on && ((s_lo && rlo < U - tol && !(THR && rlo >= Q.s2)) || (s_hi && rhi > V + tol));
		const unsigned long long mL = __ballot(openL), mR = __ballot(openR);
		const int posL = __popcll(mL & below) + __popcll(mR & below), posR = posL + (openL ? 1 : 0);
		if (openL) {
			if (llo < Olo) Olo = llo;
			if (lhi > Ohi) Ohi = lhi;
			if (posL < NTG_EXTREMA_CAP) {
#pragma unroll
				for (int s = 0; s < KD; s++) { if (s <= Dl) M.list[posL * KD + s] = Lp.b[s]; }
				M.keys[posL] = ((long long)j << 32) | (long long)(2 * i);
			}
		} else if (on) {
			if (llo < Rlo) Rlo = llo;
			if (lhi > Rhi) Rhi = lhi;
		}
		if (openR) {
			if (rlo < Olo) Olo = rlo;
			if (rhi > Ohi) Ohi = rhi;
			if (posR < NTG_EXTREMA_CAP) {
#pragma unroll
				for (int s = 0; s < KD; s++) { if (s <= Dl) M.list[posR * KD + s] = Rp.b[s]; }
				M.keys[posR] = ((long long)j << 32) | (long long)(2 * i + 1);
			}
		} else if (on) {
			if (rlo < Rlo) Rlo = rlo;
			if (rhi > Rhi) Rhi = rhi;
		}
		npieces += 2 * nopen;
		nopen = __popcll(mL) + __popcll(mR);
	}
	__builtin_amdgcn_wave_barrier();   // the next row's list starts behind this row's loads
	ext_wave_range(Rlo, Rhi);
	if (__ballot(nan) != 0ull) {
		res[0] = res[1] = res[2] = res[3] = NAN; tw[0] = tw[1] = NAN; status = NTG_EXTREMA_NAN;
	} else {
		res[0] = Rlo; res[1] = U; res[2] = V; res[3] = Rhi; tw[0] = tU; tw[1] = tV;
	}
}

// level-0 polygons of a row of ntg_batch_extrema: a linear row's (env_poly_lin, the whole interval: piece 0 of 1) or a sum-of-squares row's
template <int KM>
struct ExtRowSrc {
	const ExtArgs &A; const SosTables &T; const ExtLds &M;
	bool lin; const double *lr; int row, cl, D; SosRow R; EnvClass C;
	__device__ __forceinline__ EnvPoly<2 * KM - 1> operator()(int j) const
	{
		constexpr int KD = 2 * KM - 1;
		EnvPoly<KD> P;
		if (lin) {
			const EnvPoly<KM> L = env_poly_lin<KM>(A.lin, lr, cl, D, C, M.tab, M.xrow, j, 0, 0);
#pragma unroll
			for (int s = 0; s < KD; s++) P.b[s] = 0.0;
#pragma unroll
			for (int s = 0; s < KM; s++) P.b[s] = L.b[s];
		} else P = sos_poly<KM>(T, row - A.lin.nltc, R, C, M.wl, M.tab, M.xrow, M.prow, j, 0, 0);
		return P;
	}
};

// one row of problem b
template <int KM>
__device__ __forceinline__ void ext_row(const ExtArgs &A, const SosTables &T, const ExtLds &M, int row, int lane, double (&res)[4], double (&tw)[2], int &status, int &npieces)
{
	const bool lin = row < A.lin.nltc;
	const double *lr = A.lin.ltc + (size_t)(lin ? row : 0) * A.lin.nz;
	const SosRow R = T.row[lin ? 0 : row - A.lin.nltc];   // (a linear row reads none of it)
	int cl = R.cl, D = R.D, flag = R.flag;
	if (lin) { const EnvRowShape sh = env_row_shape(A.lin, T.c, lr); cl = sh.cl; D = sh.D; flag = sh.flag; }
	if (!flag) {
		res[0] = -INFINITY; res[1] = INFINITY; res[2] = -INFINITY; res[3] = INFINITY;
		tw[0] = tw[1] = NAN; status = NTG_EXTREMA_NONE; npieces = 0;
		return;
	}
	const EnvClass C = T.c[cl];
	const ExtRun Q{M.kns + A.q.koff[cl], M.tab + C.hoff, C.l, D, A.q.max_depth, A.q.sides, A.q.tol, INFINITY};
	const ExtRowSrc<KM> src{A, T, M, lin, lr, row, cl, D, R, C};
	ext_levels<KM, false>(Q, M, src, lane, res, tw, status, npieces);
}

// The outputs of a problem, by one wave: every row's figures as they come, and the largest violation of the attained (av, ak) and of the
// certified (cv, ck) values over the rows folded so far
struct ExtOut {
	const CertBisect &Q; int lane;
	double av = 0.0, cv = 0.0; long long ak = -1, ck = -1;
	__device__ __forceinline__ bool want_v() const { return Q.viol || Q.where; }
	__device__ __forceinline__ void row(size_t at, const double (&res)[4], const double (&tw)[2], int status, int npieces) const
	{
		if (lane != 0) return;
		if (Q.ext) { Q.ext[4 * at] = res[0]; Q.ext[4 * at + 1] = res[1]; Q.ext[4 * at + 2] = res[2]; Q.ext[4 * at + 3] = res[3]; }
		if (Q.when) { Q.when[2 * at] = tw[0]; Q.when[2 * at + 1] = tw[1]; }
		if (Q.status) Q.status[at] = status;
		if (Q.npieces) Q.npieces[at] = npieces;
	}
	// row idx with the bounds (l, u)
	__device__ __forceinline__ void fold(double l, double u, const double (&res)[4], int idx)
	{
		const double a = env_viol(l, u, res[1], res[2]), c = env_viol(l, u, res[0], res[3]);   // of the attained values, of the certified ones
		env_take(av, ak, a, (a > 0.0 || a != a) ? (long long)idx : -1ll);
		env_take(cv, ck, c, (c > 0.0 || c != c) ? (long long)idx : -1ll);
	}
	__device__ __forceinline__ void problem(int b) const
	{
		if (!want_v() || lane != 0) return;
		if (Q.viol) { Q.viol[2 * (size_t)b] = ak < 0 ? 0.0 : av; Q.viol[2 * (size_t)b + 1] = ck < 0 ? 0.0 : cv; }
		if (Q.where) { Q.where[2 * (size_t)b] = (int)ak; Q.where[2 * (size_t)b + 1] = (int)ck; }
	}
};

// every row of problem b, by one wave whose x row and parameter row are in M
template <int KM>
__device__ __forceinline__ void ext_problem(const ExtArgs &A, const SosTables &T, const ExtLds &M, int b, int lane)
{
	const int nltc = A.lin.nltc, nrow = nltc + A.sos.nrow;
	ExtOut O{A.q, lane};
	for (int row = 0; row < nrow; row++) {
		double res[4], tw[2];
		int status, npieces;
		ext_row<KM>(A, T, M, row, lane, res, tw, status, npieces);
		O.row((size_t)b * nrow + row, res, tw, status, npieces);
		if (O.want_v()) {   // (every row has flag 1: the host has refused the others)
			const int slot = row < nltc ? A.lin.slot0 + row : A.sos.slot0 + row - nltc;
			O.fold(A.g.lower[(size_t)b * A.g.nbounds + slot], A.g.upper[(size_t)b * A.g.nbounds + slot], res, row);
		}
	}
	O.problem(b);
}

template <int NT, int KM>
__global__ void __launch_bounds__(NT)
extrema_shared_kernel(ExtArgs A)
{
	extern __shared__ __attribute__((aligned(16))) char smem_raw[];
	constexpr int NW = NT / 64, KD = 2 * KM - 1;
	__shared__ SosTables T;
	const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
	double *wl = reinterpret_cast<double *>(smem_raw);    // the product tables, unfolded
	double *tab = wl + NTG_SOS_WFULL;                     // weights and interval lengths of every basis class
	double *kns = tab + A.g.ne;                           // breaks of every basis class
	double *mine = kns + A.q.nk + (size_t)wave * (A.g.nC + A.sos.np + NTG_EXTREMA_CAP * (KD + 1));
	double *xrow = mine, *prow = xrow + A.g.nC, *list = prow + A.sos.np;
	const ExtLds M{wl, tab, kns, xrow, prow, list, reinterpret_cast<long long *>(list + NTG_EXTREMA_CAP * KD)};
	sos_stage(A.sos, A.g, T, tid);
	sos_unfold(A.sos, wl, tid, NT);
	env_build_classes(A.g, tab, kns, A.q.koff, tid, NT);
	for (int b0 = blockIdx.x * NW; b0 < A.g.batch; b0 += gridDim.x * NW) {
		const int b = b0 + wave;
		if (b >= A.g.batch) continue;
		__builtin_amdgcn_wave_barrier();   // the problem before is done with the rows
		env_stage_rows(A.g, &A.sos, b, xrow, prow, lane, 64);
		__builtin_amdgcn_wave_barrier();
		ext_problem<KM>(A, T, M, b, lane);
	}
}

// per-problem grids: one basis class; every wave builds the weights of its own problem
template <int NT, int KM>
__global__ void __launch_bounds__(NT)
extrema_pp_kernel(ExtArgs A)
{
	extern __shared__ __attribute__((aligned(16))) char smem_raw[];
	constexpr int NW = NT / 64, KD = 2 * KM - 1;
	__shared__ SosTables T;
	const EnvClass C = A.g.c[0];
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	double *wl = reinterpret_cast<double *>(smem_raw);
	double *tab = wl + NTG_SOS_WFULL + (size_t)wave * (A.g.ne + A.q.nk + A.g.nC + A.sos.np + NTG_EXTREMA_CAP * (KD + 1));
	double *kns = tab + A.g.ne, *xrow = kns + A.q.nk, *prow = xrow + A.g.nC, *list = prow + A.sos.np;
	const ExtLds M{wl, tab, kns, xrow, prow, list, reinterpret_cast<long long *>(list + NTG_EXTREMA_CAP * KD)};
	sos_stage(A.sos, A.g, T, threadIdx.x);
	sos_unfold(A.sos, wl, threadIdx.x, NT);
	const int per_pass = gridDim.x * NW;
	for (int b0 = 0; b0 < A.g.batch; b0 += per_pass) {   // (the same trip count for every wave of the grid: the barriers below are uniform)
		const int b = b0 + blockIdx.x * NW + wave;
		const bool on = b < A.g.batch;
		__syncthreads();
		if (on) env_stage_pp(A.g, &A.sos, b, kns, xrow, prow, lane);
		__syncthreads();
		if (on) env_build(kns, C, tab + C.eoff, tab + C.hoff, lane, 64);
		__syncthreads();
		if (on) ext_problem<KM>(A, T, M, b, lane);
	}
}
