// minmax.hpp -- ntg_batch_minmax: the minimum and maximum over the horizon of lattice expressions of quadratic forms declared AT THE CALL,
//   h_g(t) = OUTER_k INNER_{j in clause k} m_kj(t),   m = q_form(z(t)) + d,   d = c + fprm_b[pc],   OUTER, INNER = min or max:
// the outside of a convex polygon (min over t of the max of its face distances), the inside of a box or lane, a corridor of overlapping boxes
// (max over t of min over boxes of max over faces), coverage by beacons.  min and max are monotone, so with every member enclosed by
// [plo_m, phi_m] on a piece the same expression over the plo and over the phi encloses h_g, and its value at a piece end is the expression
// over the members' end points, which de Casteljau carries over bit for bit.  The bisection of extrema.hpp applies to pieces that carry the
// polygons of all members of a group.
//
// Per (problem, group), the definition of include/ntg_amd.h:
//   level 0   mm_member_poly on every knot interval j of the group's basis class: form_poly (forms.hpp) of the member's form, + d on every
//             point, elevated to the group's degree.
//   levels    minmax_levels: ext_levels (extrema.hpp) on pieces of nm polygons -- a third twin of that loop beside ratio_levels and
//             trig_levels, kept in step by hand and held in step by the tests: tests/bisect_oracle.py is the one written sequence all of
//             them are tested against (this one by tests/test_gpu_minmax.py).  It shares ext_split, ext_time, ext_last, ExtRun and ExtOut
//             with them.
// A piece of 16 polygons of 11 points is 176 doubles: it is never in registers at once.  The work list is MEMBER-MAJOR, list[member][slot]
// [PW], and a level makes two sweeps over the members:
//   sweep 1   member by member: load the parent's polygon, split it (ext_split), fold plo, phi of both children and the value at the new end
//             into the lattice figures (MmFig).  Nothing is stored.
//   then      the open / retire decisions and the ballots, as in ext_levels.
//   sweep 2   member by member: load the parent's polygon again, split it again, store the open children at their new slots.
// The list is updated in place, not double buffered: within one wave the loads of member m precede its stores in program order, LDS
// operations of a wave complete in order, and the stores of member m touch nothing of member m + 1.  Splitting twice costs a few hundred
// flops per piece and frees the loop from any dependence on the register budget; a second list would halve the members or the waves that fit
// the LDS.  Level 0 follows the same plan: the members' polygons are formed once for the figures and once more for the stores (and a third
// time on grids of more than 64 intervals, where a lane's figures do not stay in registers between the rounds).
// A polygon takes PW = KP | 1 doubles of the list (KP its points: 6, 11 or 19), an odd number, so that the lanes' 8-byte reads of their own
// slots spread over the banks.  No member is pruned: every member of an open piece is halved.
//
//   minmax_shared_kernel  plans on their own grid: persistent workgroups of four, two or one waves; the product tables, the extraction weights
//                         and the breaks of every basis class are built once into LDS; every wave then streams problems with its own x row,
//                         fprm row and work list.  No workgroup barrier after the set-up.
//   minmax_pp_kernel      per-problem grids: the same, with breaks and weights of the wave's own problem.
// The form, term, member and group tables are read from the kernel argument at wave-uniform indices.  No scratch in HBM, no atomics, nothing
// depends on the batch around a problem.  Every private array is indexed by unrolled loop counters only.
#pragma once
#include "forms.hpp"

// what the kernels know of a member's form: its row, the group's class, its terms in the flat table
struct MinmaxFormOf {
	const MinmaxArgs &A; FormRow R; EnvClass C;
	__device__ __forceinline__ const FormTerm &term(int t) const { return A.term[R.t0 + t]; }
};

// One figure of the lattice expression, folded member by member in declared order: vi over the members of the current clause, vo over the
// clauses closed so far; wi / wo the member that decides each.  A strict comparison keeps the first on a tie: the smallest index in a
// clause, the smallest clause in the group.  mx: max (true) or min
struct MmFig {
	double vi = 0.0, vo = 0.0; int wi = -1, wo = -1;
	__device__ __forceinline__ void member(double v, int m, bool first, bool mx) { if (first || (mx ? v > vi : v < vi)) { vi = v; wi = m; } }
	__device__ __forceinline__ void clause(bool first, bool mx) { if (first || (mx ? vi > vo : vi < vo)) { vo = vi; wo = wi; } }
};

// (value, time, member) minimum / maximum: on equal values the smaller time, on equal times the smaller member; a NaN is never taken
__device__ __forceinline__ void mm_take_min(double &v, double &t, double &w, double ov, double ot, double ow) { if (ov < v || (ov == v && (ot < t || (ot == t && ow < w)))) { v = ov; t = ot; w = ow; } }
__device__ __forceinline__ void mm_take_max(double &v, double &t, double &w, double ov, double ot, double ow) { if (ov > v || (ov == v && (ot < t || (ot == t && ow < w)))) { v = ov; t = ot; w = ow; } }
template <int BIT>
__device__ __forceinline__ void mm_xchg_step(double &u, double &tu, double &wu, double &v, double &tv, double &wv)
{
	const double ou = lane_xchg<BIT>(u), otu = lane_xchg<BIT>(tu), owu = lane_xchg<BIT>(wu), ov = lane_xchg<BIT>(v), otv = lane_xchg<BIT>(tv), owv = lane_xchg<BIT>(wv);
	mm_take_min(u, tu, wu, ou, otu, owu); mm_take_max(v, tv, wv, ov, otv, owv);
}
// every lane gets the wave's (U, tU, wU), (V, tV, wV)
__device__ __forceinline__ void mm_wave_ends(double &u, double &tu, double &wu, double &v, double &tv, double &wv)
{
	mm_xchg_step<1>(u, tu, wu, v, tv, wv); mm_xchg_step<2>(u, tu, wu, v, tv, wv); mm_xchg_step<4>(u, tu, wu, v, tv, wv);
	mm_xchg_step<8>(u, tu, wu, v, tv, wv); mm_xchg_step<16>(u, tu, wu, v, tv, wv); mm_xchg_step<32>(u, tu, wu, v, tv, wv);
}

// The level-0 polygon of member m of a group on knot interval j: its form's polygon (form_poly: rule 1 of ntg_batch_forms), + d on every
// point unless the member declares none (pc = -1 and c = 0.0), elevated to the group's degree
template <int KM, int KP>
__device__ __forceinline__ EnvPoly<KP> mm_member_poly(const MinmaxArgs &A, const MinmaxGroup &G, const EnvClass C, const ExtLds &M, int m, int j)
{
#pragma clang fp contract(off)
	constexpr int KD = 2 * KM - 1;
	static_assert(KP <= KD, "the instance's polygon is a prefix of form_poly's");
	const MinmaxMem Q = A.mem[G.m0 + m];
	const MinmaxFormOf F{A, A.row[Q.form], C};
	EnvPoly<KD> P = form_poly<KM>(F, M, j);
	const int D = F.R.D;
	if (Q.pc >= 0 || Q.c != 0.0) {
		const double d = Q.c + (Q.pc >= 0 ? M.prow[Q.pc] : 0.0);
#pragma unroll
		for (int s = 0; s < KD; s++) { if (s <= D) P.b[s] = P.b[s] + d; }
	}
	for (int u = D; u < G.D; u++) P.elevate(u);
	EnvPoly<KP> R;
#pragma unroll
	for (int s = 0; s < KP; s++) R.b[s] = P.b[s];
	return R;
}

// polygon of member m in slot pos of the work list
template <int KP>
__device__ __forceinline__ double *mm_slot(double *list, int m, int pos) { return list + ((size_t)m * NTG_EXTREMA_CAP + pos) * (KP | 1); }
template <int KP>
__device__ __forceinline__ void mm_store(double *list, int m, int pos, const EnvPoly<KP> &P, int D)
{
	double *e = mm_slot<KP>(list, m, pos);
#pragma unroll
	for (int s = 0; s < KP; s++) { if (s <= D) e[s] = P.b[s]; }
}
template <int KP>
__device__ __forceinline__ void mm_load(double *list, int m, int pos, bool on, EnvPoly<KP> &P, int D)
{
	const double *e = mm_slot<KP>(list, m, pos);
	if (on) {
#pragma unroll
		for (int s = 0; s < KP; s++) P.b[s] = s <= D ? e[s] : 0.0;
	} else {
#pragma unroll
		for (int s = 0; s < KP; s++) P.b[s] = 0.0;
	}
}

// The definition's levels for one group, by one wave.  res = {min_lo, min_hi, max_lo, max_hi}, tw = {t_min, t_max}, wh = the members that
// decide h_g there; every lane returns the same figures
template <int KM, int KP>
__device__ __forceinline__ void minmax_levels(const ExtRun &Q, const ExtLds &M, const MinmaxArgs &A, const MinmaxGroup &G, const EnvClass C, int lane,
                                              double (&res)[4], double (&tw)[2], int (&wh)[2], int &status, int &npieces)
{
	const int D = Q.D, nm = G.nm;
	const bool omax = G.outer == NTG_MINMAX_MAX, imax = G.inner == NTG_MINMAX_MAX;
	const unsigned int clast = G.clast;
	const double *kn = Q.kn, *hh = Q.hh;
	const double tol = Q.tol;
	const bool s_lo = Q.sides & 1, s_hi = Q.sides & 2;
	const unsigned long long below = (1ull << lane) - 1ull;
	double U = INFINITY, tU = INFINITY, wU = -1.0, V = -INFINITY, tV = INFINITY, wV = -1.0;   // the same in every lane after a level's butterfly
	double Rlo = INFINITY, Rhi = -INFINITY;   // retired pieces, this lane's
	double Olo = INFINITY, Ohi = -INFINITY;   // open pieces of the current level, this lane's: they retire when the loop stops on them
	bool nan = false;
	int nopen = 0;

	// level 0: lane + 64 t takes interval j.  npass rounds for the ends; then per pass a round for the decisions, which need U and V of the
	// whole level, and a round that forms the members' polygons again and stores those of the open pieces.  A lane's figures (l <= 64) stay
	// in registers between the first two; otherwise the decisions' round forms them again, the same way.
	const int npass = (Q.l + 63) >> 6;
	double plo = 0.0, phi = 0.0;
	bool pnan = false, open = false;
	int pos = 0;
	unsigned long long mo = 0ull;
	for (int it = 0; it < 3 * npass; it++) {
		const int mode = it < npass ? 0 : 1 + ((it - npass) & 1);   // 0: ends, 1: decisions, 2: stores
		const int j = lane + 64 * (mode == 0 ? it : (it - npass) >> 1);
		const bool on = j < Q.l;
		const int nmr = (mode == 1 && npass == 1) || (mode == 2 && mo == 0ull) ? 0 : nm;
		MmFig fLo, fHi, fE0, fE1;
		bool cf = true, gf = true;
		for (int m = 0; m < nmr; m++) {
			EnvPoly<KP> P;
#pragma unroll
			for (int s = 0; s < KP; s++) P.b[s] = 0.0;
			if (on) P = mm_member_poly<KM, KP>(A, G, C, M, m, j);
			if (mode == 2) {
				if (open && pos < NTG_EXTREMA_CAP) mm_store<KP>(M.list, m, pos, P, D);
				continue;
			}
			double lo, hi;
			P.range(D, lo, hi);
			fLo.member(lo, m, cf, imax); fHi.member(hi, m, cf, imax);
			fE0.member(P.b[0], m, cf, imax); fE1.member(ext_last<KP>(P, D), m, cf, imax);
			if (m == 0) pnan = false;
			pnan = pnan || lo != lo || hi != hi;
			cf = false;
			if ((clast >> m) & 1u) {
				fLo.clause(gf, omax); fHi.clause(gf, omax); fE0.clause(gf, omax); fE1.clause(gf, omax);
				gf = false; cf = true;
			}
		}
		if (nmr > 0 && mode != 2) { plo = fLo.vo; phi = fHi.vo; }
		if (mode == 0) {
			if (on) {
				mm_take_min(U, tU, wU, fE0.vo, kn[j], (double)fE0.wo); mm_take_min(U, tU, wU, fE1.vo, kn[j + 1], (double)fE1.wo);
				mm_take_max(V, tV, wV, fE0.vo, kn[j], (double)fE0.wo); mm_take_max(V, tV, wV, fE1.vo, kn[j + 1], (double)fE1.wo);
			}
			if (it == npass - 1) mm_wave_ends(U, tU, wU, V, tV, wV);
		} else if (mode == 1) {
			open = false;
			if (on) {
				nan = nan || pnan;
				open = (s_lo && plo < U - tol) || (s_hi && phi > V + tol);
			}
			mo = __ballot(open);
			pos = nopen + __popcll(mo & below);
			if (open) {
				if (plo < Olo) Olo = plo;
				if (phi > Ohi) Ohi = phi;
			} else if (on) {
				if (plo < Rlo) Rlo = plo;
				if (phi > Rhi) Rhi = phi;
			}
		} else {
			if (open && pos < NTG_EXTREMA_CAP) M.keys[pos] = (long long)j << 32;
			nopen += __popcll(mo);
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
		asm volatile("" : "+s"(Dl));   // the degree's masks are formed where they are used, level by level (ext_levels)
		const double inv = 1.0 / (double)(1 << (lam + 1));
		long long key = 0;
		__builtin_amdgcn_wave_barrier();   // the list of level lam is whole
		if (on) key = M.keys[lane];
		const int j = (int)(key >> 32), i = (int)(key & 0xffffffffll);
		// sweep 1: the figures of both children (the outer ends are the parent's: taken a level ago, same values, same times, same members)
		MmFig fLlo, fLhi, fRlo, fRhi, fEm;
		bool cf = true, gf = true;
		for (int m = 0; m < nm; m++) {
			EnvPoly<KP> Lp, Rp;
			mm_load<KP>(M.list, m, lane, on, Rp, Dl);
			ext_split<KP>(Lp, Rp, Dl);   // Rp becomes the right child, Lp the left one
			double a0, a1, b0, b1;
			Lp.range(Dl, a0, a1); Rp.range(Dl, b0, b1);
			nan = nan || a0 != a0 || a1 != a1 || b0 != b0 || b1 != b1;
			fLlo.member(a0, m, cf, imax); fLhi.member(a1, m, cf, imax); fRlo.member(b0, m, cf, imax); fRhi.member(b1, m, cf, imax);
			fEm.member(Rp.b[0], m, cf, imax);
			cf = false;
			if ((clast >> m) & 1u) {
				fLlo.clause(gf, omax); fLhi.clause(gf, omax); fRlo.clause(gf, omax); fRhi.clause(gf, omax); fEm.clause(gf, omax);
				gf = false; cf = true;
			}
		}
		const double llo = fLlo.vo, lhi = fLhi.vo, rlo = fRlo.vo, rhi = fRhi.vo;
		if (on) {
			const double tm = ext_time(kn, hh, j, 2 * i + 1, lam + 1, inv);
			mm_take_min(U, tU, wU, fEm.vo, tm, (double)fEm.wo);
			mm_take_max(V, tV, wV, fEm.vo, tm, (double)fEm.wo);
		}
		mm_wave_ends(U, tU, wU, V, tV, wV);
		const bool openL = on && ((s_lo && llo < U - tol) || (s_hi && lhi > V + tol));
		const bool openR = on && ((s_lo && rlo < U - tol) || (s_hi && rhi > V + tol));
		const unsigned long long mL = __ballot(openL), mR = __ballot(openR);
		const int posL = __popcll(mL & below) + __popcll(mR & below), posR = posL + (openL ? 1 : 0);
		if (openL) {
			if (llo < Olo) Olo = llo;
			if (lhi > Ohi) Ohi = lhi;
		} else if (on) {
			if (llo < Rlo) Rlo = llo;
			if (lhi > Rhi) Rhi = lhi;
		}
		if (openR) {
			if (rlo < Olo) Olo = rlo;
			if (rhi > Ohi) Ohi = rhi;
		} else if (on) {
			if (rlo < Rlo) Rlo = rlo;
			if (rhi > Rhi) Rhi = rhi;
		}
		// sweep 2: the open children into the list, member by member; every lane has member m of its parent in registers before a child is stored
		if ((mL | mR) != 0ull) {
			for (int m = 0; m < nm; m++) {
				EnvPoly<KP> Lp, Rp;
				mm_load<KP>(M.list, m, lane, on, Rp, Dl);
				__builtin_amdgcn_wave_barrier();
				ext_split<KP>(Lp, Rp, Dl);
				if (openL && posL < NTG_EXTREMA_CAP) mm_store<KP>(M.list, m, posL, Lp, Dl);
				if (openR && posR < NTG_EXTREMA_CAP) mm_store<KP>(M.list, m, posR, Rp, Dl);
				__builtin_amdgcn_wave_barrier();
			}
			if (openL && posL < NTG_EXTREMA_CAP) M.keys[posL] = ((long long)j << 32) | (long long)(2 * i);
			if (openR && posR < NTG_EXTREMA_CAP) M.keys[posR] = ((long long)j << 32) | (long long)(2 * i + 1);
		}
		npieces += 2 * nopen;
		nopen = __popcll(mL) + __popcll(mR);
	}
	__builtin_amdgcn_wave_barrier();   // the next group's list starts behind this group's loads
	ext_wave_range(Rlo, Rhi);
	if (__ballot(nan) != 0ull) {
		res[0] = res[1] = res[2] = res[3] = NAN; tw[0] = tw[1] = NAN; wh[0] = wh[1] = -1; status = NTG_EXTREMA_NAN;
	} else {
		res[0] = Rlo; res[1] = U; res[2] = V; res[3] = Rhi; tw[0] = tU; tw[1] = tV; wh[0] = (int)wU; wh[1] = (int)wV;
	}
}

// every group of problem b, by one wave whose x row and fprm row are in M
template <int KM, int KP>
__device__ __forceinline__ void minmax_problem(const MinmaxArgs &A, const ExtLds &M, int b, int lane)
{
	const int ngroup = A.ngroup;
	ExtOut O{A.q, lane};
	for (int g = 0; g < ngroup; g++) {
		const MinmaxGroup &G = A.grp[g];
		const EnvClass C = A.g.c[G.cl];
		const ExtRun Q{M.kns + A.q.koff[G.cl], M.tab + C.hoff, C.l, G.D, A.q.max_depth, A.q.sides, A.q.tol, INFINITY};
		double res[4], tw[2];
		int wh[2], status, npieces;
		minmax_levels<KM, KP>(Q, M, A, G, C, lane, res, tw, wh, status, npieces);
		const size_t at = (size_t)b * ngroup + g;
		O.row(at, res, tw, status, npieces);
		if (A.which && lane == 0) { A.which[2 * at] = wh[0]; A.which[2 * at + 1] = wh[1]; }
		if (O.want_v()) O.fold(A.glo[at], A.ghi[at], res, g);
	}
	O.problem(b);
}

template <int KM, int KP>
__global__ void __launch_bounds__(256)
minmax_shared_kernel(MinmaxArgs A)
{
	extern __shared__ __attribute__((aligned(16))) char smem_raw[];
	__shared__ unsigned int pas[NTG_FORM_PASCAL * NTG_FORM_PASCAL];
	const int NT = blockDim.x, NW = NT >> 6;
	const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
	const ExtStage S = ntg_minmax_layout(A).wave(reinterpret_cast<double *>(smem_raw), wave);
	const ExtLds M = S.view();   // (the kernel stages through S; everything below reads through M)
	form_build_products(S.wl, pas, tid, NT);
	env_build_classes(A.g, S.tab, S.kns, A.q.koff, tid, NT);
	for (int b0 = blockIdx.x * NW; b0 < A.g.batch; b0 += gridDim.x * NW) {
		const int b = b0 + wave;
		if (b >= A.g.batch) continue;
		__builtin_amdgcn_wave_barrier();   // the problem before is done with the rows
		env_stage_rows(A.g, nullptr, b, S.xrow, nullptr, lane, 64);
		// cert_stage_fprm (extrema.hpp) written out, here and below: through the helper these instances allocate their registers differently
		for (int i = lane; i < A.nfp; i += 64) S.prow[i] = A.fprm[(size_t)b * A.nfp + i];
		__builtin_amdgcn_wave_barrier();
		minmax_problem<KM, KP>(A, M, b, lane);
	}
}

// per-problem grids: one basis class; every wave builds the weights of its own problem
template <int KM, int KP>
__global__ void __launch_bounds__(256)
minmax_pp_kernel(MinmaxArgs A)
{
	extern __shared__ __attribute__((aligned(16))) char smem_raw[];
	__shared__ unsigned int pas[NTG_FORM_PASCAL * NTG_FORM_PASCAL];
	const int NT = blockDim.x, NW = NT >> 6;
	const EnvClass C = A.g.c[0];
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const ExtStage S = ntg_minmax_layout(A).wave(reinterpret_cast<double *>(smem_raw), wave);
	const ExtLds M = S.view();
	form_build_products(S.wl, pas, threadIdx.x, NT);
	const int per_pass = gridDim.x * NW;
	for (int b0 = 0; b0 < A.g.batch; b0 += per_pass) {   // (the same trip count for every wave of the grid: the barriers below are uniform)
		const int b = b0 + blockIdx.x * NW + wave;
		const bool on = b < A.g.batch;
		__syncthreads();
		if (on) {
			env_stage_pp(A.g, nullptr, b, S.kns, S.xrow, nullptr, lane);
			for (int i = lane; i < A.nfp; i += 64) S.prow[i] = A.fprm[(size_t)b * A.nfp + i];
		}
		__syncthreads();
		if (on) env_build(S.kns, C, S.tab + C.eoff, S.tab + C.hoff, lane, 64);
		__syncthreads();
		if (on) minmax_problem<KM, KP>(A, M, b, lane);
	}
}
