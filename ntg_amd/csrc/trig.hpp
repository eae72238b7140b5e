// trig.hpp -- ntg_batch_trig: the minimum and maximum over the horizon of sums of sines and cosines of the flat flag declared AT THE CALL,
//   h(z) = sum_t w_t g_t(theta_t),   theta_t = sum_i coef_i z[ent_i] + phase + fprm_b[pp],   g = sin, cos or the identity,
// the manipulator's tip height sin qa + sin(qa + qb) + sin(qa + qb + qc), its reach, a wall in front of it.  On a knot interval every angle is
// a polynomial with a Bezier polygon Theta; about the centre c of that polygon sin(theta) = sin c + cos c (theta - c) + R, |R| <= rho^2 / 2
// with rho the polygon's radius.  The linear part is a polygon again, the remainder is of the order of the gap between a polygon and its
// function, so the bisection of extrema.hpp converges as it does there.
//
// Per (problem, form), the definition of include/ntg_amd.h:
//   level 0   trig_poly on every knot interval j of the form's basis class: per term the entries' polygons as forms.hpp forms a factor
//             (form_factor, shift 0), times coef, elevated, summed, the phase added.  The LIN terms' weighted polygons are summed into one.
//   levels    trig_levels: ext_levels (extrema.hpp) on pieces of up to NTG_TRIG_MAXTERMS polygons -- a third twin of that loop, kept in
//             step by hand like ratio_levels, and held in step by the tests: tests/bisect_oracle.py is the one written sequence all of
//             them are tested against (this one by tests/test_gpu_trig.py).  A piece is halved polygon by polygon (ext_split); its
//             enclosure (trig_range) and the attained value at its new end (trig_end) call sincos once per SIN / COS term.  The two outer
//             ends of a parent were taken a level earlier with the same bits and the same times, so only the middle end is evaluated.
// A work-list element is NTG_TRIG_MAXTERMS polygons of KM doubles and two doubles of padding: every polygon starts at 16 bytes and a lane
// reads and writes its own piece with 16-byte accesses; the element is an odd number of 16-byte slots.  The list is updated in place as in
// ext_levels: every parent is in registers (4 KM doubles) before a child is stored.
//
//   trig_shared_kernel  plans on their own grid: persistent workgroups of four (or two) waves; the extraction weights and the breaks of every
//                       basis class are built once into LDS; every wave then streams problems with its own x row, fprm row and work list.
//   trig_pp_kernel      per-problem grids: the same, with breaks and weights of the wave's own problem.
// The form and term tables are read from the kernel argument at wave-uniform indices.  No scratch in HBM, no atomics, nothing depends on the
// batch around a problem.  Every private array is indexed by unrolled loop counters only.
#pragma once
#include "forms.hpp"

template <int KM>
struct TrigPiece { EnvPoly<KM> th[NTG_TRIG_MAXTERMS]; };

// what the kernels know of form f
struct TrigOf { const TrigArgs &A; int f; TrigRow R; EnvClass C; };

// The angle polygon of term Q on knot interval j at degree dt: every entry's polygon times its coef, elevated to dt, the entries summed in
// declared order, then the phase
template <int KM>
__device__ __forceinline__ EnvPoly<KM> trig_angle(const TrigTerm &Q, const EnvClass C, const ExtLds &M, int j, double h, int dt)
{
#pragma clang fp contract(off)
	EnvPoly<KM> S;
#pragma unroll
	for (int s = 0; s < KM; s++) S.b[s] = 0.0;
	for (int i = 0; i < Q.nent; i++) {
		EnvPoly<KM> P;
		const int d = form_factor<KM>(P, C, M.tab, M.xrow, Q.iC[i], Q.r[i], 0.0, j, h);
		const double cf = Q.coef[i];
#pragma unroll
		for (int s = 0; s < KM; s++) P.b[s] = s <= d ? cf * P.b[s] : 0.0;
		for (int u = d; u < dt; u++) P.elevate(u);
#pragma unroll
		for (int s = 0; s < KM; s++) { if (s <= dt) S.b[s] = S.b[s] + P.b[s]; }
	}
	const double ph = Q.phase + (Q.pp >= 0 ? M.prow[Q.pp] : 0.0);
#pragma unroll
	for (int s = 0; s < KM; s++) { if (s <= dt) S.b[s] = S.b[s] + ph; }
	return S;
}

// The level-0 piece of a form on knot interval j: the angle polygons of its SIN and COS terms at the form's degree, then the sum of its LIN
// terms' weighted polygons (w times the angle at the term's own degree, elevated, added in declared order: rule 1d of ntg_batch_forms)
template <int KM>
__device__ __forceinline__ TrigPiece<KM> trig_poly(const TrigOf &F, const ExtLds &M, int j)
{
#pragma clang fp contract(off)
	const EnvClass C = F.C;
	const int D = F.R.D, ntrig = F.R.ntrig, nlin = F.R.nlin;
	const double h = M.tab[C.hoff + j];
	EnvPoly<KM> lam;
#pragma unroll
	for (int s = 0; s < KM; s++) lam.b[s] = 0.0;
	for (int t = ntrig; t < ntrig + nlin; t++) {
		const TrigTerm &Q = F.A.term[F.f][t];
		const int dt = Q.dt;
		const double w = Q.w;
		const EnvPoly<KM> Th = trig_angle<KM>(Q, C, M, j, h, dt);
		EnvPoly<2 * KM - 1> G;   // (form_poly's polygon, so that the elevation is the instance of EnvPoly::elevate that forms.hpp runs: rule 5 asks for its bits)
#pragma unroll
		for (int s = 0; s < 2 * KM - 1; s++) G.b[s] = 0.0;
#pragma unroll
		for (int s = 0; s < KM; s++) G.b[s] = s <= dt ? w * Th.b[s] : 0.0;
		for (int u = dt; u < D; u++) G.elevate(u);
#pragma unroll
		for (int s = 0; s < KM; s++) { if (s <= D) lam.b[s] = lam.b[s] + G.b[s]; }
	}
	TrigPiece<KM> Pc;
#pragma unroll
	for (int t = 0; t < NTG_TRIG_MAXTERMS; t++) {
		if (t < ntrig) Pc.th[t] = trig_angle<KM>(F.A.term[F.f][t], C, M, j, h, D);
		else if (t == ntrig && nlin > 0) Pc.th[t] = lam;
		else {
#pragma unroll
			for (int s = 0; s < KM; s++) Pc.th[t].b[s] = 0.0;
		}
	}
	return Pc;
}

// rule 2: the enclosure [plo, phi] of the form on a piece
template <int KM>
__device__ __forceinline__ void trig_range(const TrigOf &F, const TrigPiece<KM> &Pc, int D, double &plo, double &phi)
{
#pragma clang fp contract(off)
	const int ntrig = F.R.ntrig, nlin = F.R.nlin;
	EnvPoly<KM> P;
#pragma unroll
	for (int s = 0; s < KM; s++) P.b[s] = 0.0;
	double rem = 0.0;
#pragma unroll
	for (int t = 0; t < NTG_TRIG_MAXTERMS; t++) {
		if (t < ntrig) {
			const TrigTerm &Q = F.A.term[F.f][t];
			const double w = Q.w;
			const bool cs = Q.kind == NTG_TRIG_COS;
			double lo, hi, sn, cn;
			Pc.th[t].range(D, lo, hi);
			const double c = 0.5 * (lo + hi);
			const double rho = env_max(hi - c, c - lo);
			sincos(c, &sn, &cn);
			const double a = cs ? cn : sn, b = cs ? -sn : cn;   // (C - S x is C + (-S) x, bit for bit)
#pragma unroll
			for (int s = 0; s < KM; s++) { if (s <= D) P.b[s] = P.b[s] + w * (a + b * (Pc.th[t].b[s] - c)); }
			rem = rem + fabs(w) * rho * rho * 0.5;
		} else if (t == ntrig && nlin > 0) {
#pragma unroll
			for (int s = 0; s < KM; s++) { if (s <= D) P.b[s] = P.b[s] + Pc.th[t].b[s]; }
		}
	}
	P.range(D, plo, phi);
	plo = plo - rem; phi = phi + rem;
	if (nlin == 0) {   // |h| <= W whatever the polygons say (a NaN stays)
		if (plo < -F.R.W) plo = -F.R.W;
		if (phi > F.R.W) phi = F.R.W;
	}
}

// rule 3: the form's value at the first (LAST = false) or last end of a piece
template <int KM, bool LAST>
__device__ __forceinline__ double trig_end(const TrigOf &F, const TrigPiece<KM> &Pc, int D)
{
#pragma clang fp contract(off)
	const int ntrig = F.R.ntrig, nlin = F.R.nlin;
	double v = 0.0;
#pragma unroll
	for (int t = 0; t < NTG_TRIG_MAXTERMS; t++) {
		const double th = LAST ? ext_last<KM>(Pc.th[t], D) : Pc.th[t].b[0];
		if (t < ntrig) {
			const TrigTerm &Q = F.A.term[F.f][t];
			double sn, cn;
			sincos(th, &sn, &cn);
			v = v + Q.w * (Q.kind == NTG_TRIG_COS ? cn : sn);
		} else if (t == ntrig && nlin > 0) v = v + th;
	}
	return v;
}

// a piece in the work list: element pos, polygon t at 16 bytes
template <int KM>
__device__ __forceinline__ void trig_store(double *list, int pos, const TrigPiece<KM> &Pc, int np)
{
	static_assert(KM % 2 == 0, "a polygon is a whole number of 16-byte words");
	double2 *e = reinterpret_cast<double2 *>(list + (size_t)pos * (NTG_TRIG_MAXTERMS * KM + 2));
#pragma unroll
	for (int t = 0; t < NTG_TRIG_MAXTERMS; t++) {
		if (t < np) {
#pragma unroll
			for (int q = 0; q < KM / 2; q++) e[t * (KM / 2) + q] = make_double2(Pc.th[t].b[2 * q], Pc.th[t].b[2 * q + 1]);
		}
	}
}
template <int KM>
__device__ __forceinline__ void trig_load(const double *list, int pos, TrigPiece<KM> &Pc, int np)
{
	const double2 *e = reinterpret_cast<const double2 *>(list + (size_t)pos * (NTG_TRIG_MAXTERMS * KM + 2));
#pragma unroll
	for (int t = 0; t < NTG_TRIG_MAXTERMS; t++) {
#pragma unroll
		for (int q = 0; q < KM / 2; q++) {
			double2 v = make_double2(0.0, 0.0);
			if (t < np) v = e[t * (KM / 2) + q];
			Pc.th[t].b[2 * q] = v.x; Pc.th[t].b[2 * q + 1] = v.y;
		}
	}
}

// The definition's levels for one form, by one wave: ext_levels on pieces of np polygons.  res = {min_lo, min_hi, max_lo, max_hi},
// tw = {t_min, t_max}; every lane returns the same figures
template <int KM>
__device__ __forceinline__ void trig_levels(const ExtRun &Q, const ExtLds &M, const TrigOf &F, int lane, double (&res)[4], double (&tw)[2], int &status, int &npieces)
{
	const int D = Q.D, np = F.R.ntrig + (F.R.nlin > 0 ? 1 : 0);
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
	// level.  One piece per lane (l <= 64) stays in registers between the rounds; otherwise the second round forms it again, the same way.
	const int npass = (Q.l + 63) >> 6;
	TrigPiece<KM> Pc;
#pragma unroll
	for (int t = 0; t < NTG_TRIG_MAXTERMS; t++) {
#pragma unroll
		for (int s = 0; s < KM; s++) Pc.th[t].b[s] = 0.0;
	}
	for (int it = 0; it < 2 * npass; it++) {
		const bool second = it >= npass;
		const int j = lane + 64 * (second ? it - npass : it);
		const bool on = j < Q.l;
		if (on && (!second || npass > 1)) Pc = trig_poly<KM>(F, M, j);
		if (!second) {
			if (on) {
				const double e0 = trig_end<KM, false>(F, Pc, D), e1 = trig_end<KM, true>(F, Pc, D);
				ext_take_min(U, tU, e0, kn[j]); ext_take_min(U, tU, e1, kn[j + 1]);
				ext_take_max(V, tV, e0, kn[j]); ext_take_max(V, tV, e1, kn[j + 1]);
			}
			if (it == npass - 1) ext_wave_ends(U, tU, V, tV);
		} else {
			double plo = 0.0, phi = 0.0;
			bool open = false;
			if (on) {
				trig_range<KM>(F, Pc, D, plo, phi);
				nan = nan || plo != plo || phi != phi;
				open = (s_lo && plo < U - tol) || (s_hi && phi > V + tol);
			}
			const unsigned long long m = __ballot(open);
			const int pos = nopen + __popcll(m & below);
			if (open) {
				if (plo < Olo) Olo = plo;
				if (phi > Ohi) Ohi = phi;
				if (pos < NTG_EXTREMA_CAP) {
					trig_store<KM>(M.list, pos, Pc, np);
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
		asm volatile("" : "+s"(Dl));   // the degree's masks are formed where they are used, level by level (ext_levels)
		const double inv = 1.0 / (double)(1 << (lam + 1));
		TrigPiece<KM> Lp, Rp;
		long long key = 0;
		__builtin_amdgcn_wave_barrier();   // the list of level lam is whole
		trig_load<KM>(M.list, lane, Rp, on ? np : 0);
		if (on) key = M.keys[lane];
		__builtin_amdgcn_wave_barrier();   // every parent is in registers before a child is stored
		const int j = (int)(key >> 32), i = (int)(key & 0xffffffffll);
#pragma unroll
		for (int t = 0; t < NTG_TRIG_MAXTERMS; t++) {
			if (t < np) ext_split<KM>(Lp.th[t], Rp.th[t], Dl);   // Rp becomes the right child, Lp the left one
			else {
#pragma unroll
				for (int s = 0; s < KM; s++) Lp.th[t].b[s] = 0.0;
			}
		}
		double llo = 0.0, lhi = 0.0, rlo = 0.0, rhi = 0.0;
		if (on) {
			const double em = trig_end<KM, false>(F, Rp, Dl);   // (the outer ends are the parent's: taken a level ago, same values, same times)
			const double tm = ext_time(kn, hh, j, 2 * i + 1, lam + 1, inv);
			ext_take_min(U, tU, em, tm);
			ext_take_max(V, tV, em, tm);
			trig_range<KM>(F, Lp, Dl, llo, lhi); trig_range<KM>(F, Rp, Dl, rlo, rhi);
			nan = nan || llo != llo || lhi != lhi || rlo != rlo || rhi != rhi;
		}
		ext_wave_ends(U, tU, V, tV);
		const bool openL = on && ((s_lo && llo < U - tol) || (s_hi && lhi > V + tol));
		const bool openR = on && ((s_lo && rlo < U - tol) || (s_hi && rhi > V + tol));
		const unsigned long long mL = __ballot(openL), mR = __ballot(openR);
		const int posL = __popcll(mL & below) + __popcll(mR & below), posR = posL + (openL ? 1 : 0);
		if (openL) {
			if (llo < Olo) Olo = llo;
			if (lhi > Ohi) Ohi = lhi;
			if (posL < NTG_EXTREMA_CAP) {
				trig_store<KM>(M.list, posL, Lp, np);
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
				trig_store<KM>(M.list, posR, Rp, np);
				M.keys[posR] = ((long long)j << 32) | (long long)(2 * i + 1);
			}
		} else if (on) {
			if (rlo < Rlo) Rlo = rlo;
			if (rhi > Rhi) Rhi = rhi;
		}
		npieces += 2 * nopen;
		nopen = __popcll(mL) + __popcll(mR);
	}
	__builtin_amdgcn_wave_barrier();   // the next form's list starts behind this form's loads
	ext_wave_range(Rlo, Rhi);
	if (__ballot(nan) != 0ull) {
		res[0] = res[1] = res[2] = res[3] = NAN; tw[0] = tw[1] = NAN; status = NTG_EXTREMA_NAN;
	} else {
		res[0] = Rlo; res[1] = U; res[2] = V; res[3] = Rhi; tw[0] = tU; tw[1] = tV;
	}
}

// every form of problem b, by one wave whose x row and fprm row are in M
template <int KM>
__device__ __forceinline__ void trig_problem(const TrigArgs &A, const ExtLds &M, int b, int lane)
{
	const int nform = A.nform;
	ExtOut O{A.q, lane};
	for (int f = 0; f < nform; f++) {
		const TrigRow R = A.row[f];
		const EnvClass C = A.g.c[R.cl];
		const TrigOf F{A, f, R, C};
		const ExtRun Q{M.kns + A.q.koff[R.cl], M.tab + C.hoff, C.l, R.D, A.q.max_depth, A.q.sides, A.q.tol, INFINITY};
		double res[4], tw[2];
		int status, npieces;
		trig_levels<KM>(Q, M, F, lane, res, tw, status, npieces);
		const size_t at = (size_t)b * nform + f;
		O.row(at, res, tw, status, npieces);
		if (O.want_v()) O.fold(A.flo[at], A.fhi[at], res, f);
	}
	O.problem(b);
}

template <int KM>
__global__ void __launch_bounds__(256)
trig_shared_kernel(TrigArgs A)
{
	extern __shared__ __attribute__((aligned(16))) char smem_raw[];
	const int NT = blockDim.x, NW = NT >> 6;
	const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
	const ExtStage S = ntg_trig_layout(A, NTG_TRIG_MAXTERMS * KM + 2).wave(reinterpret_cast<double *>(smem_raw), wave);
	const ExtLds M = S.view();   // (the kernel stages through S; everything below reads through M)
	env_build_classes(A.g, S.tab, S.kns, A.q.koff, tid, NT);
	for (int b0 = blockIdx.x * NW; b0 < A.g.batch; b0 += gridDim.x * NW) {
		const int b = b0 + wave;
		if (b >= A.g.batch) continue;
		__builtin_amdgcn_wave_barrier();   // the problem before is done with the rows
		env_stage_rows(A.g, nullptr, b, S.xrow, nullptr, lane, 64);
		cert_stage_fprm(A.fprm, A.nfp, b, S.prow, lane);
		__builtin_amdgcn_wave_barrier();
		trig_problem<KM>(A, M, b, lane);
	}
}

// per-problem grids: one basis class; every wave builds the weights of its own problem
template <int KM>
__global__ void __launch_bounds__(256)
trig_pp_kernel(TrigArgs A)
{
	extern __shared__ __attribute__((aligned(16))) char smem_raw[];
	const int NW = blockDim.x >> 6;
	const EnvClass C = A.g.c[0];
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const ExtStage S = ntg_trig_layout(A, NTG_TRIG_MAXTERMS * KM + 2).wave(reinterpret_cast<double *>(smem_raw), wave);
	const ExtLds M = S.view();
	const int per_pass = gridDim.x * NW;
	for (int b0 = 0; b0 < A.g.batch; b0 += per_pass) {   // (the same trip count for every wave of the grid: the barriers below are uniform)
		const int b = b0 + blockIdx.x * NW + wave;
		const bool on = b < A.g.batch;
		__syncthreads();
		if (on) { env_stage_pp(A.g, nullptr, b, S.kns, S.xrow, nullptr, lane); cert_stage_fprm(A.fprm, A.nfp, b, S.prow, lane); }
		__syncthreads();
		if (on) env_build(S.kns, C, S.tab + C.eoff, S.tab + C.hoff, lane, 64);
		__syncthreads();
		if (on) trig_problem<KM>(A, M, b, lane);
	}
}
