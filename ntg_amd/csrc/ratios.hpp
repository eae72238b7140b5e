// ratios.hpp -- ntg_batch_ratios: the minimum and maximum over the horizon of RATIOS of products of the quadratic forms ntg_batch_forms takes,
//   R(t) = prod_a q_{num[a]}(z(t)) / prod_b q_{den[b]}(z(t)):
// the squared curvature T T / (S S S) of the kinematic car, its squared lateral acceleration T T / S, the heading slope y' / x'.  On a knot
// interval numerator and denominator are polynomials; with both as Bezier polygons of one degree and every denominator point d_i > 0,
//   N / Q = sum_i (n_i / d_i) (d_i B_i / sum_j d_j B_j)
// is a convex combination of the quotients n_i / d_i, so they bound the ratio on the piece and the end quotients are attained.  De Casteljau
// halves both polygons, and ntg_batch_extrema's bisection applies to the pair.
//
// Per (problem, ratio), the definition of include/ntg_amd.h:
//   level 0   form_poly (forms.hpp) of every form named, on every knot interval of the ratio's basis class; each side the chain G = F_0,
//             G = G (x) F_a of Bezier products on the table W_{d,e} of the chain's degree d so far and the form's degree e (an empty side: the
//             point 1); the side of lower degree elevated to DR = max(dN, dD).
//   levels    ext_levels' sequence (extrema.hpp) on pairs: the ends' quotients into U / V, a piece open if its quotients reach below U - tol
//             (above V + tol) or a denominator point is <= 0; an end with denominator <= 0 stops the loop after its level: status POLE.
// The level loop is written out here, not an instance of ext_levels: ratio_levels follows ext_levels line by line -- the same level-0
// rounds, the same ballots and list positions, the same retirement, the same split routine (ext_split).  What differs is the piece (two
// polygons of up to 25 points), its range (a row of divisions guarded by the denominator's sign) and the exit on a pole.  ext_levels was
// twice generalised over a piece type.  The first time the condition was identical assembly of the existing instances, which no change
// of the template meets.  The second time the condition was equal bits, no worse registers and a rate within the run-to-run spread: bits and
// registers held, the ratio instances were even faster, but the single-polygon instances of extrema and separation lost 1 to 2 %.
// With a denominator of ones the two loops take the same decisions on the same bits (n / 1.0 == n), which tests/test_gpu_ratios.py holds
// them to; tests/golden/bisect_calls.npz holds both to recorded results.  The loops are kept in step by hand and held in step by the tests:
// tests/bisect_oracle.py is the one written sequence every level loop of the library is tested against, this one by tests/test_gpu_ratios.py.
//
//   ratios_shared_kernel  plans on their own grid: persistent workgroups of four waves (two where four work lists do not fit); the forms'
//                         product tables, the chains' product tables, the extraction weights and the breaks of every basis class are built once
//                         into LDS; every wave then streams problems with its own x row, fprm row and work list.  No workgroup barrier after
//                         the set-up.
//   ratios_pp_kernel      per-problem grids: the same, with breaks and weights of the wave's own problem.
// The chains' tables reach C(24,12)^2 = 7.3e12: their binomials are formed in doubles, exact below 2^53, and only the pairs of degrees the
// call's chains use are built (at most NTG_RATIO_MAXPAIRS, listed by the host).  No scratch in HBM, no atomics, nothing depends on the batch
// around a problem.  Every private array is indexed by unrolled loop counters only.
#pragma once
#include "forms.hpp"

// a piece: numerator and denominator polygons of one degree
template <int KR>
struct RatPoly { EnvPoly<KR> n, d; };

// a byte of the kernel argument at a wave-uniform index, as a scalar (the compiler reads bytes through the vector memory path)
__device__ __forceinline__ int ratio_u8(unsigned char v) { return __builtin_amdgcn_readfirstlane((int)v); }

// C(n, r) in a double, exact: every intermediate is an integer below 2^53 (n <= 24)
__device__ __forceinline__ double ratio_binom(int n, int r)
{
	if (r > n - r) r = n - r;
	double c = 1.0;
	for (int i = 1; i <= r; i++) c = c * (double)(n - r + i) / (double)i;
	return c;
}

// the product tables of the call's chains: W_{d,e}[i][j] = C(d,i) C(e,j) / C(d+e,i+j), the numerator exact, the division the one rounding
__device__ __forceinline__ void ratio_build_products(const RatioArgs &A, double *pw, int tid, int nthr)
{
	for (int q = 0, nq = ratio_u8(A.npair); q < nq; q++) {
		const int d = ratio_u8(A.pd[q]), e = ratio_u8(A.pe[q]);
		double *W = pw + __builtin_amdgcn_readfirstlane((int)A.poff[q]);
		for (int at = tid; at < (d + 1) * (e + 1); at += nthr) {
			const int i = at / (e + 1), j = at - i * (e + 1);
			W[at] = (ratio_binom(d, i) * ratio_binom(e, j)) / ratio_binom(d + e, i + j);
		}
	}
	__syncthreads();
}

// G (degree d) (x) F (degree e): h_m = sum_{i + j = m} W[i][j] g_i f_j, i ascending, every product and every sum rounded
template <int KR, int KD>
__device__ __forceinline__ EnvPoly<KR> ratio_product(const EnvPoly<KR> &G, const EnvPoly<KD> &F, const double *W, int d, int e)
{
#pragma clang fp contract(off)
	EnvPoly<KR> H;
#pragma unroll
	for (int m = 0; m < KR; m++) {
		double acc = 0.0;
#pragma unroll
		for (int i = 0; i < KR; i++) {
			const int c = m - i;
			if (c >= 0 && c < KD) { if (i <= d && c <= e) acc += W[i * (e + 1) + c] * G.b[i] * F.b[c]; }
		}
		H.b[m] = acc;
	}
	return H;
}

// level-0 pair of ratio R on knot interval j: both sides' chains, the lower side elevated to DR
template <int KM, int KR>
__device__ __forceinline__ RatPoly<KR> ratio_poly(const RatioArgs &A, const RatioRow &R, int DR, const ExtLds &M, const double *pw, int j)
{
	constexpr int KD = 2 * KM - 1;
	static_assert(KD <= KR, "a form's polygon starts a chain");
	RatPoly<KR> P;
	EnvPoly<KD> Q;     // the polygon of form `have`, the last one built: a form repeated in adjacent places (a power: T T, S S S) is built once.
	                   // A repeat that is not adjacent ({0, 1, 0}, or the same form on both sides with another between) is built again: the
	                   // same bits, only more work
	int have = -1;
#pragma unroll
	for (int s = 0; s < KD; s++) Q.b[s] = 0.0;
	for (int side = 0; side < 2; side++) {
		const int nf = ratio_u8(side ? R.nden : R.nnum);
		EnvPoly<KR> G;
#pragma unroll
		for (int s = 0; s < KR; s++) G.b[s] = s == 0 ? 1.0 : 0.0;
		int d = 0;
		for (int a = 0; a < nf; a++) {
			const int f = ratio_u8(side ? R.den[a] : R.num[a]);
			const FormRow FR = A.f.row[f];
			const FormOf F{A.f, f, FR, A.f.g.c[FR.cl]};
			if (f != have) { Q = form_poly<KM>(F, M, j); have = f; }
			if (a == 0) {
#pragma unroll
				for (int s = 0; s < KD; s++) G.b[s] = Q.b[s];
			} else {
				const int q = ratio_u8(side ? R.pd[a - 1] : R.pn[a - 1]);
				G = ratio_product<KR, KD>(G, Q, pw + __builtin_amdgcn_readfirstlane((int)A.poff[q]), d, FR.D);
			}
			d += FR.D;
		}
		for (int u = d; u < DR; u++) G.elevate(u);
		if (side) P.d = G;
		else P.n = G;
	}
	return P;
}

// the quotients of a pair: their range, or (-inf, +inf) where a denominator point is not positive; a NaN in either polygon: (NaN, NaN)
template <int KR>
__device__ __forceinline__ void ratio_range(const RatPoly<KR> &P, int D, double &lo, double &hi)
{
	bool pos = true, nan = false;
	lo = INFINITY; hi = -INFINITY;
#pragma unroll
	for (int s = 0; s < KR; s++) {
		if (s <= D) {
			const double n = P.n.b[s], d = P.d.b[s], q = n / d;
			nan = nan || n != n || d != d;
			pos = pos && d > 0.0;
			if (q < lo) lo = q;
			if (q > hi) hi = q;
		}
	}
	if (!pos) { lo = -INFINITY; hi = INFINITY; }
	if (nan) lo = hi = NAN;
}

// an end of a piece: its quotient into (U, tU) / (V, tV) where the denominator is positive; a denominator <= 0 marks the pole
__device__ __forceinline__ void ratio_end(double n, double d, double t, double &U, double &tU, double &V, double &tV, bool &pole)
{
	if (d > 0.0) {
		const double q = n / d;
		ext_take_min(U, tU, q, t); ext_take_max(V, tV, q, t);
	} else if (d <= 0.0) pole = true;
}

// The definition's levels for one ratio, by one wave: ext_levels' sequence on pairs.  list: [NTG_EXTREMA_CAP][2 KR], numerator first
template <int KM, int KR>
__device__ __forceinline__ void ratio_levels(const ExtRun &Q, const ExtLds &M, const RatioArgs &A, const RatioRow &R, const double *pw, int lane, double (&res)[4], double (&tw)[2], int &status, int &npieces)
{
	constexpr int KL = 2 * KR;
	const int D = Q.D;
	const double *kn = Q.kn, *hh = Q.hh;
	const double tol = Q.tol;
	const bool s_lo = Q.sides & 1, s_hi = Q.sides & 2;
	const unsigned long long below = (1ull << lane) - 1ull;
	double U = INFINITY, tU = INFINITY, V = -INFINITY, tV = INFINITY;   // the same in every lane after a level's butterfly
	double Rlo = INFINITY, Rhi = -INFINITY;   // retired pieces, this lane's
	double Olo = INFINITY, Ohi = -INFINITY;   // open pieces of the current level, this lane's
	bool nan = false, pole = false;
	int nopen = 0;

	// level 0, as in ext_levels: the ends first, then the decisions
	const int npass = (Q.l + 63) >> 6;
	RatPoly<KR> P;
#pragma unroll
	for (int s = 0; s < KR; s++) { P.n.b[s] = 0.0; P.d.b[s] = 0.0; }
	for (int it = 0; it < 2 * npass; it++) {
		const bool second = it >= npass;
		const int j = lane + 64 * (second ? it - npass : it);
		const bool on = j < Q.l;
		if (on && (!second || npass > 1)) P = ratio_poly<KM, KR>(A, R, D, M, pw, j);
		if (!second) {
			if (on) {
				ratio_end(P.n.b[0], P.d.b[0], kn[j], U, tU, V, tV, pole);
				ratio_end(ext_last<KR>(P.n, D), ext_last<KR>(P.d, D), kn[j + 1], U, tU, V, tV, pole);
			}
			if (it == npass - 1) {
				ext_wave_ends(U, tU, V, tV);
				pole = __ballot(pole) != 0ull;
			}
		} else {
			double plo = 0.0, phi = 0.0;
			bool open = false;
			if (on) {
				ratio_range<KR>(P, D, plo, phi);
				nan = nan || plo != plo || phi != phi;
				open = !pole && ((s_lo && plo < U - tol) || (s_hi && phi > V + tol));
			}
			const unsigned long long m = __ballot(open);
			const int pos = nopen + __popcll(m & below);
			if (open) {
				if (plo < Olo) Olo = plo;
				if (phi > Ohi) Ohi = phi;
				if (pos < NTG_EXTREMA_CAP) {
#pragma unroll
					for (int s = 0; s < KR; s++) { if (s <= D) { M.list[pos * KL + s] = P.n.b[s]; M.list[pos * KL + KR + s] = P.d.b[s]; } }
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

	// levels: the open pairs of level lam are in the list; their children form level lam + 1
	status = NTG_EXTREMA_OK;
	for (int lam = 0; lam <= Q.max_depth; lam++) {
		if (pole || nopen == 0) break;
		if (lam == Q.max_depth || nopen > NTG_EXTREMA_CAP) {
			status = lam == Q.max_depth ? NTG_EXTREMA_DEPTH : NTG_EXTREMA_FULL;
			if (Olo < Rlo) Rlo = Olo;
			if (Ohi > Rhi) Rhi = Ohi;
			break;
		}
		Olo = INFINITY; Ohi = -INFINITY;
		const bool on = lane < nopen;
		int Dl = D;
		asm volatile("" : "+s"(Dl));   // the degree's masks are formed where they are used, level by level
		const double inv = 1.0 / (double)(1 << (lam + 1));
		RatPoly<KR> Lp, Rp;
		long long key = 0;
		__builtin_amdgcn_wave_barrier();   // the list of level lam is whole
		if (on) {
#pragma unroll
			for (int s = 0; s < KR; s++) { Rp.n.b[s] = s <= Dl ? M.list[lane * KL + s] : 0.0; Rp.d.b[s] = s <= Dl ? M.list[lane * KL + KR + s] : 0.0; }
			key = M.keys[lane];
		} else {
#pragma unroll
			for (int s = 0; s < KR; s++) { Rp.n.b[s] = 0.0; Rp.d.b[s] = 0.0; }
		}
		__builtin_amdgcn_wave_barrier();   // every parent is in registers before a child is stored
		const int j = (int)(key >> 32), i = (int)(key & 0xffffffffll);
		ext_split<KR>(Lp.n, Rp.n, Dl);
		ext_split<KR>(Lp.d, Rp.d, Dl);
		double llo = 0.0, lhi = 0.0, rlo = 0.0, rhi = 0.0;
		if (on) {
			const double t0 = ext_time(kn, hh, j, 2 * i, lam + 1, inv), tm = ext_time(kn, hh, j, 2 * i + 1, lam + 1, inv), t1 = ext_time(kn, hh, j, 2 * i + 2, lam + 1, inv);
			ratio_end(Lp.n.b[0], Lp.d.b[0], t0, U, tU, V, tV, pole);
			ratio_end(Rp.n.b[0], Rp.d.b[0], tm, U, tU, V, tV, pole);
			ratio_end(ext_last<KR>(Rp.n, Dl), ext_last<KR>(Rp.d, Dl), t1, U, tU, V, tV, pole);
			ratio_range<KR>(Lp, Dl, llo, lhi); ratio_range<KR>(Rp, Dl, rlo, rhi);
			nan = nan || llo != llo || lhi != lhi || rlo != rlo || rhi != rhi;
		}
		ext_wave_ends(U, tU, V, tV);
		pole = __ballot(pole) != 0ull;
		npieces += 2 * nopen;
		if (pole) break;
		const bool openL = on && ((s_lo && llo < U - tol) || (s_hi && lhi > V + tol));
		const bool openR = on && ((s_lo && rlo < U - tol) || (s_hi && rhi > V + tol));
		const unsigned long long mL = __ballot(openL), mR = __ballot(openR);
		const int posL = __popcll(mL & below) + __popcll(mR & below), posR = posL + (openL ? 1 : 0);
		if (openL) {
			if (llo < Olo) Olo = llo;
			if (lhi > Ohi) Ohi = lhi;
			if (posL < NTG_EXTREMA_CAP) {
#pragma unroll
				for (int s = 0; s < KR; s++) { if (s <= Dl) { M.list[posL * KL + s] = Lp.n.b[s]; M.list[posL * KL + KR + s] = Lp.d.b[s]; } }
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
				for (int s = 0; s < KR; s++) { if (s <= Dl) { M.list[posR * KL + s] = Rp.n.b[s]; M.list[posR * KL + KR + s] = Rp.d.b[s]; } }
				M.keys[posR] = ((long long)j << 32) | (long long)(2 * i + 1);
			}
		} else if (on) {
			if (rlo < Rlo) Rlo = rlo;
			if (rhi > Rhi) Rhi = rhi;
		}
		nopen = __popcll(mL) + __popcll(mR);
	}
	__builtin_amdgcn_wave_barrier();   // the next ratio's list starts behind this ratio's loads
	ext_wave_range(Rlo, Rhi);
	if (__ballot(nan) != 0ull) {
		res[0] = res[1] = res[2] = res[3] = NAN; tw[0] = tw[1] = NAN; status = NTG_EXTREMA_NAN;
	} else if (pole) {
		res[0] = -INFINITY; res[1] = INFINITY; res[2] = -INFINITY; res[3] = INFINITY; tw[0] = tw[1] = NAN; status = NTG_RATIO_POLE;
	} else {
		res[0] = Rlo; res[1] = U; res[2] = V; res[3] = Rhi; tw[0] = tU; tw[1] = tV;
	}
}

// every ratio of problem b, by one wave whose x row and fprm row are in M
template <int KM, int KR>
__device__ __forceinline__ void ratio_problem(const RatioArgs &A, const ExtLds &M, const double *pw, int b, int lane)
{
	const FormArgs &F = A.f;
	const int nratio = ratio_u8(A.nratio);
	ExtOut O{F.q, lane};
	for (int r = 0; r < nratio; r++) {
		const RatioRow &R = A.r[r];
		const int cl = ratio_u8(R.cl);
		const EnvClass C = F.g.c[cl];
		const ExtRun Q{M.kns + F.q.koff[cl], M.tab + C.hoff, C.l, ratio_u8(R.DR), F.q.max_depth, F.q.sides, F.q.tol, INFINITY};
		double res[4], tw[2];
		int status, npieces;
		ratio_levels<KM, KR>(Q, M, A, R, pw, lane, res, tw, status, npieces);
		const size_t at = (size_t)b * nratio + r;
		O.row(at, res, tw, status, npieces);
		if (O.want_v()) O.fold(F.flo[at], F.fhi[at], res, r);
	}
	O.problem(b);
}

// the wave's part of the dynamic LDS, its list elements as wide as the instance's piece (npw comes from the kernel argument as a short: made
// a scalar again); the chains' product tables lie behind the forms' in front: wl + NTG_FORM_WALL
template <int KR>
__device__ __forceinline__ ExtStage ratio_lds(const RatioArgs &A, double *base, int wave)
{
	BisectLds L = ntg_ratios_layout(A, 2 * KR);
	L.front = __builtin_amdgcn_readfirstlane(L.front);
	return L.wave(base, wave);
}

// (launched with 64 A.nw threads: the workgroup's size is the call's, not the instance's)
template <int KM, int KR>
__global__ void __launch_bounds__(NTG_EXTREMA_NT)
ratios_shared_kernel(RatioArgs A)
{
	extern __shared__ __attribute__((aligned(16))) char smem_raw[];
	__shared__ unsigned int pas[NTG_FORM_PASCAL * NTG_FORM_PASCAL];
	const FormArgs &F = A.f;
	const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, NT = blockDim.x, NW = NT >> 6;
	const ExtStage S = ratio_lds<KR>(A, reinterpret_cast<double *>(smem_raw), wave);
	const ExtLds M = S.view();
	double *pw = S.wl + NTG_FORM_WALL;
	form_build_products(S.wl, pas, tid, NT);
	ratio_build_products(A, pw, tid, NT);
	env_build_classes(F.g, S.tab, S.kns, F.q.koff, tid, NT);
	for (int b0 = blockIdx.x * NW; b0 < F.g.batch; b0 += gridDim.x * NW) {
		const int b = b0 + wave;
		if (b >= F.g.batch) continue;
		__builtin_amdgcn_wave_barrier();   // the problem before is done with the rows
		env_stage_rows(F.g, nullptr, b, S.xrow, nullptr, lane, 64);
		cert_stage_fprm(F.fprm, F.nfp, b, S.prow, lane);
		__builtin_amdgcn_wave_barrier();
		ratio_problem<KM, KR>(A, M, pw, b, lane);
	}
}

// per-problem grids: one basis class; every wave builds the weights of its own problem
template <int KM, int KR>
__global__ void __launch_bounds__(NTG_EXTREMA_NT)
ratios_pp_kernel(RatioArgs A)
{
	extern __shared__ __attribute__((aligned(16))) char smem_raw[];
	__shared__ unsigned int pas[NTG_FORM_PASCAL * NTG_FORM_PASCAL];
	const FormArgs &F = A.f;
	const EnvClass C = F.g.c[0];
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, NT = blockDim.x, NW = NT >> 6;
	const ExtStage S = ratio_lds<KR>(A, reinterpret_cast<double *>(smem_raw), wave);
	const ExtLds M = S.view();
	double *pw = S.wl + NTG_FORM_WALL;
	form_build_products(S.wl, pas, threadIdx.x, NT);
	ratio_build_products(A, pw, threadIdx.x, NT);
	const int per_pass = gridDim.x * NW;
	for (int b0 = 0; b0 < F.g.batch; b0 += per_pass) {   // (the same trip count for every wave of the grid: the barriers below are uniform)
		const int b = b0 + blockIdx.x * NW + wave;
		const bool on = b < F.g.batch;
		__syncthreads();
		if (on) { env_stage_pp(F.g, nullptr, b, S.kns, S.xrow, nullptr, lane); cert_stage_fprm(F.fprm, F.nfp, b, S.prow, lane); }
		__syncthreads();
		if (on) env_build(S.kns, C, S.tab + C.eoff, S.tab + C.hoff, lane, 64);
		__syncthreads();
		if (on) ratio_problem<KM, KR>(A, M, pw, b, lane);
	}
}
