// eval.hpp -- the evaluation: augmented-Lagrangian rows, the cost passes (Z = M C, functors, banded gradient,
// quadrature), the constraint rows and their Jacobian, and eval_kernel on top of them.  sqp_kernel.hpp evaluates
// through eval_cost; hostpath.hip uses cost_phase2 for the host-callback kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "ntg_dev.hpp"
#include "families.hpp"
#include "wave_ops.hpp"
#include "lds_tables.hpp"

// tuning knob: minimum waves per SIMD the register allocator must leave room for
#ifndef NTG_EVAL_WAVES
#define NTG_EVAL_WAVES 2
#endif
// phase clock of eval_kernel (variant builds only, tests/tools_jac_clock.py): s_memtime ticks of workgroup 0's first lane per phase
#ifdef NTG_EVAL_CLOCK
// accumulators in LDS: a global read-modify-write here would wait for vmcnt(0), i.e. for the wave's outstanding stores -- the clock would
// charge the drain of the emission's stores to the emission
#define EVCLK(slot) do { if (blockIdx.x == 0 && threadIdx.x == 0) { const unsigned long long t_ = __builtin_readcyclecounter(); ntg_evclk_s[slot] += t_ - ntg_evclk_s[15]; ntg_evclk_s[15] = t_; } } while (0)
#define EVCLK0() do { if (blockIdx.x == 0 && threadIdx.x == 0) { for (int i_ = 0; i_ < 15; i_++) ntg_evclk_s[i_] = 0; ntg_evclk_s[15] = __builtin_readcyclecounter(); } } while (0)
#define EVCLK_DECL __shared__ unsigned long long ntg_evclk_s[16];
#define EVCLK_TK (blockIdx.x == 0 ? ntg_evclk_s + 4 : nullptr)
#define EVCLK_ARG , unsigned long long *ntg_evclk_s
#define EVCLK_PASS , ntg_evclk_s
#else
#define EVCLK(slot) do { } while (0)
#define EVCLK0() do { } while (0)
#define EVCLK_DECL
#define EVCLK_TK nullptr
#define EVCLK_ARG
#define EVCLK_PASS
#endif

// Augmented-Lagrangian state of one problem: with mu > 0 the evaluation returns
//   F_A = F + sum_j (t_j^2 - lam_j^2)/(2 mu),  t_j = mu (v_j - clamp(v_j, bl_j, bu_j)),  v_j = c_j + lam_j/mu
// and its gradient g + J' t; t (the next multiplier estimate) is written to tnew.  mu == 0: plain F.
struct ALState {
	double mu;
	const double *lam;   // [ncnln] current multipliers (HBM)
	double *tnew;        // [ncnln] multiplier estimates of the last evaluation (HBM)
	const double *lo, *up; // this problem's rows of lowerb/upperb [nbounds]
	// QP-based SQP step (ntg_solve_opts.hessian = 3, qpdual.hpp): 1 = the evaluation returns the l1 merit function F + mu sum_j viol_j with the
	// gradient of F alone, and tnew receives the row VALUES c_j (what the QP subproblem linearises); 2 = the gradient of the Lagrangian
	// with the multipliers lam (the final pass that recovers the linear rows' multipliers), tnew receives lam.  0 = augmented Lagrangian.
	int qp;
};

// one constraint value -> multiplier estimate t; adds the row's augmented-Lagrangian term and squared scaled residual
__device__ __forceinline__ double al_row(double mu, double lamj, double l, double u, double cj, double &psi, double &rv2, int qp = 0)
{
	if (qp) {   // l1 merit: weight mu on the violation of the row's bounds; the same scaled residual as below for a feasible row with lam = 0
		const double pc = cj < l ? l : (cj > u ? u : cj), rc = (cj - pc) / (1.0 + fabs(cj));
		psi += mu * fabs(cj - pc);
		rv2 += rc * rc;
		return qp == 2 ? lamj : 0.0;
	}
	const double v = cj + lamj / mu;
	const double pj = v < l ? l : (v > u ? u : v);
	// c - p: |c - b| for an active row, min(slack, lam/mu) for a feasible one -- zero only when feasibility AND
	// complementarity hold (the measure of LANCELOT / ALGENCAN)
	const double t = mu * (v - pj), rj = (cj - pj) / (1.0 + fabs(cj));
	psi += (t - lamj) * (t + lamj) / (2.0 * mu);   // factored: no cancellation when c is tiny
	rv2 += rj * rj;
	return t;
}

// bound slot (index into lowerb/upperb) of linear row r: [lic; ltc constraint-major x breakpoint; lfc] (constraints.c:5-33)
__device__ __forceinline__ int lin_slot(const NtgDims &D, int r)
{
	if (r < D.nlic) return r;
	if (r < D.nlic + D.nltc * D.P) return D.nlic + (r - D.nlic) / D.P;
	return D.nlic + D.nltc + (r - D.nlic - D.nltc * D.P);
}

// Linear rows declared as inequalities (ntg_spec.lin_ineq): c_j = A_j x enters the augmented Lagrangian like a
// nonlinear row with a constant Jacobian.  Lanes take rows; t_j goes to LDS (tI) for the gradient pass and to HBM
// (the next multiplier estimate).  Runs between the functor pass and the quadrature / gather pass.
struct LinIneq {
	int nI; const int *irow, *rptr, *rcol, *cptr, *crow; const double *rval, *cval; double *tI;
};
template <int NT>
__device__ __forceinline__ void lin_ineq_phase(const NtgDims &D, const LinIneq &li, const double *sx, const ALState &al, double &psi, double &rv2)
{
	for (int j = threadIdx.x; j < li.nI; j += NT) {
		double cj = 0.0;
		for (int e = li.rptr[j]; e < li.rptr[j + 1]; e++) cj += li.rval[e] * sx[li.rcol[e]];
		const int slot = lin_slot(D, li.irow[j]), row = D.ncnln + j;
		const double t = al_row(al.mu, al.lam[row], al.lo[slot], al.up[slot], cj, psi, rv2);
		al.tnew[row] = t;
		li.tI[j] = t;
	}
}

// per-breakpoint cost functor pass: Z = M C, then ucf/icf/fcf -> fvals, dfz, dfi, dff in LDS
template <int FAM, int NOUT, int K, int NT, int CHM = 0>
__device__ __forceinline__ void cost_phase1(const NtgDims &D, const Smem &S, const double *sx, const ALState &al,
                                            double &psi, double &rv2, bool chm_ok = false)
{
	using Fam = Family<FAM>;
	constexpr int DM = Fam::DM, NZ = NOUT > 0 ? DM * NOUT : NTG_MAX_NZ;
	const int P = D.P, nout = NOUT > 0 ? NOUT : D.nout, nz = D.nz;
	const int tid = threadIdx.x;
	constexpr bool HASCON = Fam::NNLIC + Fam::NNLTC + Fam::NNLFC > 0;
	constexpr int NI = Fam::NNLIC > 0 ? Fam::NNLIC : 1, NTc = Fam::NNLTC > 0 ? Fam::NNLTC : 1, NF = Fam::NNLFC > 0 ? Fam::NNLFC : 1;
	const bool alon = HASCON && al.mu > 0.0;
	const int b0 = D.nlic + D.nltc + D.nlfc;   // first nonlinear slot of lowerb/upperb
	const FamCall<Fam> fc{ntg_prm_row<FAM>(), D.nnltc};
	psi = 0.0; rv2 = 0.0;
	// one constraint value -> AL term, violation, multiplier estimate; returns t
	auto al_term = [&](double cj, int row, int slot) -> double {
		const double t = al_row(al.mu, al.lam[row], al.lo[slot], al.up[slot], cj, psi, rv2, al.qp);
		al.tnew[row] = al.qp == 1 ? cj : t;
		return t;
	};
	lds_sync(); // sx complete, previous users of dfz/fvals done
	if ((D.nucf || (alon && D.nnltc))) {
		const u64 zmask = alon ? (D.tcost_mask | D.tcon_mask) : D.tcost_mask;
		// the channel-mask shortcuts apply when this pass uses exactly "channels CHM of every output" (wave-uniform)
		const bool chm_now = NOUT > 0 && CHM != 0 && chm_ok && zmask == chm_full_mask(CHM, NOUT > 0 ? NOUT : 1, DM);
		for (int i = tid; i < P; i += NT) {                       // cost.c:103-109
			double z[NZ], df[NZ], f = 0.0;
			compute_z<NOUT, K, DM, CHM>(D, S, sx, i, zmask, z, chm_now);
			if (D.nucf) fc.ucf(nout, i, z, f, df);
			else {
#pragma unroll
				for (int v = 0; v < NZ; v++) df[v] = 0.0;
			}
			S.fvals[i] = f;
			const double w = S.wts[i];
#pragma unroll
			for (int v = 0; v < NZ; v++) df[v] *= w;
			if (HASCON && alon && D.nnltc) {                      // constraints.c:148-155 folded into the same pass
				double c[NTc], t[NTc];
				double tape[Fam::TAPE];
				fc.template nltc_val<NZ>(nout, i, z, c, tape);
#pragma unroll
				for (int j = 0; j < NTc; j++) t[j] = j < D.nnltc ? al_term(c[j], D.nnlic + j * P + i, b0 + D.nnlic + j) : 0.0;
				fc.template nltc_vjp<NZ>(nout, nz, i, z, t, df, tape);   // df += J' t, constraint-major like the dense loop
			}
			if (chm_now) {
				// the weighted-gradient rows are (output, channel of CHM) in flag order: row = o NCH + rank(r)
				constexpr int NCH = chm_count(CHM);
#pragma unroll
				for (int o = 0; o < (NOUT > 0 ? NOUT : 1); o++)
#pragma unroll
					for (int r = 0; r < DM; r++) { if ((CHM >> r) & 1) S.dfz[(o * NCH + chm_rank(CHM, r)) * (P + 1) + i] = df[DM * o + r]; }
			} else {
#pragma unroll
				for (int v = 0; v < NZ; v++) { if (v < nz && D.tav_row[v] >= 0 && D.tav_row[v] < S.tav_rows) S.dfz[D.tav_row[v] * (P + 1) + i] = df[v]; }
			}
		}
	}
	if ((D.nicf || (alon && D.nnlic)) && tid == 0) {              // cost.c:4-36, constraints.c:88-117
		double z[NZ], df[NZ], f = 0.0;
		compute_z<NOUT, K, DM>(D, S, sx, 0, alon ? (D.icost_mask | D.icon_mask) : D.icost_mask, z);
		if (D.nicf) fc.icf(nout, z, f, df); else for (int v = 0; v < nz; v++) df[v] = 0.0;
		if (HASCON && alon && D.nnlic) {
			double c[NI], dc[NI * NZ];
			fc.nlicf(nout, z, c, dc);
			for (int j = 0; j < D.nnlic; j++) { const double t = al_term(c[j], j, b0 + j); for (int v = 0; v < nz; v++) df[v] += t * dc[j * nz + v]; }
		}
		for (int v = 0; v < nz; v++) S.dfi[v] = df[v];
		S.dfi[nz] = f;
	}
	if ((D.nfcf || (alon && D.nnlfc)) && tid == (NT > 64 ? 64 : 0)) {   // cost.c:141-174, constraints.c:165-195
		double z[NZ], df[NZ], f = 0.0;
		compute_z<NOUT, K, DM>(D, S, sx, P - 1, alon ? (D.fcost_mask | D.fcon_mask) : D.fcost_mask, z);
		if (D.nfcf) fc.fcf(nout, z, f, df); else for (int v = 0; v < nz; v++) df[v] = 0.0;
		if (HASCON && alon && D.nnlfc) {
			double c[NF], dc[NF * NZ];
			fc.nlfcf(nout, z, c, dc);
			for (int j = 0; j < D.nnlfc; j++) { const double t = al_term(c[j], D.nnlic + D.nnltc * P + j, b0 + D.nnlic + D.nnltc + j); for (int v = 0; v < nz; v++) df[v] += t * dc[j * nz + v]; }
		}
		for (int v = 0; v < nz; v++) S.dff[v] = df[v];
		S.dff[nz] = f;
	}
}

// quadrature + banded gradient assembly from the per-breakpoint values in LDS (fvals, dfz,
// dfi, dff); shared by the device-functor path and the host-callback path of ntg()
template <int NOUT, int K, int NT, int DM, int EPT, bool SHARED = false, int CHM = 0>
__device__ __forceinline__ double cost_phase2(const NtgDims &D, const Smem &S, double *sg, double *gnorm2, const CoefMap<EPT> &cm,
                                              bool hasI, bool hasF, double psi, double rv2, double *Fpure, double *rv2_out,
                                              const LinIneq *li = nullptr, bool chm_ok = false, double *defer = nullptr)
{
	const int P = D.P, nout = NOUT > 0 ? NOUT : D.nout, nz = D.nz;
	const int tid = threadIdx.x;
	lds_sync();
	// trapezoid of the running cost (integrator.c:21-24); per-interval terms across the lanes,
	// wavefront reduction
	double acc[4] = {0.0, 0.0, psi, rv2};
	if (D.nucf)
		for (int i = tid; i < P - 1; i += NT)
			acc[0] += (S.bps[i + 1] - S.bps[i]) * (S.fvals[i + 1] + S.fvals[i]) / 2;
	// gradient: the reference integrates the dense nbps x nC matrix column by column
	// (cost.c:117-134, integrator.c:44-48); here every lane owns a coefficient and takes the same
	// sum node-wise, g[c] = sum_s colv[c][s] * (w_i df_i)[coli[c][s]], over the non-zeros of column c
	// of the collocation matrix only.  The column form is s-major ([s][cl]): lanes with consecutive
	// coefficients read consecutive LDS words.
	const int W4u = (SHARED && NOUT > 0 && D.uniform) ? D.cls_W[0] : 0;
	if (NOUT > 0 && !hasI && !hasF && (W4u == 8 || W4u == 12 || W4u == 16)) {
		// (SHARED: chosen per kernel where it measured faster -- the evaluation kernel with 3 or more outputs, the solve
		// of the large configs.)  One basis class: column cl of the collocation matrix is the same for every output.  A lane takes one
		// local coefficient cl for a share of the outputs: the packed (value index, breakpoint) entries and the
		// basis values of the column are read ONCE and reused for each of its outputs; only the weighted gradient
		// rows differ.  Per coefficient the sum runs over the derivative channels, then the column entries --
		// the same order as the per-coefficient form below, so the two are bit-identical.
		auto gather = [&](auto Wtag) {
			constexpr int W = decltype(Wtag)::value;
			constexpr int NO = NOUT > 0 ? NOUT : 1;
			const int nco = D.ncoef[0];
			const int G = max(1, min(NT / nco, NO)), OPG = (NO + G - 1) / G;   // lane groups, outputs per group
			for (int i = tid; i < G * nco; i += NT) {
				const int grp = i / nco, cl = i - grp * nco, o0 = grp * OPG;
				double a[NO];
#pragma unroll
				for (int j = 0; j < NO; j++) a[j] = 0.0;
#pragma unroll
				for (int r = 0; r < DM; r++) {
					const bool fixed = CHM != 0 && chm_ok;               // wave-uniform; with CHM the channel set is a constant
					if (fixed ? !((CHM >> r) & 1) : !((D.tav_rmask >> r) & 1)) continue;
					const int chc = S.chcol[r];
					if (!fixed && chc < 0) continue;
					const double *rv = S.rowv + S.chrow[r];
					int i0; unsigned int pe[W];
					colp_load<W>(S.colp + chc + cl * colp_words(W), i0, pe);
					double vv[W];
#pragma unroll
					for (int s2 = 0; s2 < W; s2++) vv[s2] = rv[pe[s2]];
#pragma unroll
					for (int j = 0; j < NO; j++) {
						const int o = o0 + j;
						if (j >= OPG || o >= NO) break;
						const int row = fixed ? o * chm_count(CHM) + chm_rank(CHM, r) : S.tavrow[DM * o + r];
						if (row < 0) continue;
						const double *wdf = S.dfz + row * (P + 1) + i0;   // consecutive breakpoints: constant offsets
						double ww[W];
#pragma unroll
						for (int s2 = 0; s2 < W; s2++) ww[s2] = wdf[s2];
#pragma unroll
						for (int s2 = 0; s2 < W; s2++) a[j] += vv[s2] * ww[s2];
					}
				}
#pragma unroll
				for (int j = 0; j < NO; j++) {
					const int o = o0 + j;
					if (j >= OPG || o >= NO) break;
					sg[o * nco + cl] = a[j];
					acc[1] += a[j] * a[j];
				}
			}
		};
		if (W4u == 8) gather(std::integral_constant<int, 8>());
		else if (W4u == 12) gather(std::integral_constant<int, 12>());
		else gather(std::integral_constant<int, 16>());
	} else if (NOUT > 0 && !hasI && !hasF) {
		// all (breakpoint, block column) pairs of a column are read first, then all values and
		// weighted gradients, then the FMAs: two LDS round trips per coefficient, independent of W
		auto gather = [&](auto Wtag) {
			constexpr int W = decltype(Wtag)::value;   // 0: run-time width
#pragma unroll
			for (int e = 0; e < EPT; e++) {
				const int c = tid + e * NT;
				if (c >= D.nC) break;
				double dIn = 0.0;
				const int o = cm.o[e], cl = cm.cl[e];
				const int *oi = S.oinfo + o * 10;
				const int chb = oi[6], nc = oi[9], Wr = oi[8];
#pragma unroll
				for (int r = 0; r < DM; r++) {
					const bool fixed = CHM != 0 && chm_ok;               // wave-uniform; with CHM the channel set is a constant
					if (fixed ? !((CHM >> r) & 1) : !((D.tav_rmask >> r) & 1)) continue;
					const int row = fixed ? o * chm_count(CHM) + chm_rank(CHM, r) : S.tavrow[DM * o + r], chc = S.chcol[chb + r];
					if (!fixed && (row < 0 || chc < 0)) continue;
					const double *rv = S.rowv + S.chrow[chb + r]; const double *wdf = S.dfz + row * (P + 1);
					if (W > 0) {
						constexpr int WC = W > 0 ? W : 4;
						int i0; unsigned int pe[WC];
						colp_load<WC>(S.colp + chc + cl * colp_words(WC), i0, pe);
						double vv[WC], ww[WC];
#pragma unroll
						for (int s2 = 0; s2 < WC; s2++) { vv[s2] = rv[pe[s2]]; ww[s2] = wdf[i0 + s2]; }
#pragma unroll
						for (int s2 = 0; s2 < WC; s2++) dIn += vv[s2] * ww[s2];
					} else {
						const unsigned int *cp = S.colp + chc + cl * colp_words(Wr);
						const int i0 = (int)cp[0];
						for (int s2 = 0; s2 < Wr; s2++) dIn += rv[(cp[1 + s2 / 2] >> (16 * (s2 & 1))) & 0xffffu] * wdf[i0 + s2];
					}
				}
				sg[c] = dIn;
				acc[1] += dIn * dIn;
				__builtin_amdgcn_sched_barrier(0);   // keep the slots sequential: their temporaries share registers
			}
		};
		const int W4 = D.uniform ? D.cls_W[0] : 1000;
		if (W4 == 8) gather(std::integral_constant<int, 8>());
		else if (W4 == 12) gather(std::integral_constant<int, 12>());
		else if (W4 == 16) gather(std::integral_constant<int, 16>());
		else gather(std::integral_constant<int, 0>());
	} else {
		for (int c = tid; c < D.nC; c += NT) {
			int o = 0;
			while (o + 1 < nout && S.oinfo[(o + 1) * 10 + 4] <= c) o++;
			const int *oi = S.oinfo + o * 10;
			const int k = oi[0], d = oi[3], iz = oi[5], cl = c - oi[4], chb = oi[6], W4 = oi[8], nc = oi[9];
			const int *coff = S.off + oi[7];
			double dI = 0.0, dIn = 0.0, dF = 0.0;
			for (int r = 0; r < d; r++) {
				const int row = S.tavrow[iz + r], chc = S.chcol[chb + r], chr = S.chrow[chb + r];
				if (row >= 0 && chc >= 0) {
					const unsigned int *cp = S.colp + chc + cl * colp_words(W4); const double *wdf = S.dfz + row * (P + 1) + (int)cp[0];
					for (int s = 0; s < W4; s++) dIn += S.rowv[chr + ((cp[1 + s / 2] >> (16 * (s & 1))) & 0xffffu)] * wdf[s];
				}
				if (chr >= 0) {
					if (hasI && cl < k) dI += S.dfi[iz + r] * S.rowv[chr + cl * P];                // colloc.c:243-260 (block 0)
					const int ol = coff[P - 1];
					if (hasF && cl >= ol && cl < ol + k) dF += S.dff[iz + r] * S.rowv[chr + (cl - ol) * P + P - 1];   // colloc.c:287-316
				}
			}
			double g = dI + dIn + dF;                             // Vector3Add (matrix.c:177)
			if (NOUT == 0 && li) {                                // + A_I' t of the linear inequality rows (generic instances only)
				double a = 0.0;
				for (int e = li->cptr[c]; e < li->cptr[c + 1]; e++) a += li->cval[e] * li->tI[li->crow[e]];
				g += a;
			}
			sg[c] = g;
			acc[1] += g * g;
		}
	}
	if (defer) {   // the caller folds these four partial sums into a reduction of its own (sqp_kernel: with the line search's slope)
		defer[0] = acc[0]; defer[1] = acc[1]; defer[2] = acc[2]; defer[3] = acc[3];
		return 0.0;
	}
	block_sum<NT, 4>(acc, S);
	const double I = D.nicf ? S.dfi[nz] : 0.0, Ff = D.nfcf ? S.dff[nz] : 0.0;
	*gnorm2 = acc[1];
	const double Fp = I + acc[0] + Ff;                            // ntg.c:328
	if (Fpure) *Fpure = Fp;
	if (rv2_out) *rv2_out = acc[3];
	return Fp + acc[2];
}

// NPfunobj (ntg.c:274-335): F and the full gradient into LDS vector sg.  Returns F; *gnorm2
// receives |g|^2.  Every lane of the workgroup must call it (it contains barriers).
template <int FAM, int NOUT, int K, int NT, int EPT, bool SHARED = false, int CHM = 0>
__device__ __forceinline__ double eval_cost(const NtgDims &D, const Smem &S, const double *sx, double *sg, double *gnorm2,
                                            const CoefMap<EPT> &cm, const ALState &al, double *Fpure = nullptr,
                                            double *rv2_out = nullptr, unsigned long long *tk = nullptr, const LinIneq *li = nullptr,
                                            bool chm_ok = false, double *defer = nullptr)
{
	using Fam = Family<FAM>;
	constexpr bool HASCON = Fam::NNLIC + Fam::NNLTC + Fam::NNLFC > 0;
	const bool alon = HASCON && al.mu > 0.0;
	unsigned long long t0 = 0;
	if (tk) t0 = __builtin_amdgcn_s_memtime();
	double psi, rv2;
	cost_phase1<FAM, NOUT, K, NT, CHM>(D, S, sx, al, psi, rv2, chm_ok);
	const bool lin_on = NOUT == 0 && li && li->nI > 0 && al.mu > 0.0;
	if (lin_on) lin_ineq_phase<NT>(D, *li, sx, al, psi, rv2);   // sx was complete before the functor pass
	if (tk) { lds_sync(); const unsigned long long t1 = __builtin_amdgcn_s_memtime(); tk[6] += t1 - t0; t0 = t1; }
	const double F = cost_phase2<NOUT, K, NT, Fam::DM, EPT, SHARED, CHM>(D, S, sg, gnorm2, cm, D.nicf || (alon && D.nnlic), D.nfcf || (alon && D.nnlfc),
	                                          psi, rv2, Fpure, rv2_out, lin_on ? li : nullptr,
	                                          chm_ok && (alon ? (D.tcost_mask | D.tcon_mask) : D.tcost_mask) == chm_full_mask(CHM, NOUT > 0 ? NOUT : 1, Fam::DM),
	                                          defer);
	if (tk) { const unsigned long long t1 = __builtin_amdgcn_s_memtime(); tk[7] += t1 - t0; }
	return F;
}

// Per-lane decode of the banded Jacobian's row emission (eval_constraints, the pair form), once per workgroup: lane ln of a wave owns the
// pair of entries (2 e2, 2 e2 + 1) of row slot rsub; tab[i][ln] = (scratch offset or -1, table offset) of the i-th derivative channel that
// contributes to ANY entry.  Returns false (nothing written) when the pair form does not apply: generic instance, odd order, a row wider
// than a wave's 64 pairs.
template <int NOUT, int K, int DM>
__device__ __forceinline__ bool emit_decode(const NtgDims &D, const Smem &S, int *emit_tab)
{
	if (!(NOUT > 0 && K > 0 && K % 2 == 0 && DM <= NTG_MAX_ORDER) || !emit_tab) return false;
	const int s2 = D.sumk >> 1, P = D.P;
	if (s2 > 64 || (D.sumk & 1)) return false;
	if (threadIdx.x >= 64) return true;
	const int ln = threadIdx.x, rpi = 64 / s2, rsub = ln / s2, e2 = ln - rsub * s2;
	const bool live = rsub < rpi;
	const int e = 2 * e2, o = min(e / (K > 0 ? K : 1), NOUT > 0 ? NOUT - 1 : 0), q = e - o * K, cc = D.cls[o], iz = DM * o;
	unsigned um = 0;
#pragma unroll
	for (int r = 0; r < DM; r++) {
		const bool on = live && S.tcomp[iz + r] >= 0 && S.chrow[cc * NTG_MAX_ORDER + r] >= 0;
		if (__ballot(on) != 0ull) um |= 1u << r;
	}
	um = __builtin_amdgcn_readfirstlane(um);
	const int na = __popc(um);
	int2 *tab = reinterpret_cast<int2 *>(emit_tab + 68);
#pragma unroll
	for (int i = 0; i < DM; i++) {
		if (i >= na) break;   // the layout holds the listed channels only
		const int r = um ? __ffs(um) - 1 : 0;
		const bool have = um != 0;
		um &= um - 1;
		const int comp = S.tcomp[iz + r], chr = S.chrow[cc * NTG_MAX_ORDER + r];
		const bool on = live && have && comp >= 0 && chr >= 0;
		tab[i * 64 + ln] = make_int2(on ? comp * P : -1, on ? chr + q * P : 0);
	}
	emit_tab[ln] = live ? (e2 | (rsub << 16)) : -1;
	if (ln == 0) emit_tab[64] = na;
	return true;
}

// NPfuncon (ntg.c:337-371, constraints.c:36-195): residuals and banded Jacobian rows straight
// to HBM.  Row order [initial; trajectory constraint-major x breakpoint; final].
template <int FAM, int NOUT, int K, int NT>
__device__ __forceinline__ void eval_constraints(const NtgDims &D, const Smem &S, const double *sx, int mode,
                                 double *c_out, double *jband, double *cjac, double *scratch, int scratch_cap, const int *emit_tab EVCLK_ARG)
{
	using Fam = Family<FAM>;
	constexpr int DM = Fam::DM, NZ = NOUT > 0 ? DM * NOUT : NTG_MAX_NZ;
	constexpr int NI = Fam::NNLIC > 0 ? Fam::NNLIC : 1, NTc = Fam::NNLTC > 0 ? Fam::NNLTC : 1, NF = Fam::NNLFC > 0 ? Fam::NNLFC : 1;
	const int P = D.P, nout = NOUT > 0 ? NOUT : D.nout, nz = D.nz, tid = threadIdx.x;
	const FamCall<Fam> fc{ntg_prm_row<FAM>(), D.nnltc};
	auto emit_row = [&](int row, int bp, const double *dcrow, double *jb) {
		for (int o = 0; o < nout; o++) {
			const int k = D.order[o], cc = D.cls[o], d = D.d[o];
			const int col0 = D.iC[o] + S.off[cc * P + bp];
			for (int q = 0; q < k; q++) {
				double a = 0.0;
				for (int r = 0; r < d; r++) {
					const int chr = S.chrow[cc * NTG_MAX_ORDER + r];
					if (chr >= 0) a += dcrow[D.iz[o] + r] * S.rowv[chr + q * P + bp];
				}
				if (jb) jb[(size_t)row * D.sumk + D.koff[o] + q] = a;
				if (cjac) cjac[(size_t)(col0 + q) * D.ncnln + row] = a;
			}
		}
	};
	if (Fam::NNLIC > 0 && D.nnlic && tid == 0) {
		double z[NZ], c[NI], dc[NI * NZ];
		compute_z<NOUT, K, DM>(D, S, sx, 0, D.icon_mask, z);
		fc.nlicf(nout, z, c, dc);
		for (int j = 0; j < D.nnlic; j++) {
			if (c_out && mode != 1) c_out[j] = c[j];
			if (mode != 0) emit_row(j, 0, dc + j * nz, jband);
		}
	}
	// Trajectory rows.  The banded Jacobian of one constraint is P consecutive rows of sum(k) entries: a contiguous block
	// of memory.  With one lane per breakpoint each store instruction would scatter 8-byte words sum(k)*8 bytes apart;
	// instead the lanes first leave the functor's derivatives dc[j][v] (v in the trajectory-constraint active variables --
	// a constraint depends on nothing else, ntg.h:57-60) in LDS, by breakpoint, and then walk the block in memory order:
	// consecutive lanes, consecutive words.  The LDS area is the weighted-gradient rows of the cost pass, which runs after
	// this; constraints are processed in chunks that fit it.
	const int ncomp = __popcll(D.tcon_mask);
	const bool coalesced = Fam::NNLTC > 0 && D.nnltc && jband && mode != 0 && ncomp > 0 && ncomp * P <= scratch_cap;
	constexpr u64 TV = Fam::TCON_VARS;
	const bool sparse_vars = TV != ~0ull && (D.tcon_mask & ~TV) == 0ull;   // every flagged entry is one the family's rows can touch
	if (Fam::NNLTC > 0 && D.nnltc) {
		const int chunk = coalesced ? max(1, min(D.nnltc, scratch_cap / (ncomp * P))) : D.nnltc;
		// with one breakpoint per lane (P <= NT) the flag, the values and the functor's tape are computed once and kept in
		// registers across the chunks; otherwise they are recomputed per chunk
		const bool keep = P <= NT;
		double z[NZ], c[NTc], tape[Fam::TAPE];
		for (int j0 = 0; j0 < D.nnltc; j0 += chunk) {
			const int jn = min(chunk, D.nnltc - j0);
			for (int i = tid; i < P; i += NT) {
				if (!keep || j0 == 0) {
					compute_z<NOUT, K, DM>(D, S, sx, i, D.tcon_mask, z);
					fc.template nltc_val<NZ>(nout, i, z, c, tape);
					EVCLK(6);
				}
				for (int j = j0; j < j0 + jn; j++) {
					const int row = D.nnlic + j * P + i;              // constraints.c:139,153
					if (c_out && mode != 1) c_out[row] = c[j];
					if (mode == 0) continue;
					// row j of the functor's Jacobian = J' e_j: one (sparse, for the large families) vjp instead of a dense
					// [ncon][nz] array in registers
					double t[NTc], dcr[NZ];
#pragma unroll
					for (int jj = 0; jj < NTc; jj++) t[jj] = jj == j ? 1.0 : 0.0;
#pragma unroll
					for (int v = 0; v < NZ; v++) dcr[v] = 0.0;
					fc.template nltc_vjp<NZ>(nout, nz, i, z, t, dcr, tape);
					if (cjac || !coalesced) emit_row(row, i, dcr, coalesced ? nullptr : jband);
					if (coalesced && sparse_vars) {
						// the family says which flag entries its rows can touch: only those are copied (12 of config E's 36, 6 of D's 20;
						// the walk over all NZ entries with a wave-uniform branch each was 5 k cycles per constraint)
#pragma unroll
						for (int v = 0; v < NZ; v++)
							if (((TV >> v) & 1ull) && ((D.tcon_mask >> v) & 1ull))   // compact index: scalar bit count, nothing kept in registers
								scratch[((j - j0) * ncomp + __popcll(D.tcon_mask & ((1ull << v) - 1ull))) * P + i] = dcr[v];
					} else if (coalesced) {
						int comp = 0;
#pragma unroll
						for (int v = 0; v < NZ; v++)
							if (v < nz && ((D.tcon_mask >> v) & 1ull)) { scratch[((j - j0) * ncomp + comp) * P + i] = dcr[v]; comp++; }
					}
				}
			}
			if (coalesced) {
				lds_sync();
				EVCLK(1);
				// a wave takes whole rows (stride NW); its lanes are the entries of the row, 64 at a time: a store
				// instruction writes 64 consecutive words, and what an entry needs to know about itself -- output, block
				// column, which derivative channels contribute -- is decoded once per lane, outside the loop over rows
				constexpr int NW = NT / 64, RMAX = NOUT > 0 ? DM : NTG_MAX_ORDER;
				const int sumk = D.sumk, nrows = jn * P, wv = tid >> 6, ln = tid & 63;
				double *dst = jband + (size_t)(D.nnlic + j0 * P) * sumk;
				// entries [e0, e0 + width) of 64 / width rows per step: a row narrower than a wave shares it with its neighbours
				// (sum(k) = 32: two rows per store instruction; the 8 left-over entries of a 72-entry row: eight rows)
				auto emit_pass = [&](int e0, int width) {
					const int rpi = 64 / width, rsub = ln / width, e = e0 + ln % width;
					if (rsub >= rpi) return;
					int o = 0;
					if (NOUT > 0 && K > 0) o = e / (K > 0 ? K : 1);    // one order for every output
					else while (o + 1 < nout && D.koff[o + 1] <= e) o++;
					const int q = e - (NOUT > 0 && K > 0 ? o * K : D.koff[o]), cc = D.cls[o], d = NOUT > 0 ? DM : D.d[o];
					const int iz = NOUT > 0 ? DM * o : D.iz[o];
					int cof[RMAX], rof[RMAX];                          // scratch / rowv offsets of the contributing channels, -1: none
#pragma unroll
					for (int r = 0; r < RMAX; r++) {
						const int comp = r < d ? S.tcomp[iz + r] : -1, chr = r < d ? S.chrow[cc * NTG_MAX_ORDER + r] : -1;
						const bool on = comp >= 0 && chr >= 0;
						cof[r] = on ? comp * P : -1; rof[r] = on ? chr + q * P : 0;
					}
					const int step = NW * rpi;
					int row = wv * rpi + rsub, jc = row / P, bp = row - jc * P;
					for (; row < nrows; row += step) {
						double a = 0.0;
#pragma unroll
						for (int r = 0; r < RMAX; r++)
							if (cof[r] >= 0) a += scratch[jc * ncomp * P + cof[r] + bp] * S.rowv[rof[r] + bp];
						dst[(size_t)row * sumk + e] = a;
						bp += step;
						while (bp >= P) { bp -= P; jc++; }
					}
				};
				// The tuned instances (one even order for every output, 16-byte aligned rows) emit PAIRS of adjacent entries: a lane
				// owns block columns (q, q + 1) of one output -- the functor's derivative is shared by the pair, the store is 16 bytes
				// per lane (1 KB per wave instruction).  The phase is bound by instruction issue (one or two waves per SIMD: ~8 cycles
				// per instruction, measured 760 cycles per 128 stored words before), so what counts is instructions per stored word:
				//  * the derivative channels that contribute to ANY entry of the wave (a wave-uniform set: the trajectory-constraint
				//    active variables name few derivatives -- 2 of config D's 6 channels, 1 of config E's 4) are compacted into a
				//    list once; the row loop is instantiated for the list's length NA and touches nothing else;
				//  * every load of a trip is unconditional (a lane whose entry lacks a listed channel multiplies by zero) and all of
				//    them -- UR rows x NA channels x 3 -- are in flight before the first is used: the empty asm makes every operand
				//    live at one point; under this kernel's register pressure the scheduler otherwise pairs each read with its wait;
				//  * the breakpoint index wraps branch-free.
				//  * what a lane needs to know about its pair is the same for every problem: it is decoded once per workgroup into LDS
				//    (emit_decode, called by eval_kernel before the problem loop) and costs 1 + NA reads here; decoding it per problem
				//    (two integer divisions, 4 DM table lookups, DM ballots) was HALF of the phase: 6.5 k of 13.5 k cycles, config D.
				auto emit_pairs = [&]() {
					const int s2 = sumk >> 1, rpi = 64 / s2;
					const int pk = emit_tab[ln];
					if (pk < 0) return;
					const int e2 = pk & 0xffff, rsub = pk >> 16;
					const int2 *tab = reinterpret_cast<const int2 *>(emit_tab + 68);
					const int na = __builtin_amdgcn_readfirstlane(emit_tab[64]);
					const int step = NW * rpi, cs = ncomp * P;
					double2 *dst2 = reinterpret_cast<double2 *>(dst);
					auto rows = [&](auto na_) {
						constexpr int NA = decltype(na_)::value, UR = NA == 1 ? 4 : (NA == 2 ? 4 : (NA <= 4 ? 2 : 1));
						int cofA[NA > 0 ? NA : 1], rofA[NA > 0 ? NA : 1]; double useA[NA > 0 ? NA : 1];
#pragma unroll
						for (int i = 0; i < NA; i++) {
							const int2 t = tab[i * 64 + ln];
							cofA[i] = max(t.x, 0); rofA[i] = t.y; useA[i] = t.x >= 0 ? 1.0 : 0.0;
						}
						int row = wv * rpi + rsub, jc = 0, bp = row;
						while (bp >= P) { bp -= P; jc++; }
						EVCLK(4);
						if (step <= P) {
							for (; row + (UR - 1) * step < nrows; row += UR * step) {
								int jcu[UR], bpu[UR];
								jcu[0] = jc; bpu[0] = bp;
#pragma unroll
								for (int u = 1; u < UR; u++) {
									const int bb = bpu[u - 1] + step; const bool w = bb >= P;
									bpu[u] = bb - (w ? P : 0); jcu[u] = jcu[u - 1] + (w ? 1 : 0);
								}
								double sa[UR][NA > 0 ? NA : 1], r0[UR][NA > 0 ? NA : 1], r1[UR][NA > 0 ? NA : 1];
#pragma unroll
								for (int u = 0; u < UR; u++)
#pragma unroll
									for (int i = 0; i < NA; i++) {
										sa[u][i] = scratch[jcu[u] * cs + cofA[i] + bpu[u]];
										r0[u][i] = S.rowv[rofA[i] + bpu[u]];
										r1[u][i] = S.rowv[rofA[i] + P + bpu[u]];
									}
#pragma unroll
								for (int u = 0; u < UR; u++)
#pragma unroll
									for (int i = 0; i < NA; i++) asm volatile("" : "+v"(sa[u][i]), "+v"(r0[u][i]), "+v"(r1[u][i]));
#pragma unroll
								for (int u = 0; u < UR; u++) {
									double a0 = 0.0, a1 = 0.0;
#pragma unroll
									for (int i = 0; i < NA; i++) { const double t = sa[u][i] * useA[i]; a0 += t * r0[u][i]; a1 += t * r1[u][i]; }
									dst2[(size_t)(row + u * step) * s2 + e2] = make_double2(a0, a1);
								}
								{ const int bb = bpu[UR - 1] + step; const bool w = bb >= P; bp = bb - (w ? P : 0); jc = jcu[UR - 1] + (w ? 1 : 0); }
							}
						}
						for (; row < nrows; row += step) {
							double a0 = 0.0, a1 = 0.0;
#pragma unroll
							for (int i = 0; i < NA; i++) {
								const double t = scratch[jc * cs + cofA[i] + bp] * useA[i];
								a0 += t * S.rowv[rofA[i] + bp]; a1 += t * S.rowv[rofA[i] + P + bp];
							}
							dst2[(size_t)row * s2 + e2] = make_double2(a0, a1);
							bp += step;
							while (bp >= P) { bp -= P; jc++; }
						}
					};
					if (na == 0) rows(std::integral_constant<int, 0>{});
					else if (na == 1) rows(std::integral_constant<int, 1>{});
					else if (na == 2) rows(std::integral_constant<int, 2>{});
					else if (na == 3) rows(std::integral_constant<int, 3>{});
					else if (na == 4) rows(std::integral_constant<int, 4>{});
					else if (na == 5) rows(std::integral_constant<int, (RMAX >= 5 ? 5 : 0)>{});
					else if (na == 6) rows(std::integral_constant<int, (RMAX >= 6 ? 6 : 0)>{});
					else if (na == 7) rows(std::integral_constant<int, (RMAX >= 7 ? 7 : 0)>{});
					else rows(std::integral_constant<int, (RMAX >= 8 ? 8 : 0)>{});
					EVCLK(5);
				};
				if (emit_tab && ((uintptr_t)dst & 15) == 0) emit_pairs();
				else
				for (int e0 = 0; e0 < sumk; e0 += 64) emit_pass(e0, min(64, sumk - e0));
				lds_sync();
				EVCLK(2);
			}
		}
	}
	if (Fam::NNLFC > 0 && D.nnlfc && tid == (NT > 64 ? 64 : 0)) {
		double z[NZ], c[NF], dc[NF * NZ];
		compute_z<NOUT, K, DM>(D, S, sx, P - 1, D.fcon_mask, z);
		fc.nlfcf(nout, z, c, dc);
		for (int j = 0; j < D.nnlfc; j++) {
			const int row = D.nnlic + D.nnltc * P + j;
			if (c_out && mode != 1) c_out[row] = c[j];
			if (mode != 0) emit_row(row, P - 1, dc + j * nz, jband);
		}
	}
}

// Persistent workgroups stride over the batch; tables are staged once per workgroup.
// BANDONLY: the instance for the common full request (mode 2: values, gradient, residuals, banded Jacobian rows; no dense Jacobian) with
// that request as a compile-time fact -- the dense-row path, the per-entry scatter and the mode tests are not in its code at all (the
// general instance of config D is 26.6 k instructions with 3.1 k scalar-spill instructions among them).
template <int FAM, int NOUT, int K, int NT, int EPT, int CHM, bool BANDONLY = false>
__global__ void __launch_bounds__(NT, NTG_EVAL_WAVES)
eval_kernel(NtgDims D, NtgTables T, SmemLayout L, int batch, int mode, const double *__restrict__ x,
            double *__restrict__ f, double *__restrict__ g, double *__restrict__ c,
            double *__restrict__ jband, double *__restrict__ cjac)
{
	if (BANDONLY) { mode = 2; cjac = nullptr; }
	extern __shared__ __attribute__((aligned(16))) char smem_raw[];
	EVCLK_DECL
	Smem S(smem_raw, L, D, T);
	const bool pp = T.pp_rowv != 0;   // per-problem grids: the value tables are staged again for every problem
	if (!pp) stage_tables<NT>(D, T, S, smem_raw, L);
	const int *emit_tab = nullptr;   // the row emission's decode depends on the plan only (not on the grid's values): once per workgroup
	if (L.emit >= 0 && jband && mode != 0) {
		if (pp) stage_tables<NT>(D, T, S, smem_raw, L, blockIdx.x < batch ? blockIdx.x : 0);
		lds_sync();
		if (emit_decode<NOUT, K, Family<FAM>::DM>(D, S, (int *)(smem_raw + L.emit))) emit_tab = (const int *)(smem_raw + L.emit);
	}
	double *sg = S.x;   // the gradient is assembled (owner lanes, after the last read of x) into the x buffer
	lds_sync();
	CoefMap<EPT> cm;
	if (NOUT > 0) make_coefmap<NT, EPT>(D, S, cm);   // the host only picks a NOUT > 0 instance when nC <= EPT NT
	// software pipeline over problems: the coefficient vector of the NEXT problem is already in
	// flight (registers) while the current one is evaluated
	constexpr int XE = EPT;
	const bool xreg = D.nC <= XE * NT;
	double xn[XE];
	if (xreg && (int)blockIdx.x < batch) {
#pragma unroll
		for (int e = 0; e < XE; e++) { const int i = threadIdx.x + e * NT; xn[e] = i < D.nC ? x[(size_t)blockIdx.x * D.nC + i] : 0.0; }
	}
	EVCLK0();
	for (int b = blockIdx.x; b < batch; b += gridDim.x) {
		lds_sync();
		if (pp) { stage_tables<NT>(D, T, S, smem_raw, L, b); lds_sync(); }
		if constexpr (fam_prm_kind<Family<FAM>>() != 0) { ntg_prm_publish<FAM>(T, b); lds_sync(); }
		if (xreg) {
#pragma unroll
			for (int e = 0; e < XE; e++) { const int i = threadIdx.x + e * NT; if (i < D.nC) S.x[i] = xn[e]; }
			const int bn = b + gridDim.x;
			if (bn < batch) {
#pragma unroll
				for (int e = 0; e < XE; e++) { const int i = threadIdx.x + e * NT; xn[e] = i < D.nC ? x[(size_t)bn * D.nC + i] : 0.0; }
			}
		} else {
			for (int i = threadIdx.x; i < D.nC; i += NT) S.x[i] = x[(size_t)b * D.nC + i];
		}
		const int P1 = D.P + 1;
		EVCLK(0);
		if (D.ncnln && (c || jband || cjac)) {   // constraints first: they still need x, the cost pass overwrites it with g
			lds_sync();
			eval_constraints<FAM, NOUT, K, NT>(D, S, S.x, mode, c ? c + (size_t)b * D.ncnln : nullptr,
			                                jband ? jband + (size_t)b * D.ncnln * D.sumk : nullptr,
			                                cjac ? cjac + (size_t)b * D.ncnln * D.nC : nullptr,
			                                S.dfz, L.dfz_rows * (P1) + ntg_dfz_tail(D), emit_tab EVCLK_PASS);
		}
		double gn2;
		const double F = eval_cost<FAM, NOUT, K, NT, EPT, (NOUT >= 3), CHM>(D, S, S.x, sg, &gn2, cm, ALState{0.0, nullptr, nullptr, nullptr, nullptr},
		                                                                   nullptr, nullptr, EVCLK_TK, nullptr, CHM != 0);
		if (f && mode != 1 && threadIdx.x == 0) f[b] = F;
		if (g && mode != 0)
			for (int i = threadIdx.x; i < D.nC; i += NT) g[(size_t)b * D.nC + i] = sg[i];
		EVCLK(3);
	}
#ifdef NTG_EVAL_CLOCK
	if (blockIdx.x == 0 && threadIdx.x == 0) {
		printf("evclk: stage-x %llu functor %llu emission %llu cost+g %llu | emission: prologue %llu rows %llu | functor: z+val %llu | cost: phase1 %llu phase2 %llu\n", ntg_evclk_s[0], ntg_evclk_s[1], ntg_evclk_s[2], ntg_evclk_s[3], ntg_evclk_s[4], ntg_evclk_s[5], ntg_evclk_s[6], ntg_evclk_s[10], ntg_evclk_s[11]);
	}
#endif
}
