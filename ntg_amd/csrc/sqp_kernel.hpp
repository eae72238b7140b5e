// sqp_kernel.hpp -- sqp_kernel: one workgroup solves one problem from start to finish, on the evaluation (eval.hpp), the
// direction pieces (direction.hpp), the line search (linesearch.hpp) and the Newton / QP steps (newton.hpp).  Included by
// solve_impl.hpp only, i.e. by the units that instantiate the kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "ntg_dev.hpp"
#include "families.hpp"
#include "linesearch.hpp"
#include "nwt_map.hpp"
#include "wave_ops.hpp"
#include "newton.hpp"
#include "lds_tables.hpp"
#include "eval.hpp"
#include "direction.hpp"

// tuning knobs: minimum waves per SIMD the register allocator must leave room for; the direction
// form of the quasi-Newton memory (apply_dform) on or off, and how many of its vectors one reduction round covers
#ifndef NTG_SQP_WAVES
#define NTG_SQP_WAVES 2
#endif
#ifndef NTG_DFORM
#define NTG_DFORM 1
#endif
#ifndef NTG_DF_G
#define NTG_DF_G 4
#endif

// One workgroup solves one problem from start to finish (ntg.c:250: the npsol_ call).
// The loop below has ONE evaluation site (funobj + projection at the trial point sxt); what the
// result means is decided by `state`: the first evaluation, a line-search trial, a forced
// acceptance, or the final multiplier estimate.  One site keeps the assembly code inlined once
// and the register state (coefficient map, line search) out of scratch.
// BIG: the coefficient vectors no longer fit in LDS next to the tables (config E: nC = 2196).  Only the trial point
// (read across lanes by Z = M C at every evaluation) stays in LDS; x, gp, gp+, d and g live in a per-problem HBM/L2
// workspace `vec_all`.  They are touched element-wise by their owner lane, except in the projection, the feasibility
// step and the preconditioner, which read a handful of entries across lanes behind a full barrier.
// NWT: the structured Newton mode (ntg_solve_opts.hessian = 2, newton.hpp): W is the inverse of the banded second-order
// model of the augmented Lagrangian, refactored at every major iteration; no quasi-Newton pairs.  The solve starts with
// a pass on the objective alone (mu = 0, "phase 0") before the augmented-Lagrangian passes.
// (The Newton instances of 256 lanes run one wave per SIMD anyway -- one workgroup per CU, by LDS -- and are compiled for it: the
// inlined factorisation and assembly then keep their window tiles and addresses in registers instead of scratch.)
// QPM (with NWT): the QP-based SQP step (ntg_solve_opts.hessian = 3, qpdual.hpp) replaces the augmented-Lagrangian
// passes after phase 0.
template <int FAM, int NOUT, int K, int NT, int EPT, bool BIG, bool HESS, int CHM, bool NWT = false, bool QPM = false>
__global__ void __launch_bounds__(NT, (NWT && NT <= 256) ? 1 : NTG_SQP_WAVES)
sqp_kernel(NtgDims D, NtgTables T, SmemLayout L, SolveParams sp, int batch,
           const double *__restrict__ lower, const double *__restrict__ upper, double *__restrict__ xio,
           double *__restrict__ objective, int *__restrict__ inform_out, int *__restrict__ iters_out,
           int *__restrict__ nfev_out, double *__restrict__ clambda, double *__restrict__ hist_all,
           double *__restrict__ al_all, double *__restrict__ vec_all, double *__restrict__ nwt_all)
{
	extern __shared__ __attribute__((aligned(16))) char smem_raw[];
	const int b = blockIdx.x, tid = threadIdx.x, n = D.nC, m = D.mE /* rows kept by projection */, P = D.P;
	if (b >= batch) return;
	Smem S(smem_raw, L, D, T, b);
	const int npad = (n + 1) & ~1;
	double *gv = BIG ? vec_all + (size_t)b * 5 * npad : nullptr;
	double *sx = BIG ? gv : S.x, *sxt = S.vecs, *sgp = BIG ? gv + npad : S.vecs + npad,
	       *sgpt = BIG ? gv + 2 * npad : S.vecs + 2 * npad, *sd = BIG ? gv + 3 * npad : S.vecs + 3 * npad,
	       *st = sxt /* t = W gp+ lives in the trial-point buffer once x is committed */,
	       *sg = BIG ? gv + 4 * npad : S.vecs + 4 * npad, *tmp = S.vecs + (BIG ? 1 : 5) * npad;
	double *hist = hist_all + (size_t)b * sp.memcap * (2 * n + 2);   // pair i: [s (n) | u (n) | rho | c2]
	const double *hrc = L.hrc_n >= sp.memcap ? S.rho : nullptr;
	// one vector per major (apply_dform): problems without augmented-Lagrangian passes (the direction is never re-projected), a memory that
	// cannot fill up before the iteration limit, link scalars in LDS
	constexpr bool DF_OK = !NWT && !BIG && EPT <= 4 && Family<FAM>::NNLIC + Family<FAM>::NNLTC + Family<FAM>::NNLFC == 0;
	const bool dform = DF_OK && NTG_DFORM && D.nI == 0 && D.nC <= 3 * NT && hrc != nullptr && sp.memcap >= sp.itlim && L.hrc_n > sp.memcap;   // pair scalars (rho, c2): LDS for memories that fit, else with the pair in HBM
	stage_tables<NT>(D, T, S, smem_raw, L, b);
	ntg_prm_publish<FAM>(T, b);   // (families with parameters; the barrier below orders it before the first evaluation)
	NtgTables Tw = T;   // the preconditioner blocks of this problem (per-problem grids) or the shared ones (stride 0)
	if (HESS && T.n0b) Tw.n0b = T.n0b + (size_t)b * T.pp_n0b;
	if (NWT && T.nwt_k0) { Tw.nwt_k0 = T.nwt_k0 + (size_t)b * T.pp_k0; Tw.nwt_lf = T.nwt_lf + (size_t)b * T.pp_lf; }   // ... and the Newton mode's cost model / free-output factors
	for (int i = tid; i < n; i += NT) sx[i] = xio[(size_t)b * n + i];
	lds_sync();
	CoefMap<EPT> cm;
	if (NOUT > 0) make_coefmap<NT, EPT>(D, S, cm);

	enum { ST_INIT = 0, ST_LS = 1, ST_FORCE = 2, ST_FINAL = 3, ST_REEVAL = 4, ST_QP = 5 /* QP-based SQP step: evaluation of the l1 merit function */ };
	using Fam = Family<FAM>;
	constexpr bool HASCON = Fam::NNLIC + Fam::NNLTC + Fam::NNLFC > 0;
	const int ncn = D.ncnln;
	// linear rows declared as inequalities ride the same loop; only the generic instances carry that code
	constexpr bool LIN = NOUT == 0;
	const int nI = LIN ? D.nI : 0, nal = ncn + nI;
	// augmented-Lagrangian state (nonlinear rows, then linear inequality rows): multipliers and their estimates live in HBM
	double *al_lam = al_all + (size_t)b * 2 * (ncn + D.nI), *al_t = al_lam + ncn + D.nI;
	// diagnostic phase clock (sp.stamps): cycles spent in eval / project / history (structured Newton mode: model assembly) / W0 (Newton: factor + solve) / rest
	// Variant builds only (-DNTG_CLOCK: tools/mkvariant2.sh; tests/tools_newton.py, tests/tools_stamps.py): compiled in, the eight 64-bit
	// accumulators and the time base are 18 registers live across the whole kernel (the wave kernel gained 10 % when its clock went).
#ifdef NTG_CLOCK
	unsigned long long tk[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tlast = 0;
#define NTG_STAMP(slot) do { if (sp.stamps) { const unsigned long long now_ = __builtin_amdgcn_s_memtime(); tk[slot] += now_ - tlast; tlast = now_; } } while (0)
#define NTG_CLOCK_TK(cond) ((cond) ? tk : nullptr)
	if (sp.stamps) tlast = __builtin_amdgcn_s_memtime();
#else
#define NTG_STAMP(slot) do { } while (0)
#define NTG_CLOCK_TK(cond) ((unsigned long long *)nullptr)
#endif
	const bool alprob = (HASCON && ncn > 0) || nI > 0;   // rows handled by the augmented-Lagrangian loop
	ALState al{(alprob && (!NWT || sp.warm)) ? 10.0 : 0.0, al_lam, al_t, lower + (size_t)b * D.nbounds, upper + (size_t)b * D.nbounds};
	// structured Newton mode: band matrix / factor and the per-breakpoint blocks of this problem (HBM), flags
	using FamN = Family<FAM>;
	constexpr int NWT_CG2 = FamN::CG * FamN::CG, NWT_CG2S = FamN::CG;
	// per problem: the groups' band arrays, [two-sided factorisation: their reversed arrays,] the per-breakpoint blocks
	const size_t nwt_ksz = (size_t)D.nwt_ngrp * D.nwt_ng * (D.nwt_hb + 1) + (D.nwt_tw ? (size_t)D.nwt_ngrp * (16 * D.nwt_jb + 48) * (D.nwt_hb + 1) : 0);
	// (QP-based SQP step: + the slots' columns U = W J' [NTG_QP_MAXA][npad] and the QP's multipliers of the previous major iteration [ncnln])
	const size_t ncq = (size_t)((D.ncnln + 1) & ~1);   // rows of the QP's per-row arrays: multipliers, c, J W g, derivative rows [CG], J U [NTG_QP_MAXA]
	const size_t qp_pp = QPM ? (size_t)ntg_qp_maxa(D.nwt_ngrp, NT) * npad + ncq * (3 + NWT_CG2S + ntg_qp_maxa(D.nwt_ngrp, NT)) : 0;
	double *nwt_K = NWT ? nwt_all + (size_t)b * (nwt_ksz + (size_t)D.nwt_ngrp * D.P * NWT_CG2 + qp_pp) : nullptr;
	double *nwt_B = NWT ? nwt_K + nwt_ksz : nullptr;
	double *qp_U = NWT ? nwt_B + (size_t)D.nwt_ngrp * D.P * NWT_CG2 : nullptr, *qp_lamq = NWT ? qp_U + (size_t)ntg_qp_maxa(D.nwt_ngrp, NT) * npad : nullptr;
	const NwtPair nwt_q{D.nwt_ng, D.nwt_hb, D.nwt_ja, D.nwt_jb};
	const int nwt_lena = 16 * (D.nwt_ja + 3) + 48, nwt_lenb = 16 * (D.nwt_jb + 3) + 48;
	// LDS of the mode (the area at L.nwt_y): the groups' solve vectors, the factorisation panels (one per factoring wave), the free outputs' vectors
	const int nwt_yall = D.nwt_ngrp * (D.nwt_tw ? nwt_lena + nwt_lenb : 16 * ((D.nwt_ng + 15) >> 4) + 48), nwt_npan = (D.nwt_tw ? 2 : 1) * D.nwt_ngrp;
	bool nwt_curv = false;        // the current factor includes the constraint curvature
	bool nwt_k0_only = false;     // the current factor is the cost model's alone (nwt_refresh_ex without blocks)
	int nwt_bad = 0;              // diagnostic: non-positive pivots replaced in Gauss-Newton factorisations (wave 0's count)
	int nwt_nfact = 0, nwt_nfail = 0, nwt_napply = 0;   // diagnostic (sp.stamps == 3): factorisations, of which not positive definite, solves
	bool phase0 = NWT && alprob && !sp.warm;  // the pass on the objective alone is still running (a warm start goes straight to the multipliers it was given)
	int *nwt_flag = (int *)(smem_raw + L.red) + 2 * (32 * (NT / 64) + 2) - 2;   // last word pair of the reduction scratch: "not positive definite"
	// K = model at the trial point buffer `xs` (must be the iterate x; needs the multiplier estimates al_t of the evaluation
	// at x), factored; then out = W v.  allow_curv = false: Gauss-Newton terms only.
	// tsrc / mu_gn: the multipliers of the curvature term and the weight of the Gauss-Newton term -- the estimates al_t and the penalty al.mu
	// for the augmented Lagrangian; the QP's multipliers al_lam and 0 for the QP-based SQP step (the Lagrangian's Hessian on the band)
	auto nwt_refresh_ex = [&](const double *xs, bool allow_curv, const double *tsrc, double mu_gn, bool blocks) __attribute__((always_inline)) {
		const int ngp = D.nwt_ngrp, ng = D.nwt_ng, hb = D.nwt_hb, P2 = D.P;
		const int wave = tid >> 6;
		// Without blocks the matrix is the cost model K0 -- a constant of the problem: while the factor in nwt_K is K0's (the majors of the pass
		// on the objective alone, the QP step's no-curvature regime) there is nothing to assemble or factor again.  Same matrix, same factor:
		// the iterates are bit for bit those of refactoring every time.
		if (!blocks && nwt_k0_only) return;
		unsigned long long *nwt_act = (unsigned long long *)((double *)(smem_raw + L.nwt_y) + (NT / 64) * NWT_STAGE);   // after the assembly's staging buffers
		double *panel = (double *)(smem_raw + L.nwt_y) + nwt_yall;
		for (int attempt = (allow_curv && blocks) ? 0 : 1; attempt < 2; attempt++) {
			const bool curv = attempt == 0;
			if (blocks) {
				constexpr int DM = FamN::DM, NZ = NOUT > 0 ? DM * NOUT : NTG_MAX_NZ, NTc = FamN::NNLTC > 0 ? FamN::NNLTC : 1;
				lds_sync();
				for (int i = tid; i < P2; i += NT) {
					double z[NZ], t[NTc];
					compute_z<NOUT, K, DM>(D, S, xs, i, D.tcon_mask, z);
#pragma unroll
					for (int j = 0; j < NTc; j++) t[j] = j < D.nnltc ? tsrc[D.nnlic + j * P2 + i] : 0.0;
					for (int g = 0; g < ngp; g++) {
						double Bk[NWT_CG2];
						FamCall<FamN>{ntg_prm_row<FAM>(), D.nnltc}.template nltc_block<NZ>(NOUT > 0 ? NOUT : D.nout, g, z, t, mu_gn, curv, Bk);
						bool nzb = false;
#pragma unroll
						for (int e = 0; e < NWT_CG2; e++) { nwt_B[((size_t)g * P2 + i) * NWT_CG2 + e] = Bk[e]; nzb = nzb || Bk[e] != 0.0; }
						// which breakpoints carry a non-zero block: one 64-bit word per wave and sweep (a wave's lanes are 64 consecutive
						// breakpoints), read by the assembly to skip intervals that add nothing before it requests anything
						const unsigned long long mb = __ballot(nzb);
						if ((tid & 63) == 0) nwt_act[g * ((P2 + 63) >> 6) + (i >> 6)] = mb;
					}
				}
				__syncthreads();
			}
			NTG_STAMP(6);
			if (tid == 0) nwt_flag[0] = 0;
			nwt_assemble<NT, FamN::CG>(D, Tw, S.rowv, S.chrow, S.off, blocks ? nwt_B : nullptr, nwt_K, (double *)(smem_raw + L.nwt_y), NTG_CLOCK_TK(sp.stamps == 4));   // ends with a full barrier
			NTG_STAMP(3);
			if (D.nwt_tw) {   // two waves per group (wave uniform: every wave takes this branch)
				const int f = nwt_factor_pairs(nwt_K, nwt_K + (size_t)ngp * ng * (hb + 1), ngp, nwt_q, panel, curv ? 1 : 0, nwt_flag);
				if (f && !curv) nwt_bad += f;
			} else if (wave < ngp) {
				const int f = nwt_factor_wave((nwt_glb_dp)(nwt_K + (size_t)wave * ng * (hb + 1)), ng, hb, (nwt_lds_dp)(panel + (size_t)wave * NWT_PANEL), curv ? 1 : 0, 1 << 20);
				if (f && curv && (tid & 63) == 0) nwt_flag[0] = 1;
				if (f && !curv) nwt_bad += f;
			}
			__syncthreads();
			NTG_STAMP(7);
			nwt_curv = curv;
			nwt_nfact++;
			if (nwt_flag[0] == 0) break;
			nwt_nfail++;
		}
		nwt_k0_only = !blocks;
	};
	auto nwt_refresh = [&](const double *xs, bool allow_curv) __attribute__((always_inline)) { nwt_refresh_ex(xs, allow_curv, al_t, al.mu, al.mu > 0.0); };
	// restore = false: the caller keeps using the borrowed area (the QP-based SQP step's slots live behind the solve vectors) and puts
	// the zero padding of the weighted-gradient rows back itself (nwt_restore)
	auto nwt_restore = [&]() __attribute__((always_inline)) {
		for (int r = tid; r < L.dfz_rows; r += NT) S.dfz[r * (D.P + 1) + D.P] = 0.0;
		for (int i = tid; i < ntg_dfz_tail(D); i += NT) S.dfz[L.dfz_rows * (D.P + 1) + i] = 0.0;
		lds_sync();
	};
	auto nwt_apply = [&](const double *v, double *out, bool restore = true) __attribute__((always_inline)) {
		const int ngp = D.nwt_ngrp, ng = D.nwt_ng, hb = D.nwt_hb, ylen = 16 * ((ng + 15) >> 4) + 48;
		const int wave = tid >> 6;
		double *yv = (double *)(smem_raw + L.nwt_y);
		nwt_napply++;
		if (BIG) __syncthreads(); else lds_sync();
		const bool tw = D.nwt_tw != 0;
		const int ngt = ng - 16 * D.nwt_jb;   // two-sided: entries of the top part and the separator (vector a), the rest reversed (vector b)
		double *yb = yv + (size_t)ngp * nwt_lena;
		if (tw) {
			for (int i = tid; i < ngp * nwt_lena; i += NT) { const int g = i / nwt_lena, pp = i - g * nwt_lena; yv[i] = pp < ngt ? v[T.nwt_map[g * ng + pp]] : 0.0; }
			for (int i = tid; i < ngp * nwt_lenb; i += NT) { const int g = i / nwt_lenb, pp = i - g * nwt_lenb; yb[i] = pp < 16 * D.nwt_jb ? v[T.nwt_map[g * ng + ng - 1 - pp]] : 0.0; }
		} else
		for (int i = tid; i < ngp * ylen; i += NT) {
			const int g = i / ylen, pp = i - g * ylen;
			yv[i] = pp < ng ? v[T.nwt_map[g * ng + pp]] : 0.0;
		}
		// free outputs (in no nonlinear row): their vectors sit behind the groups' vectors and panels; the factor is the plan's
		const int nfo = D.nwt_nfo, ngf = D.nwt_ngf, hbf = D.nwt_hbf, ylenf = 16 * ((ngf + 15) >> 4) + 48;
		double *yvf = yv + (size_t)nwt_yall + (size_t)nwt_npan * NWT_PANEL;
		const int wfree = tw ? 2 * ngp : ngp;   // first wave that takes a free output
		for (int i = tid; i < nfo * ylenf; i += NT) {
			const int f = i / ylenf, pp = i - f * ylenf;
			yvf[i] = pp < ngf ? v[T.nwt_map[ngp * ng + f * ngf + pp]] : 0.0;
		}
		auto free_solves = [&] {
			if (wave >= wfree && wave < wfree + nfo) nwt_solve_wave((nwt_glb_cdp)(Tw.nwt_lf + (size_t)(wave - wfree) * ngf * (hbf + 1)), ngf, hbf, (nwt_lds_dp)(yvf + (size_t)(wave - wfree) * ylenf));
		};
		if (tw) {
			__syncthreads();
			nwt_solve_pairs(nwt_K, nwt_K + (size_t)ngp * ng * (hb + 1), ngp, nwt_q, yv, yb, free_solves);   // ends with a workgroup barrier
		} else {
			lds_sync();
			if (wave < ngp) nwt_solve_wave((nwt_glb_cdp)(nwt_K + (size_t)wave * ng * (hb + 1)), ng, hb, (nwt_lds_dp)(yv + (size_t)wave * ylen));
			else free_solves();
			lds_sync();
		}
		for (int c = tid; c < n; c += NT) {
			const int pos = T.nwt_pos[c];
			double o = 0.0;
			if (pos >= ngp * ng) { const int pf = pos - ngp * ng; o = yvf[(pf / ngf) * ylenf + (pf % ngf)]; }
			else if (pos >= 0) {
				const int g = pos / ng, pp = pos - g * ng;
				o = !tw ? yv[g * ylen + pp] : (pp < ngt ? yv[g * nwt_lena + pp] : yb[g * nwt_lenb + (ng - 1 - pp)]);
			}
			out[c] = o;
		}
		if (BIG) __syncthreads(); else lds_sync();
		// the area borrowed from the weighted-gradient rows goes back with its zero padding restored (stage_tables)
		if (restore) nwt_restore();
	};

	// =====================================================================================================================
	// QP-based SQP step on the band model (QPM; ntg_solve_opts.hessian = 3; qpdual.hpp).  Per major iteration:
	//   K = cost model + sum_j lam_j d2c_j/dz2 on the band (nwt_refresh_ex with the QP's multipliers), factored;
	//   the dual active-set QP of every coupling group on its SLOTS (rows in the working set): a row enters when the model step violates
	//   its linearised bound most; its column U = W J' is ONE band solve (the groups' entering rows share the solve: W is block diagonal
	//   by group), its entries of S = J W J' are products of derivative rows with Z = M U at the slots' breakpoints; the passive-set
	//   solves run on the group's slots in LDS, by the lanes of the group's wave (qpdual.hpp, qp_passive_solve_wave);
	//   p = -W g - sum_a lam_a U_a.
	// The line search backtracks on the l1 merit function, which the one evaluation site returns in this mode (ALState::qp).
	// =====================================================================================================================
	const int QA = ntg_qp_maxa(D.nwt_ngrp, NT), QPD = ntg_qp_doubles(QA);   // slots per coupling group, LDS doubles of a group's slot state
	// (the slots are addressed through LDS-typed pointers: ds_read / ds_write instead of FLAT accesses, which would also count in vmcnt and wait
	// for whatever the wave has in flight to HBM)
	typedef __attribute__((address_space(3))) int *lds_ip;
	typedef QpSlotsT<lds_dp, lds_ip> QpSlots;
	const int qp_ylenf = 16 * ((D.nwt_ngf + 15) >> 4) + 48;
	lds_dp qpbase = (lds_dp)((double *)(smem_raw + L.nwt_y) + nwt_yall + nwt_npan * NWT_PANEL + D.nwt_nfo * qp_ylenf);
	lds_dp qpred = qpbase + D.nwt_ngrp * QPD;   // [waves][rows per breakpoint][2] scratch of the entering-row search
	double qp_rho = 1.0, qp_phi0 = 0.0, qp_D = 0.0, qp_alpha = 1.0, qp_viol1 = 0.0, qp_pn = 0.0, qp_xn = 0.0, qp_lmax = 0.0, qp_gl = 0.0;
	int qp_k = 0, qp_over = 0, qp_nsolve = 0, qp_ncol = 0, qp_nocurv = 0, qp_fell = 0, qp_ntab = 0;
	bool qp_first = true, qp_full = false, qp_last = false;   // qp_last: the final pass evaluates at the point the last step led to   // qp_full: a group's working set did not hold every row the last QP wanted
	(void)qp_over; (void)qp_nsolve; (void)qp_ncol; (void)qp_fell; (void)qp_ntab;
	// flag entry (index into z) of variable u of group g
	auto qp_flag = [&](int g, int u) __attribute__((always_inline)) { return FamN::DM * (g * D.nwt_go + (int)((D.nwt_upack >> (8 * u + 4)) & 15u)) + (int)((D.nwt_upack >> (8 * u)) & 15u); };
	// Row caches of one major iteration (HBM, per problem): for every trajectory row (constraint-major, like c) its value c, J W g, its
	// derivative row on the group's CG flag entries, and -- per slot index -- J U (the row times the slot's column): the entering-row
	// search, the entries of S and the right-hand sides are then reads and short sums, no evaluation-shaped pass per QP iteration.
	double *qp_c = qp_lamq + ncq, *qp_jwg = qp_c + ncq, *qp_a = qp_jwg + ncq, *qp_JU = qp_a + (size_t)ncq * FamN::CG;
	// one pass over the breakpoints: lane = breakpoint.  what = 0: c, derivative rows (at x = sx) and J W g (W g = sd); what = 1: J U of
	// the columns just formed (U = sxt; slot index flag[0] of the row's group)
	auto qp_rows_pass = [&](int what) __attribute__((always_inline)) {
		constexpr int DM = FamN::DM, NZ = NOUT > 0 ? DM * NOUT : NTG_MAX_NZ, NTc = FamN::NNLTC > 0 ? FamN::NNLTC : 1;
		for (int i = tid; i < P; i += NT) {
			double zv[NZ];
			compute_z<NOUT, K, DM>(D, S, what == 0 ? sd : sxt, i, D.tcon_mask, zv);
			if (what == 0) {
				double z[NZ], c[NTc], tape[FamN::TAPE];
				compute_z<NOUT, K, DM>(D, S, sxt, i, D.tcon_mask, z);   // (the trial-point buffer holds x here -- in LDS also for the BIG layouts, whose x lives in HBM)
				FamCall<FamN>{ntg_prm_row<FAM>(), D.nnltc}.template nltc_val<NZ>(NOUT > 0 ? NOUT : D.nout, i, z, c, tape);
#pragma unroll
				for (int j = 0; j < NTc; j++) {
					if (j >= D.nnltc) continue;
					double df[NZ], t[NTc];
#pragma unroll
					for (int v = 0; v < NZ; v++) df[v] = 0.0;
#pragma unroll
					for (int jj = 0; jj < NTc; jj++) t[jj] = jj == j ? 1.0 : 0.0;
					FamCall<FamN>{ntg_prm_row<FAM>(), D.nnltc}.template nltc_vjp<NZ>(NOUT > 0 ? NOUT : D.nout, D.nz, i, z, t, df, tape);
					const int g = FamN::row_group(j), row = j * P + i;
					double jw = 0.0;
					for (int u = 0; u < FamN::CG; u++) {
						const int fl = qp_flag(g, u);
						double av = 0.0, zz = 0.0;
#pragma unroll
						for (int v = 0; v < NZ; v++) if (v == fl) { av = df[v]; zz = zv[v]; }
						qp_a[(size_t)row * FamN::CG + u] = av;
						jw += av * zz;
					}
					qp_c[row] = c[j]; qp_jwg[row] = jw;
				}
			} else {
#pragma unroll
				for (int j = 0; j < NTc; j++) {
					if (j >= D.nnltc) continue;
					const int g = FamN::row_group(j), row = j * P + i;
					QpSlots q(qpbase + g * QPD, QA);
					const int acol = q.flag[0];
					if (acol < 0) continue;
					double ju = 0.0;
					for (int u = 0; u < FamN::CG; u++) {
						const int fl = qp_flag(g, u);
						double zz = 0.0;
#pragma unroll
						for (int v = 0; v < NZ; v++) if (v == fl) zz = zv[v];
						ju += qp_a[(size_t)row * FamN::CG + u] * zz;
					}
					qp_JU[(size_t)acol * ncq + row] = ju;
				}
			}
		}
	};
	// derivative rows (for the scatter of J'), J W g and r = bound - c of the slots of every group (one lane per slot): reads of the caches
	auto qp_slot_rows = [&](bool only_new) __attribute__((always_inline)) {
		const int ngp = D.nwt_ngrp, b0 = D.nlic + D.nltc + D.nlfc + D.nnlic;
		for (int e = tid; e < ngp * QA; e += NT) {
			const int g = e / QA, a = e - g * QA;
			QpSlots q(qpbase + g * QPD, QA);
			if (a >= *q.ns || (only_new && a != q.flag[0])) continue;
			const int row = q.row[a], j = row / P;
			for (int u = 0; u < FamN::CG; u++) q.ar[a * NTG_QP_MAXCG + u] = qp_a[(size_t)row * FamN::CG + u];
			q.jwg[a] = qp_jwg[row];
			q.rr[a] = (q.sgn[a] < 0 ? al.lo[b0 + j] : al.up[b0 + j]) - qp_c[row];
		}
	};
	// the columns U = W J' of the slots named by flag[0] of every group (-1: none), their J U over all rows and their entries of S
	auto qp_column = [&]() __attribute__((always_inline)) {
		const int ngp = D.nwt_ngrp, ng = D.nwt_ng, go = D.nwt_go, kk = K > 0 ? K : D.order[0];
		__syncthreads();
		if (D.nwt_tab && !nwt_curv && !T.pp_k0) {   // (the current factor is the cost model's: K0 -- of the plan's grid, whose tables these are)
			// The model is the cost model K0 (no constraint curvature any more in this solve): W M_i' per breakpoint and M_k W M_i' per pair
			// of breakpoints are the plan's tables (NtgTables::nwt_tu, nwt_g) -- the column and its J U are short combinations of table
			// rows, no band solve, no breakpoint pass.
			// (the column itself is not stored: the step's p = -W g - sum_a lam_a U_a combines the table rows of the slots with a multiplier, once)
			constexpr int CGc = FamN::CG, NTc2 = FamN::NNLTC > 0 ? FamN::NNLTC : 1;
			if (tid < ngp) { QpSlots q(qpbase + tid * QPD, QA); const int a = q.flag[0]; if (a >= 0) q.tab[a] = 1; }
			for (int i2 = tid; i2 < P; i2 += NT) {
#pragma unroll
				for (int j = 0; j < NTc2; j++) {
					if (j >= D.nnltc) continue;
					const int g = FamN::row_group(j), row = j * P + i2;
					QpSlots q(qpbase + g * QPD, QA);
					const int a = q.flag[0];
					if (a < 0) continue;
					const int i = q.row[a] % P;
					const double *gp2 = T.nwt_g + ((size_t)i2 * P + i) * CGc * CGc;
					double ju = 0.0;
#pragma unroll
					for (int v = 0; v < CGc; v++) {
						double sv = 0.0;
#pragma unroll
						for (int u = 0; u < CGc; u++) sv += gp2[v * CGc + u] * q.ar[a * NTG_QP_MAXCG + u];
						ju += qp_a[(size_t)row * CGc + v] * sv;
					}
					qp_JU[(size_t)a * ncq + row] = ju;
				}
			}
			__syncthreads();
			for (int e = tid; e < ngp * QA; e += NT) {
				const int g = e / QA, a2 = e - g * QA;
				QpSlots q(qpbase + g * QPD, QA);
				const int bcol = q.flag[0];
				if (bcol < 0 || a2 >= *q.ns) continue;
				q.S[a2 <= bcol ? NTG_QP_TR(bcol, a2) : NTG_QP_TR(a2, bcol)] = qp_JU[(size_t)bcol * ncq + q.row[a2]];
			}
			qp_ntab++;
			__syncthreads();
			return;
		}
		for (int c = tid; c < n; c += NT) sgpt[c] = 0.0;
		__syncthreads();
		for (int e = tid; e < ngp * go * kk; e += NT) {
			const int g = e / (go * kk), r = e - g * go * kk, ov = r / kk, qq = r - ov * kk;
			QpSlots q(qpbase + g * QPD, QA);
			const int a = q.flag[0];
			if (a < 0) continue;
			const int i = q.row[a] % P;
			double val = 0.0;
			for (int u = 0; u < FamN::CG; u++)
				if ((int)((D.nwt_upack >> (8 * u + 4)) & 15u) == ov) val += q.ar[a * NTG_QP_MAXCG + u] * S.rowv[S.chrow[(int)((D.nwt_upack >> (8 * u)) & 15u)] + qq * P + i];
			sgpt[D.iC[g * go + ov] + S.off[i] + qq] = val;
		}
		__syncthreads();
		nwt_apply(sgpt, sxt, false);
		__syncthreads();
		for (int c = tid; c < n; c += NT) {
			const int pos = T.nwt_pos[c];
			if (pos >= 0 && pos < ngp * ng) {
				QpSlots q(qpbase + (pos / ng) * QPD, QA);
				const int a = q.flag[0];
				if (a >= 0) qp_U[(size_t)a * npad + c] = sxt[c];
			}
		}
		if (tid < ngp) { QpSlots q(qpbase + tid * QPD, QA); const int a = q.flag[0]; if (a >= 0) q.tab[a] = 0; }
		qp_rows_pass(1);
		__syncthreads();
		for (int e = tid; e < ngp * QA; e += NT) {
			const int g = e / QA, a2 = e - g * QA;
			QpSlots q(qpbase + g * QPD, QA);
			const int bcol = q.flag[0];
			if (bcol < 0 || a2 >= *q.ns) continue;   // (the whole row and column of the slot: a reused slot sits in the middle)
			q.S[a2 <= bcol ? NTG_QP_TR(bcol, a2) : NTG_QP_TR(a2, bcol)] = qp_JU[(size_t)bcol * ncq + q.row[a2]];
		}
		qp_ncol++;
		__syncthreads();
	};
	// one major iteration's QP at x (sx = sxt), g (sg), multipliers al_lam, previous QP multipliers qp_lamq: leaves p in sgp, the QP's
	// multipliers in qp_lamq, |p|, |x|, g.p and the largest multiplier in the qp_* scalars
	double qp_gp = 0.0;
	auto qp_major = [&]() __attribute__((always_inline)) {
		const int ngp = D.nwt_ngrp, ng = D.nwt_ng, wave = tid >> 6, lane = tid & 63, b0 = D.nlic + D.nltc + D.nlfc + D.nnlic;
		constexpr int NTc = FamN::NNLTC > 0 ? FamN::NNLTC : 1;
		double qp_bl[NTc], qp_bu[NTc];   // the rows' bounds (one pair per row function), read once per major
#pragma unroll
		for (int j = 0; j < NTc; j++) { qp_bl[j] = j < D.nnltc ? al.lo[b0 + j] : 0.0; qp_bu[j] = j < D.nnltc ? al.up[b0 + j] : 0.0; }
		__syncthreads();   // the multipliers crossed lanes through HBM
		// After the model with the constraint curvature was not positive definite at two major iterations in a row the curvature is not tried
		// again in this solve: the model is then the cost model, the same matrix at every later major -- its factor is kept (no block pass, no
		// assembly, no factorisation; oracle/sqp.c sqpqp_run has the same rule and the measurements behind it)
		if (qp_nocurv < 2) { nwt_refresh_ex(sxt, true, al_lam, 0.0, true); qp_nocurv = nwt_curv ? 0 : qp_nocurv + 1; }
		nwt_apply(sg, sd, false);   // W g
		NTG_STAMP(4);
		__syncthreads();
		qp_rows_pass(0);
		// slots of the previous major's working set, in row order (a wave per group: ballot + prefix count)
		if (wave < ngp) {
			QpSlots q(qpbase + wave * QPD, QA);
			int cnt = 0;
			for (int j = 0; j < D.nnltc; j++) {
				if (FamN::row_group(j) != wave) continue;
				for (int i0 = 0; i0 < P; i0 += 64) {
					const int i = i0 + lane;
					const double lq = i < P ? qp_lamq[D.nnlic + j * P + i] : 0.0;
					const bool nz = lq != 0.0;
					const unsigned long long mk = __ballot(nz);
					const int slot = cnt + __popcll(mk & ((1ull << lane) - 1ull));
					if (nz && slot < QA) { q.row[slot] = j * P + i; q.sgn[slot] = lq > 0.0 ? 1 : -1; q.inP[slot] = 1; q.nu[slot] = q.nu0[slot] = fabs(lq); }
					cnt += __popcll(mk);
				}
			}
			if (lane == 0) { *q.ns = cnt < QA ? cnt : QA; q.flag[0] = -1; q.flag[1] = 0; q.flag[2] = cnt > QA ? 1 : 0; }
		}
		__syncthreads();
		qp_slot_rows(false);
		__syncthreads();
		NTG_STAMP(5);   // (variant builds: row caches + slots of the carried-over working set)
		int nswarm = 0;   // the first iterations form the columns of the slots carried over (one band solve per slot index, all groups at once)
		for (int g = 0; g < ngp; g++) { QpSlots q(qpbase + g * QPD, QA); nswarm = max(nswarm, *q.ns); }
		for (int it = 0; it < 5 * QA + 8; it++) {
			__syncthreads();
			bool docol = false;
			if (it < nswarm) {
				if (tid < ngp) { QpSlots q(qpbase + tid * QPD, QA); q.flag[0] = it < *q.ns ? it : -1; }
				docol = true;
			} else {
			if (wave < ngp) { QpSlots q(qpbase + wave * QPD, QA); qp_nsolve += qp_passive_solve_wave(q, lane, QA); }
			__syncthreads();
			// most violated linearised bound of every trajectory row function among the rows outside the passive set:
			// c + J p = c - J W g - sum_a lam_a (J U_a)
			double bw[NTc]; int bk[NTc];
#pragma unroll
			for (int j = 0; j < NTc; j++) { bw[j] = 0.0; bk[j] = 0x7fffffff; }
			for (int i = tid; i < P; i += NT) {
#pragma unroll
				for (int j = 0; j < NTc; j++) {
					if (j >= D.nnltc) continue;
					const int row = j * P + i;
					QpSlots q(qpbase + FamN::row_group(j) * QPD, QA);
					const int ns = *q.ns;
					double lin = qp_c[row] - qp_jwg[row];
					int pas = 0;   // bit 0 / 1: the row's upper / lower side is passive
					for (int a = 0; a < ns; a++) {
						const double nua = q.nu[a];
						if (nua != 0.0) lin -= (q.sgn[a] < 0 ? -nua : nua) * qp_JU[(size_t)a * ncq + row];
						if (q.inP[a] && q.row[a] == row) pas |= q.sgn[a] < 0 ? 2 : 1;
					}
					const double bl = qp_bl[j], bu = qp_bu[j];
					const double wu = (bu < 1e19 && !(pas & 1)) ? lin - bu : -1.0, wl = (bl > -1e19 && !(pas & 2)) ? bl - lin : -1.0;
					const bool up = wu >= wl;
					const double w = up ? wu : wl, bound = up ? bu : bl;
					if (!(w > 1e-9 * (1.0 + fabs(bound)))) continue;
					const int key = 2 * row + (up ? 0 : 1);
					if (w > bw[j] || (w == bw[j] && key < bk[j])) { bw[j] = w; bk[j] = key; }
				}
			}
#pragma unroll
			for (int j = 0; j < NTc; j++) {
#pragma unroll
				for (int sh = 1; sh < 64; sh <<= 1) {
					const double ow = __shfl_xor(bw[j], sh); const int ok = __shfl_xor(bk[j], sh);
					if (ow > bw[j] || (ow == bw[j] && ok < bk[j])) { bw[j] = ow; bk[j] = ok; }
				}
				if (lane == 0) { qpred[(wave * NTc + j) * 2] = bw[j]; qpred[(wave * NTc + j) * 2 + 1] = (double)bk[j]; }
			}
			__syncthreads();
			if (wave < ngp && lane == 0) {
				QpSlots q(qpbase + wave * QPD, QA);
				double w = 0.0; int key = 0x7fffffff;
				for (int wv = 0; wv < NT / 64; wv++)
					for (int j = 0; j < D.nnltc; j++) {
						if (FamN::row_group(j) != wave) continue;
						const double ow = qpred[(wv * NTc + j) * 2]; const int ok = (int)qpred[(wv * NTc + j) * 2 + 1];
						if (ow > w || (ow == w && ok < key)) { w = ow; key = ok; }
					}
				q.flag[0] = -1; q.flag[1] = 0;
				if (w > 0.0) {
					const int row = key >> 1, sg = (key & 1) ? -1 : 1, ns = *q.ns;
					int a = -1;
					for (int a2 = 0; a2 < ns; a2++) if (q.row[a2] == row && q.sgn[a2] == sg) a = a2;
					if (a >= 0) { q.inP[a] = 1; q.flag[1] = 1; }   // a slot that left comes back: its column and entries of S are there
					else if (ns < QA) { q.row[ns] = row; q.sgn[ns] = sg; q.inP[ns] = 1; q.nu[ns] = 0.0; q.nu0[ns] = 0.0; q.flag[0] = ns; q.flag[1] = 1; *q.ns = ns + 1; }
					else {
						// every slot taken: a slot whose row left the passive set is given to the new row (its column, its J U and its row AND
						// column of S are formed anew by qp_column); none: the working set of this major is full
						int fr = -1;
						for (int a2 = 0; a2 < ns; a2++) if (!q.inP[a2] && fr < 0) fr = a2;
						if (fr >= 0) { q.row[fr] = row; q.sgn[fr] = sg; q.inP[fr] = 1; q.nu[fr] = 0.0; q.nu0[fr] = 0.0; q.flag[0] = fr; q.flag[1] = 1; }
						else q.flag[2] = 1;
					}
				}
			}
			__syncthreads();
			bool anycol = false, any = false;
			for (int g = 0; g < ngp; g++) { QpSlots q(qpbase + g * QPD, QA); anycol = anycol || q.flag[0] >= 0; any = any || q.flag[1] != 0; }
			if (!any) break;
			if (anycol) { qp_slot_rows(true); docol = true; }
			}
			NTG_STAMP(2);
			if (docol) { qp_column(); NTG_STAMP(0); }   // (the one call site: the band solve inside is inlined)
		}
		__syncthreads();
		// the QP's multipliers (signed: > 0 at an upper bound), the step p = -W g - sum_a lam_a U_a, the scalars of the exit test and of the
		// merit function
		NTG_STAMP(2);
		for (int j = tid; j < D.ncnln; j += NT) qp_lamq[j] = 0.0;
		__syncthreads();
		double lm = 0.0;
		for (int g = 0; g < ngp; g++) {
			QpSlots q(qpbase + g * QPD, QA);
			const int ns = *q.ns;
			for (int a = 0; a < ns; a++) { const double nua = q.nu[a]; lm = fmax(lm, fabs(nua)); if (tid == 0 && nua != 0.0) qp_lamq[D.nnlic + q.row[a]] = q.sgn[a] < 0 ? -nua : nua; }
			if (q.flag[2]) { qp_over++; qp_full = true; }
		}
		qp_lmax = lm;
		// ... and |Z'(g + J'lam)|, the reduced gradient of the Lagrangian with the QP's multipliers (the free coefficients span null(A_E)):
		// the optimality measure of the exit test, the same one the other modes use
		double r3[4] = {0.0, 0.0, 0.0, 0.0};
		const int go2 = D.nwt_go, kk2 = K > 0 ? K : D.order[0];
		for (int c = tid; c < n; c += NT) {
			const int pos = T.nwt_pos[c];
			double pc = -sd[c], gl = sg[c];
			if (pos >= 0 && pos < ngp * ng) {
				const int g = pos / ng, pp = pos - g * ng, ov = pp % go2, cl = D.nwt_clo + pp / go2;
				QpSlots q(qpbase + g * QPD, QA);
				const int ns = *q.ns;
				for (int a = 0; a < ns; a++) {
					const double nua = q.nu[a];
					if (nua == 0.0) continue;
					const double la = q.sgn[a] < 0 ? -nua : nua;
					const int i = q.row[a] % P, qq = cl - S.off[i];
					if (q.tab[a]) {   // the slot's column from the plan's table: U = sum_u a_u K0^-1 M_i' e_u
						double uv = 0.0;
						for (int u = 0; u < FamN::CG; u++) uv += q.ar[a * NTG_QP_MAXCG + u] * T.nwt_tu[((size_t)i * FamN::CG + u) * ng + pp];
						pc -= la * uv;
					} else pc -= la * qp_U[(size_t)a * npad + c];
					if (qq >= 0 && qq < kk2)
						for (int u = 0; u < FamN::CG; u++)
							if ((int)((D.nwt_upack >> (8 * u + 4)) & 15u) == ov) gl += la * q.ar[a * NTG_QP_MAXCG + u] * S.rowv[S.chrow[(int)((D.nwt_upack >> (8 * u)) & 15u)] + qq * P + i];
				}
			}
			const double xc = sx[c];
			sgp[c] = pc; r3[0] += pc * pc; r3[1] += xc * xc; r3[2] += sg[c] * pc;
			if (pos >= 0) r3[3] += gl * gl;
		}
		block_sum<NT, 4>(r3, S);
		qp_pn = sqrt(r3[0]); qp_xn = sqrt(r3[1]); qp_gp = r3[2]; qp_gl = sqrt(r3[3]);
		nwt_restore();
		NTG_STAMP(3);   // (variant builds: the step and its scalars -- shares the slot with the model assembly, which the QP step seldom runs)
		__syncthreads();
	};
	// (per-problem grids: this problem's values of the rows, NtgTables::pp_ilin)
	const LinIneq lin{nI, T.irow, T.icsr_ptr, T.icsr_col, T.icsc_ptr, T.icsc_row, T.icsr_val + (size_t)b * T.pp_ilin, T.icsc_val + (size_t)b * T.pp_ilin,
	                  (double *)(smem_raw + L.tI)};
	int inform = 4, iter = 0, nfev = 0, npairs = 0, state = ST_INIT;
	// ---- scope check (uniform): linear rows are equalities unless the plan declared them inequalities ----
	{
		double bad[1] = {0.0};
		for (int s = tid; s < D.nlic + D.nltc + D.nlfc; s += NT) {
			const double l = lower[(size_t)b * D.nbounds + s], u = upper[(size_t)b * D.nbounds + s];
			const bool ineq = D.nI > 0 && T.linflag[s] != 0;
			if (ineq ? !(l <= u) : l != u) bad[0] += 1.0;
		}
		block_sum<NT, 1>(bad, S);
		if (bad[0] != 0.0 || (ncn > 0 && !HASCON) || (D.nI > 0 && !LIN) || (nal > 0 && sp.fixed_iters)) inform = 9;
	}
	double F = 0.0, Fp = 0.0, gn2 = 0.0, rv2 = 0.0, alpha = 0.0, pnorm = 0.0;
	double sri = sp.sr, rvprev = HUGE_VAL;   // inner tolerance and best violation so far (AL outer loop)
	int outer = 0, inner_inform = 4;
	bool at_x = true, weak = false;
	double mfres = 0.0;   // diagnostic: linear residual seen by the last feasibility step
	bool final_pass = false;   // the multiplier pass ran: S.lam belongs to the gradient with the estimates al_t, report those
	if (inform != 9) {
		// ---- linear feasibility: x += A'(AA')^-1 (b - A x) ----
		auto make_feasible = [&]() {
			if (m <= 0) return;
			if (BIG) __syncthreads();   // x lives in HBM/L2 and the rows of A read it across lanes
			else lds_sync();
			for (int r = tid; r < m; r += NT) {
				const int s = lin_slot(D, D.nI > 0 ? T.erow[r] : r);
				double a = 0.0;
				for (int e = S.csr_ptr[r]; e < S.csr_ptr[r + 1]; e++) a += S.csr_val[e] * sx[S.csr_col[e]];
				tmp[r] = lower[(size_t)b * D.nbounds + s] - a;
			}
			lds_sync();
			if (sp.stamps == 2) { mfres = 0.0; for (int r = 0; r < m; r++) mfres = fmax(mfres, fabs(tmp[r])); }
			for (int r = tid; r < m; r += NT) {
				double a = 0.0;
				for (int e = S.sinv_ptr[r]; e < S.sinv_ptr[r + 1]; e++) a += S.sinv_val[e] * tmp[S.sinv_col[e]];
				tmp[m + r] = a;   // not S.lam: that holds the multiplier estimate reported in clambda
			}
			lds_sync();
			for (int c = tid; c < n; c += NT) {
				double s = 0.0;
				for (int e = S.csc_ptr[c]; e < S.csc_ptr[c + 1]; e++) s += S.csc_val[e] * tmp[m + S.csc_row[e]];
				sx[c] += s;
			}
			lds_sync();
		};
		make_feasible();
		for_vec<NT>(n, [&](int c) { sxt[c] = sx[c]; });
		if (alprob) {
			// cold: multipliers 0.  Warm (ntg_solve_opts.warm_start): the estimates the previous solve of this batch left in the workspace
			// (shifted with the horizon by ntg_batch_mpc_shift_multipliers) are the starting multipliers
			for (int j = tid; j < nal; j += NT) {
				if (sp.warm) al_lam[j] = al_t[j];
				else { al_lam[j] = 0.0; if (NWT) al_t[j] = 0.0; }
			}
			sri = fmax(sp.sr, 1e-3);
			__syncthreads();   // multipliers cross lanes through HBM: full barrier
			if (QPM && sp.warm) {
				// warm start of the QP-based SQP step (receding horizon): no pass on the objective alone -- the QP's first working set is the rows
				// the shifted multipliers of the previous solve name (ntg.h:64-68: what istate / clambda were meant to carry)
				for (int j = tid; j < ncn; j += NT) qp_lamq[j] = al_lam[j];
				al.mu = qp_rho = 1.0; al.qp = 1; state = ST_QP; qp_first = true;
				__syncthreads();
			}
		}
		NTG_STAMP(0);

		// line-search state lives in LDS (17 doubles would otherwise sit in every lane's registers);
		// each step works on a register copy and lane 0 publishes it back between two barriers
		// two copies of the line-search state: every lane advances its own register copy, lane 0 stores the result into the
		// OTHER copy, which is first read after the barriers of the next evaluation -- no barrier for the hand-over
		LineSearch *lsb = (LineSearch *)(smem_raw + L.ls);
		int lsi = 0;
		double ls_a = 0.0;   // current trial step (every lane)
		double r4[4] = {0, 0, 0, 0};   // gp.d, d.d, x.x, gp.gp of the current iterate
		bool finished = false;
		for (;;) {
			// ================= the one evaluation site =================
			// The evaluation leaves its four sums (quadrature, |g|^2, penalty, violation) as per-lane partials; the
			// projection pass adds the slope of the line search, and ONE workgroup reduction serves all five.
			double part[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, gdummy;
			(void)eval_cost<FAM, NOUT, K, NT, EPT, (NT >= 256), CHM>(D, S, sxt, sg, &gdummy, cm, al, nullptr, nullptr, NTG_CLOCK_TK(sp.stamps && !NWT),
			                                                        LIN ? &lin : nullptr, CHM != 0, part);
			NTG_STAMP(1);
			if (state != ST_FINAL && state != ST_REEVAL && !(QPM && state == ST_QP)) {
				project<NT, BIG>(D, S, sg, sgpt, tmp, sd, &part[4]);
				NTG_STAMP(2);
				block_sum<NT, 5>(part, S);
			} else {
				double p4[4] = {part[0], part[1], part[2], part[3]};
				block_sum<NT, 4>(p4, S);
				part[0] = p4[0]; part[1] = p4[1]; part[2] = p4[2]; part[3] = p4[3];
			}
			const double Fpn = (D.nicf ? S.dfi[D.nz] : 0.0) + part[0] + (D.nfcf ? S.dff[D.nz] : 0.0);   // ntg.c:328
			const double Fn = Fpn + part[2], gn2n = part[1], rv2n = part[3];
			if (state == ST_FINAL) {
				if (QPM && qp_last) { Fp = Fpn; F = Fn; rv2 = rv2n; nfev++; }
				// multipliers estimate lam = (AA')^-1 A g at the final point
				if (BIG) __syncthreads(); else lds_sync();
				for (int r = tid; r < m; r += NT) {
					double a = 0.0;
					for (int e = S.csr_ptr[r]; e < S.csr_ptr[r + 1]; e++) a += S.csr_val[e] * sg[S.csr_col[e]];
					tmp[r] = a;
				}
				lds_sync();
				for (int r = tid; r < m; r += NT) {
					double a = 0.0;
					for (int e = S.sinv_ptr[r]; e < S.sinv_ptr[r + 1]; e++) a += S.sinv_val[e] * tmp[S.sinv_col[e]];
					S.lam[r] = a;
				}
				lds_sync();
				final_pass = true;
				break;
			}
			nfev++;
			if (QPM && state == ST_QP) {
				// ---- QP-based SQP step: Fn is the l1 merit function F + rho sum_j viol_j at the trial point (at x itself the first time) ----
				bool qp_exit = false, qp_to_al = false;
				if (!qp_first) {
					if (!(Fn <= qp_phi0 + 1e-4 * qp_alpha * fmin(qp_D, 0.0) + 1e-14 * fabs(qp_phi0))) {
						if (++qp_k >= 25) qp_to_al = true;   // no acceptable step along the QP's direction (x and the multipliers are those of the last accepted point)
						else {
							qp_alpha *= 0.5;
							const double a = qp_alpha;
							for_vec<NT>(n, [&](int c) { sxt[c] = sx[c] + a * sgp[c]; });
							continue;
						}
					} else {
						const double a = qp_alpha;
						for_vec<NT>(n, [&](int c) { sx[c] = sxt[c]; });
						for (int j = tid; j < ncn; j += NT) al_lam[j] += a * (qp_lamq[j] - al_lam[j]);
						iter++;
					}
				}
				if (!qp_exit && !qp_to_al) {
					qp_first = false;
					F = Fn; Fp = Fpn; gn2 = gn2n; rv2 = rv2n; at_x = true;
					qp_viol1 = part[2] / qp_rho;
					if (iter >= sp.itlim) { inform = 4; qp_exit = true; }
				}
				if (!qp_exit && !qp_to_al) {
					qp_major();
					if (qp_full) qp_to_al = true;
				}
				if (qp_to_al) {
					// The working set of a group is full (NTG_QP_MAXA slots; rows active along a whole arc of the trajectory: the QP was not
					// solved, and its step would not restore feasibility), or the l1 merit function found no acceptable step along the QP's
					// direction.  This problem continues with the augmented-Lagrangian passes of the structured Newton mode from the current
					// point and the current multipliers (the warm-start path of hessian = 2): the mode is never less robust than that one.
					{
						al.qp = 0; al.mu = 10.0; qp_fell++;
						sri = fmax(sp.sr, 1e-3); rvprev = HUGE_VAL; outer = 0;
						npairs = 0; finished = false; inner_inform = 4; state = ST_INIT; weak = false; at_x = true;
						__syncthreads();
						for_vec<NT>(n, [&](int c) { sxt[c] = sx[c]; });
						continue;
					}
				}
				if (!qp_exit) {
					// exit: the step is small, the rows are feasible, and the reduced gradient of the Lagrangian meets NPSOL's optimality tolerance
					if (qp_pn <= 1e-2 * sp.sr * (1.0 + qp_xn) && sqrt(rv2) <= 1e-8 && qp_gl <= 0.1 * sp.sr * (1.0 + fmax(1.0 + fabs(Fp), sqrt(gn2)))) {
						// the last step is taken (it is below the exit tolerance, but K is large: the point it leads to is stationary to rounding --
						// a solve that ends right after phase 0 would otherwise keep that pass's looser tolerance); the final pass below
						// evaluates there: objective, multipliers of the linear rows
						for (int j = tid; j < ncn; j += NT) al_lam[j] = qp_lamq[j];
						for_vec<NT>(n, [&](int c) { sx[c] += sgp[c]; });
						inform = 0; qp_exit = true; qp_last = true;
					} else {
						if (qp_rho < 1.5 * qp_lmax + 1e-3) qp_rho = 2.0 * qp_lmax + 1e-3;
						al.mu = qp_rho;
						qp_D = qp_gp - qp_rho * qp_viol1; qp_phi0 = Fp + qp_rho * qp_viol1; qp_alpha = 1.0; qp_k = 0;
						for_vec<NT>(n, [&](int c) { sxt[c] = sx[c] + sgp[c]; });
						continue;
					}
				}
				// exit: one more pass for the linear rows' multipliers, with the gradient of the Lagrangian (ALState::qp = 2)
				__syncthreads();
				if (m > 0) {   // (always: the pass also leaves the multipliers in the workspace, where a warm start of the next solve finds them)
					state = ST_FINAL; al.qp = 2;
					make_feasible();   // before the pass that evaluates the multipliers: the x that is reported is the x they belong to
					lds_sync();
					for_vec<NT>(n, [&](int c) { sxt[c] = sx[c]; });
					continue;
				}
				break;
			}
			bool new_major = false;
			if (state == ST_REEVAL) {   // constraint values and multiplier estimates refreshed at x
				F = Fn; Fp = Fpn; gn2 = gn2n; rv2 = rv2n; at_x = true;
			} else {
			if (state == ST_INIT) {
				F = Fn; Fp = Fpn; gn2 = gn2n; rv2 = rv2n; at_x = true;
				for_vec<NT>(n, [&](int c) { sgp[c] = sgpt[c]; });
				if (NWT) { nwt_refresh(sxt, true); nwt_apply(sgp, sd); }
				else apply_w0<NT, BIG, HESS>(D, Tw, sp.hessian, sgp, sd, sxt, S.oinfo);
				r4[0] = r4[1] = r4[2] = r4[3] = 0.0;
				for_vec<NT>(n, [&](int c) { r4[0] += sgp[c] * sd[c]; r4[1] += sd[c] * sd[c]; r4[2] += sx[c] * sx[c]; r4[3] += sgp[c] * sgp[c]; });
				block_sum<NT, 4>(r4, S);
				NTG_STAMP(4);
				new_major = true;
			} else {
				int rc = 1;
				if (state == ST_LS) {
					const double dd[1] = {part[4]};   // gp+ . (-d), reduced together with the evaluation's sums
					LineSearch lsr = lsb[lsi];
					rc = lsr.step(Fn, dd[0]);
					ls_a = lsr.a;
					if (tid == 0) lsb[lsi ^ 1] = lsr;
					lsi ^= 1;
				}
				if (rc == 0 || rc == 2) {
					if (rc == 2) state = ST_FORCE;
					const double a = ls_a;
					for_vec<NT>(n, [&](int c) { sxt[c] = sx[c] + a * (-sd[c]); });
					NTG_STAMP(5);
					continue;
				}
				if (rc != 1) {
					const double tolg = sri * (1.0 + fmax(1.0 + fabs(F), sqrt(gn2)));
					if ((npairs > 0 || (NWT && nwt_curv)) && sqrt(r4[3]) > tolg) {
						// line search failed with a non-trivial W: drop the pairs and retry from the same point with W0
						// (structured Newton mode: with the Gauss-Newton factor at x; sxt is rebuilt from x first)
						npairs = 0;
						if (NWT) { lds_sync(); for_vec<NT>(n, [&](int c) { sxt[c] = sx[c]; }); nwt_refresh(sxt, false); nwt_apply(sgp, sd); }
						else apply_w0<NT, BIG, HESS>(D, Tw, sp.hessian, sgp, sd, sxt, S.oinfo);
						double r2[2] = {0, 0};
						for_vec<NT>(n, [&](int c) { r2[0] += sgp[c] * sd[c]; r2[1] += sd[c] * sd[c]; });
						block_sum<NT, 2>(r2, S);
						r4[0] = r2[0]; r4[1] = r2[1];
						new_major = true;
					} else {
						// no further decrease obtainable: converged within tolerance, or "optimal but not to the
						// requested accuracy" (NPSOL inform 1) within 10^3 of it, else failure (6)
						const double gpn0 = sqrt(r4[3]);
						if (gpn0 <= tolg) inner_inform = 0;
						else if (gpn0 <= 1e3 * tolg) { inner_inform = 0; weak = true; }
						else inner_inform = 6;
						finished = true; at_x = false;
					}
				} else {
					alpha = ls_a;
					// accept: commit x (frees sxt, which then holds t), t = W gp+, u = t - d, pair (s, u) to HBM
					for_vec<NT>(n, [&](int c) { sg[c] = alpha * (-sd[c]); sx[c] = sxt[c]; });   // sg = the step s
					if (!NWT && npairs == sp.memcap) { npairs = 0; apply_w0<NT, BIG, HESS>(D, Tw, sp.hessian, sgp, sd, sxt, S.oinfo); } // memory full: restart
					NTG_STAMP(5);
					bool conv_now = false;
					if (NWT && !sp.fixed_iters) {
						// The exit test of this major needs |x| and |gp+| only.  Taken BEFORE the model is rebuilt: a pass that ends here
						// (every pass ends on an accepted step) would otherwise assemble and factor a matrix nobody uses -- one of the
						// 2.7 (config D) refreshes per pass.
						double r2[2] = {0, 0};
						for_vec<NT>(n, [&](int c) { const double xn = sx[c], gq = sgpt[c]; r2[0] += xn * xn; r2[1] += gq * gq; });
						block_sum<NT, 2>(r2, S);
						conv_now = alpha * pnorm <= sri * (1.0 + sqrt(r2[0])) && sqrt(r2[1]) <= sri * (1.0 + fmax(1.0 + fabs(Fn), sqrt(gn2n)));
						if (conv_now) {
							for_vec<NT>(n, [&](int c) { sgp[c] = sgpt[c]; });
							r4[2] = r2[0]; r4[3] = r2[1];
							F = Fn; Fp = Fpn; gn2 = gn2n; rv2 = rv2n;
							iter++;
							inner_inform = 0; finished = true;
							lds_sync();
						}
					}
					if (!conv_now) {
					if (NWT) { nwt_refresh(sxt, true); nwt_apply(sgpt, st); }   // sxt still holds the accepted point; st (= sxt) is written last
					else apply_w0<NT, BIG, HESS, true>(D, Tw, sp.hessian, sgpt, st, sxt, S.oinfo);
					NTG_STAMP(4);
					// register-resident pairs: 3 coefficients per lane, 6 pairs per round; the 5-coefficient instances (config E)
					// take 3 pairs per round
					if (DF_OK && dform) {
						if (npairs == 0) for_vec<NT>(n, [&](int c) { hist[c] = sd[c]; });   // a chain starts: d_0 (read back by the owner lanes only)
						apply_dform<NT, 3, NTG_DF_G>(D, S, hist, npairs + 1, sgpt, st, hrc);
					} else
					apply_history<NT, (EPT > 4 ? 5 : 3), (EPT > 4 ? 3 : NTG_HIST_G)>(D, S, hist, npairs, sgpt, st, hrc);
					NTG_STAMP(3);
					double r6[6] = {0, 0, 0, 0, 0, 0};
					for_vec<NT>(n, [&](int c) {
						const double s = sg[c], y = sgpt[c] - sgp[c], u = st[c] - sd[c], gpn = sgpt[c];
						r6[0] += s * y; r6[1] += y * u; r6[2] += s * gpn; r6[3] += u * gpn; r6[4] += s * s; r6[5] += y * y;
					});
					block_sum<NT, 6>(r6, S);
					const bool upd = !NWT && r6[0] > 1e-12 * sqrt(r6[4]) * sqrt(r6[5]);
					const double rho = upd ? 1.0 / r6[0] : 0.0, c2 = upd ? rho * (1.0 + rho * r6[1]) : 0.0;
					r4[0] = r4[1] = r4[2] = r4[3] = 0.0;
					const bool df = DF_OK && dform;
					for_vec<NT>(n, [&](int c) {
						const double s = sg[c], u = st[c] - sd[c];
						if (upd && !df) { hist[(size_t)npairs * (2 * n + 2) + c] = s; hist[(size_t)npairs * (2 * n + 2) + n + c] = u; }
						const double dn = upd ? st[c] - rho * (s * r6[3] + u * r6[2]) + c2 * s * r6[2] : st[c];
						if (df) hist[(size_t)(npairs + 1) * n + c] = dn;   // the chain's next vector
						const double xn = sx[c], gq = sgpt[c];
						sgp[c] = gq;
						sd[c] = dn;
						r4[0] += gq * dn; r4[1] += dn * dn; r4[2] += xn * xn; r4[3] += gq * gq;
					});
					if (df) {
						// link scalars of this major (see apply_dform); omega = -(s.g)/(s.y) > 0 whenever the update is taken
						double le = 0.0, lf = 0.0;
						if (upd) {
							const double omega = 1.0 - rho * r6[2], theta = rho * r6[2] - alpha * c2 * r6[2] + alpha * rho * r6[3];
							const double beta = 1.0 / omega, gamma = -theta * beta - 1.0;
							le = rho * alpha * beta; lf = 2.0 * rho * alpha * gamma + c2 * alpha * alpha;
						}
						if (tid == 0) { S.rho[2 * npairs] = le; S.rho[2 * npairs + 1] = lf; }
						npairs++;
					} else if (upd) {
						if (tid == 0) {
							if (hrc) { S.rho[2 * npairs] = rho; S.rho[2 * npairs + 1] = c2; }   // read after the barriers of the block_sum below
							else { hist[(size_t)npairs * (2 * n + 2) + 2 * n] = rho; hist[(size_t)npairs * (2 * n + 2) + 2 * n + 1] = c2; }
						}
						npairs++;
					}
					if (!hrc) {
						__threadfence_block();
						__syncthreads();   // rho/c2 of the new pair go through HBM/L2: needs the full barrier (vmcnt(0))
					}
					block_sum<NT, 4>(r4, S);
					F = Fn; Fp = Fpn; gn2 = gn2n; rv2 = rv2n;
					iter++;
					if (!sp.fixed_iters && alpha * pnorm <= sri * (1.0 + sqrt(r4[2])) &&
					    sqrt(r4[3]) <= sri * (1.0 + fmax(1.0 + fabs(F), sqrt(gn2)))) { inner_inform = 0; finished = true; }
					else new_major = true;
					}
				}
			}
			}
			if (new_major) {
				// ---- start of a major iteration at (sx, sgp, sd) ----
				if (iter >= sp.itlim) { inner_inform = 4; finished = true; }
				else {
					if (al.mu > 0.0 && m > 0) {
						// Under a large penalty |g| >> |Z'g|: the rounding error of the projection, relative to |g|, is then
						// a visible fraction of gp and of d = W gp, and x would creep off A x = b along the path.
						// Projecting the direction itself leaves an error relative to |d| only.  (g's buffer is free here.)
						project<NT, BIG>(D, S, sd, sg, tmp);
						double r2[2] = {0, 0};
						for_vec<NT>(n, [&](int c) { const double dn = sg[c]; sd[c] = dn; r2[0] += sgp[c] * dn; r2[1] += dn * dn; });
						block_sum<NT, 2>(r2, S);
						r4[0] = r2[0]; r4[1] = r2[1];
					}
					double dphi0 = -r4[0];
					pnorm = sqrt(r4[1]);
					const double xnorm = sqrt(r4[2]), gpnorm = sqrt(r4[3]);
					const double tolg = sri * (1.0 + fmax(1.0 + fabs(F), sqrt(gn2)));
					if (pnorm == 0.0 || !(dphi0 < 0.0)) {
						if (pnorm != 0.0) { // W lost definiteness numerically: restart from W0 once
							npairs = 0;
							if (NWT) { lds_sync(); for_vec<NT>(n, [&](int c) { sxt[c] = sx[c]; }); nwt_refresh(sxt, false); nwt_apply(sgp, sd); }
							else apply_w0<NT, BIG, HESS>(D, Tw, sp.hessian, sgp, sd, sxt, S.oinfo);
							double r2[2] = {0, 0};
							for_vec<NT>(n, [&](int c) { r2[0] += sgp[c] * sd[c]; r2[1] += sd[c] * sd[c]; });
							block_sum<NT, 2>(r2, S);
							r4[0] = r2[0]; r4[1] = r2[1];
							dphi0 = -r2[0]; pnorm = sqrt(r2[1]);
						}
						if (pnorm == 0.0 || !(dphi0 < 0.0)) { inner_inform = (gpnorm <= tolg) ? 0 : 6; finished = true; }
					}
					if (!finished && !sp.fixed_iters && gpnorm <= 1e-3 * tolg) { inner_inform = 0; finished = true; }
					if (!finished) {
						const double amax = sp.steplimit * (1.0 + xnorm) / pnorm;
						const double a = amax < 1.0 ? amax : 1.0;
						if (tid == 0) lsb[lsi ^ 1].init(F, dphi0, a, amax, sp.ls_mu, sp.ls_eta, sp.ls_maxfev);
						lsi ^= 1; ls_a = a;
						state = ST_LS;
						for_vec<NT>(n, [&](int c) { sxt[c] = sx[c] + a * (-sd[c]); });
					}
				}
			}
			NTG_STAMP(5);
			if (finished && phase0) {
				// the pass on the objective alone is over: switch the augmented Lagrangian on (multipliers 0) and start its first pass
				phase0 = false;
				if (inner_inform == 4) { inform = 4; break; }
				if (QPM) {   // QP-based SQP from the unconstrained optimum: multipliers 0, merit weight 1
					for (int j = tid; j < ncn; j += NT) { al_lam[j] = 0.0; qp_lamq[j] = 0.0; }
					al.mu = qp_rho = 1.0; al.qp = 1;
					state = ST_QP; qp_first = true; finished = false;
					__syncthreads();
					make_feasible();   // like every further pass of the other modes: the first projection leaves a residual of rounding x cond(A A')
					for_vec<NT>(n, [&](int c) { sxt[c] = sx[c]; });
					continue;
				}
				al.mu = 10.0;
				npairs = 0; finished = false; inner_inform = 4; state = ST_INIT; weak = false; at_x = true;
				lds_sync();
				for_vec<NT>(n, [&](int c) { sxt[c] = sx[c]; });
				continue;
			}
			if (finished) {
				if (al.mu > 0.0) {
					// ---- multiplier / penalty update of the augmented Lagrangian ----
					if (!at_x) {   // inner solve ended on a rejected trial: refresh c, t at x first
						state = ST_REEVAL;
						lds_sync();
						for_vec<NT>(n, [&](int c) { sxt[c] = sx[c]; });
						continue;
					}
					const double rv = sqrt(rv2);
					bool done_al = false;
					bool take = false;
					if (inner_inform == 6) { inform = 6; done_al = true; }
					else if (rv <= 1e-8 && sri <= sp.sr && inner_inform == 0) { take = true; inform = weak ? 1 : 0; done_al = true; }
					else if (inner_inform == 4) { inform = 4; done_al = true; }
					else {
						if (rv <= 0.25 * rvprev) { take = true; rvprev = rv; }
						else al.mu *= 10.0;
						outer++;
						if (outer >= 30) { inform = 3; done_al = true; }
					}
					// on exit the multipliers stay as they are: x is stationary for the augmented Lagrangian of the CURRENT
					// multipliers, whose estimates t (al_t) are the ones consistent with it and the ones reported
					// the estimates al_t were stored by other lanes / waves during the last evaluation (row -> lane of its
					// breakpoint); only LDS barriers followed on some paths: drain the stores before any lane reads them
					__syncthreads();
					if (take && !done_al) for (int j = tid; j < nal; j += NT) al_lam[j] = al_t[j];
					__syncthreads();   // multipliers cross lanes through HBM: full barrier
					if (!done_al) {
						sri = fmax(sp.sr, fmin(1e-3, 0.1 * rvprev));
						npairs = 0; finished = false; inner_inform = 4; state = ST_INIT; weak = false;
						make_feasible();   // steps stay in null(A) only to rounding: re-project before every further pass
						for_vec<NT>(n, [&](int c) { sxt[c] = sx[c]; });
						continue;
					}
				} else inform = (inner_inform == 0 && weak) ? 1 : inner_inform;
				if (clambda && m > 0 && (D.q_use || al.mu > 0.0 || !at_x)) {   // one more pass for the multipliers (the Q form does not
				                                                       // produce them; projecting directions overwrote the estimate; a solve that
				                                                       // ended on a rejected line-search trial projected last at that trial, not at x)
					state = ST_FINAL;
					lds_sync();
					for_vec<NT>(n, [&](int c) { sxt[c] = sx[c]; });
					continue;
				}
				break;
			}
		}
		// many hundreds of majors under a large penalty let x drift off A x = b by rounding: restore it
		if (al.mu > 0.0) make_feasible();
	}
	lds_sync();
	for (int i = tid; i < n; i += NT) xio[(size_t)b * n + i] = sx[i];
	NTG_STAMP(5);
	if (clambda) {
		const int mall = D.nclin, ntot = n + mall + D.ncnln;   // NPSOL's layout: coefficients, all linear rows, nonlinear rows
		const double *al_rep = al_t;     // estimates of the last evaluation at x: g = A_E' lam_E - [A_I; J]' t
		(void)final_pass;
		__syncthreads();                 // al_t was written by other lanes
		for (int i = tid; i < ntot; i += NT) {
			double v = 0.0;
			if (inform != 9 && i >= n) {
				if (i < n + mall) {
					const int e = D.nI > 0 ? T.rowmap[i - n] : i - n;   // equality index, or -(j+1) for inequality row j
					v = e >= 0 ? S.lam[e] : (al.mu > 0.0 ? -al_rep[ncn - e - 1] : 0.0);
				} else if (al.mu > 0.0) v = -al_rep[i - n - mall];
			}
			clambda[(size_t)b * ntot + i] = v;
		}
#ifdef NTG_CLOCK
		if ((sp.stamps == 1 || sp.stamps == 4) && tid == 0) for (int i = 0; i < 8; i++) clambda[(size_t)b * ntot + i] = (double)tk[i];
#endif
		if (sp.stamps == 3 && tid == 0) {   // diagnostic: work counters of the structured Newton mode
			double *o = clambda + (size_t)b * ntot;
			o[0] = nwt_nfact; o[1] = nwt_nfail; o[2] = nwt_napply; o[3] = outer; o[4] = iter; o[5] = nfev; o[6] = qp_nsolve; o[7] = qp_ncol; o[8] = qp_over; o[9] = qp_fell; o[10] = qp_ntab;
		}
		if (sp.stamps == 2 && tid == 0) {   // diagnostic: state of the augmented-Lagrangian loop at exit
			double *o = clambda + (size_t)b * ntot;
			o[0] = sqrt(rv2); o[1] = al.mu; o[2] = outer; o[3] = sri; o[4] = rvprev; o[5] = inner_inform; o[6] = NWT ? (double)nwt_bad : mfres; o[7] = F;
		}
	}
#undef NTG_STAMP
#undef NTG_CLOCK_TK
	if (tid == 0) {
		if (objective) objective[b] = Fp;
		if (inform_out) inform_out[b] = inform;
		if (iters_out) iters_out[b] = iter;
		if (nfev_out) nfev_out[b] = nfev;
	}
}
