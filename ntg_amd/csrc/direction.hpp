// direction.hpp -- the pieces of a search direction of sqp_kernel: the projection onto null(A), the preconditioner W0
// (apply_n0, apply_n0_block, apply_w0) and the quasi-Newton memory in pair form (apply_history) and in direction form
// (apply_dform).  Used by sqp_kernel.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include "ntg_dev.hpp"
#include "wave_ops.hpp"
#include "lds_tables.hpp"

// tuning knobs: how many quasi-Newton pairs one reduction round of apply_history covers
#ifndef NTG_HIST_G
#define NTG_HIST_G 6
#endif
#ifndef NTG_HIST_PIPE
#define NTG_HIST_PIPE 2   // pairs per round of the double-buffered sweep (pair scalars in LDS, 3 coefficients per lane); 0 = off
#endif
#ifndef NTG_HIST_ZIGZAG
#define NTG_HIST_ZIGZAG 0
#endif

// ------------------------------------------------------------------------------------------
// SQP pieces
// ------------------------------------------------------------------------------------------
// gp = g - A'(AA')^-1 A g  (projection onto null(A)); S.lam receives the multipliers estimate.
// A is kept sparse (CSR for A g, CSC for A' lam); (AA')^-1 is a small dense matrix.
// With dneg != nullptr the pass also accumulates this lane's share of gp . (-dneg) into *slope (the directional
// derivative the line search needs) and leaves the closing barrier to the reduction that follows.
template <int NT, bool BIG>
__device__ __forceinline__ void project(const NtgDims &D, const Smem &S, const double *sg, double *sgp, double *tmp /* LDS [nclin] */,
                                        const double *dneg = nullptr, double *slope = nullptr)
{
	const int m = D.mE, tid = threadIdx.x;
	if (BIG) __syncthreads();   // g lives in HBM/L2 and is read across lanes
	else lds_sync();
	if (m == 0) {
		for (int c = tid; c < D.nC; c += NT) { const double gq = sg[c]; sgp[c] = gq; if (dneg) *slope += gq * (-dneg[c]); }
		if (!dneg) lds_sync();
		return;
	}
	if (D.q_use) {
		// gp = g - Q g with Q = A'(AA')^-1 A stored as ELL over its non-zero rows: one pass, no
		// intermediate barrier; the padded entries (value 0, column 0) keep every load unconditional
		const int w = D.q_w;
		for_vec<NT>(D.nC, [&](int c) {
			const int t = S.q_idx[c];
			double s = 0.0;
			if (t >= 0) {
#pragma unroll 4
				for (int e = 0; e < w; e++) s += S.q_val[t * w + e] * sg[S.q_col[t * w + e]];
			}
			const double gq = sg[c] - s;
			sgp[c] = gq;
			if (dneg) *slope += gq * (-dneg[c]);
		});
		if (!dneg) lds_sync();
		return;
	}
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
	for (int c = tid; c < D.nC; c += NT) {
		double s = 0.0;
		for (int e = S.csc_ptr[c]; e < S.csc_ptr[c + 1]; e++) s += S.csc_val[e] * S.lam[S.csc_row[e]];
		const double gq = sg[c] - s;
		sgp[c] = gq;
		if (dneg) *slope += gq * (-dneg[c]);
	}
	if (!dneg) lds_sync();
}

typedef const __attribute__((address_space(3))) double *lds_cdp;
typedef const __attribute__((address_space(3))) int *lds_cip;
typedef __attribute__((address_space(3))) double *lds_dp;
typedef const __attribute__((address_space(1))) double *glb_cdp;
typedef __attribute__((address_space(1))) double *glb_dp;
typedef const __attribute__((address_space(1))) unsigned short *glb_cusp;
// a coefficient vector of the solve lives in LDS, or (BIG layouts) in the per-problem HBM workspace: the out-of-line routines below take
// it with its address space in the type (template flag G = "global"), so that they contain no FLAT instruction (ntg_amd/call_audit.py R2)
template <bool G> struct VecPtr { typedef lds_dp rw; typedef lds_cdp ro; };
template <> struct VecPtr<true> { typedef glb_dp rw; typedef glb_cdp ro; };
// out = W0 v for the collocation preconditioner (ELL, rows streamed from L2).  Kept out of line:
// it runs a handful of times per solve and must not add to the register pressure of the main loop.
template <int NT, bool VG, bool OG>
__device__ __attribute__((noinline)) void apply_n0(int n, int w, glb_cdp n0, glb_cusp n0c, typename VecPtr<VG>::ro v, typename VecPtr<OG>::rw out)
{
	for (int c = threadIdx.x; c < n; c += NT) {
		double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
		int s = 0;
		for (; s + 4 <= w; s += 4) {   // four independent chains: the L2 loads of a row overlap
			a0 += n0[(size_t)(s + 0) * n + c] * v[n0c[(size_t)(s + 0) * n + c]];
			a1 += n0[(size_t)(s + 1) * n + c] * v[n0c[(size_t)(s + 1) * n + c]];
			a2 += n0[(size_t)(s + 2) * n + c] * v[n0c[(size_t)(s + 2) * n + c]];
			a3 += n0[(size_t)(s + 3) * n + c] * v[n0c[(size_t)(s + 3) * n + c]];
		}
		for (; s < w; s++) a0 += n0[(size_t)s * n + c] * v[n0c[(size_t)s * n + c]];
		out[c] = (a0 + a1) + (a2 + a3);
	}
}

// out = W0 v when W0 is block diagonal by output with equally sized dense blocks, few of them distinct (one basis
// class, the same constraint pattern at the ends; outputs with the same cost derivative share a block): the one
// GEMM-shaped piece of the path,  Out(nco x nout) = sum_b W_b (nco x nco) V_b (nco x nout),  V_b = the columns of the
// outputs that use block b.  It runs on the matrix cores: v_mfma_f64_16x16x4_f64 tiles, a wave owns row tiles of 16
// coefficients and sweeps k in steps of 4.  Register layout of the instruction (probed on gfx950): lane l supplies
// A[i = l%16][k = l/16] and B[k = l/16][j = l%16] and receives D[i = 4r + l/16][j = l%16], r = 0..3.
//   A = W_b: s-major in HBM/L2 ([s][row], symmetric), so the 16 lanes of a k read 16 consecutive words;
//   B = V:   staged in LDS laid out like v ([output][coefficient]); column j >= nout or of another block is 0.
// Rows of W_b beyond nco are zero padding (spad rows, a multiple of 16); `out` may alias `stage`: the result tiles
// stay in registers until every wave has finished reading.
typedef double ntg_d4 __attribute__((ext_vector_type(4)));
template <int NT, bool VG, bool OG>
__device__ __attribute__((noinline)) void apply_n0_block(int nC, int nout, int nco, int spad, int nblk, glb_cdp wb,
                                                         lds_cip oinfo, typename VecPtr<VG>::ro v, lds_dp stage_w, typename VecPtr<OG>::rw out)
{
	constexpr int NW = NT / 64, TMAX = 4, U = 4;   // nco <= NT (checked by the caller): at most NT/16 = 4 NW row tiles
	lds_sync();   // previous readers of stage are done
	for (int c = threadIdx.x; c < nC; c += NT) stage_w[c] = v[c];   // owner lanes: v may live in HBM
	lds_sync();
	lds_cdp stage = (lds_cdp)stage_w;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
	const int ntile = (nco + 15) >> 4;
	const int myblk = li < nout ? oinfo[li * 10 + 2] : -1;
	lds_cdp bcol = stage + (li < nout ? li : 0) * nco;
	ntg_d4 acc[TMAX];
#pragma unroll
	for (int t = 0; t < TMAX; t++) acc[t] = ntg_d4{0.0, 0.0, 0.0, 0.0};
	for (int b = 0; b < nblk; b++) {
		glb_cdp wbb = wb + (size_t)b * spad * nco + li;
		const bool mine = myblk == b;
		for (int k0 = 0; k0 < spad; k0 += 4 * U) {   // spad is a multiple of 16 = 4 U
			// U k-steps of loads first (L2 latency overlaps), then their matrix instructions
			double av[U][TMAX], bv[U];
#pragma unroll
			for (int u = 0; u < U; u++) {
				const int k = k0 + 4 * u + lk;
				bv[u] = mine ? bcol[min(k, nco - 1)] : 0.0;   // k >= nco: W's row is zero padding
				glb_cdp wk = wbb + (size_t)k * nco;
#pragma unroll
				for (int t = 0; t < TMAX; t++) av[u][t] = (wave + t * NW < ntile) ? wk[(wave + t * NW) * 16] : 0.0;
			}
#pragma unroll
			for (int u = 0; u < U; u++)
#pragma unroll
				for (int t = 0; t < TMAX; t++)
					if (wave + t * NW < ntile) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u][t], bv[u], acc[t], 0, 0, 0);
		}
	}
	lds_sync();   // every read of stage is done: out may be the same buffer
	if (li < nout) {
#pragma unroll
		for (int t = 0; t < TMAX; t++) {
			const int tile = wave + t * NW;
			if (tile < ntile) {
#pragma unroll
				for (int r = 0; r < 4; r++) { const int row = tile * 16 + 4 * r + lk; if (row < nco) out[li * nco + row] = acc[t][r]; }
			}
		}
	}
}

// out = W0 v : identity on null(A) (cold start) or the collocation preconditioner.  `stage` is an LDS buffer of
// nC doubles that is free at every call site (the trial point: it is rebuilt from x and d afterwards).
// HESS = false: the instance is only ever launched with the identity cold start (NPSOL's mode, the fixed-work
// benchmark): no preconditioner code, in particular no out-of-line calls, in its main loop.
// OLDS: `out` is an LDS vector even in the BIG layout (t = W gp+ lives in the trial-point buffer)
template <int NT, bool BIG, bool HESS, bool OLDS = false>
__device__ __forceinline__ void apply_w0(const NtgDims &D, const NtgTables &T, int hessian, const double *v, double *out, double *stage, const int *oinfo)
{
	constexpr bool VG = BIG, OG = BIG && !OLDS;
	if (!HESS) {
		lds_sync();
		for_vec<NT>(D.nC, [&](int c) { out[c] = v[c]; });
		lds_sync();
		return;
	}
	if (hessian == 1 && T.n0b && T.n0b_n <= NT) {
		apply_n0_block<NT, VG, OG>(D.nC, D.nout, T.n0b_n, T.n0b_sp, T.n0b_nblk, (glb_cdp)T.n0b, (lds_cip)oinfo, (typename VecPtr<VG>::ro)v, (lds_dp)stage, (typename VecPtr<OG>::rw)out);
		if (BIG) __syncthreads();   // out may live in HBM and was written by row, not by owner lane
		else lds_sync();
		return;
	}
	if (BIG) __syncthreads();   // v lives in HBM/L2 and apply_n0 reads it across lanes
	else lds_sync();
	if (hessian == 1 && T.n0) apply_n0<NT, VG, OG>(D.nC, T.n0_w, (glb_cdp)T.n0, (glb_cusp)T.n0c, (typename VecPtr<VG>::ro)v, (typename VecPtr<OG>::rw)out);
	else for_vec<NT>(D.nC, [&](int c) { out[c] = v[c]; });
	lds_sync();
}

// t += (sum of the stored rank-2 BFGS terms) v.  Pairs are streamed from HBM/L2 once, G at a
// time: 2G partial dots per lane, ONE workgroup reduction, then the axpys from the registers
// that still hold the pair elements.
template <int NT, int EPT = 3, int G = NTG_HIST_G>
__device__ __forceinline__ void apply_history(const NtgDims &D, const Smem &S, const double *hist, int npairs,
                              const double *v, double *t, const double *hrc = nullptr)
{
	const int n = D.nC, tid = threadIdx.x;
#if NTG_HIST_PIPE > 0
	if (EPT <= 3 && NT <= 128 && n <= EPT * NT && hrc) {   // (one workgroup per CU, NT >= 256: fewer, larger rounds are faster -- config D 162 vs 190 ms)
		constexpr int PG = NTG_HIST_PIPE;
		// Two register buffers of PG pairs: the loads of round r+1 are in flight while round r is reduced.  Every load is
		// unconditional (pair index clamped to the newest pair, column clamped to n-1) so that the waits are counted
		// (vmcnt(loads of the younger round)) instead of vmcnt(0); rounds past the end get rho = c2 = 0.  The pair scalars
		// come from LDS: nothing but the pair elements in the register buffers.
		if (npairs == 0) { lds_sync(); return; }
		double vv[EPT], tt[EPT];
		int cc[EPT];
#pragma unroll
		for (int e = 0; e < EPT; e++) { const int c = tid + e * NT; cc[e] = min(c, n - 1); vv[e] = c < n ? v[c] : 0.0; tt[e] = c < n ? t[c] : 0.0; }
		{
			// odd memories are swept newest-first, even ones oldest-first: the pairs a sweep ends on are the ones the next
			// sweep (one pair longer) starts on, while they are still in L2 / the memory-side cache
			const bool rev = NTG_HIST_ZIGZAG && (npairs & 1);
			auto pidx = [&](int i) { const int j = min(i, npairs - 1); return rev ? npairs - 1 - j : j; };
			double hsA[PG][EPT], huA[PG][EPT], hsB[PG][EPT], huB[PG][EPT];
			auto load = [&](int base, double (&hs)[PG][EPT], double (&hu)[PG][EPT]) {
#pragma unroll
				for (int g = 0; g < PG; g++) {
					const double *h = hist + (size_t)pidx(base + g) * (2 * n + 2);
#pragma unroll
					for (int e = 0; e < EPT; e++) { hs[g][e] = h[cc[e]]; hu[g][e] = h[n + cc[e]]; }
				}
			};
			auto consume = [&](int base, double (&hs)[PG][EPT], double (&hu)[PG][EPT]) {
				double acc[2 * PG];
#pragma unroll
				for (int g = 0; g < PG; g++) {
					acc[2 * g] = 0.0; acc[2 * g + 1] = 0.0;
#pragma unroll
					for (int e = 0; e < EPT; e++) { acc[2 * g] += hs[g][e] * vv[e]; acc[2 * g + 1] += hu[g][e] * vv[e]; }
				}
				block_sum<NT, 2 * PG>(acc, S);
#pragma unroll
				for (int g = 0; g < PG; g++) {
					const bool on = base + g < npairs;
					const int pi = pidx(base + g);
					const double live = on ? 1.0 : 0.0, rho = hrc[2 * pi] * live, c2 = hrc[2 * pi + 1] * live;   // unconditional LDS reads
#pragma unroll
					for (int e = 0; e < EPT; e++)
						tt[e] += -rho * (hs[g][e] * acc[2 * g + 1] + hu[g][e] * acc[2 * g]) + c2 * hs[g][e] * acc[2 * g];
				}
			};
			load(0, hsA, huA);
			for (int base = 0; base < npairs; base += 2 * PG) {
				load(base + PG, hsB, huB);
				consume(base, hsA, huA);
				if (base + PG >= npairs) break;
				load(base + 2 * PG, hsA, huA);
				consume(base + PG, hsB, huB);
			}
#pragma unroll
			for (int e = 0; e < EPT; e++) { const int c = tid + e * NT; if (c < n) t[c] = tt[e]; }
			lds_sync();
			return;
		}
	}
#endif
	if (n <= EPT * NT) {
		double vv[EPT], tt[EPT];
#pragma unroll
		for (int e = 0; e < EPT; e++) { const int c = tid + e * NT; vv[e] = c < n ? v[c] : 0.0; tt[e] = c < n ? t[c] : 0.0; }
		for (int base = 0; base < npairs; base += G) {
			const int cnt = min(G, npairs - base);
			double hs[G][EPT], hu[G][EPT], acc[2 * G];
#pragma unroll
			for (int g = 0; g < G; g++) {
				acc[2 * g] = 0.0; acc[2 * g + 1] = 0.0;
				const double *h = hist + (size_t)(base + g) * (2 * n + 2);
#pragma unroll
				for (int e = 0; e < EPT; e++) {
					const int c = tid + e * NT;
					const bool on = g < cnt && c < n;
					hs[g][e] = on ? h[c] : 0.0;
					hu[g][e] = on ? h[n + c] : 0.0;
				}
			}
#pragma unroll
			for (int g = 0; g < G; g++)
#pragma unroll
				for (int e = 0; e < EPT; e++) { acc[2 * g] += hs[g][e] * vv[e]; acc[2 * g + 1] += hu[g][e] * vv[e]; }
			block_sum<NT, 2 * G>(acc, S);
#pragma unroll
			for (int g = 0; g < G; g++) {
				if (g < cnt) {
					const double *hh = hrc ? hrc + 2 * (base + g) : hist + (size_t)(base + g) * (2 * n + 2) + 2 * n;
					const double rho = hh[0], c2 = hh[1];
#pragma unroll
					for (int e = 0; e < EPT; e++)
						tt[e] += -rho * (hs[g][e] * acc[2 * g + 1] + hu[g][e] * acc[2 * g]) + c2 * hs[g][e] * acc[2 * g];
				}
			}
		}
#pragma unroll
		for (int e = 0; e < EPT; e++) { const int c = tid + e * NT; if (c < n) t[c] = tt[e]; }
		lds_sync();
		return;
	}
	for (int base = 0; base < npairs; base += 4) {
		const int cnt = min(4, npairs - base);
		double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
		for (int c = tid; c < n; c += NT) {
			const double vv = v[c];
#pragma unroll
			for (int g = 0; g < 4; g++) {
				if (g < cnt) {
					const double *h = hist + (size_t)(base + g) * (2 * n + 2);
					acc[2 * g] += h[c] * vv;
					acc[2 * g + 1] += h[n + c] * vv;
				}
			}
		}
		block_sum<NT, 8>(acc, S);
		for (int c = tid; c < n; c += NT) {
			double tt = t[c];
#pragma unroll
			for (int g = 0; g < 4; g++) {
				if (g < cnt) {
					const double *h = hist + (size_t)(base + g) * (2 * n + 2);
					const double s = h[c], u = h[n + c], rho = hrc ? hrc[2 * (base + g)] : h[2 * n], c2 = hrc ? hrc[2 * (base + g) + 1] : h[2 * n + 1];
					tt += -rho * (s * acc[2 * g + 1] + u * acc[2 * g]) + c2 * s * acc[2 * g];
				}
			}
			t[c] = tt;
		}
	}
	lds_sync();
}

// The same quasi-Newton operator from ONE stored vector per major iteration (half the history traffic of apply_history).
// With exact bookkeeping the pair (s_i, u_i) of major i lies in the span of two consecutive search directions: s_i = -alpha_i d_i and,
// because d_{i+1} = W_{i+1} g_{i+1} = omega_i t_i + theta_i d_i with t_i = W_i g_{i+1}, u_i = t_i - d_i = beta_i d_{i+1} + gamma_i d_i.
// Substituting into the rank-two terms gives  W_k v = W0 v + sum_j kappa_j d_j,  kappa = (symmetric tridiagonal) (d_j . v):
//   kappa_j = f_j delta_j + e_j delta_{j+1} + e_{j-1} delta_{j-1},   e_i = rho_i alpha_i beta_i,  f_i = 2 rho_i alpha_i gamma_i + c2_i alpha_i^2.
// HBM holds the chain d_0 .. d_{nv-1} (the last one is the current direction), LDS the link scalars (e_i, f_i); a skipped update is a
// null link (0, 0).  Rounds of G vectors through two register buffers like apply_history; the vector a round ends on is carried in
// registers into the next round (its link reaches across).
template <int NT, int EPT, int G>
__device__ __forceinline__ void apply_dform(const NtgDims &D, const Smem &S, const double *hist, int nv, const double *v, double *t, const double *links)
{
	const int n = D.nC, tid = threadIdx.x;
	double vv[EPT], tt[EPT], dc[EPT], dcl = 0.0;
	int cc[EPT];
#pragma unroll
	for (int e = 0; e < EPT; e++) { const int c = tid + e * NT; cc[e] = min(c, n - 1); vv[e] = c < n ? v[c] : 0.0; tt[e] = c < n ? t[c] : 0.0; dc[e] = 0.0; }
	double hA[G][EPT], hB[G][EPT];
	auto load = [&](int base, double (&h)[G][EPT]) {   // unconditional: past the end the newest vector again (its links are masked)
#pragma unroll
		for (int g = 0; g < G; g++) {
			const double *p = hist + (size_t)min(base + g, nv - 1) * n;
#pragma unroll
			for (int e = 0; e < EPT; e++) h[g][e] = p[cc[e]];
		}
	};
	auto consume = [&](int base, double (&h)[G][EPT]) {
		double acc[G];
#pragma unroll
		for (int g = 0; g < G; g++) {
			acc[g] = 0.0;
#pragma unroll
			for (int e = 0; e < EPT; e++) acc[g] += h[g][e] * vv[e];
		}
		block_sum<NT, G>(acc, S);
#pragma unroll
		for (int g = 0; g < G; g++) {
			const int i = base - 1 + g;   // link i joins vector i (left) and vector i+1 = base+g (right)
			const bool on = i >= 0 && i < nv - 1;
			const int ii = on ? i : 0;
			const double le = on ? links[2 * ii] : 0.0, lf = on ? links[2 * ii + 1] : 0.0;
			const double dl = g == 0 ? dcl : acc[g > 0 ? g - 1 : 0], dr = acc[g];
			const double a = le * dr + lf * dl, b = le * dl;
#pragma unroll
			for (int e = 0; e < EPT; e++) tt[e] += (g == 0 ? dc[e] : h[g > 0 ? g - 1 : 0][e]) * a + h[g][e] * b;
		}
#pragma unroll
		for (int e = 0; e < EPT; e++) dc[e] = h[G - 1][e];
		dcl = acc[G - 1];
	};
	load(0, hA);
	for (int base = 0; base < nv; base += 2 * G) {
		load(base + G, hB);
		consume(base, hA);
		if (base + G >= nv) break;
		load(base + 2 * G, hA);
		consume(base + G, hB);
	}
#pragma unroll
	for (int e = 0; e < EPT; e++) { const int c = tid + e * NT; if (c < n) t[c] = tt[e]; }
	lds_sync();
}
