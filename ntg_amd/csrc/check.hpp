// check.hpp -- check_kernel: the trajectory rows of solved problems at arbitrary times (ntg_batch_check), fused: flat flag
// (SplineInterp, colloc.c:476-481) -> linear rows ltc . z and the family's nonlinear rows -> violation of the row bounds -> maximum per
// problem.  No flag ever reaches HBM.  Included by the per-family translation units (fam_*.hip) and by include/ntg_amd_family.hpp.
//
// Mapping: lanes are times.  A workgroup owns one tile of NTG_CHECK_NT times and walks over the problems of its group (blockIdx.y,
// stride gridDim.y).  The basis values of the tile -- the [t][q][r] table basis_kernel wrote -- are read coalesced and kept TRANSPOSED
// in LDS ([class][q][r][lane], rows padded by one double): a lane's reads of "its" time are then consecutive words across the wave
// instead of k d doubles apart.  On the shared grid the tile's table is staged once per workgroup and serves every problem of the group;
// on per-problem grids every problem brings its own.  The problem's coefficient row is staged in LDS once per problem, the flag of a
// lane's time lives in registers (compile-time indices: every output of a family has maxderiv DM).
// Reduction: the per-lane maximum carries its key row * ntimes + time index; 64 lanes by DPP / permlane exchanges, the waves of the
// workgroup through LDS, the tiles of a problem through one (violation, key) pair per tile in HBM that check_final_kernel (times.hip)
// scans.  Maxima with a total order on ties (the smaller key wins): no floating-point atomics, the result does not depend on the order
// in which anything ran.
#pragma once
#include "families.hpp"
#include "wave_ops.hpp"
#include "time_tile.hpp"   // (for the launcher only: the kernel below has the tile's steps written out)

// the (violation, key) maximum of two candidates; key < 0: no violation seen
__device__ __forceinline__ void check_take(double &bv, long long &bk, double ov, long long ok)
{
	if (ov > bv || (ov == bv && ok >= 0 && (bk < 0 || ok < bk))) { bv = ov; bk = ok; }
}
template <int BIT>
__device__ __forceinline__ void check_xchg_step(double &bv, long long &bk)
{
	const double ov = lane_xchg<BIT>(bv);
	const long long ok = __double_as_longlong(lane_xchg<BIT>(__longlong_as_double(bk)));   // (moved as two 32-bit halves: no arithmetic on it)
	check_take(bv, bk, ov, ok);
}

template <int FAM, int NZMAX>
__global__ void __launch_bounds__(NTG_CHECK_NT)
check_kernel(NtgDims D, NtgTables T, CheckArgs a)
{
	using Fam = Family<FAM>;
	constexpr int NT = NTG_CHECK_NT, LD = NT + 1, DM = Fam::DM, NOUTMAX = NZMAX / DM, NR = Fam::NNLTC > 0 ? Fam::NNLTC : 1;
	extern __shared__ __attribute__((aligned(16))) char smem_raw[];
	__shared__ double r_v[NT / 64];
	__shared__ long long r_k[NT / 64];
	double *s_tab = reinterpret_cast<double *>(smem_raw);        // [sumkd][LD]
	double *s_x = s_tab + (size_t)a.sumkd * LD;                  // [npad]
	int *s_off = reinterpret_cast<int *>(s_x + ((D.nC + 1) & ~1));   // [nclass][NT]
	const int tid = threadIdx.x, ntimes = a.ntimes, nz = D.nz, nout = D.nout;
	const int tile0 = blockIdx.x * NT, nval = min(NT, ntimes - tile0);
	const bool live = tid < nval;
	const int tl = live ? tid : nval - 1, t = tile0 + tl;   // lanes past the end repeat the tile's last time and report nothing
	const int nrows = D.nltc + D.nnltc;
	const int slot_l = D.nlic, slot_n = D.nlic + D.nltc + D.nlfc + D.nnlic;   // bound slots of the trajectory rows (order lic, ltc, lfc, nlic, nltc, nlfc)
	for (int bl = blockIdx.y; bl < a.nb; bl += gridDim.y) {
		const int b = a.b0 + bl;   // bl: problem within this launch (the per-problem time tables are indexed by it), b: problem of the batch
		if (bl != (int)blockIdx.y) __syncthreads();   // the previous problem's readers are done
		if (a.pp || bl == (int)blockIdx.y) {
			for (int c = 0; c < D.nclass; c++) {
				const int kd = D.cls_k[c] * D.cls_d[c], n = nval * kd;
				const double *src = a.tblk + (a.pp ? (size_t)bl * a.pp_tab : (size_t)a.gbase[c]) + (size_t)tile0 * kd;
				double *dst = s_tab + (size_t)a.lbase[c] * LD;
				// (e / kd without an integer divide per element: e < 128 k d <= 12800 and k d <= 100, so the float quotient of e + 0.5 is
				// exact to 1e-5 of a value that stays 0.005 away from every integer)
#ifndef NTG_CHECK_DIRECT
				const float rkd = 1.0f / (float)kd;
				for (int e = tid; e < n; e += NT) { const int te = (int)(((float)e + 0.5f) * rkd), qr = e - te * kd; dst[qr * LD + te] = src[e]; }
#else
				(void)n; (void)src; (void)dst;
#endif
				s_off[c * NT + tid] = a.toff[(size_t)(a.pp ? bl : c) * ntimes + t];
			}
		}
		for (int i = tid; i < D.nC; i += NT) s_x[i] = a.x[(size_t)b * D.nC + i];
		ntg_prm_publish<FAM>(T, b);
		__syncthreads();
		// flat flag of this lane's time: z[iz[o] + r] = sum_q D^r B_{off+q}(t) C[iC[o] + off + q]   (colloc.c:476-481, q ascending)
		double z[NZMAX];
#pragma unroll
		for (int v = 0; v < NZMAX; v++) z[v] = 0.0;
#pragma unroll
		for (int o = 0; o < NOUTMAX; o++) {
			if (o < nout) {
				const int c = D.cls[o], k = D.order[o];
#ifndef NTG_CHECK_DIRECT
				constexpr int TS = LD;
				const double *tb = s_tab + (size_t)a.lbase[c] * LD + tl;
#else   // tuning builds only (-DNTG_CHECK_DIRECT): no LDS copy, every lane reads its time's [q][r] block from the table
				constexpr int TS = 1;
				const double *tb = a.tblk + (a.pp ? (size_t)bl * a.pp_tab : (size_t)a.gbase[c]) + (size_t)t * k * DM;
#endif
				const double *cx = s_x + D.iC[o] + s_off[c * NT + tl];
				for (int q = 0; q < k; q++) {
					const double cq = cx[q];
#pragma unroll
					for (int r = 0; r < DM; r++) z[DM * o + r] += tb[(q * DM + r) * TS] * cq;
				}
			}
		}
		double bv = 0.0; long long bk = -1;
		auto row = [&](int r, int slot, double cv) {
			if (a.rows && live) a.rows[((size_t)b * nrows + r) * ntimes + t] = cv;
			if (a.lo) {
				const double lo = a.lo[(size_t)b * D.nbounds + slot], up = a.up[(size_t)b * D.nbounds + slot];
				double v = 0.0;
				if (fabs(lo) < NTG_INF_BOUND) v = fmax(v, lo - cv);
				if (fabs(up) < NTG_INF_BOUND) v = fmax(v, cv - up);
				if (live && v > bv) { bv = v; bk = (long long)r * ntimes + t; }   // rows ascend: on equal violations the first row stays
			}
		};
		for (int j = 0; j < D.nltc; j++) {
			const double *lr = a.ltc + (size_t)j * nz;
			double acc = 0.0;
#pragma unroll
			for (int v = 0; v < NZMAX; v++) { if (v < nz) acc += lr[v] * z[v]; }
			row(j, slot_l + j, acc);
		}
		if constexpr (Fam::NNLTC > 0) {
			if (D.nnltc > 0) {
				// breakpoint index a callback receives: the last breakpoint of the problem's grid at or before the time
				const double *bps = T.bps + (size_t)b * T.pp_bps;
				const double tv = a.times[(size_t)b * a.times_stride + t];
				int ilo = 0, ihi = D.P;
				while (ihi - ilo > 1) { const int mid = (ilo + ihi) >> 1; if (bps[mid] <= tv) ilo = mid; else ihi = mid; }
				double c[NR], tape[Fam::TAPE];
#pragma unroll
				for (int j = 0; j < NR; j++) c[j] = 0.0;
				FamCall<Fam>{ntg_prm_row<FAM>(), D.nnltc}.template nltc_val<NZMAX>(nout, ilo, z, c, tape);
#pragma unroll
				for (int j = 0; j < NR; j++) { if (j < D.nnltc) row(D.nltc + j, slot_n + j, c[j]); }
			}
		}
		if (a.pviol) {
			check_xchg_step<1>(bv, bk); check_xchg_step<2>(bv, bk); check_xchg_step<4>(bv, bk);
			check_xchg_step<8>(bv, bk); check_xchg_step<16>(bv, bk); check_xchg_step<32>(bv, bk);
			if ((tid & 63) == 0) { r_v[tid >> 6] = bv; r_k[tid >> 6] = bk; }
			__syncthreads();
			if (tid == 0) {
				for (int w = 1; w < NT / 64; w++) check_take(bv, bk, r_v[w], r_k[w]);
				const size_t pi = (size_t)b * gridDim.x + blockIdx.x;
				a.pviol[pi] = bv; a.pkey[pi] = bk;
			}
		}
	}
}

// what tile_launch (time_tile.hpp) asks of a time-tile kernel
struct CheckTile {
	using Args = CheckArgs;
	static constexpr size_t LDS_MAX = NTG_CHECK_LDS_MAX;
	static const CheckArgs &tile(const CheckArgs &a) { return a; }
	template <int FAM, int NZMAX> static auto kernel() { return check_kernel<FAM, NZMAX>; }
	template <class Fam> static bool refuses(const NtgDims &D) { return D.nnltc > Fam::NNLTC; }
};
