// cost.hpp -- cost_kernel: the running cost of solved problems at arbitrary times under any quadrature (ntg_batch_cost), fused: flat flag
// (SplineInterp, colloc.c:476-481) -> the family's running cost L = ucf(z) (the integrand of IntegratedCost, cost.c) -> weighted sum per
// problem.  No flag and no gradient ever reaches HBM.  Included by the per-family translation units (fam_*.hip) and by
// include/ntg_amd_family.hpp.
//
// Mapping: check_kernel's, through the functions of time_tile.hpp: lanes are times, a workgroup owns one tile of NTG_CHECK_NT times and walks over the problems of
// its group; the tile's basis table transposed in LDS, the coefficient row staged per problem, the flag in registers.
// Sum, in a fixed order: a lane's term w_i L_i (0 past the end of the tile); the 64 lanes of a wave by the butterfly lane ^ 1, 2, 4, 8,
// 16, 32 (every lane ends with the same double: an addition's operands commute); the waves of the workgroup through LDS in index order;
// the tiles of a problem through one partial per tile in HBM that cost_final_kernel (times.hip) adds in tile order.  No floating-point
// atomics: the result does not depend on the order in which anything ran, nor on the batch around a problem.
#pragma once
#include "families.hpp"
#include "wave_ops.hpp"
#include "time_tile.hpp"

template <int BIT>
__device__ __forceinline__ void cost_xchg_step(double &s) { s += lane_xchg<BIT>(s); }

template <int FAM, int NZMAX>
__global__ void __launch_bounds__(NTG_CHECK_NT)
cost_kernel(NtgDims D, NtgTables T, CostArgs ca)
{
	using Fam = Family<FAM>;
	constexpr int NT = NTG_CHECK_NT, DM = Fam::DM, NOUTMAX = NZMAX / DM;
	extern __shared__ __attribute__((aligned(16))) char smem_raw[];
	__shared__ double r_s[NT / 64];
	const CheckArgs &a = ca.t;
	const TileLds s = tile_lds(smem_raw, D, a);
	const int tid = threadIdx.x, ntimes = a.ntimes, nout = D.nout;
	const int tile0 = blockIdx.x * NT, nval = min(NT, ntimes - tile0);
	const bool live = tid < nval;
	const int tl = live ? tid : nval - 1, t = tile0 + tl;   // lanes past the end repeat the tile's last time and add nothing
	for (int bl = blockIdx.y; bl < a.nb; bl += gridDim.y) {
		const int b = a.b0 + bl;   // bl: problem within this launch (the per-problem time tables are indexed by it), b: problem of the batch
		tile_stage<FAM>(D, T, a, s, bl, b, tile0, nval, t);
		double z[NZMAX];   // flat flag of this lane's time
		tile_flag<DM, NZMAX>(D, a, s, bl, t, tl, z);
		// the family's running cost; its gradient goes to registers nothing reads (no family has a value-only form).  The callbacks loop
		// over the outputs: with the number of outputs a constant the loop unrolls and the flag stays in registers, so the instances by
		// flag size call it once per possible count (at most 8 copies); the widest instance does so for its own count only and otherwise
		// indexes the flag at run time (private memory)
		const int ibp = tile_bp_index(D, T, a, b, t);
		const FamCall<Fam> fam{ntg_prm_row<FAM>(), D.nnltc};
		double f = 0.0, df[NZMAX];
		if constexpr (NOUTMAX <= 8) {
#pragma unroll
			for (int n = 1; n <= NOUTMAX; n++) { if (nout == n) fam.ucf(n, ibp, z, f, df); }
		} else {
			if (nout == NOUTMAX) fam.ucf(NOUTMAX, ibp, z, f, df); else fam.ucf(nout, ibp, z, f, df);
		}
		if (ca.vals && live) ca.vals[(size_t)b * ntimes + t] = f;
		if (ca.pcost) {
			double sum = live ? ca.weights[(size_t)b * a.times_stride + t] * f : 0.0;
			cost_xchg_step<1>(sum); cost_xchg_step<2>(sum); cost_xchg_step<4>(sum);
			cost_xchg_step<8>(sum); cost_xchg_step<16>(sum); cost_xchg_step<32>(sum);
			if ((tid & 63) == 0) r_s[tid >> 6] = sum;
			__syncthreads();
			if (tid == 0) {
				for (int w = 1; w < NT / 64; w++) sum += r_s[w];
				ca.pcost[(size_t)b * gridDim.x + blockIdx.x] = sum;
			}
		}
	}
}

// what tile_launch (time_tile.hpp) asks of a time-tile kernel
struct CostTile {
	using Args = CostArgs;
	static constexpr size_t LDS_MAX = NTG_CHECK_LDS_MAX;
	static const CheckArgs &tile(const CostArgs &ca) { return ca.t; }
	template <int FAM, int NZMAX> static auto kernel() { return cost_kernel<FAM, NZMAX>; }
	template <class Fam> static bool refuses(const NtgDims &) { return false; }
};
