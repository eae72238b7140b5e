// wave_ops.hpp -- wavefront and workgroup primitives (gfx950): the LDS-only barrier, DPP moves and lane exchanges, the
// wave sums (one, few, many values), the workgroup sum on top of them, and the lane-owns-elements loop.  Used by every
// device header that reduces or exchanges across lanes: the solve and evaluation layers, the wave solver, the audits.
#pragma once
#include <hip/hip_runtime.h>

// ------------------------------------------------------------------------------------------
// reductions: sum K values over the workgroup, result broadcast to every lane
// ------------------------------------------------------------------------------------------
// Workgroup barrier for LDS-only hand-offs.  __syncthreads() also drains vmcnt(0), which would
// serialise every in-flight HBM load (history pairs, prefetched coefficient vectors) behind each of
// the many barriers of this kernel; LDS visibility only needs lgkmcnt(0) on both sides.
__device__ __forceinline__ void lds_sync()
{
	asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier\n\ts_waitcnt lgkmcnt(0)" ::: "memory");
}

// 64-lane wavefront sum with DPP (row shifts + row broadcasts stay in the VALU; __shfl_down
// would go through ds_bpermute, i.e. the LDS crossbar, ~100 cycles per hop).  The total lands
// in lane 63 and is broadcast from there through an SGPR.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_add(double v)
{
	const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROW_MASK, 0xf, false);
	const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROW_MASK, 0xf, false);
	return v + __hiloint2double(hi, lo);   // disabled / out-of-row lanes contribute +0.0
}
__device__ __forceinline__ double wave_sum(double v)
{
	v = dpp_add<0x111, 0xf>(v);   // row_shr:1
	v = dpp_add<0x112, 0xf>(v);   // row_shr:2
	v = dpp_add<0x114, 0xf>(v);   // row_shr:4
	v = dpp_add<0x118, 0xf>(v);   // row_shr:8   -> lane 15 of every row holds its row total
	v = dpp_add<0x142, 0xa>(v);   // row_bcast:15 into rows 1 and 3
	v = dpp_add<0x143, 0xc>(v);   // row_bcast:31 into rows 2 and 3 -> lane 63 holds the wave total
	const int lo = __builtin_amdgcn_readlane(__double2loint(v), 63);
	const int hi = __builtin_amdgcn_readlane(__double2hiint(v), 63);
	return __hiloint2double(hi, lo);
}

// exchange a double with the lane whose index differs in one bit (1, 2, 4, 8: DPP inside a row of
// 16; 16: ds_swizzle; 32: bpermute)
template <int CTRL, int BANK>
__device__ __forceinline__ double dpp_mov(double v, double old)
{
	const int lo = __builtin_amdgcn_update_dpp(__double2loint(old), __double2loint(v), CTRL, 0xf, BANK, false);
	const int hi = __builtin_amdgcn_update_dpp(__double2hiint(old), __double2hiint(v), CTRL, 0xf, BANK, false);
	return __hiloint2double(hi, lo);
}
// a DPP move without an "old" operand, so no register is zeroed in front of it: a permutation or rotation inside a row (every lane
// has a source), or a shift whose out-of-range lanes read 0 from the DPP unit itself through bound_ctrl (the wave solver's from_prev /
// from_next) -- the same value in the same lanes as an "old" operand of 0
template <int CTRL>
__device__ __forceinline__ double dpp_perm(double v)
{
	const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xf, 0xf, true);
	const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xf, 0xf, true);
	return __hiloint2double(hi, lo);
}
template <int BIT>
__device__ __forceinline__ double lane_xchg(double v)
{
	if (BIT == 1) return dpp_perm<0xB1>(v);                                // quad_perm [1,0,3,2]
	if (BIT == 2) return dpp_perm<0x4E>(v);                                // quad_perm [2,3,0,1]
	if (BIT == 4) return dpp_mov<0x114, 0xA>(v, dpp_mov<0x104, 0x5>(v, 0.0)); // row_shl:4 into banks 0,2 ; row_shr:4 into banks 1,3
	if (BIT == 8) return dpp_perm<0x128>(v);                               // row_ror:8
	if (BIT == 16) {
		const int lo = __builtin_amdgcn_ds_swizzle(__double2loint(v), 0x401F), hi = __builtin_amdgcn_ds_swizzle(__double2hiint(v), 0x401F);
		return __hiloint2double(hi, lo);
	}
	return __shfl_xor(v, 32, 64);
}

// t(lane) + t(lane ^ 16) / t(lane) + t(lane ^ 32) in every lane, in the VALU: gfx950's v_permlane16_swap / v_permlane32_swap exchange
// the odd rows (the upper half) of one register with the even rows (the lower half) of another -- applied to two copies of t they leave
// "my half's value" in one and "the other half's" in the other, and the sum of the two is the same number in both partners (the earlier
// form went through the LDS crossbar: ds_swizzle + ds_bpermute, two ~100-cycle round trips at the end of every butterfly).
template <int BIT>
__device__ __forceinline__ double xsum_rows(double t)
{
	const int lo = __double2loint(t), hi = __double2hiint(t);
	if constexpr (BIT == 16) {
		const auto r = __builtin_amdgcn_permlane16_swap(lo, lo, false, false), s = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
		return __hiloint2double(s[0], r[0]) + __hiloint2double(s[1], r[1]);
	} else {
		const auto r = __builtin_amdgcn_permlane32_swap(lo, lo, false, false), s = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
		return __hiloint2double(s[0], r[0]) + __hiloint2double(s[1], r[1]);
	}
}

// Sums of a FEW (1..3) per-lane values over the wavefront, every lane receives all of them.  Row stage by rotation (DPP row_ror 1, 2, 4,
// 8: every lane of a row ends up with its row's total, no masked-out lanes and therefore no zero-initialised "old" operands), the two
// cross-row stages on the permlane swaps, the stages of the KV values interleaved (independent chains: with one wave per SIMD nothing
// else hides the DPP latency; the earlier form ran KV complete 6-stage row_shr / row_bcast chains one after the other, 36 instructions
// each).  Lanes of a row add in different orders, so the result is taken from ONE lane (readfirstlane) -- a scalar, known uniform.
__device__ __forceinline__ double uniform_of(double v)   // lane 0's value, as a scalar
{
	return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
}
template <int KV>
__device__ __forceinline__ void wave_sums_few(double (&v)[KV])
{
#pragma unroll
	for (int k = 0; k < KV; k++) v[k] += dpp_perm<0x121>(v[k]);   // row_ror:1
#pragma unroll
	for (int k = 0; k < KV; k++) v[k] += dpp_perm<0x122>(v[k]);   // row_ror:2
#pragma unroll
	for (int k = 0; k < KV; k++) v[k] += dpp_perm<0x124>(v[k]);   // row_ror:4
#pragma unroll
	for (int k = 0; k < KV; k++) v[k] += dpp_perm<0x128>(v[k]);   // row_ror:8
#pragma unroll
	for (int k = 0; k < KV; k++) v[k] = xsum_rows<16>(v[k]);
#pragma unroll
	for (int k = 0; k < KV; k++) v[k] = xsum_rows<32>(v[k]);
#pragma unroll
	for (int k = 0; k < KV; k++) v[k] = uniform_of(v[k]);
}

// Sum KV (<= 16) per-lane values over the 64 lanes with the "halving" butterfly: at the step of
// bit b a lane keeps the half of its values whose index has bit b equal to its own lane bit and
// hands the other half to its partner, so the number of live values halves every step (15 exchanges
// for 16 values instead of 16 x 6).  Afterwards lane L holds the wave total of value L & 15.
template <int KV, int N, int BIT>
__device__ __forceinline__ void halve_step(const double *in, double *out, int lane)
{
	const bool hi = (lane & BIT) != 0;
#pragma unroll
	for (int j = 0; j < N / 2; j++) {
		// original indices covered by in[2j] / in[2j+1] start at (2j)*BIT and (2j+1)*BIT: skip all-padding pairs
		if ((2 * j) * BIT >= KV) { out[j] = 0.0; continue; }
		const double a = in[2 * j], b = ((2 * j + 1) * BIT < KV) ? in[2 * j + 1] : 0.0;
		const double keep = hi ? b : a, send = hi ? a : b;
		out[j] = keep + lane_xchg<BIT>(send);
	}
}
template <int KV>
__device__ __forceinline__ double wave_sum_many(const double *v, int lane)   // v has 16 slots, KV valid
{
	double a[8], b[4], c[2], d[1];
	halve_step<KV, 16, 1>(v, a, lane);
	halve_step<KV, 8, 2>(a, b, lane);
	halve_step<KV, 4, 4>(b, c, lane);
	halve_step<KV, 2, 8>(c, d, lane);
	double t = d[0];
	t = xsum_rows<16>(t);
	t = xsum_rows<32>(t);
	return t;
}

// The cross-wave scratch is double buffered (S.red_sel alternates between two halves): a buffer is rewritten two calls after it was
// read, and the barrier of the call in between already orders those, so ONE barrier per reduction is enough (a single buffer needs a
// second one in front of the writes).
template <int NT, int K, class SM>
__device__ __forceinline__ void block_sum(double (&v)[K], const SM &S)
{
	constexpr int NW = NT / 64;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	if (K >= 4) {
		double w[16];
#pragma unroll
		for (int k = 0; k < 16; k++) w[k] = k < K ? v[k] : 0.0;
		const double t = wave_sum_many<K>(w, lane);   // lane L: wave total of value L & 15
		double *red = S.red + (S.red_sel ? 16 * NW : 0);
		S.red_sel ^= 1;
		if (lane < K) red[lane * NW + wave] = t;
		lds_sync();
#pragma unroll
		for (int k = 0; k < K; k++) {
			double s2 = red[k * NW];
#pragma unroll
			for (int w2 = 1; w2 < NW; w2++) s2 += red[k * NW + w2];
			v[k] = s2;
		}
		return;
	}
#pragma unroll
	for (int k = 0; k < K; k++) v[k] = wave_sum(v[k]);
	if (NW == 1) return;
	double *red = S.red + (S.red_sel ? 16 * NW : 0);
	S.red_sel ^= 1;
	if (lane == 0) {
#pragma unroll
		for (int k = 0; k < K; k++) red[k * NW + wave] = v[k];
	}
	lds_sync();
#pragma unroll
	for (int k = 0; k < K; k++) {
		double s = red[k * NW];
#pragma unroll
		for (int w = 1; w < NW; w++) s += red[k * NW + w];
		v[k] = s;
	}
}

// every lane owns the vector elements c = tid + e*NT.  For n <= 3*NT the three slots are unrolled
// so that their (independent) LDS dependency chains overlap; longer vectors take the plain loop.
template <int NT, class F>
__device__ __forceinline__ void for_vec(int n, F f)
{
	if (n <= 3 * NT) {
#pragma unroll
		for (int e = 0; e < 3; e++) { const int c = threadIdx.x + e * NT; if (c < n) f(c); }
	} else {
		for (int c = threadIdx.x; c < n; c += NT) f(c);
	}
}
