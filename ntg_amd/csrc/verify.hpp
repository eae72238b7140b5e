// verify.hpp -- verify_kernel: the analytic derivatives of a family's six callbacks against central differences (ntg_batch_verify),
// fused: flat flag at every breakpoint (SplineInterp, colloc.c:476-481) -> the callback at z and at z +- h e_v for every flag entry v
// -> relative error of the analytic derivative, and what a callback returns for entries its active-variable list does not name ->
// maxima per problem and slot.  It stands where NPSOL's derivative verification stands behind the reference (ntg.c:249-253).  No flag
// and no gradient ever reaches HBM.  Included by the per-family translation units (fam_*.hip) and by include/ntg_amd_family.hpp.
//
// The definition (include/ntg_amd.h repeats it; tests/verify_oracle.py restates it on the CPU):
//   h = 2^-17 max(1, |z_v|), zp = z_v + h, zm = z_v - h, fd = (f(zp) - f(zm)) / (zp - zm)       only entry v moves
//   an = df[v] or dc[j][v] at the unperturbed z, scale = max(1, |f(z)|, |an|, |fd|)
//   err  = max |fd - an| / scale           over the entries v the slot's own active-variable list names
//   leak = max max(|an|, |fd|) / scale     over the entries it does not name
// Slots, in this order everywhere: icf, ucf, fcf, nlicf, nltcf, nlfcf (NTG_VERIFY_NSLOT).  Initial slots are audited at breakpoint 0,
// final slots at the last breakpoint, trajectory slots at every breakpoint; a slot the plan does not use is not called.
//
// Mapping: cost_kernel's, through the functions of time_tile.hpp, with the BREAKPOINTS as the times: lanes are breakpoints, a workgroup
// owns one tile of NTG_CHECK_NT of them and walks over the problems of its group.  The breakpoint index a callback receives is the
// lane's own index (the times are the breakpoints, so no search).
// Registers: the flag is never indexed with a run-time v.  A run-time loop over v holds a two-trip loop over the sign (not unrolled: one
// copy of the callback for both) whose body builds the perturbed flag by an unrolled select and calls the callback; the analytic entry and z_v are picked by unrolled selects too.  With
// the number of outputs a constant (the nout == n dispatch of cost.hpp, flags of at most 8 outputs) everything stays in registers; the
// widest instances index the Jacobian at run time (private memory).
// Reduction: a candidate is (value, key) with key = (function * nbps + breakpoint) * nz + entry; the larger value wins, on equal
// values the smaller key, a NaN beats every number (ntg_batch_kkt's rule) and among NaNs the smaller key wins: a total order, so the
// butterfly over the 64 lanes (lane ^ 1, 2, 4, 8, 16, 32), the waves through LDS in index order and the tiles of a problem through one
// partial per tile (verify_final_kernel, times.hip) give a result that does not depend on the order in which anything ran.
#pragma once
#include "families.hpp"
#include "wave_ops.hpp"
#include "time_tile.hpp"

// candidate (ov, ok) against the best so far (bv, bk); the start is (0, -1): a value of 0 never enters, its place stays -1
__device__ __forceinline__ void verify_take(double &bv, long long &bk, double ov, long long ok)
{
	const bool on = ov != ov, bn = bv != bv;
	if (on ? (!bn || ok < bk) : (!bn && (ov > bv || (ov == bv && ov > 0.0 && ok < bk)))) { bv = ov; bk = ok; }
}
template <int BIT>
__device__ __forceinline__ void verify_xchg_step(double &bv, long long &bk)
{
	const double ov = lane_xchg<BIT>(bv);
	const long long ok = __double_as_longlong(lane_xchg<BIT>(__longlong_as_double(bk)));   // (moved as two 32-bit halves: no arithmetic on it)
	verify_take(bv, bk, ov, ok);
}
// the larger of the two; a NaN, once in, stays
__device__ __forceinline__ double verify_max(double a, double b) { return (b > a || b != b) ? b : a; }

// rows a family's callback of a slot may write (1 for the costs)
template <class Fam, int SLOT> constexpr int verify_rows()
{
	const int n = SLOT < 3 ? 1 : SLOT == 3 ? Fam::NNLIC : SLOT == 4 ? Fam::NNLTC : Fam::NNLFC;
	return n > 0 ? n : 1;
}
template <class Fam, int SLOT>
__device__ __forceinline__ void verify_call(const FamCall<Fam> &fam, int nout, int ibp, const double *z, double *c, double *dc)
{
	if constexpr (SLOT == 0) fam.icf(nout, z, c[0], dc);
	else if constexpr (SLOT == 1) fam.ucf(nout, ibp, z, c[0], dc);
	else if constexpr (SLOT == 2) fam.fcf(nout, z, c[0], dc);
	else if constexpr (SLOT == 3) fam.nlicf(nout, z, c, dc);
	else if constexpr (SLOT == 4) fam.nltcf(nout, ibp, z, c, dc);
	else fam.nlfcf(nout, z, c, dc);
}

// One slot at this lane's breakpoint ibp: nf functions (1, or the plan's rows of the slot), flag entries [0, DM nout).  use: the lane's
// point belongs to the slot.  Leaves the lane's best candidates of the two maxima in (ev, ek) and (lv, lk).
// The two trips of the sign loop share one copy of the callback; nothing in them is selected by the sign (selects by the trip count become
// a two-element array in private memory): the trip's point is z_v + sg h and the difference f(zp) - f(zm) accumulates as d += sg f with
// sg = +-1 -- both exact, the same doubles as zp, zm and the difference of the two values.
// FIXED: nout is a constant of the caller, so dc's stride is one too and the analytic entry is picked by an unrolled select; otherwise
// (the widest instances) the Jacobian lives in private memory anyway and is indexed there.
template <class Fam, int SLOT, int NZMAX, bool FIXED>
__device__ __forceinline__ void verify_slot(const FamCall<Fam> &fam, int nout, int nf, int ibp, int nbps, const double *z, u64 mask, bool use,
                                            double &ev, long long &ek, double &lv, long long &lk)
{
	constexpr int NF = verify_rows<Fam, SLOT>();
	const int nz = Fam::DM * nout;
	double c0[NF], an[NF * NZMAX];
#pragma unroll
	for (int j = 0; j < NF; j++) c0[j] = 0.0;
#pragma unroll
	for (int i = 0; i < NF * NZMAX; i++) an[i] = 0.0;
	verify_call<Fam, SLOT>(fam, nout, ibp, z, c0, an);
	for (int v = 0; v < nz; v++) {
		double zv = 0.0;
#pragma unroll
		for (int u = 0; u < NZMAX; u++) zv = u == v ? z[u] : zv;
		const double h = 0x1p-17 * fmax(1.0, fabs(zv)), zp = zv + h, zm = zv - h;
		double d[NF];
#pragma unroll
		for (int j = 0; j < NF; j++) d[j] = 0.0;
		double sg = 1.0;
#pragma unroll 1
		for (int trip = 0; trip < 2; trip++, sg = -sg) {
			const double zs = zv + sg * h;
			double zq[NZMAX], c[NF], dc[NF * NZMAX];
#pragma unroll
			for (int u = 0; u < NZMAX; u++) zq[u] = u == v ? zs : z[u];
#pragma unroll
			for (int j = 0; j < NF; j++) c[j] = 0.0;
			verify_call<Fam, SLOT>(fam, nout, ibp, zq, c, dc);   // (its gradient goes to registers nothing reads)
#pragma unroll
			for (int j = 0; j < NF; j++) d[j] += sg * c[j];
		}
		const bool named = (mask >> v) & 1ull;
#pragma unroll
		for (int j = 0; j < NF; j++) {
			if (j < nf) {
				double a = 0.0;
				if constexpr (FIXED) {
#pragma unroll
					for (int u = 0; u < NZMAX; u++) a = u == v ? an[j * nz + u] : a;
				} else a = an[j * nz + v];
				const double fd = d[j] / (zp - zm);
				const double scale = fmax(fmax(1.0, fabs(c0[j])), fmax(fabs(a), fabs(fd)));
				const long long key = ((long long)j * nbps + ibp) * nz + v;
				// (both maxima see every candidate, the one it does not belong to as a 0, which never enters: a choice between the two
				// pairs of references would put them into private memory)
				verify_take(ev, ek, use && named ? fabs(fd - a) / scale : 0.0, key);
				verify_take(lv, lk, use && !named ? verify_max(fabs(a), fabs(fd)) / scale : 0.0, key);
			}
		}
	}
}

// A slot's two maxima over the wave: the lane's candidates through the butterfly, then lane 0 of the wave leaves them in
// r_v / r_k [2 SLOT + (0: err, 1: leak)][wave].  on: the slot is used and this tile holds a point of it (the same for every lane of the
// workgroup); an unused slot leaves (0, -1).
template <class Fam, int SLOT, int NZMAX, bool FIXED>
__device__ __forceinline__ void verify_slot_wave(const FamCall<Fam> &fam, bool on, int nout, int nf, int t, int nbps, const double *z, u64 mask, bool use,
                                                 double (*r_v)[NTG_CHECK_NT / 64], long long (*r_k)[NTG_CHECK_NT / 64])
{
	const int tid = threadIdx.x;
	double ev = 0.0, lv = 0.0; long long ek = -1, lk = -1;
	if (on) {
		verify_slot<Fam, SLOT, NZMAX, FIXED>(fam, nout, nf, t, nbps, z, mask, use, ev, ek, lv, lk);
		verify_xchg_step<1>(ev, ek); verify_xchg_step<2>(ev, ek); verify_xchg_step<4>(ev, ek);
		verify_xchg_step<8>(ev, ek); verify_xchg_step<16>(ev, ek); verify_xchg_step<32>(ev, ek);
		verify_xchg_step<1>(lv, lk); verify_xchg_step<2>(lv, lk); verify_xchg_step<4>(lv, lk);
		verify_xchg_step<8>(lv, lk); verify_xchg_step<16>(lv, lk); verify_xchg_step<32>(lv, lk);
	}
	if ((tid & 63) == 0) { r_v[2 * SLOT][tid >> 6] = ev; r_k[2 * SLOT][tid >> 6] = ek; r_v[2 * SLOT + 1][tid >> 6] = lv; r_k[2 * SLOT + 1][tid >> 6] = lk; }
}

// the six slots of one lane; nout may be a constant of the caller (the flag then stays in registers)
template <int FAM, int NZMAX, bool FIXED>
__device__ __forceinline__ void verify_point(const NtgDims &D, int nout, int t, bool live, bool first_tile, bool last_tile, const double *z,
                                             double (*r_v)[NTG_CHECK_NT / 64], long long (*r_k)[NTG_CHECK_NT / 64])
{
	using Fam = Family<FAM>;
	const FamCall<Fam> fam{ntg_prm_row<FAM>(), D.nnltc};
	const int P = D.P;
	verify_slot_wave<Fam, 0, NZMAX, FIXED>(fam, D.nicf > 0 && first_tile, nout, 1, t, P, z, D.icost_mask, live && t == 0, r_v, r_k);
	verify_slot_wave<Fam, 1, NZMAX, FIXED>(fam, D.nucf > 0, nout, 1, t, P, z, D.tcost_mask, live, r_v, r_k);
	verify_slot_wave<Fam, 2, NZMAX, FIXED>(fam, D.nfcf > 0 && last_tile, nout, 1, t, P, z, D.fcost_mask, live && t == P - 1, r_v, r_k);
	verify_slot_wave<Fam, 3, NZMAX, FIXED>(fam, Fam::NNLIC > 0 && D.nnlic > 0 && first_tile, nout, D.nnlic, t, P, z, D.icon_mask, live && t == 0, r_v, r_k);
	verify_slot_wave<Fam, 4, NZMAX, FIXED>(fam, Fam::NNLTC > 0 && D.nnltc > 0, nout, D.nnltc, t, P, z, D.tcon_mask, live, r_v, r_k);
	verify_slot_wave<Fam, 5, NZMAX, FIXED>(fam, Fam::NNLFC > 0 && D.nnlfc > 0 && last_tile, nout, D.nnlfc, t, P, z, D.fcon_mask, live && t == P - 1, r_v, r_k);
}

// cost.hpp's nout == n dispatch (flags of at most 8 outputs), as a chain of instances: a loop over n that the compiler declines to unroll
// would leave the count a run-time value
template <int FAM, int NZMAX, int N>
__device__ __forceinline__ void verify_dispatch(const NtgDims &D, int nout, int t, bool live, bool first_tile, bool last_tile, const double *z,
                                                double (*r_v)[NTG_CHECK_NT / 64], long long (*r_k)[NTG_CHECK_NT / 64])
{
	if (nout == N) verify_point<FAM, NZMAX, true>(D, N, t, live, first_tile, last_tile, z, r_v, r_k);
	else if constexpr (N < NZMAX / Family<FAM>::DM) verify_dispatch<FAM, NZMAX, N + 1>(D, nout, t, live, first_tile, last_tile, z, r_v, r_k);
}

template <int FAM, int NZMAX>
__global__ void __launch_bounds__(NTG_CHECK_NT)
verify_kernel(NtgDims D, NtgTables T, VerifyArgs va)
{
	using Fam = Family<FAM>;
	constexpr int NT = NTG_CHECK_NT, DM = Fam::DM, NOUTMAX = NZMAX / DM, NQ = 2 * NTG_VERIFY_NSLOT;
	extern __shared__ __attribute__((aligned(16))) char smem_raw[];
	__shared__ double r_v[NQ][NT / 64];
	__shared__ long long r_k[NQ][NT / 64];
	const CheckArgs &a = va.t;
	const TileLds s = tile_lds(smem_raw, D, a);
	const int tid = threadIdx.x, ntimes = a.ntimes, nout = D.nout;   // ntimes: the breakpoints, D.P
	const int tile0 = blockIdx.x * NT, nval = min(NT, ntimes - tile0);
	const bool live = tid < nval;
	const int tl = live ? tid : nval - 1, t = tile0 + tl;   // lanes past the end repeat the tile's last breakpoint and report nothing
	const bool first_tile = tile0 == 0, last_tile = tile0 + nval == ntimes;
	for (int bl = blockIdx.y; bl < a.nb; bl += gridDim.y) {
		const int b = a.b0 + bl;   // bl: problem within this launch (the per-problem time tables are indexed by it), b: problem of the batch
		tile_stage<FAM>(D, T, a, s, bl, b, tile0, nval, t);   // (its first barrier also ends the previous problem's reads of r_v / r_k)
		double z[NZMAX];   // flat flag of this lane's breakpoint
		tile_flag<DM, NZMAX>(D, a, s, bl, t, tl, z);
		if constexpr (NOUTMAX <= 8) {
			verify_dispatch<FAM, NZMAX, 1>(D, nout, t, live, first_tile, last_tile, z, r_v, r_k);
		} else {
			if (nout == NOUTMAX) verify_point<FAM, NZMAX, false>(D, NOUTMAX, t, live, first_tile, last_tile, z, r_v, r_k);
			else verify_point<FAM, NZMAX, false>(D, nout, t, live, first_tile, last_tile, z, r_v, r_k);
		}
		__syncthreads();
		if (tid < NQ) {
			double bv = r_v[tid][0]; long long bk = r_k[tid][0];
			for (int w = 1; w < NT / 64; w++) verify_take(bv, bk, r_v[tid][w], r_k[tid][w]);
			const size_t pi = ((size_t)b * gridDim.x + blockIdx.x) * NQ + tid;
			va.pval[pi] = bv; va.pkey[pi] = bk;
		}
	}
}

// what tile_launch (time_tile.hpp) asks of a time-tile kernel; the callbacks get the whole flag of DM nout entries
struct VerifyTile {
	using Args = VerifyArgs;
	static constexpr size_t LDS_MAX = NTG_VERIFY_LDS_MAX;
	static const CheckArgs &tile(const VerifyArgs &va) { return va.t; }
	template <int FAM, int NZMAX> static auto kernel() { return verify_kernel<FAM, NZMAX>; }
	template <class Fam> static bool refuses(const NtgDims &D)
	{
		return D.nz != Fam::DM * D.nout || D.nnlic > Fam::NNLIC || D.nnltc > Fam::NNLTC || D.nnlfc > Fam::NNLFC;
	}
};
