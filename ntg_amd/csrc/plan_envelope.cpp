// plan_envelope.cpp -- ntg_batch_envelope behind include/ntg_amd.h: what it refuses, the basis class of every linear trajectory row (from
// the host mirror of ltc), the LDS tables' layout and the launch.  The arithmetic is in envelope.hpp.  No family callback runs, so the call
// serves every built-in family and every loaded module, and reads no per-problem parameters.  It allocates nothing.
#include "plan_priv.hpp"

extern "C" int ntg_batch_envelope(const ntg_plan *p, int batch, const double *d_x, int nsub, const double *d_lower, const double *d_upper,
                                  double *d_lo, double *d_hi, double *d_row_lo, double *d_row_hi, double *d_viol, int *d_where, void *stream)
{
	if (!p) return fail(NTG_E_BADARG, "null plan");
	if (batch <= 0) return 0;
	if (!d_x) return fail(NTG_E_BADARG, "null argument");
	if (nsub < 0 || nsub > NTG_ENVELOPE_MAX_NSUB) return fail(NTG_E_BADARG, "nsub must lie in 0 .. " + std::to_string(NTG_ENVELOPE_MAX_NSUB));
	const bool want_v = d_viol || d_where, want_r = d_row_lo || d_row_hi || want_v;
	if (!d_lo && !d_hi && !want_r) return fail(NTG_E_BADARG, "no output asked for: pass d_lo, d_hi, d_row_lo, d_row_hi, d_viol or d_where");
	if (want_v && (!d_lower || !d_upper)) return fail(NTG_E_BADARG, "d_viol / d_where need the bounds d_lower and d_upper");
	const NtgDims &D = p->D;
	if (want_r && D.nltc == 0) return fail(NTG_E_BADARG, "the plan has no linear trajectory rows (nltc == 0)");
	if (p->grid_batch && batch != p->grid_batch) return fail(NTG_E_BADARG, "the plan carries per-problem grids for another batch size");
	if (D.family == NTG_FAM_HOST) return fail(NTG_E_UNSUPPORTED, "host-callback plans are not taken by the batch calls");
	if (want_r) {   // every row's polygon lives on the pieces of one basis class
		for (int i = 0; i < D.nltc; i++) {
			const double *row = p->h_linrows.data() + (size_t)(D.nlic + i) * D.nz;
			int first = -1;
			for (int o = 0; o < D.nout; o++)
				for (int r = 0; r < D.d[o]; r++) {
					if (row[D.iz[o] + r] == 0.0) continue;
					if (first < 0) first = o;
					else if (D.cls[o] != D.cls[first])
						return fail(NTG_E_UNSUPPORTED, "linear trajectory row " + std::to_string(i) + " names outputs " + std::to_string(first) + " and " + std::to_string(o) +
						                                   " of different basis classes: its envelope has no common pieces (the entry envelope d_lo / d_hi is still served)");
				}
		}
	}
	EnvArgs A{};
	A.nout = D.nout; A.nz = D.nz; A.nC = D.nC; A.nclass = D.nclass; A.batch = batch; A.nsub = nsub; A.nltc = D.nltc; A.nbounds = D.nbounds; A.slot0 = D.nlic;
	A.pp = p->grid_batch ? 1 : 0;
	for (int o = 0; o < D.nout; o++) { A.cls[o] = D.cls[o]; A.d[o] = D.d[o]; A.iC[o] = D.iC[o]; A.iz[o] = D.iz[o]; }
	for (int c = 0; c < D.nclass; c++) {
		EnvClass &C = A.c[c];
		C.k = D.cls_k[c]; C.m = D.cls_m[c]; C.l = D.cls_l[c];
		C.eoff = A.ne; A.ne += C.l * C.k * C.k;
		C.hoff = A.ne; A.ne += C.l;
		A.lmax = std::max(A.lmax, C.l); A.kmax = std::max(A.kmax, C.k);
		A.knots[c] = A.pp ? p->d_grid_knots : p->d_knots[c];
	}
	A.npc = A.lmax << nsub;
	if (ntg_envelope_lds(A) > NTG_ENVELOPE_LDS_MAX) return fail(NTG_E_UNSUPPORTED, "the extraction tables of this plan exceed 64 KiB of LDS");
	A.x = d_x; A.ltc = p->d_ltc; A.lower = d_lower; A.upper = d_upper;
	A.lo = d_lo; A.hi = d_hi; A.row_lo = d_row_lo; A.row_hi = d_row_hi; A.viol = d_viol; A.where = d_where;
	HIPCHK(hipSetDevice(p->device));
	HIPCHK(ntg_launch_envelope(A, plan_ncu(p), (hipStream_t)stream));
	return 0;
}
