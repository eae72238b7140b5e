// plan_build.cpp -- plan construction behind include/ntg_amd.h: the setup phase of ntg() (ntg.c:114-229) for one grid.  The spec is
// validated before anything is allocated; then the stages run in order -- basis classes and their tables (basis_kernel), channel tables
// and column forms, linear rows with (A A')^-1 and the projector, the structured-Newton tables -- each allocating through one DevOwner
// that the finished plan takes over.  Also here: the preconditioner (built on the first hessian = 1 solve) and the plan's queries.
// No numerical fallback lives on the host: it only factors the tiny (nclin x nclin) A A' and the preconditioner's blocks.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <utility>
#include "plan_priv.hpp"
#include "family_module.hpp"

// ---------------- small dense helpers (row-major, host) ----------------
bool chol_lower(std::vector<double> &a, int n)
{
	for (int j = 0; j < n; j++) {
		double d = a[(size_t)j * n + j];
		for (int k = 0; k < j; k++) d -= a[(size_t)j * n + k] * a[(size_t)j * n + k];
		if (!(d > 0.0)) return false;
		d = std::sqrt(d); a[(size_t)j * n + j] = d;
		for (int i = j + 1; i < n; i++) {
			double s = a[(size_t)i * n + j];
			for (int k = 0; k < j; k++) s -= a[(size_t)i * n + k] * a[(size_t)j * n + k];
			a[(size_t)i * n + j] = s / d;
		}
	}
	return true;
}
void chol_solve(const std::vector<double> &L, int n, double *b)
{
	for (int i = 0; i < n; i++) { double s = b[i]; for (int k = 0; k < i; k++) s -= L[(size_t)i * n + k] * b[k]; b[i] = s / L[(size_t)i * n + i]; }
	for (int i = n - 1; i >= 0; i--) { double s = b[i]; for (int k = i + 1; k < n; k++) s -= L[(size_t)k * n + i] * b[k]; b[i] = s / L[(size_t)i * n + i]; }
}

static void pad_if_empty(Sparse &s)
{
	s.nnz = (int)s.idx.size();
	if (s.idx.empty()) { s.idx.push_back(0); s.val.push_back(0.0); }
}
Sparse dense_to_csr(const double *A, int nr, int nc, const int *sel)
{
	Sparse s;
	s.ptr.assign(nr + 1, 0);
	for (int i = 0; i < nr; i++) {
		const double *row = A + (size_t)(sel ? sel[i] : i) * nc;
		for (int c = 0; c < nc; c++) if (row[c] != 0.0) { s.idx.push_back(c); s.val.push_back(row[c]); }
		s.ptr[i + 1] = (int)s.idx.size();
	}
	pad_if_empty(s);
	return s;
}
Sparse dense_to_csc(const double *A, int nr, int nc, const int *sel)
{
	Sparse s;
	s.ptr.assign(nc + 1, 0);
	for (int c = 0; c < nc; c++) {
		for (int i = 0; i < nr; i++) { const double v = A[(size_t)(sel ? sel[i] : i) * nc + c]; if (v != 0.0) { s.idx.push_back(i); s.val.push_back(v); } }
		s.ptr[c + 1] = (int)s.idx.size();
	}
	pad_if_empty(s);
	return s;
}

static u64 av_mask(const NtgDims &D, const ntg_av *av, int nav, bool *ok)
{
	u64 m = 0;
	for (int i = 0; i < nav; i++) {
		if (av[i].output < 0 || av[i].output >= D.nout || av[i].deriv < 0 || av[i].deriv >= D.d[av[i].output]) { *ok = false; continue; }
		m |= 1ull << (D.iz[av[i].output] + av[i].deriv);
	}
	return m;
}

// ---- stage 0: the spec is checked and the dimensions and masks derived from it, before anything is allocated ----
static int dims_from_spec(const ntg_spec *s, NtgDims &D)
{
	std::memset(&D, 0, sizeof(D));
	D.nout = s->nout; D.P = s->nbps; D.family = s->family;
	D.nlic = s->nlic; D.nltc = s->nltc; D.nlfc = s->nlfc;
	D.nnlic = s->nnlic; D.nnltc = s->nnltc; D.nnlfc = s->nnlfc;
	D.nicf = s->nicf; D.nucf = s->nucf; D.nfcf = s->nfcf;
	int nz = 0, nC = 0, sumk = 0;
	for (int o = 0; o < s->nout; o++) {
		const int k = s->order[o], m = s->mult[o], l = s->kninterv[o], d = s->maxderiv[o];
		if (k < 1 || k > NTG_MAX_ORDER || m < 0 || m >= k || l < 1 || d < 1 || d > k)
			return fail(NTG_E_BADARG, "bad spline spec (order<=NTG_MAX_ORDER, 0<=mult<order, 1<=maxderiv<=order)");
		D.order[o] = k; D.mult[o] = m; D.ninterv[o] = l; D.d[o] = d;
		D.ncoef[o] = l * (k - m) + m;                         // colloc.c:67
		D.iC[o] = nC; D.iz[o] = nz; D.koff[o] = sumk;         // colloc.c:41-49
		nC += D.ncoef[o]; nz += d; sumk += k;
	}
	if (nz > NTG_MAX_NZ) return fail(NTG_E_BADARG, "sum(maxderiv) exceeds NTG_MAX_NZ");
	D.nC = nC; D.nz = nz; D.sumk = sumk;
	D.nclin = s->nlic + s->nltc * s->nbps + s->nlfc;           // ntg.c:156
	D.ncnln = s->nnlic + s->nnltc * s->nbps + s->nnlfc;        // ntg.c:157
	D.nbounds = s->nlic + s->nltc + s->nlfc + s->nnlic + s->nnltc + s->nnlfc;
	const NtgFamily *fam = ntg_family(s->family);   // nullptr: the host-callback path, or unknown
	if (!fam && s->family != NTG_FAM_HOST) return fail(NTG_E_BADARG, "unknown problem family");
	if (fam && fam->shape) {   // built in: the family's own shape rule, with its text
		for (int o = 0; o < s->nout; o++)
			if (D.d[o] != fam->dm) return fail(NTG_E_UNSUPPORTED, "device family: wrong maxderiv (5 for the quadrotor family, 3 otherwise)");
		if (const char *why = fam->shape(*s)) return fail(NTG_E_BADARG, why);
	} else if (fam) {          // a module: the descriptor's limits
		const std::string who = std::string("family module ") + fam->name;
		for (int o = 0; o < s->nout; o++)
			if (D.d[o] != fam->dm) return fail(NTG_E_UNSUPPORTED, who + ": wrong maxderiv (the family has " + std::to_string(fam->dm) + ")");
		if (s->nnlic > fam->nnlic || s->nnltc > fam->nnltc || s->nnlfc > fam->nnlfc)
			return fail(NTG_E_BADARG, who + " has " + std::to_string(fam->nnlic) + "/" + std::to_string(fam->nnltc) + "/" + std::to_string(fam->nnlfc) +
			                              " nonlinear constraints (initial/trajectory/final)");
		if (fam->nout > 0 && s->nout != fam->nout) return fail(NTG_E_BADARG, who + " has " + std::to_string(fam->nout) + " outputs");
	}

	bool ok = true;
	D.icost_mask = av_mask(D, s->icostav, s->nicostav, &ok);
	D.tcost_mask = av_mask(D, s->tcostav, s->ntcostav, &ok);
	D.fcost_mask = av_mask(D, s->fcostav, s->nfcostav, &ok);
	D.icon_mask = av_mask(D, s->icav, s->nicav, &ok);
	D.tcon_mask = av_mask(D, s->tcav, s->ntcav, &ok);
	D.fcon_mask = av_mask(D, s->fcav, s->nfcav, &ok);
	if (!ok) return fail(NTG_E_BADARG, "active variable out of range");
	// rows of the running-cost gradient kept on chip: the declared trajectory-cost active
	// variables (device functors return zero elsewhere); every flag entry for host callbacks,
	// whose df[] the reference uses in full (cost.c:107-108)
	D.ntav = 0;
	for (int v = 0; v < NTG_MAX_NZ; v++) D.tav_row[v] = -1;
	for (int v = 0; v < nz; v++)
		if (s->family == NTG_FAM_HOST || ((D.tcost_mask >> v) & 1ull)) D.tav_row[v] = (signed char)D.ntav++;
	D.ntav_cost = D.ntav;   // the evaluation's cost pass touches these rows only; the augmented Lagrangian of the solve the ones below too
	for (int v = 0; v < nz; v++)
		if (D.tav_row[v] < 0 && ((D.tcon_mask >> v) & 1ull)) D.tav_row[v] = (signed char)D.ntav++;
	return 0;
}

// ---- stage 1: basis classes -- outputs with identical (knots, order, mult, maxderiv) share a table -- and their tables, from basis_kernel ----
static int build_basis(ntg_plan *p, const ntg_spec *s, DevOwner &own)
{
	NtgDims &D = p->D;
	p->h_knots.resize(s->nout);
	for (int o = 0; o < s->nout; o++) p->h_knots[o].assign(s->knots[o], s->knots[o] + s->kninterv[o] + 1);
	D.nclass = 0;
	std::vector<int> &rep = p->class_rep;
	int blk_total = 0;
	for (int o = 0; o < s->nout; o++) {
		int c = -1;
		for (int j = 0; j < D.nclass; j++) {
			const int r = rep[j];
			if (D.order[r] == D.order[o] && D.mult[r] == D.mult[o] && D.d[r] == D.d[o] && D.ninterv[r] == D.ninterv[o] &&
			    p->h_knots[r] == p->h_knots[o]) { c = j; break; }
		}
		if (c < 0) {
			c = D.nclass++;
			rep.push_back(o);
			D.cls_blk[c] = blk_total;
			D.cls_k[c] = D.order[o]; D.cls_d[c] = D.d[o]; D.cls_l[c] = D.ninterv[o]; D.cls_m[c] = D.mult[o];
			blk_total += s->nbps * D.order[o] * D.d[o];
		}
		D.cls[o] = c;
	}
	D.blk_total = blk_total;
	D.tav_rmask = 0;
	for (int o = 0; o < s->nout; o++) for (int r = 0; r < D.d[o]; r++) if (D.tav_row[D.iz[o] + r] >= 0) D.tav_rmask |= 1 << r;
	D.uniform = D.nclass == 1;
	for (int o = 1; o < s->nout; o++) if (D.ncoef[o] != D.ncoef[0]) D.uniform = 0;

	double *d_bps = nullptr, *d_blk = nullptr; int *d_off = nullptr;
	p->h_bps.assign(s->bps, s->bps + s->nbps);
	if (own.upload(&d_bps, s->bps, (size_t)s->nbps) || own.alloc(&d_blk, (size_t)blk_total) || own.alloc(&d_off, (size_t)D.nclass * s->nbps)) return NTG_E_HIP;
	for (int c = 0; c < D.nclass; c++) {
		const int o = rep[c];
		double *d_kn = nullptr;   // kept: ntg_batch_interp evaluates the basis at other times
		if (own.upload(&d_kn, p->h_knots[o].data(), p->h_knots[o].size())) return NTG_E_HIP;
		hipError_t e = ntg_launch_basis(1, D.ninterv[o], D.order[o], D.mult[o], D.d[o], s->nbps, d_kn, d_bps, 0, 0,
		                                d_blk + D.cls_blk[c], d_off + (size_t)c * s->nbps, nullptr);
		hipError_t e2 = hipDeviceSynchronize();
		p->d_knots.push_back(d_kn);
		if (e != hipSuccess || e2 != hipSuccess) return fail(NTG_E_HIP, "basis kernel failed");
	}
	p->h_blk.resize(blk_total); p->h_off.resize((size_t)D.nclass * s->nbps);
	if (hipMemcpy(p->h_blk.data(), d_blk, (size_t)blk_total * 8, hipMemcpyDeviceToHost) != hipSuccess ||
	    hipMemcpy(p->h_off.data(), d_off, p->h_off.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail(NTG_E_HIP, "reading the basis tables back failed");
	std::memset(&p->T, 0, sizeof(p->T));
	p->T.bps = d_bps; p->T.blk = d_blk; p->T.off = d_off;
	return 0;
}

// ---- stage 2: active (class, derivative) channels -- a derivative row is kept on chip only if some active variable (any of the six
//      lists) uses it; host callbacks use all of them -- by breakpoint (rowv) and by column (colp, and colv by value for class 0) ----
static int build_channels(ntg_plan *p, const ntg_spec *s, DevOwner &own)
{
	NtgDims &D = p->D;
	NtgTables &T = p->T;
	const std::vector<int> &rep = p->class_rep;
	const u64 all = D.icost_mask | D.tcost_mask | D.fcost_mask | D.icon_mask | D.tcon_mask | D.fcon_mask;
	std::vector<int> chrow((size_t)D.nclass * NTG_MAX_ORDER, -1), chcol((size_t)D.nclass * NTG_MAX_ORDER, -1);
	std::vector<double> rowv; std::vector<unsigned int> colp;
	if (s->nbps > 65535) return fail(NTG_E_UNSUPPORTED, "more than 65535 breakpoints");
	for (int c = 0; c < D.nclass; c++) {
		const int k = D.cls_k[c], dd = D.cls_d[c], P = s->nbps, nc = D.ncoef[rep[c]];
		const double *blk = p->h_blk.data() + D.cls_blk[c];
		const int *off = p->h_off.data() + (size_t)c * P;
		// support width of the column form (same for every derivative of the class)
		std::vector<int> cnt(nc, 0);
		for (int i = 0; i < P; i++) for (int q = 0; q < k; q++) cnt[off[i] + q]++;
		int W = 0; for (int v : cnt) W = std::max(W, v);
		const int W4 = (W + 3) & ~3;
		D.cls_W[c] = W4; D.cls_nc[c] = nc;
		for (int r = 0; r < dd; r++) {
			bool active = s->family == NTG_FAM_HOST;
			for (int o = 0; o < s->nout; o++) if (D.cls[o] == c && ((all >> (D.iz[o] + r)) & 1ull)) active = true;
			if (!active) continue;
			chrow[(size_t)c * NTG_MAX_ORDER + r] = (int)rowv.size();
			chcol[(size_t)c * NTG_MAX_ORDER + r] = (int)colp.size();
			for (int q = 0; q < k; q++) for (int i = 0; i < P; i++) rowv.push_back(blk[((size_t)i * k + q) * dd + r]);
			rowv.push_back(0.0);   // value index k*P: the zero the padding entries of a column point to
			// column cl: word 0 = its first breakpoint (the breakpoints of a column are consecutive because the block
			// offsets are non-decreasing), then W4 16-bit value indices q*P+i, two per word, padded with k*P
			if ((size_t)k * P >= 65535) return fail(NTG_E_UNSUPPORTED, "order*nbps exceeds the 16-bit column index");
			const size_t base = colp.size();
			const int WW = colp_words(W4);
			colp.resize(base + (size_t)WW * nc, 0u);
			std::vector<int> fill(nc, 0), first(nc, 0);
			std::vector<unsigned int> idx((size_t)nc * W4, (unsigned int)(k * P));
			for (int i = 0; i < P; i++) for (int q = 0; q < k; q++) {
				const int cl = off[i] + q, sidx = fill[cl]++;
				if (sidx == 0) first[cl] = i;
				else if (first[cl] + sidx != i) return fail(NTG_E_UNSUPPORTED, "breakpoints of a basis function are not consecutive");
				idx[(size_t)cl * W4 + sidx] = (unsigned int)(q * P + i);
			}
			for (int cl = 0; cl < nc; cl++) {
				unsigned int *w = &colp[base + (size_t)cl * WW];
				w[0] = (unsigned int)first[cl];
				for (int s2 = 0; s2 < W4; s2++) w[1 + s2 / 2] |= idx[(size_t)cl * W4 + s2] << (16 * (s2 & 1));
			}
		}
	}
	// the same columns by value (class 0; see NtgDims::colv_total)
	{
		std::vector<double> colv;
		const int c = 0, nc = D.ncoef[rep[c]], W4 = D.cls_W[c], WW = colp_words(W4);
		D.colv_stride = W4 + 2;
		for (int r = 0; r < NTG_MAX_ORDER; r++) D.ch_colv0[r] = -1;
		for (int r = 0; r < D.cls_d[c]; r++) {
			if (chcol[(size_t)c * NTG_MAX_ORDER + r] < 0) continue;
			D.ch_colv0[r] = (int)colv.size();
			const double *rv = rowv.data() + chrow[(size_t)c * NTG_MAX_ORDER + r];
			for (int cl = 0; cl < nc; cl++) {
				const unsigned int *w = &colp[(size_t)chcol[(size_t)c * NTG_MAX_ORDER + r] + (size_t)cl * WW];
				for (int s2 = 0; s2 < W4; s2++) colv.push_back(rv[(w[1 + s2 / 2] >> (16 * (s2 & 1))) & 0xffffu]);
				colv.push_back((double)w[0]);
				colv.push_back(0.0);
			}
		}
		D.colv_total = (int)colv.size();
		if (colv.empty()) colv.push_back(0.0);
		if (own.upload(&T.colv, colv.data(), colv.size())) return NTG_E_HIP;
	}
	// breakpoint groups of class 0 (NtgDims::ig_n)
	{
		const int P = s->nbps; const int *off = p->h_off.data();
		int n = 0; bool ok = true;
		for (int i = 0; i < P && ok;) { int j = i; while (j < P && off[j] == off[i]) j++; if (n >= 64 || j - i > 6) ok = false; else D.igb[n++] = (unsigned short)i; i = j; }
		D.ig_n = ok ? n : 0;
		if (ok) D.igb[n] = (unsigned short)P;
	}
	D.row_total = (int)rowv.size(); D.col_total = (int)colp.size();
	if (colp.empty()) colp.push_back(0);
	if (own.upload(&T.rowv, rowv.data(), rowv.size()) || own.upload(&T.colp, colp.data(), colp.size()) ||
	    own.upload(&T.chrow, chrow.data(), chrow.size()) || own.upload(&T.chcol, chcol.data(), chcol.size())) return NTG_E_HIP;
	p->h_chrow = chrow;
	for (int r = 0; r < NTG_MAX_ORDER; r++) { D.ch_row0[r] = chrow[r]; D.ch_col0[r] = chcol[r]; }
	return 0;
}

// ---- stage 3b: the projector Q = A'(AA')^-1 A.  Only the coefficients some constraint touches have a non-zero row; those rows are kept
//      as ELL (zero padded) when that is small ----
static int build_projector(ntg_plan *p, const std::vector<double> &Ad, const std::vector<double> &Sinv, DevOwner &own)
{
	NtgDims &D = p->D;
	NtgTables &T = p->T;
	const int m = D.mE, nC = D.nC;
	std::vector<double> SA((size_t)m * nC, 0.0), Q((size_t)nC * nC, 0.0);
	for (int i = 0; i < m; i++) for (int j = 0; j < m; j++) { const double sij = Sinv[(size_t)i * m + j]; if (sij != 0.0) for (int c = 0; c < nC; c++) SA[(size_t)i * nC + c] += sij * Ad[(size_t)j * nC + c]; }
	for (int i = 0; i < m; i++) for (int a = 0; a < nC; a++) { const double aia = Ad[(size_t)i * nC + a]; if (aia != 0.0) for (int c = 0; c < nC; c++) Q[(size_t)a * nC + c] += aia * SA[(size_t)i * nC + c]; }
	std::vector<short> qidx(nC, -1); int nt = 0, w = 0;
	for (int a = 0; a < nC; a++) { int cnt = 0; for (int c = 0; c < nC; c++) if (Q[(size_t)a * nC + c] != 0.0) cnt++; if (cnt) { qidx[a] = (short)std::min(nt, 32000); nt++; w = std::max(w, cnt); } }
	if (!(nt > 0 && nt < 32000 && (size_t)nt * w * 12 + (size_t)nC * 2 <= 16 * 1024)) return 0;
	std::vector<int> qcol((size_t)nt * w, 0); std::vector<double> qval((size_t)nt * w, 0.0);
	for (int a = 0; a < nC; a++) if (qidx[a] >= 0) { int e = 0; for (int c = 0; c < nC; c++) if (Q[(size_t)a * nC + c] != 0.0) { qcol[(size_t)qidx[a] * w + e] = c; qval[(size_t)qidx[a] * w + e] = Q[(size_t)a * nC + c]; e++; } }
	if (own.upload(&T.q_idx, qidx.data(), qidx.size()) || own.upload(&T.q_col, qcol.data(), qcol.size()) || own.upload(&T.q_val, qval.data(), qval.size())) return NTG_E_HIP;
	D.q_use = 1; D.q_nt = nt; D.q_w = w;
	// Rows that pin whole coefficients (the usual initial / final conditions: a derivative at an end point touches the first /
	// last r + 1 coefficients only): range(A') is spanned by m unit vectors and Q is the identity on those coefficients, zero
	// elsewhere -- g - Q g just zeroes the pinned entries (NtgDims::q_pin, used by the wave kernel).  Decided on the computed Q
	// itself, to 1e-9 (the accuracy (A A')^-1 gives it is ~1e-10): the reference's cumulative-add linspace (ntg.c:374-389) puts
	// the last breakpoint an ulp or two off the last knot, so rows of ~1e-15 for the neighbouring coefficients exist too.
	int npin = 0; double dev = 0.0;
	std::vector<unsigned char> pinned(nC, 0);
	for (int a = 0; a < nC; a++) if (qidx[a] >= 0) {
		const bool pin = Q[(size_t)a * nC + a] > 0.5;
		npin += pin ? 1 : 0; pinned[a] = pin ? 1 : 0;
		for (int c = 0; c < nC; c++) dev = std::max(dev, std::fabs(Q[(size_t)a * nC + c] - ((pin && a == c) ? 1.0 : 0.0)));
	}
	D.q_pin = (npin == m && dev <= 1e-9) ? 1 : 0;
	if (D.q_pin && own.upload(&T.q_pinned, pinned.data(), pinned.size())) return NTG_E_HIP;
	if (getenv("NTG_AMD_DEBUG_PLAN")) fprintf(stderr, "projector: %d non-zero rows, %d equality rows, width %d, %d pinned, max |Q - I_pinned| %.3e -> q_pin %d\n", nt, m, w, npin, dev, D.q_pin);
	p->h_qidx = qidx; p->h_qcol = qcol; p->h_qval = qval;
	return 0;
}

// ---- stage 3: linear constraint rows on the device (linrows_kernel), split into equality and inequality rows, (A A')^-1 on the host ----
static int build_linear(ntg_plan *p, const ntg_spec *s, DevOwner &own)
{
	NtgDims &D = p->D;
	NtgTables &T = p->T;
	const int nz = D.nz, nC = D.nC;
	{
		DevOwner tmp;   // the user's rows: needed by the kernel only
		double *d_lic = nullptr, *d_ltc = nullptr, *d_lfc = nullptr, *d_ab = nullptr; int *d_rbp = nullptr;
		if (tmp.upload(&d_lic, s->lic, (size_t)s->nlic * nz) || tmp.upload(&d_ltc, s->ltc, (size_t)s->nltc * nz) || tmp.upload(&d_lfc, s->lfc, (size_t)s->nlfc * nz) ||
		    own.alloc(&d_ab, (size_t)D.nclin * D.sumk) || own.alloc(&d_rbp, (size_t)D.nclin)) return NTG_E_HIP;
		hipError_t e = ntg_launch_linrows(D, T, d_lic, d_ltc, d_lfc, d_ab, d_rbp, nullptr);
		hipError_t e2 = hipDeviceSynchronize();
		tmp.free_all();
		if (e != hipSuccess || e2 != hipSuccess) return fail(NTG_E_HIP, "linrows kernel failed");
		p->h_aband.resize((size_t)D.nclin * D.sumk); p->h_rbp.resize(D.nclin);
		if (hipMemcpy(p->h_aband.data(), d_ab, p->h_aband.size() * 8, hipMemcpyDeviceToHost) != hipSuccess ||
		    hipMemcpy(p->h_rbp.data(), d_rbp, p->h_rbp.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail(NTG_E_HIP, "reading the linear rows back failed");
		T.aband = d_ab; T.rbp = d_rbp;
	}
	// dense rows; split into the equality rows (kept satisfied by projection) and the rows declared as
	// inequalities (spec->lin_ineq, handled by the augmented-Lagrangian loop like nonlinear rows)
	const int mall = D.nclin;
	std::vector<double> Aall((size_t)mall * nC, 0.0);
	ntg_plan_dense_A(p, Aall.data());
	std::vector<int> erow, irow, rowmap(mall), linflag((size_t)std::max(1, s->nlic + s->nltc + s->nlfc), 0);
	for (int r = 0; r < mall; r++) {
		const int slot = lin_row(D, r).slot;
		const bool ineq = s->lin_ineq && s->lin_ineq[slot] != 0;
		linflag[slot] = ineq ? 1 : 0;
		if (ineq) { rowmap[r] = -(int)irow.size() - 1; irow.push_back(r); } else { rowmap[r] = (int)erow.size(); erow.push_back(r); }
	}
	const int m = (int)erow.size(), nI = (int)irow.size();
	D.mE = m; D.nI = nI;
	std::vector<double> Ad((size_t)std::max(m, 1) * nC, 0.0);
	for (int i = 0; i < m; i++) std::copy(&Aall[(size_t)erow[i] * nC], &Aall[(size_t)erow[i] * nC] + nC, &Ad[(size_t)i * nC]);
	if (erow.empty()) erow.push_back(0);
	if (own.upload(&T.erow, erow.data(), erow.size()) || own.upload(&T.rowmap, rowmap.data(), rowmap.size()) || own.upload(&T.linflag, linflag.data(), linflag.size())) return NTG_E_HIP;
	if (nI > 0) {   // inequality rows: CSR (c = A_r x) and CSC (g += A_r' t)
		const Sparse R = dense_to_csr(Aall.data(), nI, nC, irow.data()), C = dense_to_csc(Aall.data(), nI, nC, irow.data());
		if (own.upload(&T.irow, irow.data(), irow.size()) || own.upload(&T.icsr_ptr, R.ptr.data(), R.ptr.size()) ||
		    own.upload(&T.icsr_col, R.idx.data(), R.idx.size()) || own.upload(&T.icsr_val, R.val.data(), R.val.size()) ||
		    own.upload(&T.icsc_ptr, C.ptr.data(), C.ptr.size()) || own.upload(&T.icsc_row, C.idx.data(), C.idx.size()) ||
		    own.upload(&T.icsc_val, C.val.data(), C.val.size())) return NTG_E_HIP;
		p->h_irow = irow; p->h_icsr_ptr = R.ptr; p->h_icsr_col = R.idx; p->h_icsc_ptr = C.ptr; p->h_icsc_row = C.idx;
	}
	// S = A_E A_E' -> S^-1
	std::vector<double> S((size_t)m * m, 0.0);
	for (int i = 0; i < m; i++) for (int j = 0; j <= i; j++) {
		double a = 0.0;
		for (int c = 0; c < nC; c++) a += Ad[(size_t)i * nC + c] * Ad[(size_t)j * nC + c];
		S[(size_t)i * m + j] = a; S[(size_t)j * m + i] = a;
	}
	p->lin_ok = chol_lower(S, m);
	std::vector<double> Sinv((size_t)m * m, 0.0), col(m);
	if (p->lin_ok) {
		for (int j = 0; j < m; j++) {
			std::fill(col.begin(), col.end(), 0.0); col[j] = 1.0;
			chol_solve(S, m, col.data());
			for (int i = 0; i < m; i++) Sinv[(size_t)i * m + j] = col[i];
		}
		for (int i = 0; i < m; i++) for (int j = 0; j < i; j++) { // symmetrise
			const double a = 0.5 * (Sinv[(size_t)i * m + j] + Sinv[(size_t)j * m + i]);
			Sinv[(size_t)i * m + j] = a; Sinv[(size_t)j * m + i] = a;
		}
	}
	if (own.upload(&T.sinv, Sinv.data(), Sinv.size())) return NTG_E_HIP;
	// sparse A_E (a unit lic row touches one output, and a derivative at an end point touches only the first/last r+1 coefficients),
	// then (A A')^-1 as CSR (block diagonal when constraint rows decouple)
	const Sparse R = dense_to_csr(Ad.data(), m, nC), C = dense_to_csc(Ad.data(), m, nC), SI = dense_to_csr(Sinv.data(), m, m);
	D.lin_nnz = R.nnz; D.sinv_nnz = SI.nnz;
	if (own.upload(&T.csr_ptr, R.ptr.data(), R.ptr.size()) || own.upload(&T.csr_col, R.idx.data(), R.idx.size()) ||
	    own.upload(&T.csr_val, R.val.data(), R.val.size()) || own.upload(&T.csc_ptr, C.ptr.data(), C.ptr.size()) ||
	    own.upload(&T.csc_row, C.idx.data(), C.idx.size()) || own.upload(&T.csc_val, C.val.data(), C.val.size()) ||
	    own.upload(&T.sinv_ptr, SI.ptr.data(), SI.ptr.size()) || own.upload(&T.sinv_col, SI.idx.data(), SI.idx.size()) ||
	    own.upload(&T.sinv_val, SI.val.data(), SI.val.size())) return NTG_E_HIP;
	p->h_csr_ptr = R.ptr; p->h_csr_col = R.idx; p->h_csc_ptr = C.ptr; p->h_csc_row = C.idx; p->h_erow = erow;
	p->h_sinv_ptr = SI.ptr; p->h_sinv_col = SI.idx;
	if (int rc = build_projector(p, Ad, Sinv, own)) return rc;
	// the general three-step operator (A g, (AA')^-1, A' lam) is staged in LDS only when Q is not used
	D.lin_lds = (!D.q_use && ((size_t)D.lin_nnz * 24 + (size_t)D.sinv_nnz * 12 + (size_t)(2 * m + nC + 3) * 4) <= 24 * 1024) ? 1 : 0;
	p->h_Adense.swap(Aall);
	p->h_AE.swap(Ad);
	return 0;
}

static int build_newton_tables(ntg_plan *p, DevOwner &own);

extern "C" int ntg_plan_create(const ntg_spec *s, int device, ntg_plan **out)
{
	if (!s || !out) return fail(NTG_E_BADARG, "null spec");
	*out = nullptr;
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
		return fail(NTG_E_NODEVICE, "no HIP device: libntg_amd has no CPU path");
	if (device < 0 || device >= ndev) return fail(NTG_E_BADARG, "bad device index");
	if (s->nout < 1 || s->nout > NTG_MAX_OUT) return fail(NTG_E_BADARG, "nout out of range (1..NTG_MAX_OUT)");
	if (s->nbps < 2) return fail(NTG_E_BADARG, "need at least 2 breakpoints");
	HIPCHK(hipSetDevice(device));
	NtgDims D0;
	if (int rc = dims_from_spec(s, D0)) return rc;

	// from here on a failure is a plain return: the plan goes with its allocations, and so does what `own` holds and the plan has not taken over
	std::unique_ptr<ntg_plan, void (*)(ntg_plan *)> plan(new ntg_plan(), ntg_plan_destroy);
	ntg_plan *p = plan.get();
	DevOwner own;
	p->device = device;
	p->D = D0;
	if (int rc = build_basis(p, s, own)) return rc;
	if (int rc = build_channels(p, s, own)) return rc;
	if (p->D.nclin > 0) { if (int rc = build_linear(p, s, own)) return rc; }
	else p->lin_ok = true;
	const int nz = p->D.nz;
	if (s->nlic > 0 && own.upload(&p->d_lic, s->lic, (size_t)s->nlic * nz)) return NTG_E_HIP;   // kept for the receding-horizon shift
	if (s->nltc > 0 && own.upload(&p->d_ltc, s->ltc, (size_t)s->nltc * nz)) return NTG_E_HIP;   // kept for ntg_batch_check
	p->h_linrows.assign((size_t)(s->nlic + s->nltc + s->nlfc) * nz, 0.0);   // the user's rows, stacked [nlic | nltc | nlfc][nz]
	if (s->nlic > 0) std::copy(s->lic, s->lic + (size_t)s->nlic * nz, p->h_linrows.begin());
	if (s->nltc > 0) std::copy(s->ltc, s->ltc + (size_t)s->nltc * nz, p->h_linrows.begin() + (size_t)s->nlic * nz);
	if (s->nlfc > 0) std::copy(s->lfc, s->lfc + (size_t)s->nlfc * nz, p->h_linrows.begin() + (size_t)(s->nlic + s->nltc) * nz);
	// keep what the preconditioner build needs
	p->tcostav.assign(s->tcostav, s->tcostav + s->ntcostav);
	p->icostav.assign(s->icostav, s->icostav + s->nicostav);
	p->fcostav.assign(s->fcostav, s->fcostav + s->nfcostav);
	if (build_newton_tables(p, own)) return NTG_E_HIP;
	own.release_into(p->owned);
	*out = plan.release();
	return 0;
}

// ---- structured Newton mode (newton.hpp): does the plan qualify, and its batch-shared tables ----
// Qualifies when: the family offers the per-group second-order blocks (couple > 0 in its descriptor: Family::COUPLE / CG / GROUP_VARS), one
// spline spec for every output, only trajectory nonlinear rows on exactly the flag entries the family's block covers, no
// linear inequality rows, and equality rows that pin a square invertible block of coefficients (the usual initial / final
// conditions): then null(A_E) = {pinned coefficients = 0} and the reduced Hessian is a principal submatrix of the band.

// What the rule leaves behind for the tables: coupling groups, free outputs and the maps between coefficients and free entries
struct NwtShape {
	int go, cg, ngrp, nfo, ng, ngf; u64 gmask;
	std::vector<char> pinned; std::vector<int> map, pos;   // NtgTables::nwt_map / nwt_pos; the free outputs' entries follow the groups'
};

// the family's block, the plan's shape, the pinned coefficients and the free entries' order; false: the mode does not apply
static bool nwt_shape(const ntg_plan *p, NwtShape &S)
{
	const NtgDims &D = p->D;
	const int dm = D.d[0];
	const NtgFamily *fam = ntg_family(D.family);
	if (!fam || fam->couple == 0) return false;
	S.go = fam->couple; S.cg = fam->cg; S.gmask = fam->group_mask;
	if (!D.uniform || D.nI > 0 || D.nnlic || D.nnlfc || D.nnltc <= 0 || !p->lin_ok) return false;
	// coupling groups; outputs left over appear in no row: FREE outputs -- their block of the model is the cost model's, the same for
	// every problem and every refresh, factored once here (nwt_lf) and solved by an otherwise idle wave
	const int go = S.go, ngrp = D.nout / go, nfo = D.nout - ngrp * go;
	S.ngrp = ngrp; S.nfo = nfo;
	if (ngrp < 1 || (nfo && !fam->free_outputs_ok)) return false;
	const int k = D.order[0], nco = D.ncoef[0], n = D.nC, m = D.mE;
	if (k * go - 1 > 32 || ngrp + nfo > 8) return false;
	u64 want = 0;
	for (int g = 0; g < ngrp; g++) want |= S.gmask << (dm * go * g);
	if (D.tcon_mask != want) return false;
	// pinned coefficients = the columns the equality rows touch; they must form a square system
	std::vector<char> &pinned = S.pinned;
	pinned.assign(n, 0);
	int npin = 0;
	// (entries at rounding level do not count: the last breakpoint of a cumulative-add linspace (ntg.c:385-388) may lie an ulp
	// past the last knot, where the spline is extrapolated and the other basis functions are ~1e-16 instead of 0; the solve
	// re-projects x and every direction onto A x = b anyway)
	for (int i = 0; i < m; i++) {
		double big = 0.0;
		for (int c = 0; c < n; c++) big = std::max(big, std::fabs(p->h_AE[(size_t)i * n + c]));
		for (int c = 0; c < n; c++) if (std::fabs(p->h_AE[(size_t)i * n + c]) > 1e-10 * big && !pinned[c]) { pinned[c] = 1; npin++; }
	}
	if (npin != m) return false;
	std::vector<int> &map = S.map, &pos = S.pos;
	pos.assign(n, -1);
	int ng = -1;
	for (int g = 0; g < ngrp; g++) {
		int cnt = 0;
		for (int cl = 0; cl < nco; cl++) for (int o = g * go; o < (g + 1) * go; o++) {
			const int c = D.iC[o] + cl;
			if (pinned[c]) continue;
			pos[c] = g * 1000000 + cnt; map.push_back(c); cnt++;
		}
		if (ng < 0) ng = cnt; else if (cnt != ng) return false;
	}
	if (ng < 1) return false;
	for (int c = 0; c < n; c++) if (pos[c] >= 0) pos[c] = (pos[c] / 1000000) * ng + pos[c] % 1000000;
	// free outputs: their free coefficients follow the groups' in the maps, output by output (ngf each)
	int ngf = 0;
	for (int f = 0; f < nfo; f++) {
		int cnt = 0;
		for (int cl = 0; cl < nco; cl++) {
			const int c = D.iC[ngrp * go + f] + cl;
			if (pinned[c]) continue;
			pos[c] = -2 - cnt; map.push_back(c); cnt++;   // provisional: -2 - index inside the output
		}
		if (f == 0) ngf = cnt; else if (cnt != ngf) return false;
	}
	if (nfo && ngf < 1) return false;
	for (int f = 0; f < nfo; f++) for (int cl = 0; cl < nco; cl++) { const int c = D.iC[ngrp * go + f] + cl; if (pos[c] <= -2) pos[c] = ngrp * ng + f * ngf + (-2 - pos[c]); }
	S.ng = ng; S.ngf = ngf;
	return true;
}

// ---- tables of the QP-based SQP step's regime without constraint curvature (NtgTables::nwt_tu, nwt_g): K0 is then the model of every
//      major iteration of every problem, so K0^-1 M_i' per breakpoint and M_k K0^-1 M_i' per pair of breakpoints are plan constants.
//      Built when all coupling groups share one cost model and the tables stay under 48 MB (tu, gt stay empty otherwise). ----
static void nwt_qp_tables(const ntg_plan *p, const NwtShape &S, const std::vector<double> &k0, u64 upack, std::vector<double> &tu, std::vector<double> &gt)
{
	const NtgDims &D = p->D;
	const int go = S.go, cg = S.cg, ngrp = S.ngrp, ng = S.ng, k = D.order[0], dm = D.d[0], P = D.P, hb = k * go - 1, ld = hb + 1;
	const int *off = p->h_off.data();
	const double *blk = p->h_blk.data();
	bool same = true;
	for (int g = 1; g < ngrp && same; g++) for (size_t e = 0; e < (size_t)ng * ld; e++) if (k0[(size_t)g * ng * ld + e] != k0[e]) { same = false; break; }
	const size_t ntu = (size_t)P * cg * ng, ngt2 = (size_t)P * P * cg * cg;
	if (!same || (ntu + ngt2) * 8 > (size_t)48 << 20 || getenv("NTG_AMD_NO_QPTAB")) return;
	// band Cholesky of K0 (group 0), compact lower band: L(i, j) at l[i * ld + (j - i + hb)]
	std::vector<double> l(k0.begin(), k0.begin() + (size_t)ng * ld);
	auto L = [&](int i, int j) -> double & { return l[(size_t)i * ld + (j - i + hb)]; };
	for (int j = 0; j < ng; j++) {
		double d = L(j, j);
		for (int t = std::max(0, j - hb); t < j; t++) d -= L(j, t) * L(j, t);
		if (!(d > 0.0)) return;
		d = std::sqrt(d); L(j, j) = d;
		for (int i = j + 1; i <= std::min(ng - 1, j + hb); i++) {
			double sv = L(i, j);
			for (int t = std::max(0, i - hb); t < j; t++) sv -= L(i, t) * L(j, t);
			L(i, j) = sv / d;
		}
	}
	tu.assign(ntu, 0.0); gt.assign(ngt2, 0.0);
	std::vector<int> uo(cg), ur(cg);
	for (int u = 0; u < cg; u++) { uo[u] = (int)((upack >> (8 * u + 4)) & 15u); ur[u] = (int)((upack >> (8 * u)) & 15u); }
	const int clo = D.nwt_clo, chi = D.nwt_chi;
	for (int i = 0; i < P; i++) for (int u = 0; u < cg; u++) {
		double *t = tu.data() + ((size_t)i * cg + u) * ng;
		for (int q = 0; q < k; q++) { const int cl = off[i] + q; if (cl >= clo && cl < chi) t[(cl - clo) * go + uo[u]] = blk[((size_t)i * k + q) * dm + ur[u]]; }
		for (int r = 0; r < ng; r++) { double sv = t[r]; for (int c2 = std::max(0, r - hb); c2 < r; c2++) sv -= L(r, c2) * t[c2]; t[r] = sv / L(r, r); }
		for (int r = ng - 1; r >= 0; r--) { double sv = t[r]; for (int c2 = r + 1; c2 <= std::min(ng - 1, r + hb); c2++) sv -= L(c2, r) * t[c2]; t[r] = sv / L(r, r); }
	}
	for (int kb = 0; kb < P; kb++) for (int i = 0; i < P; i++) for (int v = 0; v < cg; v++) for (int u = 0; u < cg; u++) {
		const double *t = tu.data() + ((size_t)i * cg + u) * ng;
		double sv = 0.0;
		for (int q = 0; q < k; q++) { const int cl = off[kb] + q; if (cl >= clo && cl < chi) sv += blk[((size_t)kb * k + q) * dm + ur[v]] * t[(cl - clo) * go + uo[v]]; }
		gt[(((size_t)kb * P + i) * cg + v) * cg + u] = sv;
	}
}

static int build_newton_tables(ntg_plan *p, DevOwner &own)
{
	NtgDims &D = p->D;
	NtgTables &T = p->T;
	D.nwt_on = 0; D.nwt_tab = 0; T.nwt_tu = T.nwt_g = nullptr;
	NwtShape S;
	if (!nwt_shape(p, S)) return 0;
	const int go = S.go, cg = S.cg, ngrp = S.ngrp, nfo = S.nfo, ng = S.ng, ngf = S.ngf, dm = D.d[0];
	const std::vector<int> &pos = S.pos;
	const int k = D.order[0], nco = D.ncoef[0], P = D.P, hb = k * go - 1, hbf = k - 1;
	// breakpoint range of every local coefficient, from the block offsets (consecutive: checked when the column form was built)
	std::vector<short> lo(nco, (short)P), hi(nco, 0);
	const int *off = p->h_off.data();
	for (int i = 0; i < P; i++) for (int q = 0; q < k; q++) { const int cl = off[i] + q; lo[cl] = (short)std::min<int>(lo[cl], i); hi[cl] = (short)std::max<int>(hi[cl], i + 1); }
	// cost model: 2 w_i on the trajectory-cost variables, 2 on the initial / final ones (diagonal in the flag: same output only)
	const int ld = hb + 1;
	std::vector<double> k0((size_t)ngrp * ng * ld, 0.0);
	const int ldf = hbf + 1;
	std::vector<double> k0f((size_t)nfo * ngf * ldf, 0.0);   // cost model of the free outputs (band of half width k - 1 each)
	const double *blk = p->h_blk.data();
	for_cost_terms(p, p->h_bps.data(), 2.0, [&](const std::vector<ntg_av> &av, int bp, double w) {
		for (const ntg_av &a : av) {
			const int o = a.output, r = a.deriv, g = o / go;
			for (int q1 = 0; q1 < k; q1++) for (int q2 = 0; q2 < k; q2++) {
				const int c1 = D.iC[o] + off[bp] + q1, c2 = D.iC[o] + off[bp] + q2;
				if (pos[c1] < 0 || pos[c2] < 0) continue;
				const double v = w * blk[((size_t)bp * k + q1) * dm + r] * blk[((size_t)bp * k + q2) * dm + r];
				if (o >= ngrp * go) {
					const int f = o - ngrp * go, p1 = pos[c1] - ngrp * ng - f * ngf, p2 = pos[c2] - ngrp * ng - f * ngf;
					if (p1 >= p2) k0f[((size_t)f * ngf + p1) * ldf + (p2 - p1 + hbf)] += v;
					continue;
				}
				const int p1 = pos[c1] - g * ng, p2 = pos[c2] - g * ng;
				if (p1 < p2) continue;
				k0[((size_t)g * ng + p1) * ld + (p2 - p1 + hb)] += v;
			}
		}
	});
	// breakpoint groups and colours; constraint flag entries of a group
	std::vector<int> ig;
	for (int i = 0; i < P;) { int j = i; while (j < P && off[j] == off[i]) j++; ig.push_back(i); ig.push_back(j - i); i = j; }
	const int nint = (int)ig.size() / 2;
	int cover = 1;
	for (int cl = 0; cl < nco; cl++) { int cnt = 0; for (int t = 0; t < nint; t++) { const int of = off[ig[2 * t]]; if (cl >= of && cl < of + k) cnt++; } cover = std::max(cover, cnt); }
	for (int t = 0; t + cover < nint; t++) if (off[ig[2 * (t + cover)]] < off[ig[2 * t]] + k) return 0;   // same-colour groups must not share coefficients
	u64 upack = 0;
	{
		int u = 0;
		for (int o = 0; o < go; o++) for (int r = 0; r < dm; r++) if ((S.gmask >> (dm * o + r)) & 1ull) { upack |= (u64)((o << 4) | r) << (8 * u); u++; }
		if (u != cg || cg > 8) return 0;
	}
	if (D.ig_n != nint) return 0;   // more than 64 groups or more than 6 breakpoints in one (see NtgDims::ig_n)
	D.nwt_nint = nint; D.nwt_cover = cover; D.nwt_upack = upack;
	// the free coefficients must be the same contiguous range [clo, chi) of every output (pinned ends)
	{
		int clo = -1, chi = -1;
		for (int cl = 0; cl < nco; cl++) if (!S.pinned[D.iC[0] + cl]) { if (clo < 0) clo = cl; chi = cl + 1; }
		if (clo < 0) return 0;
		for (int o = 0; o < D.nout; o++) for (int cl = 0; cl < nco; cl++) if ((bool)S.pinned[D.iC[o] + cl] != !(cl >= clo && cl < chi)) return 0;
		D.nwt_clo = clo; D.nwt_chi = chi;
	}
	std::vector<double> tu, gt;
	nwt_qp_tables(p, S, k0, upack, tu, gt);
	// two-sided factorisation: two waves per group when the band is long enough and the largest workgroup has the waves (newton.hpp).  The
	// cost model is then split like the band: rows of the top part and the separator stay where they are, the entries of bottom rows move
	// to the reversed array (entry (i, j) -> row n - 1 - j, same band offset), which follows the groups' top arrays in the table.
	D.nwt_tw = 0; D.nwt_ja = D.nwt_jb = 0;
	// (only while every working wave still has a SIMD of its own: with four groups -- config E, eight waves -- the second wave of a group
	// shares its SIMD with another group's, both streams are issue bound, and the measured solve was 16 % SLOWER)
	if (ng >= 128 && 2 * ngrp + nfo <= 4 && !getenv("NTG_AMD_NO_TWOSIDED")) {
		const int jt = (ng - 32) / 16;
		D.nwt_tw = 1; D.nwt_ja = (jt + 1) / 2; D.nwt_jb = jt / 2;
		const int sepn = ng - 16 * (D.nwt_ja + D.nwt_jb), ngt = 16 * D.nwt_ja + sepn, brows = 16 * D.nwt_jb + 48;
		std::vector<double> kb((size_t)ngrp * brows * ld, 0.0);
		for (int g = 0; g < ngrp; g++)
			for (int i = ngt; i < ng; i++) for (int e = 0; e <= hb; e++) {
				const int j = i - hb + e;
				double &src = k0[((size_t)g * ng + i) * ld + e];
				if (j >= 0) kb[((size_t)g * brows + (ng - 1 - j)) * ld + e] = src;
				src = 0.0;
			}
		k0.insert(k0.end(), kb.begin(), kb.end());
	}
	// the free outputs' factor, in the layout nwt_solve_wave reads (row-major band, the diagonal inverted)
	std::vector<double> lf((size_t)nfo * ngf * ldf, 0.0);
	for (int f = 0; f < nfo; f++) {
		std::vector<double> a((size_t)ngf * ngf, 0.0);
		for (int i = 0; i < ngf; i++) for (int e = 0; e <= hbf; e++) { const int j = i - hbf + e; if (j >= 0) a[(size_t)i * ngf + j] = a[(size_t)j * ngf + i] = k0f[((size_t)f * ngf + i) * ldf + e]; }
		if (!chol_lower(a, ngf)) return 0;   // a cost that leaves a free output without curvature: no structured Newton mode
		for (int i = 0; i < ngf; i++) for (int e = 0; e <= hbf; e++) { const int j = i - hbf + e; if (j >= 0) lf[((size_t)f * ngf + i) * ldf + e] = (j == i) ? 1.0 / a[(size_t)i * ngf + i] : a[(size_t)i * ngf + j]; }
	}
	if (!tu.empty()) {
		if (own.upload(&T.nwt_tu, tu.data(), tu.size()) || own.upload(&T.nwt_g, gt.data(), gt.size())) return NTG_E_HIP;
		D.nwt_tab = 1;
	}
	if (own.upload(&T.nwt_lf, lf.data(), lf.size())) return NTG_E_HIP;
	D.nwt_nfo = nfo; D.nwt_ngf = ngf; D.nwt_hbf = hbf;
	if (own.upload(&T.nwt_map, S.map.data(), S.map.size()) || own.upload(&T.nwt_pos, pos.data(), pos.size()) ||
	    own.upload(&T.nwt_k0, k0.data(), k0.size()) || own.upload(&T.nwt_lo, lo.data(), lo.size()) ||
	    own.upload(&T.nwt_hi, hi.data(), hi.size())) return NTG_E_HIP;
	D.nwt_on = 1; D.nwt_ngrp = ngrp; D.nwt_go = go; D.nwt_ng = ng; D.nwt_hb = hb; D.nwt_cg = cg;
	return 0;
}

// dense row-major [nclin][nC] A from the banded rows
void ntg_plan_dense_A(const ntg_plan *p, double *A)
{
	const NtgDims &D = p->D;
	std::fill(A, A + (size_t)D.nclin * D.nC, 0.0);
	for (int r = 0; r < D.nclin; r++)
		for (int o = 0; o < D.nout; o++) {
			const int col0 = D.iC[o] + p->h_off[(size_t)D.cls[o] * D.P + p->h_rbp[r]];
			for (int q = 0; q < D.order[o]; q++) A[(size_t)r * D.nC + col0 + q] = p->h_aband[(size_t)r * D.sumk + D.koff[o] + q];
		}
}

extern "C" void ntg_plan_destroy(ntg_plan *p)
{
	if (!p) return;
	hipSetDevice(p->device);
	for (void *q : p->owned) hipFree(q);
	for (void *q : p->grid_owned) hipFree(q);
	if (p->d_prm) hipFree(p->d_prm);
	delete p;
}

extern "C" int ntg_plan_dims(const ntg_plan *p, int *nC, int *nz, int *nclin, int *ncnln, int *nbounds, int *sumk, int *nblk)
{
	if (!p) return fail(NTG_E_BADARG, "null plan");
	if (nC) *nC = p->D.nC;
	if (nz) *nz = p->D.nz;
	if (nclin) *nclin = p->D.nclin;
	if (ncnln) *ncnln = p->D.ncnln;
	if (nbounds) *nbounds = p->D.nbounds;
	if (sumk) *sumk = p->D.sumk;
	if (nblk) { int t = 0; for (int o = 0; o < p->D.nout; o++) t += p->D.P * p->D.order[o] * p->D.d[o]; *nblk = t; }
	return 0;
}

extern "C" int ntg_plan_tables(const ntg_plan *p, double *blk, int *off, double *A)
{
	if (!p) return fail(NTG_E_BADARG, "null plan");
	const NtgDims &D = p->D;
	size_t pos = 0;
	for (int o = 0; o < D.nout; o++) {
		const size_t cnt = (size_t)D.P * D.order[o] * D.d[o];
		if (blk) std::memcpy(blk + pos, p->h_blk.data() + D.cls_blk[D.cls[o]], cnt * 8);
		if (off) std::memcpy(off + (size_t)o * D.P, p->h_off.data() + (size_t)D.cls[o] * D.P, (size_t)D.P * 4);
		pos += cnt;
	}
	if (A && D.nclin) // column-major nclin x nC
		for (int r = 0; r < D.nclin; r++)
			for (int c = 0; c < D.nC; c++) A[(size_t)c * D.nclin + r] = p->h_Adense[(size_t)r * D.nC + c];
	return 0;
}

// Dense core of the preconditioner for one block: W0 = Z (Z' H0 Z)^-1 Z' with Z = null(A) from a Householder QR of A'.
// H0 (n x n), A (m x n) and W0 (n x n) are row-major.
int precond_block(const std::vector<double> &H0, const std::vector<double> &A, int m, int n, std::vector<double> &W0)
{
	const int nr = n - m;
	if (nr <= 0) return fail(NTG_E_UNSUPPORTED, "no free directions");
	std::vector<double> Q((size_t)n * n, 0.0), R((size_t)n * std::max(m, 1), 0.0), v(n);
	for (int i = 0; i < n; i++) Q[(size_t)i * n + i] = 1.0;
	for (int j = 0; j < m; j++) for (int i = 0; i < n; i++) R[(size_t)i * m + j] = A[(size_t)j * n + i];
	for (int j = 0; j < m && j < n; j++) {
		double nrm = 0.0;
		for (int i = j; i < n; i++) nrm += R[(size_t)i * m + j] * R[(size_t)i * m + j];
		nrm = std::sqrt(nrm);
		if (nrm == 0.0) continue;
		const double alpha = R[(size_t)j * m + j] > 0 ? -nrm : nrm;
		std::fill(v.begin(), v.end(), 0.0);
		for (int i = j; i < n; i++) v[i] = R[(size_t)i * m + j];
		v[j] -= alpha;
		double vn = 0.0;
		for (int i = j; i < n; i++) vn += v[i] * v[i];
		if (vn == 0.0) continue;
		for (int c = j; c < m; c++) { double s = 0.0; for (int i = j; i < n; i++) s += v[i] * R[(size_t)i * m + c]; s = 2.0 * s / vn; for (int i = j; i < n; i++) R[(size_t)i * m + c] -= s * v[i]; }
		for (int c = 0; c < n; c++) { double s = 0.0; for (int i = j; i < n; i++) s += Q[(size_t)c * n + i] * v[i]; s = 2.0 * s / vn; for (int i = j; i < n; i++) Q[(size_t)c * n + i] -= s * v[i]; }
	}
	// Zt[j][:] = column m+j of Q ; T = H0 Z ; Hr = Z' T
	std::vector<double> Zt((size_t)nr * n), Tm((size_t)nr * n), Hr((size_t)nr * nr);
	for (int j = 0; j < nr; j++) for (int i = 0; i < n; i++) Zt[(size_t)j * n + i] = Q[(size_t)i * n + m + j];
	for (int j = 0; j < nr; j++) for (int i = 0; i < n; i++) { double s = 0.0; const double *h = &H0[(size_t)i * n], *z = &Zt[(size_t)j * n]; for (int k = 0; k < n; k++) s += h[k] * z[k]; Tm[(size_t)j * n + i] = s; }
	double tr = 0.0;
	auto form_hr = [&](double reg) {
		for (int i = 0; i < nr; i++) for (int j = 0; j <= i; j++) { double s = 0.0; const double *a = &Zt[(size_t)i * n], *b = &Tm[(size_t)j * n]; for (int k = 0; k < n; k++) s += a[k] * b[k]; Hr[(size_t)i * nr + j] = s; Hr[(size_t)j * nr + i] = s; }
		tr = 0.0; for (int i = 0; i < nr; i++) tr += Hr[(size_t)i * nr + i];
		for (int i = 0; i < nr; i++) Hr[(size_t)i * nr + i] += reg * tr / nr + 1e-300;
	};
	form_hr(1e-12);
	if (!chol_lower(Hr, nr)) { form_hr(1e-6); if (!chol_lower(Hr, nr)) return fail(NTG_E_UNSUPPORTED, "preconditioner not positive definite"); }
	{
		// H0 singular on null(A) (no equality rows: constants and ramps cost nothing): the regularised inverse would scale
		// those directions by 1e12 (1e6 after the harder regularisation) -- no preconditioner then, the solve starts from
		// the identity.  Checked after whichever factorisation succeeded.
		double lo = 1e300, hi = 0.0;
		for (int i = 0; i < nr; i++) { const double dd = Hr[(size_t)i * nr + i] * Hr[(size_t)i * nr + i]; lo = std::min(lo, dd); hi = std::max(hi, dd); }
		if (lo < 1e-9 * hi) return 1;
	}
	// X[:, c] = Hr^-1 Zt[:, c] ; W0 = Zt' X
	std::vector<double> X((size_t)n * nr), col(nr), Zc((size_t)n * nr);
	for (int c = 0; c < n; c++) { for (int i = 0; i < nr; i++) { col[i] = Zt[(size_t)i * n + c]; Zc[(size_t)c * nr + i] = col[i]; } chol_solve(Hr, nr, col.data()); for (int i = 0; i < nr; i++) X[(size_t)c * nr + i] = col[i]; }
	W0.assign((size_t)n * n, 0.0);
	for (int i = 0; i < n; i++) for (int j = 0; j <= i; j++) {
		double s = 0.0;
		const double *zi = &Zc[(size_t)i * nr], *xj = &X[(size_t)j * nr];
		for (int k = 0; k < nr; k++) s += zi[k] * xj[k];
		W0[(size_t)i * n + j] = s; W0[(size_t)j * n + i] = s;
	}
	// entries at rounding level relative to the diagonal are noise of the orthogonal factorisation: drop them
	for (int i = 0; i < n; i++) for (int j = 0; j < n; j++)
		if (i != j && std::fabs(W0[(size_t)i * n + j]) <= 1e-13 * std::sqrt(std::fabs(W0[(size_t)i * n + i] * W0[(size_t)j * n + j]))) W0[(size_t)i * n + j] = 0.0;
	return 0;
}

// W0 = Z (Z' H0 Z)^-1 Z', H0 = trapezoid-weighted sum of m m' over the cost active variables.
// Host, once per plan (shared by the whole batch).  H0 is block diagonal by output, so outputs that no row of A
// couples give independent blocks of W0: each block is factorised on its own (12 x 183^3 instead of 2196^3 for
// config E) and the result goes to HBM as ELL rows.
int build_precond(ntg_plan *p)
{
	const NtgDims &D = p->D;
	const int n = D.nC, m = D.mE, P = D.P;
	if (n - m <= 0) return fail(NTG_E_UNSUPPORTED, "no free directions");
	if (n > 65535) return fail(NTG_E_UNSUPPORTED, "preconditioner: more than 65535 coefficients");
	// components of outputs under "some row of A touches both"
	std::vector<int> comp(D.nout), outof(n);
	for (int o = 0; o < D.nout; o++) { comp[o] = o; for (int j = 0; j < D.ncoef[o]; j++) outof[D.iC[o] + j] = o; }
	for (int r = 0; r < m; r++) {
		int first = -1;
		for (int j = 0; j < n; j++) if (p->h_AE[(size_t)r * n + j] != 0.0) {
			const int c = comp[outof[j]];
			if (first < 0) first = c;
			else if (c != first) { const int lo = std::min(c, first), hi = std::max(c, first); for (int o = 0; o < D.nout; o++) if (comp[o] == hi) comp[o] = lo; first = lo; }
		}
	}
	std::vector<std::vector<std::pair<int, double>>> rows(n);   // W0 row i: (column, value), zeros dropped
	std::vector<std::vector<double>> wblocks; int nb_first = -1; bool by_output = true;   // one dense block per output, few distinct?
	for (int o0 = 0; o0 < D.nout; o0++) {
		if (comp[o0] != o0) continue;
		std::vector<int> idx, rsel, loc(n, -1);
		for (int j = 0; j < n; j++) if (comp[outof[j]] == o0) { loc[j] = (int)idx.size(); idx.push_back(j); }
		for (int r = 0; r < m; r++) { bool hit = false; for (int j : idx) if (p->h_AE[(size_t)r * n + j] != 0.0) { hit = true; break; } if (hit) rsel.push_back(r); }
		const int nb = (int)idx.size(), mb = (int)rsel.size();
		std::vector<double> H0((size_t)nb * nb, 0.0), Ab((size_t)std::max(mb, 1) * nb, 0.0), Wb;
		for_cost_terms(p, p->h_bps.data(), 1.0, [&](const std::vector<ntg_av> &av, int bp, double w) {
			for (const ntg_av &a : av) {
				const int o = a.output, k = D.order[o], d = D.d[o], c = D.cls[o];
				if (comp[o] != o0) continue;
				// an output's coefficients are contiguous in idx
				h0_add(H0, nb, loc[D.iC[o]] + p->h_off[(size_t)c * P + bp], p->h_blk.data() + D.cls_blk[c] + (size_t)bp * k * d, k, d, a.deriv, w);
			}
		});
		for (int i = 0; i < mb; i++) for (int j = 0; j < nb; j++) Ab[(size_t)i * nb + j] = p->h_AE[(size_t)rsel[i] * n + idx[j]];
		const int rc = precond_block(H0, Ab, mb, nb, Wb);
		if (rc > 0) { p->precond_ready = true; p->precond_singular = true; return 0; }   // singular model: identity start instead
		if (rc) return rc;
		{
			int nouts = 0; for (int o = 0; o < D.nout; o++) if (comp[o] == o0) nouts++;
			if (nouts != 1 || idx[0] != D.iC[o0] || (nb_first >= 0 && nb != nb_first)) by_output = false;
			else {
				nb_first = nb;
				int found = -1;
				for (size_t q = 0; q < wblocks.size(); q++) if (std::memcmp(Wb.data(), wblocks[q].data(), Wb.size() * sizeof(double)) == 0) found = (int)q;
				if (found < 0) { found = (int)wblocks.size(); wblocks.push_back(Wb); }
				p->D.n0_blk[o0] = found;
			}
		}
		for (int i = 0; i < nb; i++) for (int j = 0; j < nb; j++) if (Wb[(size_t)i * nb + j] != 0.0) rows[idx[i]].push_back({idx[j], Wb[(size_t)i * nb + j]});
	}
	DevOwner own;   // the tables are published only once all of them are on the device
	const double *d_wb = nullptr;
	const bool blocks = by_output && nb_first > 0 && nb_first * D.nout == n && wblocks.size() <= 4;
	const int spad = (nb_first + 15) & ~15;
	if (blocks) {
		// one dense block per output, kept once per distinct block: s-major (symmetric, so [s][row] == [row][s]),
		// rows padded with zeros to a multiple of 16
		std::vector<double> all(wblocks.size() * (size_t)spad * nb_first + 16, 0.0);   // +16: the last row tile reads up to 15 words past a row
		for (size_t q = 0; q < wblocks.size(); q++) std::copy(wblocks[q].begin(), wblocks[q].end(), all.begin() + q * (size_t)spad * nb_first);
		if (own.upload(&d_wb, all.data(), all.size())) return NTG_E_HIP;
		// the ELL form below stays as the fallback (block taller than the workgroup)
	}
	// ELL, s-major, zeros dropped
	int w = 0;
	for (int i = 0; i < n; i++) w = std::max(w, (int)rows[i].size());
	std::vector<double> ev((size_t)w * n, 0.0); std::vector<unsigned short> ec((size_t)w * n, 0);
	for (int i = 0; i < n; i++) { int e = 0; for (auto &cv : rows[i]) { ev[(size_t)e * n + i] = cv.second; ec[(size_t)e * n + i] = (unsigned short)cv.first; e++; } }
	const double *d_n0 = nullptr; const unsigned short *d_n0c = nullptr;
	if (own.upload(&d_n0, ev.data(), ev.size()) || own.upload(&d_n0c, ec.data(), ec.size())) return NTG_E_HIP;
	own.release_into(p->owned);
	if (blocks) { p->T.n0b = d_wb; p->T.n0b_n = nb_first; p->T.n0b_sp = spad; p->T.n0b_nblk = (int)wblocks.size(); }
	p->T.n0 = d_n0; p->T.n0c = d_n0c; p->T.n0_w = w;
	p->precond_ready = true;
	return 0;
}
