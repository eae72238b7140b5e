// plan_grids.cpp -- per-problem grids and per-problem family parameters behind include/ntg_amd.h.
// Per-problem grids: the setup phase of ntg() (ntg.c:114-229: CollocMatrix per output, LinearConstraintsMatrix) run for every problem
// of a batch on its own break sequence and breakpoints.  The plan's combinatorial structure is shared, the VALUES become per problem;
// the algebra runs on the device (grids.hip), except preconditioner blocks whose equality rows do not pin whole coefficients: dense
// n_o x n_o algebra on a few host threads, like the one-grid build_precond.  ntg_plan_set_grids runs its numbered steps in order; every
// array of a grid set is allocated through one DevOwner, so a refused grid set frees itself.
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#include "plan_priv.hpp"
#include "family_module.hpp"

// ---------------- per-problem family parameters (ntg_plan_set_params) ----------------
// doubles per problem the plan's family needs, 0 for a family without
int param_count(const ntg_plan *p)
{
	const NtgFamily *f = ntg_family(p->D.family);
	return f ? f->nparam + f->nparam_bp * p->D.P + f->nparam_row * p->D.nnltc : 0;
}

// the callbacks of eval / solve / mpc_run read problem b's parameter row: the family's parameters must be set, for this batch
int check_params(const ntg_plan *p, int batch)
{
	if (p->prm_batch && batch != p->prm_batch)
		return fail(NTG_E_BADARG, "the plan carries per-problem parameters for " + std::to_string(p->prm_batch) + " problems, not " + std::to_string(batch));
	if (!p->prm_batch && param_count(p) > 0)
		return fail(NTG_E_BADARG, "the plan's family reads " + std::to_string(param_count(p)) + " parameters per problem: set them with ntg_plan_set_params");
	return 0;
}

extern "C" int ntg_plan_param_count(const ntg_plan *p, int *nparam)
{
	if (!p || !nparam) return fail(NTG_E_BADARG, "null argument");
	*nparam = param_count(p);
	return 0;
}

extern "C" void ntg_plan_clear_params(ntg_plan *p)
{
	if (!p || !p->d_prm) return;
	hipSetDevice(p->device);
	hipDeviceSynchronize();   // queued kernels may still read the buffer
	hipFree(p->d_prm);
	p->d_prm = nullptr; p->prm_cap = 0; p->prm_batch = 0; p->prm_n = 0;
	p->T.prm = nullptr; p->T.pp_prm = 0;
}

extern "C" int ntg_plan_set_params(ntg_plan *p, int batch, int nparam, const double *d_params, void *stream)
{
	if (!p) return fail(NTG_E_BADARG, "null plan");
	if (p->D.family == NTG_FAM_HOST) return fail(NTG_E_UNSUPPORTED, "host-callback plans keep their parameters in the callbacks' own data");
	const int want = param_count(p);
	if (want == 0) return fail(NTG_E_BADARG, "the plan's family takes no per-problem parameters");
	if (nparam != want) return fail(NTG_E_BADARG, "the plan's family takes " + std::to_string(want) + " parameters per problem, not " + std::to_string(nparam));
	if (batch <= 0 || !d_params) return fail(NTG_E_BADARG, "bad argument");
	HIPCHK(hipSetDevice(p->device));
	const size_t n = (size_t)batch * nparam;
	if (n != p->prm_cap) {   // same batch x nparam: the buffer (and so its address, e.g. in a captured graph) stays
		ntg_plan_clear_params(p);
		HIPCHK(hipMalloc((void **)&p->d_prm, n * sizeof(double)));
		p->prm_cap = n;
	}
	HIPCHK(hipMemcpyAsync(p->d_prm, d_params, n * sizeof(double), hipMemcpyDeviceToDevice, (hipStream_t)stream));
	p->prm_batch = batch; p->prm_n = nparam;
	p->T.prm = p->d_prm; p->T.pp_prm = nparam;
	return 0;
}

// ---------------- per-problem grids ----------------
// the device arrays of one grid set ([batch][size] each; null: the plan has no use for it) and the sizes per problem
struct GridSet {
	double *blk = nullptr, *rowv = nullptr, *bpsc = nullptr, *csr = nullptr, *csc = nullptr, *sinv = nullptr, *q = nullptr, *knc = nullptr, *n0b = nullptr,
	       *icsr = nullptr, *icsc = nullptr, *k0 = nullptr, *lf = nullptr;
	int *off = nullptr, *err = nullptr;   // temporaries: the block offsets (checked against the plan's, then shared) and the kernels' error word
	size_t nblk, n0b_sz, k0_sz, lf_sz;
	int row_total, lin_nnz, sinv_nnz, qn, inz;
};

static void dense_AE_pp(const ntg_plan *p, const double *blk, std::vector<double> &AE)   // AE: [mE][nC] row-major
{
	const NtgDims &D = p->D;
	const int n = D.nC, m = D.mE, nz = D.nz;
	AE.assign((size_t)std::max(m, 1) * n, 0.0);
	for (int e = 0; e < m; e++) {
		const LinRow lr = lin_row(D, p->h_erow[e]);
		const double *row = p->h_linrows.data() + (size_t)lr.slot * nz;
		for (int o = 0; o < D.nout; o++) {
			const int k = D.order[o], d = D.d[o], col0 = D.iC[o] + p->h_off[lr.bp];   // one basis class: offsets of class 0
			for (int q = 0; q < k; q++) {
				double acc = 0.0;
				for (int l = 0; l < d; l++) acc += row[D.iz[o] + l] * blk[((size_t)lr.bp * k + q) * d + l];
				AE[(size_t)e * n + col0 + q] = acc;
			}
		}
	}
}

// preconditioner blocks of one grid (the distinct blocks of build_precond, same order): all[q][spad][nb]
static int precond_blocks_pp(const ntg_plan *p, const double *blk, const double *bps, const std::vector<double> &AE, double *all)
{
	const NtgDims &D = p->D;
	const int n = D.nC, m = D.mE, nb = p->T.n0b_n, spad = p->T.n0b_sp;
	for (int q = 0; q < p->T.n0b_nblk; q++) {
		const int o0 = block_output(D, q);
		if (o0 < 0) return NTG_E_UNSUPPORTED;
		const int k = D.order[o0], d = D.d[o0], c0 = D.iC[o0];
		std::vector<double> H0((size_t)nb * nb, 0.0), Wb;
		for_cost_terms(p, bps, 1.0, [&](const std::vector<ntg_av> &av, int bp, double w) {
			for (const ntg_av &a : av) if (a.output == o0) h0_add(H0, nb, p->h_off[bp], blk + (size_t)bp * k * d, k, d, a.deriv, w);
		});
		std::vector<int> rsel;
		for (int r = 0; r < m; r++) { bool hit = false; for (int j = 0; j < nb && !hit; j++) if (p->h_AE[(size_t)r * n + c0 + j] != 0.0) hit = true; if (hit) rsel.push_back(r); }
		const int mb = (int)rsel.size();
		std::vector<double> Ab((size_t)std::max(mb, 1) * nb, 0.0);
		for (int i = 0; i < mb; i++) for (int j = 0; j < nb; j++) Ab[(size_t)i * nb + j] = AE[(size_t)rsel[i] * n + c0 + j];
		if (precond_block(H0, Ab, mb, nb, Wb)) return NTG_E_UNSUPPORTED;
		std::copy(Wb.begin(), Wb.end(), all + (size_t)q * spad * nb);
	}
	return 0;
}

extern "C" void ntg_plan_clear_grids(ntg_plan *p)
{
	if (!p || !p->grid_batch) return;
	hipSetDevice(p->device);
	hipDeviceSynchronize();
	for (void *q : p->grid_owned) hipFree(q);
	p->grid_owned.clear();
	p->T = p->T_shared;
	p->T.prm = p->prm_batch ? p->d_prm : nullptr; p->T.pp_prm = p->prm_batch ? p->prm_n : 0;   // the parameters stay in force
	p->grid_batch = 0; p->d_grid_knots = nullptr;
}

// What the kernels of grids.hip left in their error word, read back once the stream has run (e: the launches' status so far).  One
// decoder for the three stages that use the word; returns 0 or the refusal.
enum GridStage { GRID_LINEAR, GRID_PRECOND, GRID_NEWTON };
static int grid_stage_result(hipError_t e, const int *d_err, hipStream_t st, GridStage stage)
{
	int herr[4] = {0, 0, 0, 0};
	if (e == hipSuccess) e = hipMemcpyAsync(herr, d_err, 12, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipStreamSynchronize(st);
	if (e != hipSuccess) return fail(NTG_E_HIP, hipGetErrorString(e));
	const std::string prob = "(problem " + std::to_string(herr[1]);
	if (stage == GRID_PRECOND) return herr[0] == 3 ? fail(NTG_E_UNSUPPORTED, "per-problem grid: preconditioner block not positive definite " + prob + ")") : 0;
	if (stage == GRID_NEWTON) return herr[0] == 3 ? fail(NTG_E_UNSUPPORTED, "per-problem grid: the cost model of a free output is not positive definite " + prob + ")") : 0;
	if (herr[0] == 1) return fail(NTG_E_BADARG, "per-problem grid: a breakpoint lies in another knot interval than in the plan's grid " + prob + ", breakpoint " + std::to_string(herr[2]) + ")");
	if (herr[0] == 2) return fail(NTG_E_UNSUPPORTED, "per-problem grid: a linear-constraint entry outside the plan's sparsity pattern " + prob + ", row " + std::to_string(herr[2]) + ")");
	if (herr[0] == 3) return fail(NTG_E_BADARG, "per-problem grid: linear constraint rows are rank deficient " + prob + ")");
	if (herr[0] == 4) return fail(NTG_E_UNSUPPORTED, "per-problem grid: a linear-constraint entry outside the plan's sparsity pattern " + prob + ", linear row " + std::to_string(herr[2]) + ", declared an inequality)");
	return 0;
}

// step 0: batch-shared inputs of the device algebra, uploaded once per plan
static int grid_shared_uploads(ntg_plan *p)
{
	if (p->d_planoff) return 0;
	const NtgDims &D = p->D;
	const int m = D.mE, qn = D.q_use ? D.q_nt * D.q_w : 0;
	std::vector<double> rows((size_t)std::max(D.nclin, 1) * D.nz, 0.0);
	std::copy(p->h_linrows.begin(), p->h_linrows.end(), rows.begin());
	std::vector<int> er(std::max(m, 1), 0);
	for (int e2 = 0; e2 < m; e2++) er[e2] = p->h_erow[e2];
	std::vector<int> r2c(std::max(D.q_nt, 1), 0);
	std::vector<unsigned char> pad((size_t)std::max(qn, 1), 0);
	if (D.q_use) {
		for (int a = 0; a < D.nC; a++) if (p->h_qidx[a] >= 0) r2c[p->h_qidx[a]] = a;
		// ELL padding: entries whose plan value is exactly 0 and that repeat column 0 behind the row's real entries
		for (int t = 0; t < D.q_nt; t++) for (int w2 = 1; w2 < D.q_w; w2++)
			if (p->h_qval[(size_t)t * D.q_w + w2] == 0.0 && p->h_qcol[(size_t)t * D.q_w + w2] == 0) pad[(size_t)t * D.q_w + w2] = 1;
	}
	DevOwner own;
	int *d_planoff = nullptr;
	if (own.upload(&d_planoff, p->h_off.data(), (size_t)D.P) || own.upload(&p->d_linrows, rows.data(), rows.size()) || own.upload(&p->d_erow, er.data(), er.size()) ||
	    own.upload(&p->d_qrow2coef, r2c.data(), r2c.size()) || own.upload(&p->d_qpad, pad.data(), pad.size())) return NTG_E_HIP;
	own.release_into(p->owned);
	p->d_planoff = d_planoff;   // set last: marks the five as uploaded
	return 0;
}

// steps 1 to 3: basis blocks and offsets of every problem -- one launch of basis_kernel (bsplvd at every collocation point,
// colloc.c:95-111); 2. channel rows in the kernels' layout + the structure check (every breakpoint in the plan's knot interval); 3. the
// algebra of the linear rows -- A_E on the plan's patterns, (A A')^-1, Q -- one wavefront per problem; 3b. the linear inequality rows'
// values (no projection: the augmented-Lagrangian loop reads them as they are); also when every row is one.  All on the device (grids.hip).
static int grid_basis_and_rows(const ntg_plan *p, int batch, const double *d_knots, const double *d_bps, const GridSet &G, hipStream_t st)
{
	const NtgDims &D = p->D;
	const int P = D.P, k = D.cls_k[0], d = D.cls_d[0], l = D.cls_l[0];
	hipError_t e = hipMemsetAsync(G.err, 0, 16, st);
	if (e == hipSuccess) e = hipMemsetAsync(G.rowv, 0, (size_t)batch * G.row_total * 8, st);
	if (e == hipSuccess) e = hipMemcpyAsync(G.bpsc, d_bps, (size_t)batch * P * 8, hipMemcpyDeviceToDevice, st);
	if (e == hipSuccess) e = hipMemcpyAsync(G.knc, d_knots, (size_t)batch * (l + 1) * 8, hipMemcpyDeviceToDevice, st);   // kept: ntg_batch_interp evaluates the basis at other times
	if (e == hipSuccess) e = ntg_launch_basis(batch, l, k, D.cls_m[0], d, P, d_knots, d_bps, l + 1, P, G.blk, G.off, st);
	if (e == hipSuccess) e = ntg_launch_grid_rows(D, batch, G.blk, G.off, p->d_planoff, G.rowv, G.err, st);
	if (e == hipSuccess && D.mE > 0) {
		NtgGridLin g{G.blk, p->d_linrows, p->d_planoff, p->d_erow, p->T.csr_ptr, p->T.csr_col, p->T.csc_ptr, p->T.csc_row, p->T.sinv_ptr, p->T.sinv_col,
		             p->T.q_col, p->d_qrow2coef, p->d_qpad, G.csr, G.csc, G.sinv, G.q, G.err};
		e = ntg_launch_grid_lin(D, batch, g, st);
	}
	if (e == hipSuccess && G.inz > 0) {
		NtgGridILin g{G.blk, p->d_linrows, p->d_planoff, p->T.irow, p->T.icsr_ptr, p->T.icsr_col, p->T.icsc_ptr, p->T.icsc_row, G.icsr, G.icsc, G.err, G.inz};
		e = ntg_launch_grid_ilin(D, batch, g, st);
	}
	return grid_stage_result(e, G.err, st, GRID_LINEAR);
}

// Can the preconditioner blocks of every grid be built on the device (grids.hip, grid_prec_kernel)?  Yes when the equality rows that
// touch a block pin whole coefficients -- null(A) is then spanned by unit vectors and W0 is the inverse of a principal submatrix of H0.
// Decided once per plan from the shared grid's A (ntg_plan::prec_dev), with the kernel's tables: fidx[q][j] = index of coefficient j of
// block q among the free ones (-1: pinned), binfo[q] = {free coefficients, derivative masks of the running / initial / final cost}.
static int grid_prec_decide(ntg_plan *p)
{
	const NtgDims &D = p->D;
	const int n = D.nC, m = D.mE, nb = p->T.n0b_n, nq = p->T.n0b_nblk;
	std::vector<int> fidx((size_t)nq * nb, -1), binfo((size_t)nq * 4, 0);
	bool okdev = !getenv("NTG_AMD_HOST_PRECOND");
	int nrmax = 0;
	for (int q = 0; q < nq && okdev; q++) {
		const int o0 = block_output(D, q);
		if (o0 < 0 || D.ncoef[o0] != nb) { okdev = false; break; }
		const int c0 = D.iC[o0];
		std::vector<char> pin(nb, 0);
		int mb = 0, npin = 0;
		for (int r = 0; r < m; r++) {
			double big = 0.0; bool hit = false;
			for (int c = 0; c < n; c++) big = std::max(big, std::fabs(p->h_AE[(size_t)r * n + c]));
			for (int j = 0; j < nb; j++) if (p->h_AE[(size_t)r * n + c0 + j] != 0.0) hit = true;
			if (!hit) continue;
			mb++;
			for (int j = 0; j < nb; j++) if (std::fabs(p->h_AE[(size_t)r * n + c0 + j]) > 1e-10 * big && !pin[j]) { pin[j] = 1; npin++; }
			// a row that also touches another block couples the blocks: not this structure
			for (int c = 0; c < n; c++) if ((c < c0 || c >= c0 + nb) && std::fabs(p->h_AE[(size_t)r * n + c]) > 1e-10 * big) okdev = false;
		}
		if (npin != mb || nb - npin < 1) { okdev = false; break; }
		int cnt = 0;
		for (int j = 0; j < nb; j++) fidx[(size_t)q * nb + j] = pin[j] ? -1 : cnt++;
		binfo[4 * q] = cnt; nrmax = std::max(nrmax, cnt);
		auto mask_of = [&](const std::vector<ntg_av> &av) { int mk = 0; for (const ntg_av &a : av) if (a.output == o0) mk |= 1 << a.deriv; return mk; };
		binfo[4 * q + 1] = D.nucf ? mask_of(p->tcostav) : 0; binfo[4 * q + 2] = D.nicf ? mask_of(p->icostav) : 0; binfo[4 * q + 3] = D.nfcf ? mask_of(p->fcostav) : 0;
	}
	if (okdev && 2 * (size_t)nrmax * (nrmax + 1) * 8 > 160 * 1024) okdev = false;
	if (okdev) {
		DevOwner own;
		if (own.upload(&p->d_pfidx, fidx.data(), fidx.size()) || own.upload(&p->d_pbinfo, binfo.data(), binfo.size())) return fail(NTG_E_HIP, "upload (preconditioner tables)");
		own.release_into(p->owned);
	}
	p->prec_dev = okdev ? 1 : 0; p->prec_nrmax = nrmax;
	return 0;
}

// step 4: the preconditioner blocks of every grid (hessian = 1), on the device where grid_prec_decide allows, else on host threads
static int grid_precond(ntg_plan *p, int batch, const double *d_bps, const GridSet &G, hipStream_t st)
{
	const NtgDims &D = p->D;
	if (p->prec_dev < 0) if (int rc = grid_prec_decide(p)) return rc;
	if (p->prec_dev == 1) {
		NtgGridPrec g{G.blk, G.bpsc, p->d_planoff, p->d_pfidx, p->d_pbinfo, G.n0b, G.err, p->T.n0b_nblk, p->T.n0b_n, p->T.n0b_sp, (int)G.n0b_sz, p->prec_nrmax};
		hipError_t e = hipMemsetAsync(G.n0b, 0, (size_t)batch * G.n0b_sz * 8, st);
		if (e == hipSuccess) e = ntg_launch_grid_prec(D, batch, g, st);
		return grid_stage_result(e, G.err, st, GRID_PRECOND);
	}
	const size_t nblk = G.nblk, n0b_sz = G.n0b_sz;
	const int P = D.P;
	std::vector<double> hblk((size_t)batch * nblk), hbps((size_t)batch * P), n0bv((size_t)batch * n0b_sz, 0.0);
	if (hipMemcpy(hblk.data(), G.blk, hblk.size() * 8, hipMemcpyDeviceToHost) != hipSuccess ||
	    hipMemcpy(hbps.data(), d_bps, hbps.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return fail(NTG_E_HIP, "reading the basis blocks back failed");
	std::atomic<int> next(0), err(0);
	auto worker = [&]() {
		std::vector<double> AE;
		for (;;) {
			const int b = next.fetch_add(1);
			if (b >= batch || err.load()) break;
			const double *blk = hblk.data() + (size_t)b * nblk;
			dense_AE_pp(p, blk, AE);
			if (precond_blocks_pp(p, blk, hbps.data() + (size_t)b * P, AE, n0bv.data() + (size_t)b * n0b_sz)) { err.store(3); break; }
		}
	};
	const unsigned nthr = std::max(1u, std::min(32u, std::thread::hardware_concurrency()));
	std::vector<std::thread> pool;
	for (unsigned t = 0; t + 1 < nthr; t++) pool.emplace_back(worker);
	worker();
	for (auto &th : pool) th.join();
	if (err.load()) return fail(NTG_E_UNSUPPORTED, "per-problem grid: preconditioner block not positive definite");
	if (hipMemcpy(G.n0b, n0bv.data(), n0bv.size() * 8, hipMemcpyHostToDevice) != hipSuccess) return fail(NTG_E_HIP, "uploading the preconditioner blocks failed");
	return 0;
}

// step 4b: the structured Newton mode's cost model and free-output factors of every grid (hessian = 2 / 3 then run on per-problem grids
// like on the plan's own; the QP-based SQP step's plan tables belong to the plan's grid and stay unused there)
static int grid_newton(const ntg_plan *p, int batch, GridSet &G, DevOwner &own, hipStream_t st)
{
	const NtgDims &D = p->D;
	G.k0_sz = (size_t)D.nwt_ngrp * D.nwt_ng * (D.nwt_hb + 1) + (D.nwt_tw ? (size_t)D.nwt_ngrp * (16 * D.nwt_jb + 48) * (D.nwt_hb + 1) : 0);
	G.lf_sz = std::max<size_t>((size_t)D.nwt_nfo * D.nwt_ngf * (D.nwt_hbf + 1), 1);
	if (own.alloc(&G.k0, (size_t)batch * G.k0_sz) || own.alloc(&G.lf, (size_t)batch * G.lf_sz)) return fail(NTG_E_HIP, "hipMalloc (per-problem cost models)");
	NtgGridNwt gn{G.rowv, G.bpsc, p->d_planoff, p->T.nwt_lo, p->T.nwt_hi, G.k0, G.lf, G.err, (int)G.k0_sz, (int)G.lf_sz};
	hipError_t e = hipMemsetAsync(G.err, 0, 16, st);
	if (e == hipSuccess) e = ntg_launch_grid_nwt(D, batch, gn, st);
	return grid_stage_result(e, G.err, st, GRID_NEWTON);
}

extern "C" int ntg_plan_set_grids(ntg_plan *p, int batch, const double *d_knots, const double *d_bps, int with_precond, void *stream)
{
	if (!p) return fail(NTG_E_BADARG, "null plan");
	if (batch <= 0 || !d_knots || !d_bps) return fail(NTG_E_BADARG, "bad argument");
	const NtgDims &D = p->D;
	if (D.family == NTG_FAM_HOST) return fail(NTG_E_UNSUPPORTED, "host-callback plans have one grid");
	if (D.nclass != 1) return fail(NTG_E_UNSUPPORTED, "per-problem grids need one basis class (every output on the same knots / order / multiplicity)");
	// Nonlinear rows are fine: their evaluation reads the same per-problem tables, and the structured Newton mode / the QP-based SQP step get
	// the cost model and the free-output factors of every grid (step 4b, grids.hip grid_nwt_kernel).  So are linear inequality rows: their
	// values on the plan's patterns come from every grid too (step 3b, grids.hip grid_ilin_kernel).
	HIPCHK(hipSetDevice(p->device));
	ntg_plan_clear_grids(p);
	if (with_precond) {
		std::lock_guard<std::mutex> lk(p->precond_mutex);
		if (!p->precond_ready) { int rc = build_precond(p); if (rc) return rc; }
		if (p->precond_singular || !p->T.n0b) return fail(NTG_E_UNSUPPORTED, "per-problem grids with the preconditioner need its block form (one dense block per output)");
	}
	hipStream_t st = (hipStream_t)stream;
	if (int rc = grid_shared_uploads(p)) return rc;
	const int P = D.P, l = D.cls_l[0];
	GridSet G;
	G.nblk = (size_t)P * D.cls_k[0] * D.cls_d[0];
	G.row_total = D.row_total; G.lin_nnz = std::max(D.lin_nnz, 1); G.sinv_nnz = std::max(D.sinv_nnz, 1); G.qn = D.q_use ? D.q_nt * D.q_w : 0;
	G.inz = D.nI > 0 ? std::max(p->h_icsr_ptr[D.nI], 1) : 0;   // entries of the inequality rows (one problem)
	G.n0b_sz = with_precond ? (size_t)p->T.n0b_nblk * p->T.n0b_sp * p->T.n0b_n + 16 : 0;
	G.k0_sz = G.lf_sz = 0;
	DevOwner own;   // every array of the grid set; a refusal below is a plain return
	const size_t B = (size_t)batch;
	if (own.alloc(&G.blk, B * G.nblk) || own.alloc(&G.off, B * P) || own.alloc(&G.err, 4) || own.alloc(&G.rowv, B * G.row_total) || own.alloc(&G.bpsc, B * P) ||
	    own.alloc(&G.csr, B * G.lin_nnz) || own.alloc(&G.csc, B * G.lin_nnz) || own.alloc(&G.sinv, B * G.sinv_nnz) || own.alloc(&G.q, B * std::max(G.qn, 1)) ||
	    own.alloc(&G.knc, B * (l + 1)) || own.alloc(&G.n0b, B * G.n0b_sz) || own.alloc(&G.icsr, B * G.inz) || own.alloc(&G.icsc, B * G.inz))
		return fail(NTG_E_HIP, "hipMalloc (per-problem grids)");
	if (int rc = grid_basis_and_rows(p, batch, d_knots, d_bps, G, st)) return rc;
	if (with_precond) if (int rc = grid_precond(p, batch, d_bps, G, st)) return rc;
	if (D.nwt_on) if (int rc = grid_newton(p, batch, G, own, st)) return rc;
	own.free_one(G.off); own.free_one(G.err);   // (blk is kept: the receding-horizon shift evaluates the whole flag at a breakpoint)
	own.release_into(p->grid_owned);
	// 5. the kernels add b * stride to the value pointers (NtgTables::pp_*)
	p->T_shared = p->T;
	p->d_grid_knots = G.knc;
	NtgTables &T = p->T;
	T.rowv = G.rowv; T.pp_rowv = G.row_total;
	T.blk = G.blk; T.pp_blk = (long long)G.nblk;   // one basis class: cls_blk[0] == 0
	T.bps = G.bpsc; T.pp_bps = P;
	if (D.mE > 0) { T.csr_val = G.csr; T.csc_val = G.csc; T.pp_lin = G.lin_nnz; T.sinv_val = G.sinv; T.pp_sinv = G.sinv_nnz; }
	if (D.q_use) { T.q_val = G.q; T.pp_q = G.qn; }
	if (with_precond) { T.n0b = G.n0b; T.pp_n0b = (long long)G.n0b_sz; T.n0 = nullptr; T.n0c = nullptr; }
	if (D.nwt_on) { T.nwt_k0 = G.k0; T.pp_k0 = (long long)G.k0_sz; T.nwt_lf = G.lf; T.pp_lf = (long long)G.lf_sz; }
	if (G.inz > 0) { T.icsr_val = G.icsr; T.icsc_val = G.icsc; T.pp_ilin = G.inz; }
	p->grid_batch = batch;
	return 0;
}

// ntg_plan_tables for one problem's grid (after ntg_plan_set_grids): its basis blocks, and A scattered from the values the device holds
// for it -- the equality rows' CSR values (grid_lin_kernel) and the inequality rows' (grid_ilin_kernel) -- on the plan's patterns
extern "C" int ntg_plan_grid_tables(const ntg_plan *p, int problem, double *blk, int *off, double *A)
{
	if (!p) return fail(NTG_E_BADARG, "null plan");
	if (!p->grid_batch) return fail(NTG_E_BADARG, "no per-problem grids are set (ntg_plan_set_grids)");
	if (problem < 0 || problem >= p->grid_batch) return fail(NTG_E_BADARG, "problem out of range of the per-problem grids");
	const NtgDims &D = p->D;
	const NtgTables &T = p->T;
	HIPCHK(hipSetDevice(p->device));
	if (blk) {   // one basis class: every output reads the same [bp][q][r] table
		const size_t nblk = (size_t)D.P * D.cls_k[0] * D.cls_d[0];
		HIPCHK(hipMemcpy(blk, T.blk + (size_t)problem * T.pp_blk, nblk * 8, hipMemcpyDeviceToHost));
		for (int o = 1; o < D.nout; o++) std::memcpy(blk + o * nblk, blk, nblk * 8);
	}
	if (off)
		for (int o = 0; o < D.nout; o++) std::memcpy(off + (size_t)o * D.P, p->h_off.data(), (size_t)D.P * 4);
	if (A && D.nclin) {   // column-major nclin x nC
		std::fill(A, A + (size_t)D.nclin * D.nC, 0.0);
		if (D.mE > 0 && D.lin_nnz > 0) {
			std::vector<double> v(D.lin_nnz);
			HIPCHK(hipMemcpy(v.data(), T.csr_val + (size_t)problem * T.pp_lin, v.size() * 8, hipMemcpyDeviceToHost));
			for (int i = 0; i < D.mE; i++)
				for (int e = p->h_csr_ptr[i]; e < p->h_csr_ptr[i + 1]; e++) A[(size_t)p->h_csr_col[e] * D.nclin + p->h_erow[i]] = v[e];
		}
		if (D.nI > 0 && p->h_icsr_ptr[D.nI] > 0) {
			std::vector<double> v(p->h_icsr_ptr[D.nI]);
			HIPCHK(hipMemcpy(v.data(), T.icsr_val + (size_t)problem * T.pp_ilin, v.size() * 8, hipMemcpyDeviceToHost));
			for (int j = 0; j < D.nI; j++)
				for (int e = p->h_icsr_ptr[j]; e < p->h_icsr_ptr[j + 1]; e++) A[(size_t)p->h_icsr_col[e] * D.nclin + p->h_irow[j]] = v[e];
		}
	}
	return 0;
}
