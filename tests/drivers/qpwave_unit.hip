// qpwave_unit.hip -- the passive-set solve the kernel runs (csrc/qpdual.hpp, qp_passive_solve_wave: all lanes of a wave) against its
// specification (qp_passive_solve: scalar) on the GPU (test infrastructure: built and run by tests/test_gpu_qpwave.py).
//   qpwave_unit <ns> <seed>          one workgroup of 64 lanes runs the wave routine on a group's slots in LDS, lane 0 the scalar routine
//                                    on a copy: exit 0 when both end at the same passive set and the multipliers agree to 1e-10
//   qpwave_unit choose <ns> <nseed>  host only (no GPU call): lists the seeds 1 .. nseed whose solve takes no decision within 1e-6 of a
//                                    tie, with the number of slots that leave the passive set -- the test's seeds were taken from here
// Inputs: ns slots, all passive, S = G G'/m + I (G: ns x m uniform in [-1, 1], m = 2 ns + 3: condition number <= about 1e3), random
// signs, right-hand sides in [-1, 1], multipliers of the previous major in [0.1, 1].
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <algorithm>
#include <vector>
#include "../../ntg_amd/csrc/newton.hpp"      // nwt_wave_sync, and through nwt_map.hpp the routines of qpdual.hpp
#include "../../ntg_amd/csrc/direction.hpp"   // lds_dp

struct Input { int ns, qa; std::vector<double> S, jwg, rr, nu; std::vector<int> sgn; };

static Input make_input(int ns, unsigned seed)
{
	Input in; in.ns = ns; in.qa = ns <= 16 ? 16 : 32;
	unsigned long long st = 0x9E3779B97F4A7C15ull * (seed + 1) + (unsigned)ns;
	auto rnd = [&] { st = st * 6364136223846793005ull + 1442695040888963407ull; return (double)(st >> 11) / 9007199254740992.0; };   // [0, 1)
	const int m = 2 * ns + 3;
	std::vector<double> G((size_t)ns * m);
	for (double &g : G) g = 2.0 * rnd() - 1.0;
	in.S.assign(in.qa * (in.qa + 1) / 2, 0.0);
	for (int a = 0; a < ns; a++) for (int b = 0; b <= a; b++) {
		double s = 0.0;
		for (int k = 0; k < m; k++) s += G[(size_t)a * m + k] * G[(size_t)b * m + k];
		in.S[NTG_QP_TR(a, b)] = s / m + (a == b ? 1.0 : 0.0);
	}
	in.jwg.resize(ns); in.rr.resize(ns); in.nu.resize(ns); in.sgn.resize(ns);
	for (int a = 0; a < ns; a++) { in.sgn[a] = rnd() < 0.5 ? -1 : 1; in.jwg[a] = 2.0 * rnd() - 1.0; in.rr[a] = 2.0 * rnd() - 1.0; in.nu[a] = 0.1 + 0.9 * rnd(); }
	return in;
}

// host slots (plain pointers) filled from an input
struct HostSlots {
	std::vector<double> mem; QpSlotsT<double *, int *> q;
	HostSlots(const Input &in) : mem(ntg_qp_doubles(in.qa), 0.0), q(mem.data(), in.qa)
	{
		*q.ns = in.ns;
		for (size_t i = 0; i < in.S.size(); i++) q.S[i] = in.S[i];
		for (int a = 0; a < in.ns; a++) { q.jwg[a] = in.jwg[a]; q.rr[a] = in.rr[a]; q.nu[a] = q.nu0[a] = in.nu[a]; q.sgn[a] = in.sgn[a]; q.inP[a] = 1; }
	}
};

// The scalar routine's rounds restated with the distance of every decision from a tie: the sign of each unknown (relative to the largest),
// and the new multiplier of every slot but the one the step stops at against the drop rule.  Returns the smallest distance, -1 if the
// restatement does not end where qp_passive_solve ends (it follows the same path or it says nothing).
static double tie_margin(const Input &in, int *left)
{
	const int ns = in.ns;
	std::vector<int> P; std::vector<double> nu(in.nu);
	for (int a = 0; a < ns; a++) P.push_back(a);
	double margin = 1.0;
	for (int round = 0; !P.empty() && round < 3 * NTG_QP_MAXA + 8; round++) {
		const int np = (int)P.size();
		std::vector<double> H((size_t)np * np, 0.0), z(np);
		for (int k = 0; k < np; k++) for (int l = 0; l <= k; l++) {
			const int a = P[k], b = P[l];
			H[(size_t)k * np + l] = in.sgn[a] * in.sgn[b] * in.S[a >= b ? NTG_QP_TR(a, b) : NTG_QP_TR(b, a)] + (k == l ? 1e-10 * in.S[NTG_QP_TR(a, a)] : 0.0);
		}
		for (int k = 0; k < np; k++) for (int l = 0; l <= k; l++) {
			double v = H[(size_t)k * np + l];
			for (int t = 0; t < l; t++) v -= H[(size_t)k * np + t] * H[(size_t)l * np + t];
			if (l == k) { if (!(v > 0.0)) return -1.0; H[(size_t)k * np + k] = sqrt(v); } else H[(size_t)k * np + l] = v / H[(size_t)l * np + l];
		}
		for (int k = 0; k < np; k++) {
			const int a = P[k];
			double v = -(in.sgn[a] * (in.jwg[a] + in.rr[a]) - 1e-10 * in.S[NTG_QP_TR(a, a)] * in.nu[a]);
			for (int t = 0; t < k; t++) v -= H[(size_t)k * np + t] * z[t];
			z[k] = v / H[(size_t)k * np + k];
		}
		for (int k = np - 1; k >= 0; k--) {
			double v = z[k];
			for (int t = k + 1; t < np; t++) v -= H[(size_t)t * np + k] * z[t];
			z[k] = v / H[(size_t)k * np + k];
		}
		double zmax = 0.0, amin = 1.0; int kmin = -1;
		for (int k = 0; k < np; k++) zmax = fmax(zmax, fabs(z[k]));
		for (int k = 0; k < np; k++) {
			margin = fmin(margin, fabs(z[k]) / zmax);
			if (!(z[k] > 0.0)) { const double al = nu[P[k]] / (nu[P[k]] - z[k]); if (al < amin) { amin = al; kmin = k; } }
		}
		if (kmin < 0) { for (int k = 0; k < np; k++) nu[P[k]] = z[k]; break; }
		std::vector<int> keep;
		for (int k = 0; k < np; k++) {
			const int a = P[k];
			const double nn = nu[a] + amin * (z[k] - nu[a]);
			if (k != kmin) margin = fmin(margin, nn / (1.0 + fabs(z[k])));
			if (!(nn > 1e-14 * (1.0 + fabs(z[k])))) nu[a] = 0.0; else { nu[a] = nn; keep.push_back(a); }
		}
		P = keep;
	}
	HostSlots h(in);
	qp_passive_solve(h.q);
	int nin = 0;
	for (int a = 0; a < ns; a++) {
		const bool mine = std::find(P.begin(), P.end(), a) != P.end();
		if (mine != (h.q.inP[a] != 0) || fabs((mine ? nu[a] : 0.0) - h.q.nu[a]) > 1e-10 * (1.0 + fabs(h.q.nu[a]))) return -1.0;
		nin += mine;
	}
	*left = ns - nin;
	return margin;
}

// slot state of both routines: [2][qpd] doubles of LDS; the inputs come from and the results go to HBM
__global__ void __launch_bounds__(64) unit_kernel(int ns, int qa, const double *S, const double *jwg, const double *rr, const double *nu, const int *sgn,
                                                  double *nu_out, int *inP_out, int *solves)
{
	extern __shared__ double sm[];
	typedef __attribute__((address_space(3))) int *lds_ip;
	const int lane = threadIdx.x, qpd = ntg_qp_doubles(qa);
	QpSlotsT<lds_dp, lds_ip> qw((lds_dp)sm, qa), qs((lds_dp)(sm + qpd), qa);
	for (int i = lane; i < 2 * qpd; i += 64) sm[i] = 0.0;
	__syncthreads();
	for (int i = lane; i < qa * (qa + 1) / 2; i += 64) { qw.S[i] = S[i]; qs.S[i] = S[i]; }
	for (int a = lane; a < ns; a += 64) {
		qw.jwg[a] = qs.jwg[a] = jwg[a]; qw.rr[a] = qs.rr[a] = rr[a]; qw.nu[a] = qs.nu[a] = qw.nu0[a] = qs.nu0[a] = nu[a];
		qw.sgn[a] = qs.sgn[a] = sgn[a]; qw.inP[a] = qs.inP[a] = 1;
	}
	if (lane == 0) { *qw.ns = ns; *qs.ns = ns; }
	__syncthreads();
	const int sw = qp_passive_solve_wave(qw, lane, qa);
	__syncthreads();
	if (lane == 0) { solves[0] = sw; solves[1] = qp_passive_solve(qs); }
	__syncthreads();
	for (int a = lane; a < ns; a += 64) { nu_out[a] = qw.nu[a]; nu_out[ns + a] = qs.nu[a]; inP_out[a] = qw.inP[a]; inP_out[ns + a] = qs.inP[a]; }
}

int main(int argc, char **argv)
{
	if (argc > 3 && !strcmp(argv[1], "choose")) {
		const int ns = atoi(argv[2]);
		for (int seed = 1; seed <= atoi(argv[3]); seed++) { int left = 0; const double mg = tie_margin(make_input(ns, seed), &left); if (mg >= 1e-6) printf("ns %d seed %d: %d slots leave, margin %.2e\n", ns, seed, left, mg); }
		return 0;
	}
	if (argc < 3) { printf("usage: qpwave_unit <ns> <seed> | choose <ns> <nseed>\n"); return 2; }
	const int ns = atoi(argv[1]);
	if (ns < 1 || ns > NTG_QP_MAXA) { printf("ns out of range\n"); return 2; }
	const Input in = make_input(ns, atoi(argv[2]));
	int left = 0;
	const double mg = tie_margin(in, &left);
	if (!(mg >= 1e-6)) { printf("ns %d seed %s: a decision within 1e-6 of a tie (margin %.2e): not a test input\n", ns, argv[2], mg); return 3; }
	double *dS, *dj, *dr, *dn, *dout; int *dsg, *dinp, *dsol;
	hipMalloc(&dS, in.S.size() * 8); hipMalloc(&dj, ns * 8); hipMalloc(&dr, ns * 8); hipMalloc(&dn, ns * 8); hipMalloc(&dout, 2 * ns * 8);
	hipMalloc(&dsg, ns * 4); hipMalloc(&dinp, 2 * ns * 4); hipMalloc(&dsol, 8);
	hipMemcpy(dS, in.S.data(), in.S.size() * 8, hipMemcpyHostToDevice); hipMemcpy(dj, in.jwg.data(), ns * 8, hipMemcpyHostToDevice);
	hipMemcpy(dr, in.rr.data(), ns * 8, hipMemcpyHostToDevice); hipMemcpy(dn, in.nu.data(), ns * 8, hipMemcpyHostToDevice);
	hipMemcpy(dsg, in.sgn.data(), ns * 4, hipMemcpyHostToDevice);
	hipLaunchKernelGGL(unit_kernel, dim3(1), dim3(64), (size_t)2 * ntg_qp_doubles(in.qa) * 8, 0, ns, in.qa, dS, dj, dr, dn, dsg, dout, dinp, dsol);
	if (hipDeviceSynchronize() != hipSuccess) { printf("kernel failed\n"); return 2; }
	std::vector<double> nu(2 * ns); std::vector<int> inP(2 * ns); int sol[2];
	hipMemcpy(nu.data(), dout, 2 * ns * 8, hipMemcpyDeviceToHost); hipMemcpy(inP.data(), dinp, 2 * ns * 4, hipMemcpyDeviceToHost); hipMemcpy(sol, dsol, 8, hipMemcpyDeviceToHost);
	int same = 1, nleft = 0; double err = 0.0, big = 0.0;
	for (int a = 0; a < ns; a++) { same = same && inP[a] == inP[ns + a]; nleft += !inP[ns + a]; err = fmax(err, fabs(nu[a] - nu[ns + a])); big = fmax(big, fabs(nu[ns + a])); }
	printf("ns %d seed %s: %d slots leave (host %d), solves wave %d scalar %d, passive sets %s, max |nu_wave - nu_scalar| / max |nu| = %.3e (tie margin %.2e)\n",
	       ns, argv[2], nleft, left, sol[0], sol[1], same ? "equal" : "DIFFER", big > 0.0 ? err / big : err, mg);
	return (same && nleft == left && (big > 0.0 ? err <= 1e-10 * big : err == 0.0)) ? 0 : 1;
}
