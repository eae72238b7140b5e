// obstacle_field_host.cpp -- TEST INFRASTRUCTURE: the NTG_FAM_OBSTACLE_FIELD family (ntg_amd/csrc/obstacle_field.hpp) as host callbacks
// with the reference's signatures (ntg.h:81-83,90-92), for the CPU oracle (oracle/liborc.so, orc_problem_make).  Compiled by a plain C++
// compiler from the SAME header the device family wraps; -ffp-contract=off like the oracle.  The problem's parameters live in file-scope
// globals, the reference's way (examples/kincar.c:43): of_set_params / of_set_nobs before each problem is built and solved.
#include "../../ntg_amd/csrc/obstacle_field.hpp"
extern "C" {
#include "../../oracle/oracle.h"
}

using ntg_amd::ObstacleField;

namespace {
constexpr int NOUT = 2, NZ = 6;
double g_prm[2 * ObstacleField::MAXOBS];
int g_m = 1;
void gather(double **zp, double *z)
{
	for (int o = 0; o < NOUT; o++)
		for (int r = 0; r < 3; r++) z[3 * o + r] = zp[o][r];
}
}  // namespace

extern "C" {
void of_set_nobs(int m) { g_m = m; }
void of_set_params(const double *prm)
{
	for (int k = 0; k < 2 * g_m; k++) g_prm[k] = prm[k];
}
void of_ucf(int *mode, int *, int *, double *f, double *df, double **zp)
{
	double z[NZ], g[NZ], v;
	gather(zp, z);
	ObstacleField::ucf(NOUT, z, v, g);
	if (*mode == 0 || *mode == 2) *f = v;
	if (*mode == 1 || *mode == 2) for (int k = 0; k < NZ; k++) df[k] = g[k];
}
void of_nltcf(int *mode, int *, int *, double *c, double **dc, double **zp)
{
	double z[NZ], cv[ObstacleField::MAXOBS], d[ObstacleField::MAXOBS * NZ];
	gather(zp, z);
	ObstacleField::dense(NOUT, g_m, z, cv, d, g_prm);
	if (*mode == 0 || *mode == 2) for (int j = 0; j < g_m; j++) c[j] = cv[j];
	if (*mode == 1 || *mode == 2)
		for (int j = 0; j < g_m; j++)
			for (int v = 0; v < NZ; v++) dc[j][v] = d[j * NZ + v];
}
// Hz (nz x nz) += sum_j t_j d2 c_j / dz dz = sum_j 2 t_j on (x, x) and (y, y)
void of_nltc_hess(int *, const double *t, double *Hz, double **)
{
	for (int j = 0; j < g_m; j++) { Hz[0 * NZ + 0] += 2.0 * t[j]; Hz[3 * NZ + 3] += 2.0 * t[j]; }
}
// what oracle/families.c sets for the built-in obstacle family: one coupling group (x, y), constraint flag entries x and y
void of_enable_newton(orc_problem *p)
{
	p->couple = 2;
	p->group_mask = (1ull << 0) | (1ull << 3);
	p->nltc_hess = of_nltc_hess;
}
// the device callbacks' arithmetic, for the finite-difference tests: z [6], t [m], out as named
void of_val(int m, const double *z, const double *prm, double *c) { ObstacleField::val(m, z, c, prm); }
void of_vjp(int m, const double *z, const double *t, const double *prm, double *df) { ObstacleField::vjp(m, z, t, df, prm); }
void of_dense(int m, const double *z, const double *prm, double *c, double *dc) { ObstacleField::dense(NOUT, m, z, c, dc, prm); }
void of_block(int m, const double *z, const double *t, double mu, int curv, const double *prm, double *B) { ObstacleField::block(m, z, t, mu, curv != 0, B, prm); }
}
