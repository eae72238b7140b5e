// tracking_host.cpp -- TEST INFRASTRUCTURE: the tracking family of ntg_amd/modules/tracking_family.hpp as host callbacks with the
// reference's signatures (ntg.h:81-83), for the CPU oracle (oracle/liborc.so, orc_problem_make).  Compiled by a plain C++ compiler from
// the SAME family header the module is built from; -ffp-contract=off like the oracle.  The problem's reference path lives in a
// file-scope global, the reference's way (examples/kincar.c:43): trk_set_params before each problem is built and solved.
#include "../../ntg_amd/modules/tracking_family.hpp"

namespace {
constexpr int NOUT = 2, NZ = 6;
const double *g_prm = nullptr;   // the caller keeps the row alive while the problem is in use
}  // namespace

extern "C" {
void trk_set_params(const double *prm) { g_prm = prm; }
void trk_ucf(int *mode, int *, int *i, double *f, double *df, double **zp)
{
	double z[NZ], g[NZ], v;
	for (int o = 0; o < NOUT; o++)
		for (int r = 0; r < 3; r++) z[3 * o + r] = zp[o][r];
	Tracking::ucf(NOUT, *i, z, v, g, g_prm);
	if (*mode == 0 || *mode == 2) *f = v;
	if (*mode == 1 || *mode == 2) for (int k = 0; k < NZ; k++) df[k] = g[k];
}
}
