// unicycle_host.cpp -- TEST INFRASTRUCTURE: the unicycle family of ntg_amd/modules/unicycle_family.hpp as host callbacks with the
// reference's signatures (ntg.h:81-83,90-92), for the CPU oracle (oracle/liborc.so, orc_problem_make).  Compiled by a plain C++
// compiler from the SAME family header the module is built from; -ffp-contract=off like the oracle.
#include "../../ntg_amd/modules/unicycle_family.hpp"

namespace {
constexpr int NOUT = 2, NZ = Unicycle::DM * NOUT;
void gather(double **zp, double *z)
{
	for (int o = 0; o < NOUT; o++)
		for (int r = 0; r < Unicycle::DM; r++) z[Unicycle::DM * o + r] = zp[o][r];
}
template <int NCON> void scatter(const double *dcf, double **dc)
{
	for (int j = 0; j < NCON; j++)
		for (int v = 0; v < NZ; v++) dc[j][v] = dcf[j * NZ + v];
}
}  // namespace

extern "C" {
void uni_icf(int *mode, int *, double *f, double *df, double **zp)
{
	double z[NZ], g[NZ], v;
	gather(zp, z);
	Unicycle::icf(NOUT, z, v, g);
	if (*mode == 0 || *mode == 2) *f = v;
	if (*mode == 1 || *mode == 2) for (int k = 0; k < NZ; k++) df[k] = g[k];
}
void uni_fcf(int *mode, int *, double *f, double *df, double **zp)
{
	double z[NZ], g[NZ], v;
	gather(zp, z);
	Unicycle::fcf(NOUT, z, v, g);
	if (*mode == 0 || *mode == 2) *f = v;
	if (*mode == 1 || *mode == 2) for (int k = 0; k < NZ; k++) df[k] = g[k];
}
void uni_ucf(int *mode, int *, int *i, double *f, double *df, double **zp)
{
	double z[NZ], g[NZ], v;
	gather(zp, z);
	Unicycle::ucf(NOUT, *i, z, v, g);
	if (*mode == 0 || *mode == 2) *f = v;
	if (*mode == 1 || *mode == 2) for (int k = 0; k < NZ; k++) df[k] = g[k];
}
void uni_nlicf(int *mode, int *, double *c, double **dc, double **zp)
{
	double z[NZ], cv[Unicycle::NNLIC], d[Unicycle::NNLIC * NZ];
	gather(zp, z);
	Unicycle::nlicf(NOUT, z, cv, d);
	if (*mode == 0 || *mode == 2) for (int j = 0; j < Unicycle::NNLIC; j++) c[j] = cv[j];
	if (*mode == 1 || *mode == 2) scatter<Unicycle::NNLIC>(d, dc);
}
void uni_nltcf(int *mode, int *, int *i, double *c, double **dc, double **zp)
{
	double z[NZ], cv[Unicycle::NNLTC], d[Unicycle::NNLTC * NZ];
	gather(zp, z);
	Unicycle::nltcf(NOUT, *i, z, cv, d);
	if (*mode == 0 || *mode == 2) for (int j = 0; j < Unicycle::NNLTC; j++) c[j] = cv[j];
	if (*mode == 1 || *mode == 2) scatter<Unicycle::NNLTC>(d, dc);
}
void uni_nlfcf(int *mode, int *, double *c, double **dc, double **zp)
{
	double z[NZ], cv[Unicycle::NNLFC], d[Unicycle::NNLFC * NZ];
	gather(zp, z);
	Unicycle::nlfcf(NOUT, z, cv, d);
	if (*mode == 0 || *mode == 2) for (int j = 0; j < Unicycle::NNLFC; j++) c[j] = cv[j];
	if (*mode == 1 || *mode == 2) scatter<Unicycle::NNLFC>(d, dc);
}
}
