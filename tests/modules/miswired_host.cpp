// miswired_host.cpp -- TEST INFRASTRUCTURE: the family with planted errors of miswired_family.hpp (next to this file) as host callbacks with the
// reference's signatures (ntg.h:81-83,90-92), for the CPU oracle (oracle/liborc.so, orc_problem_make).  Compiled by a plain C++
// compiler from the SAME family header the module is built from; -ffp-contract=off like the oracle.
#include "miswired_family.hpp"

namespace {
constexpr int NOUT = 2, NZ = Miswired::DM * NOUT;
void gather(double **zp, double *z)
{
	for (int o = 0; o < NOUT; o++)
		for (int r = 0; r < Miswired::DM; r++) z[Miswired::DM * o + r] = zp[o][r];
}
template <int NCON> void scatter(const double *dcf, double **dc)
{
	for (int j = 0; j < NCON; j++)
		for (int v = 0; v < NZ; v++) dc[j][v] = dcf[j * NZ + v];
}
}  // namespace

extern "C" {
void mw_icf(int *mode, int *, double *f, double *df, double **zp)
{
	double z[NZ], g[NZ], v;
	gather(zp, z);
	Miswired::icf(NOUT, z, v, g);
	if (*mode == 0 || *mode == 2) *f = v;
	if (*mode == 1 || *mode == 2) for (int k = 0; k < NZ; k++) df[k] = g[k];
}
void mw_fcf(int *mode, int *, double *f, double *df, double **zp)
{
	double z[NZ], g[NZ], v;
	gather(zp, z);
	Miswired::fcf(NOUT, z, v, g);
	if (*mode == 0 || *mode == 2) *f = v;
	if (*mode == 1 || *mode == 2) for (int k = 0; k < NZ; k++) df[k] = g[k];
}
void mw_ucf(int *mode, int *, int *i, double *f, double *df, double **zp)
{
	double z[NZ], g[NZ], v;
	gather(zp, z);
	Miswired::ucf(NOUT, *i, z, v, g);
	if (*mode == 0 || *mode == 2) *f = v;
	if (*mode == 1 || *mode == 2) for (int k = 0; k < NZ; k++) df[k] = g[k];
}
void mw_nlicf(int *mode, int *, double *c, double **dc, double **zp)
{
	double z[NZ], cv[Miswired::NNLIC], d[Miswired::NNLIC * NZ];
	gather(zp, z);
	Miswired::nlicf(NOUT, z, cv, d);
	if (*mode == 0 || *mode == 2) for (int j = 0; j < Miswired::NNLIC; j++) c[j] = cv[j];
	if (*mode == 1 || *mode == 2) scatter<Miswired::NNLIC>(d, dc);
}
void mw_nltcf(int *mode, int *, int *i, double *c, double **dc, double **zp)
{
	double z[NZ], cv[Miswired::NNLTC], d[Miswired::NNLTC * NZ];
	gather(zp, z);
	Miswired::nltcf(NOUT, *i, z, cv, d);
	if (*mode == 0 || *mode == 2) for (int j = 0; j < Miswired::NNLTC; j++) c[j] = cv[j];
	if (*mode == 1 || *mode == 2) scatter<Miswired::NNLTC>(d, dc);
}
void mw_nlfcf(int *mode, int *, double *c, double **dc, double **zp)
{
	double z[NZ], cv[Miswired::NNLFC], d[Miswired::NNLFC * NZ];
	gather(zp, z);
	Miswired::nlfcf(NOUT, z, cv, d);
	if (*mode == 0 || *mode == 2) for (int j = 0; j < Miswired::NNLFC; j++) c[j] = cv[j];
	if (*mode == 1 || *mode == 2) scatter<Miswired::NNLFC>(d, dc);
}
}
