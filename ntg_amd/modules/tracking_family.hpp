// tracking_family.hpp -- reference tracking as a user problem family with per-problem parameters (include/ntg_amd_family.hpp).
//
// Flat outputs x (output 0) and y (output 1), maxderiv 3: z = [x, x', x'', y, y', y''].
//   running cost   W ((x - xr_i)^2 + (y - yr_i)^2) + x''^2 + y''^2     follow the problem's own reference (xr_i, yr_i) at breakpoint i
//   parameters     NPARAM_BP = 2: prm[2 i], prm[2 i + 1] = (xr_i, yr_i) for every breakpoint i (2 nbps doubles per problem)
// No nonlinear rows; the spec's linear rows pin the ends (configs.config_TR).
//
// The callbacks are NTG_AMD_HD (host and device): the module (tracking.hip) and a plain C++ host shim compile this same header.
#pragma once
#include "ntg_amd_family.hpp"

struct Tracking : ntg_amd::FamilyDefaults<Tracking> {
	static constexpr int NPARAM_BP = 2;
	static constexpr double W = 4.0;
	static NTG_AMD_HD void ucf(int, int i, const double *z, double &f, double *df, const double *prm)
	{
		const double ex = z[0] - prm[NPARAM + NPARAM_BP * i], ey = z[3] - prm[NPARAM + NPARAM_BP * i + 1];
		f = W * (ex * ex + ey * ey) + z[2] * z[2] + z[5] * z[5];
		df[0] = 2.0 * W * ex; df[1] = 0.0; df[2] = 2.0 * z[2];
		df[3] = 2.0 * W * ey; df[4] = 0.0; df[5] = 2.0 * z[5];
	}
};
