// unicycle_family.hpp -- a planar vehicle as a user problem family, written the way a user of include/ntg_amd_family.hpp would.
//
// Flat outputs x (output 0) and y (output 1), maxderiv 3: z = [x, x', x'', y, y', y''].
//   running cost       x''^2 + y''^2                                   acceleration effort
//   initial cost       WI (x''^2 + y''^2)                              acceleration at the start
//   final cost         WF (x''^2 + y''^2)                              acceleration at the end
//   initial row        x'^2 + y'^2                                     speed^2, pinned per problem by its bounds
//   trajectory rows    x'^2 + y'^2                                     speed^2 <= vmax^2
//                      x' y'' - y' x''                                 (speed^3 x curvature: a lateral-acceleration proxy) in a band
//   final row          x'^2 + y'^2                                     final speed^2 within a range
// Linear rows of the spec pin the positions at both ends and the initial heading (configs.config_U).
//
// The callbacks are NTG_AMD_HD (host and device): the module (unicycle.hip) and a plain C++ host shim compile this same header.
#pragma once
#include "ntg_amd_family.hpp"

struct Unicycle : ntg_amd::FamilyDefaults<Unicycle> {
	static constexpr int NNLIC = 1, NNLTC = 2, NNLFC = 1;
	static constexpr double WI = 0.5, WF = 0.25;
	static NTG_AMD_HD void ucf(int, int, const double *z, double &f, double *df)
	{
		f = z[2] * z[2] + z[5] * z[5];
		df[0] = 0.0; df[1] = 0.0; df[2] = 2.0 * z[2];
		df[3] = 0.0; df[4] = 0.0; df[5] = 2.0 * z[5];
	}
	static NTG_AMD_HD void icf(int, const double *z, double &f, double *df)
	{
		f = WI * (z[2] * z[2] + z[5] * z[5]);
		df[0] = 0.0; df[1] = 0.0; df[2] = 2.0 * WI * z[2];
		df[3] = 0.0; df[4] = 0.0; df[5] = 2.0 * WI * z[5];
	}
	static NTG_AMD_HD void fcf(int, const double *z, double &f, double *df)
	{
		f = WF * (z[2] * z[2] + z[5] * z[5]);
		df[0] = 0.0; df[1] = 0.0; df[2] = 2.0 * WF * z[2];
		df[3] = 0.0; df[4] = 0.0; df[5] = 2.0 * WF * z[5];
	}
	// speed^2 and its gradient (one row of dc)
	static NTG_AMD_HD void speed2(const double *z, double *c, double *dc)
	{
		c[0] = z[1] * z[1] + z[4] * z[4];
		dc[0] = 0.0; dc[1] = 2.0 * z[1]; dc[2] = 0.0;
		dc[3] = 0.0; dc[4] = 2.0 * z[4]; dc[5] = 0.0;
	}
	static NTG_AMD_HD void nlicf(int, const double *z, double *c, double *dc) { speed2(z, c, dc); }
	static NTG_AMD_HD void nlfcf(int, const double *z, double *c, double *dc) { speed2(z, c, dc); }
	static NTG_AMD_HD void nltcf(int, int, const double *z, double *c, double *dc)
	{
		speed2(z, c, dc);
		c[1] = z[1] * z[5] - z[4] * z[2];
		dc[6] = 0.0; dc[7] = z[5]; dc[8] = -z[4];
		dc[9] = 0.0; dc[10] = -z[2]; dc[11] = z[1];
	}
};
