// miswired_family.hpp -- TEST INFRASTRUCTURE: a problem family with three PLANTED integration errors, for the tests of ntg_batch_verify
// (tests/test_gpu_verify.py, tests/test_verify_oracle.py).  It is kept out of ntg_amd/modules so that it is never shipped: nobody should
// solve with it.  Written like a user's family (include/ntg_amd_family.hpp); all six slots, DM = 3, smooth functions of order 1.
//
// Flat outputs x (output 0) and y (output 1): z = [x, x', x'', y, y', y''].
//   initial cost       (x - 1)^2 / 2 + y'^2 / 4 + x y / 10
//   running cost       x^2 / 2 + x'^2 / 10 + (x''^2 + y''^2) / 200 + sin(y) x'' / 20          DEFECT 2: the sign of df[x'']
//   final cost         (x^2 + y^2) / 2 + y'' (1 + x^2) / 20                                    DEFECT 3: reads y'', which the test plan's fcostav omits
//   initial row        x'^2 + y'^2 + x
//   trajectory rows    x^2 + y^2
//                      x' y' + cos(x)                                                          DEFECT 1: dc[1][y'] is 1 + 1/64 times too large
//   final row          x'^2 + y'^2
// Every other derivative is correct.
//
// The callbacks are NTG_AMD_HD (host and device): the module (miswired.hip) and a plain C++ host shim compile this same header.
#pragma once
#include <math.h>
#include "ntg_amd_family.hpp"

struct Miswired : ntg_amd::FamilyDefaults<Miswired> {
	static constexpr int NNLIC = 1, NNLTC = 2, NNLFC = 1;
	static NTG_AMD_HD void icf(int, const double *z, double &f, double *df)
	{
		f = 0.5 * (z[0] - 1.0) * (z[0] - 1.0) + 0.25 * z[4] * z[4] + 0.1 * z[0] * z[3];
		df[0] = (z[0] - 1.0) + 0.1 * z[3]; df[1] = 0.0; df[2] = 0.0;
		df[3] = 0.1 * z[0]; df[4] = 0.5 * z[4]; df[5] = 0.0;
	}
	static NTG_AMD_HD void ucf(int, int, const double *z, double &f, double *df)
	{
		const double s = sin(z[3]);
		f = 0.5 * z[0] * z[0] + 0.1 * z[1] * z[1] + 0.005 * (z[2] * z[2] + z[5] * z[5]) + 0.05 * s * z[2];
		df[0] = z[0]; df[1] = 0.2 * z[1];
		df[2] = -(0.01 * z[2] + 0.05 * s);   // DEFECT 2 (planted): wrong sign; the derivative is 0.01 z[2] + 0.05 sin(z[3])
		df[3] = 0.05 * cos(z[3]) * z[2]; df[4] = 0.0; df[5] = 0.01 * z[5];
	}
	static NTG_AMD_HD void fcf(int, const double *z, double &f, double *df)
	{
		// DEFECT 3 (planted): the function reads z[5] = (output 1, deriv 2), which the test plan's fcostav does not name (the solver would
		// hand it a zero there); the gradient itself is correct
		f = 0.5 * (z[0] * z[0] + z[3] * z[3]) + 0.05 * z[5] * (1.0 + z[0] * z[0]);
		df[0] = z[0] + 0.1 * z[5] * z[0]; df[1] = 0.0; df[2] = 0.0;
		df[3] = z[3]; df[4] = 0.0; df[5] = 0.05 * (1.0 + z[0] * z[0]);
	}
	static NTG_AMD_HD void speed2(const double *z, double *c, double *dc)
	{
		c[0] = z[1] * z[1] + z[4] * z[4];
		dc[0] = 0.0; dc[1] = 2.0 * z[1]; dc[2] = 0.0;
		dc[3] = 0.0; dc[4] = 2.0 * z[4]; dc[5] = 0.0;
	}
	static NTG_AMD_HD void nlicf(int, const double *z, double *c, double *dc)
	{
		speed2(z, c, dc);
		c[0] += z[0]; dc[0] = 1.0;
	}
	static NTG_AMD_HD void nlfcf(int, const double *z, double *c, double *dc) { speed2(z, c, dc); }
	static NTG_AMD_HD void nltcf(int, int, const double *z, double *c, double *dc)
	{
		c[0] = z[0] * z[0] + z[3] * z[3];
		dc[0] = 2.0 * z[0]; dc[1] = 0.0; dc[2] = 0.0;
		dc[3] = 2.0 * z[3]; dc[4] = 0.0; dc[5] = 0.0;
		c[1] = z[1] * z[4] + cos(z[0]);
		dc[6] = -sin(z[0]); dc[7] = z[4]; dc[8] = 0.0;
		dc[9] = 0.0; dc[11] = 0.0;
		dc[10] = z[1] * (1.0 + 1.0 / 64.0);   // DEFECT 1 (planted): the derivative is z[1]
	}
};
