// obstacle_field.hpp -- the arithmetic of NTG_FAM_OBSTACLE_FIELD: a per-problem field of up to MAXOBS circular obstacles.
//
// Two flat outputs x (output 0) and y (output 1), maxderiv 3: z = [x, x', x'', y, y', y''].
//   running cost      x''^2 + y''^2                           (the kincar cost)
//   trajectory rows   c_j = (x - cx_j)^2 + (y - cy_j)^2       j < m = nnltc <= MAXOBS; c_j >= r_j^2 through the bounds
//   parameters        prm = [cx_0, cy_0, ..., cx_{m-1}, cy_{m-1}] per problem (2 m doubles)
// The callbacks compile as host and device code: families.hpp wraps them as Family<NTG_FAM_OBSTACLE_FIELD>, and a plain C++ host
// shim (the CPU oracle's callbacks in the tests) compiles the same arithmetic.  With m = 1 and (cx_0, cy_0) = (20, 0.5) every
// expression is the one of Family<NTG_FAM_OBSTACLE>, operand for operand.
#pragma once

#if defined(__HIP__) || defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define NTG_OF_HD __host__ __device__ __forceinline__
#else
#define NTG_OF_HD inline
#endif

namespace ntg_amd {

struct ObstacleField {
	static constexpr int MAXOBS = 8, NZ = 6;
	static NTG_OF_HD void ucf(int nout, const double *z, double &f, double *df)
	{
		double s = 0.0;
		for (int o = 0; o < nout; o++) {
			s += z[3 * o + 2] * z[3 * o + 2];
			df[3 * o] = 0.0; df[3 * o + 1] = 0.0; df[3 * o + 2] = 2.0 * z[3 * o + 2];
		}
		f = s;
	}
	// values of the m rows
	static NTG_OF_HD void val(int m, const double *z, double *c, const double *prm)
	{
#pragma unroll
		for (int j = 0; j < MAXOBS; j++) {
			if (j < m) {
				const double dx = z[0] - prm[2 * j], dy = z[3] - prm[2 * j + 1];
				c[j] = dx * dx + dy * dy;
			}
		}
	}
	// df += J' t: row j depends on x and y only
	static NTG_OF_HD void vjp(int m, const double *z, const double *t, double *df, const double *prm)
	{
#pragma unroll
		for (int j = 0; j < MAXOBS; j++) {
			if (j < m) {
				const double dx = z[0] - prm[2 * j], dy = z[3] - prm[2 * j + 1];
				df[0] += t[j] * (2.0 * dx);
				df[3] += t[j] * (2.0 * dy);
			}
		}
	}
	// dense form: c[m], dc[m][nz] row-major (the reference's dc[constraint][variable])
	static NTG_OF_HD void dense(int nout, int m, const double *z, double *c, double *dc, const double *prm)
	{
		for (int j = 0; j < m; j++) {
			const double dx = z[0] - prm[2 * j], dy = z[3] - prm[2 * j + 1];
			c[j] = dx * dx + dy * dy;
			for (int v = 0; v < 3 * nout; v++) dc[j * 3 * nout + v] = 0.0;
			dc[j * 3 * nout] = 2.0 * dx; dc[j * 3 * nout + 3] = 2.0 * dy;
		}
	}
	// B (2 x 2, constraint flag entries x, y) = sum_j mu a_j a_j' [t_j != 0] + 2 t_j I [curv],  a_j = 2 (x - cx_j, y - cy_j): the
	// second-order model of the rows' augmented-Lagrangian terms
	static NTG_OF_HD void block(int m, const double *z, const double *t, double mu, bool curv, double *B, const double *prm)
	{
#pragma unroll
		for (int j = 0; j < MAXOBS; j++) {
			if (j < m) {
				const double dx = z[0] - prm[2 * j], dy = z[3] - prm[2 * j + 1], a0 = 2.0 * dx, a1 = 2.0 * dy, mj = t[j] != 0.0 ? mu : 0.0,
				             h = curv ? 2.0 * t[j] : 0.0;
				if (j == 0) {
					B[0] = mj * a0 * a0 + h; B[1] = mj * a0 * a1; B[2] = mj * a1 * a0; B[3] = mj * a1 * a1 + h;
				} else {
					B[0] += mj * a0 * a0 + h; B[1] += mj * a0 * a1; B[2] += mj * a1 * a0; B[3] += mj * a1 * a1 + h;
				}
			}
		}
	}
};

}  // namespace ntg_amd
