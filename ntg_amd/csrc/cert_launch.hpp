// cert_launch.hpp -- the one launcher of the time certificates (certs.hip: envelope, envelope_sos, extrema, forms, separation) and of the
// bisection calls with a translation unit of their own (ratios.hip, trig.hip, minmax.hip).  Host code.
//
// Each call has a kernel for per-problem grids (kpp: one problem per wave, a workgroup per nt / 64 problems) and one for shared grids (ksh:
// persistent workgroups; each builds its tables once, so each should stream several of the `units` of work: a workgroup for every four of
// them, no more than fill the device).  g is the call's CertBase: A.g, or A.f.g where the argument block wraps a FormArgs.
//
// The calls whose workgroup size is a figure of the launch (nw waves: ratios, trig, minmax) pass nt = 64 nw and units = (batch + nw - 1) / nw:
//   groups = (batch + nt / 64 - 1) / (nt / 64) = (batch + nw - 1) / nw = units, so
//   grid   = pp ? min(units, 8 ncu) : max(1, min((units + 3) / 4, 8 ncu)), with 64 nw threads,
// which is what their own launchers computed.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include "ntg_dev.hpp"

template <class Args>
static hipError_t launch_cert(void (*kpp)(Args), void (*ksh)(Args), const Args &A, const CertBase &g, int nt, int units, int ncu, size_t lds, hipStream_t st)
{
	const int groups = (g.batch + nt / 64 - 1) / (nt / 64);
	auto kfn = g.pp ? kpp : ksh;
	if (lds > 64 * 1024) {
		const hipError_t e = hipFuncSetAttribute((const void *)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
		if (e != hipSuccess) return e;
	}
	const int grid = g.pp ? std::min(groups, 8 * ncu) : std::max(1, std::min((units + 3) / 4, 8 * ncu));
	hipLaunchKernelGGL(kfn, dim3(grid), dim3(nt), lds, st, A);
	return hipGetLastError();
}
