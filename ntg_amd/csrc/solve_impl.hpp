// solve_impl.hpp -- what a family translation unit instantiates: the templated device code of eval_kernel and
// sqp_kernel (gfx950) and their launchers, layer by layer.  Included only by units that instantiate one of the two
// kernels: the per-family units (fam_*.hip: one per problem family, so that they compile in parallel) and the
// header of the loadable family modules (ntg_amd_family.hpp).  Everything else includes the layer it names.
#pragma once
#include "wave_ops.hpp"       // wavefront and workgroup primitives
#include "newton.hpp"         // structured Newton step (and through nwt_map.hpp the memory map, the QP step)
#include "lds_tables.hpp"     // the LDS view of a plan
#include "eval.hpp"           // the evaluation, eval_kernel
#include "direction.hpp"      // the pieces of a search direction
#include "sqp_kernel.hpp"     // sqp_kernel
#include "solve_launch.hpp"   // the launch ladders
