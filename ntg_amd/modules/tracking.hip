// tracking.hip -- the tracking family (tracking_family.hpp) as a loadable module: a plan must have its two flat outputs, and every
// problem carries its reference path as parameters (ntg_plan_set_params, 2 nbps doubles).
#include "tracking_family.hpp"

NTG_AMD_FAMILY_MODULE(Tracking, "tracking", 2)
