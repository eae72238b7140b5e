// unicycle.hip -- the unicycle family (unicycle_family.hpp) as a loadable module: a plan must have its two flat outputs.
#include "unicycle_family.hpp"

NTG_AMD_FAMILY_MODULE(Unicycle, "unicycle", 2)
