// miswired.hip -- TEST INFRASTRUCTURE: the family with planted errors (miswired_family.hpp) as a loadable module; a plan must have its
// two flat outputs.
#include "miswired_family.hpp"

NTG_AMD_FAMILY_MODULE(Miswired, "miswired", 2)
