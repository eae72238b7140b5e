// testfam_module.hip -- the built-in NTG_FAM_TESTFAM family restated as a loadable module.
//
// A built-in family maps onto the module form one to one: the functor struct of families.hpp becomes the module's family (here
// by inheritance, unchanged), and NTG_AMD_FAMILY_MODULE instantiates the same generic kernels fam_testfam.hip instantiates for it.
// The module's results are therefore bit-for-bit those of the built-in family wherever the built-in runs its generic instance --
// the yardstick of the load-and-dispatch path (tests/test_gpu_family_modules.py).
#include "ntg_amd_family.hpp"

struct TestfamModule : Family<NTG_FAM_TESTFAM> {};

NTG_AMD_FAMILY_MODULE(TestfamModule, "testfam_module", 0)
