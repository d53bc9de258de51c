// inst_g21.hip — explicit instantiations of the general-a curve kernels over a 21-limb field (512-bit curves; see ec_instances.h)
#include "ec_instances.h"
VMN_UNIT_G21(template)
