// inst_g15.hip — explicit instantiations of the general-a curve kernels over a 15-limb field (384-bit curves; see ec_instances.h)
#include "ec_instances.h"
VMN_UNIT_G15(template)
