// inst_g9.hip — explicit instantiations of the general-a curve kernels over a 9-limb field (192- and 224-bit curves; see ec_instances.h)
#include "ec_instances.h"
VMN_UNIT_G9(template)
