// inst_g10.hip — explicit instantiations of the general-a curve kernels over a 10-limb field (239- and 256-bit curves; see ec_instances.h)
#include "ec_instances.h"
VMN_UNIT_G10(template)
