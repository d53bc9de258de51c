// inst_g13.hip — explicit instantiations of the general-a curve kernels over a 13-limb field (320-bit curves; see ec_instances.h)
#include "ec_instances.h"
VMN_UNIT_G13(template)
