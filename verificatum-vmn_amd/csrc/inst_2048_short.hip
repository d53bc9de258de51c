// inst_2048_short.hip — explicit instantiations of one group of geometries (see modp_instances.h)
#include "modp_instances.h"
VMN_UNIT_2048_SHORT(template)
