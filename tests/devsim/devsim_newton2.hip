// devsim_newton2.hip -- TEST-ONLY: the probe kernels of devsim_body.h over the headers as csrc/lane_kernel.hip compiles them
// (CVX_REFINE_NEWTON2: seed plus two Newton steps in rcp / rsqrt_, the guarded h2 in jacobi_cs_dl).  The inline namespace
// CVX_UNIT_TAG of solver_core.h makes linking this unit and devsim.hip into one library legal.
#define CVX_REFINE_NEWTON2
#define DS(name) ds2_##name
#include "devsim_body.h"
