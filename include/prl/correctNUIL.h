// correctNUIL.h - drop-in for PRLib's header of the same name (src/correctNUIL.h:32): declares prl::correctNUIL with the
// reference's signature, default and CV_EXPORTS linkage.  A caller that includes "correctNUIL.h" builds against this repository
// with only its include path changed to include/prl; the declarations themselves live in prl.h.
#ifndef PRLIB_HIP_DROPIN_correctNUIL_h
#define PRLIB_HIP_DROPIN_correctNUIL_h
#include "prl.h"
#endif  // PRLIB_HIP_DROPIN_correctNUIL_h
