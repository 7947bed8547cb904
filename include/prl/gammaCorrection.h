// gammaCorrection.h - drop-in for PRLib's header of the same name (src/balance/gammaCorrection.h:33): declares prl::gammaCorrection with the
// reference's signature (no default arguments there).  A caller that includes "gammaCorrection.h" builds against this repository
// with only its include path changed to include/prl; the declarations themselves live in prl.h.
#ifndef PRLIB_HIP_DROPIN_gammaCorrection_h
#define PRLIB_HIP_DROPIN_gammaCorrection_h
#include "prl.h"
#endif  // PRLIB_HIP_DROPIN_gammaCorrection_h
