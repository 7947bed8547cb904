// balanceGrayWorldWhite.h - drop-in for PRLib's header of the same name (src/balance/balanceGrayWorldWhite.h:33): declares prl::grayWorldWhiteBalance with the
// reference's signature (no default arguments there).  A caller that includes "balanceGrayWorldWhite.h" builds against this repository
// with only its include path changed to include/prl; the declarations themselves live in prl.h.
#ifndef PRLIB_HIP_DROPIN_balanceGrayWorldWhite_h
#define PRLIB_HIP_DROPIN_balanceGrayWorldWhite_h
#include "prl.h"
#endif  // PRLIB_HIP_DROPIN_balanceGrayWorldWhite_h
