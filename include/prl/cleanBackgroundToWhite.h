// cleanBackgroundToWhite.h - drop-in for PRLib's header of the same name (src/cleanBackgroundToWhite.h:40): declares prl::cleanBackgroundToWhite with the
// reference's signature (no default arguments there).  A caller that includes "cleanBackgroundToWhite.h" builds against this repository
// with only its include path changed to include/prl; the declarations themselves live in prl.h.
#ifndef PRLIB_HIP_DROPIN_cleanBackgroundToWhite_h
#define PRLIB_HIP_DROPIN_cleanBackgroundToWhite_h
#include "prl.h"
#endif  // PRLIB_HIP_DROPIN_cleanBackgroundToWhite_h
