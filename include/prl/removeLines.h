// removeLines.h - drop-in for PRLib's header of the same name (src/removeLines.h:38): declares prl::removeLines with the
// reference's signature and CV_EXPORTS linkage.  A caller that includes "removeLines.h" builds against this repository
// with only its include path changed to include/prl; the declarations themselves live in prl.h.
#ifndef PRLIB_HIP_DROPIN_removeLines_h
#define PRLIB_HIP_DROPIN_removeLines_h
#include "prl.h"
#endif  // PRLIB_HIP_DROPIN_removeLines_h
