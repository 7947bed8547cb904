// autoCrop.h - drop-in for PRLib's header of the same name (src/border_detection/autoCrop.h:42-53): declares prl::documentContour
// and prl::autoCrop with the reference's signatures and CV_EXPORTS linkage.  A caller that includes "autoCrop.h" builds against
// this repository with only its include path changed to include/prl; the declarations themselves live in prl.h.
#ifndef PRLIB_HIP_DROPIN_autoCrop_h
#define PRLIB_HIP_DROPIN_autoCrop_h
#include "prl.h"
#endif  // PRLIB_HIP_DROPIN_autoCrop_h
