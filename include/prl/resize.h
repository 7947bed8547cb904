// resize.h - drop-in for PRLib's header of the same name (src/resize.h:32): declares prl::resize with the reference's signature
// (no defaults) and CV_EXPORTS linkage.  A caller that includes "resize.h" builds against this repository with only its include
// path changed to include/prl; the declaration itself lives in prl.h.
#ifndef PRLIB_HIP_DROPIN_resize_h
#define PRLIB_HIP_DROPIN_resize_h
#include "prl.h"
#endif  // PRLIB_HIP_DROPIN_resize_h
