// warp.h - drop-in for PRLib's header of the same name (src/warp.h:49-73): declares both prl::warpCrop overloads with the
// reference's signatures, defaults and CV_EXPORTS linkage.  A caller that includes "warp.h" builds against this repository
// with only its include path changed to include/prl; the declarations themselves live in prl.h.
#ifndef PRLIB_HIP_DROPIN_warp_h
#define PRLIB_HIP_DROPIN_warp_h
#include "prl.h"
#endif  // PRLIB_HIP_DROPIN_warp_h
