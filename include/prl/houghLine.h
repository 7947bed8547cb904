// houghLine.h - drop-in for PRLib's header of the same name (src/border_detection/houghLine.h): declares
// prl::findHoughLineContour with the reference's signature and CV_EXPORTS linkage.  A caller that includes "houghLine.h" builds
// against this repository with only its include path changed to include/prl; the declaration itself lives in prl.h.
#ifndef PRLIB_HIP_DROPIN_houghLine_h
#define PRLIB_HIP_DROPIN_houghLine_h
#include "prl.h"
#endif  // PRLIB_HIP_DROPIN_houghLine_h
