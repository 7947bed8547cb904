// blurDetection.h - drop-in for PRLib's header of the same name (src/detectors/blurDetection.h): declares prl::isBlurred with the
// reference's signature and CV_EXPORTS linkage, and the extension prl::focusMeasures.  As in the reference (blurDetection.cpp:85-89)
// prl::isBlurred returns false without looking at the image: the reference has no threshold for any of its four focus measures
// and calls none of them; prl::focusMeasures is what computes them.  A caller that includes "blurDetection.h" builds against this
// repository with only its include path changed to include/prl; the declarations themselves live in prl.h.
#ifndef PRLIB_HIP_DROPIN_blurDetection_h
#define PRLIB_HIP_DROPIN_blurDetection_h
#include "prl.h"
#endif  // PRLIB_HIP_DROPIN_blurDetection_h
