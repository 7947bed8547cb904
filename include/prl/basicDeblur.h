// basicDeblur.h - drop-in for PRLib's header of the same name (src/deblur/basicDeblur.h): declares prl::basicDeblur with the
// reference's signature, defaults (gaussianKernelSize = 0, sigmaX = 9.0, sigmaY = 0.0, imageWeight = 0.75) and CV_EXPORTS linkage.
// A caller that includes "basicDeblur.h" builds against this repository with only its include path changed to include/prl; the
// declaration itself lives in prl.h.  The reference's wienerFilter (src/deblur/wienerFilter.h, a DFT) is not provided.
#ifndef PRLIB_HIP_DROPIN_basicDeblur_h
#define PRLIB_HIP_DROPIN_basicDeblur_h
#include "prl.h"
#endif  // PRLIB_HIP_DROPIN_basicDeblur_h
