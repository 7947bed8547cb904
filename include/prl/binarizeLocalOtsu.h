// binarizeLocalOtsu.h - drop-in for PRLib's header of the same name (src/binarizations/binarizeLocalOtsu.h): declares
// prl::binarizeLocalOtsu with the reference's signature, defaults (maxValue = 255, CLAHEClipLimit = 0, GaussianBlurKernelSize = 19,
// CannyUpperThresholdCoeff = 0.15, CannyLowerThresholdCoeff = 0.01, CannyMorphIters = 1) and CV_EXPORTS linkage.  A caller that
// includes "binarizeLocalOtsu.h" builds against this repository with only its include path changed to include/prl; the declaration
// itself lives in prl.h.
#ifndef PRLIB_HIP_DROPIN_binarizeLocalOtsu_h
#define PRLIB_HIP_DROPIN_binarizeLocalOtsu_h
#include "prl.h"
#endif  // PRLIB_HIP_DROPIN_binarizeLocalOtsu_h
