// binarizePureAdaptiveGaussian.h - drop-in for PRLib's header of the same name (src/binarizations/binarizePureAdaptiveGaussian.h:33): declares
// prl::binarizePureAdaptiveGaussian with the reference's signature and CV_EXPORTS linkage.  A caller that includes "binarizePureAdaptiveGaussian.h" builds
// against this repository with only its include path changed to include/prl; the declarations themselves live in prl.h.
#ifndef PRLIB_HIP_DROPIN_binarizePureAdaptiveGaussian_h
#define PRLIB_HIP_DROPIN_binarizePureAdaptiveGaussian_h
#include "prl.h"
#endif  // PRLIB_HIP_DROPIN_binarizePureAdaptiveGaussian_h
