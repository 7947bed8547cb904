// binarizeNativeAdaptive.h - drop-in for PRLib's header of the same name (src/binarizations/binarizeNativeAdaptive.h:62-74): declares
// prl::binarizeNativeAdaptive with the reference's signature and CV_EXPORTS linkage.  A caller that includes "binarizeNativeAdaptive.h" builds
// against this repository with only its include path changed to include/prl; the declarations themselves live in prl.h.
#ifndef PRLIB_HIP_DROPIN_binarizeNativeAdaptive_h
#define PRLIB_HIP_DROPIN_binarizeNativeAdaptive_h
#include "prl.h"
#endif  // PRLIB_HIP_DROPIN_binarizeNativeAdaptive_h
