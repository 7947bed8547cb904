// binarizeAT.h - drop-in for PRLib's header of the same name (src/binarizations/binarizeAT.h:33): declares
// prl::binarizeAT with the reference's signature and CV_EXPORTS linkage.  A caller that includes "binarizeAT.h" builds
// against this repository with only its include path changed to include/prl; the declarations themselves live in prl.h.
#ifndef PRLIB_HIP_DROPIN_binarizeAT_h
#define PRLIB_HIP_DROPIN_binarizeAT_h
#include "prl.h"
#endif  // PRLIB_HIP_DROPIN_binarizeAT_h
