// denoiseSaltPepper.h - drop-in for PRLib's header of the same name (src/denoise/denoiseSaltPepper.h:40): declares
// prl::denoiseSaltPepper with the reference's signature and CV_EXPORTS linkage.  A caller that includes "denoiseSaltPepper.h" (as
// samples/denoise/denoiseSaltPepper_sample.cpp does) builds against this repository with only its include path changed to
// include/prl; the declarations themselves live in prl.h.
#ifndef PRLIB_HIP_DROPIN_denoiseSaltPepper_h
#define PRLIB_HIP_DROPIN_denoiseSaltPepper_h
#include "prl.h"
#endif  // PRLIB_HIP_DROPIN_denoiseSaltPepper_h
