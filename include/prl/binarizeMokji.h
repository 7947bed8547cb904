// binarizeMokji.h - drop-in for PRLib's header of the same name (src/binarizations/binarizeMokji.h): declares prl::binarizeMokji
// with the reference's signature, defaults and CV_EXPORTS linkage.  A caller that includes "binarizeMokji.h" builds against this
// repository with only its include path changed to include/prl; the declarations themselves live in prl.h.
#ifndef PRLIB_HIP_DROPIN_binarizeMokji_h
#define PRLIB_HIP_DROPIN_binarizeMokji_h
#include "prl.h"
#endif  // PRLIB_HIP_DROPIN_binarizeMokji_h
