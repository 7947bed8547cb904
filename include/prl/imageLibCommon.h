// imageLibCommon.h - drop-in for the part of PRLib's header of the same name (src/imageLibCommon.h) that this repository provides:
// EnhanceLocalContrastByCLAHE with the reference's signature, in the global namespace as there.  A caller that includes
// "imageLibCommon.h" builds against this repository with only its include path changed to include/prl; the declarations live beside
// their implementation (prlib_amd/csrc/prl/imageLibCommon.h, prl_host.cpp).
#ifndef PRLIB_HIP_DROPIN_imageLibCommon_h
#define PRLIB_HIP_DROPIN_imageLibCommon_h
#include "../../prlib_amd/csrc/prl/imageLibCommon.h"
#endif  // PRLIB_HIP_DROPIN_imageLibCommon_h
