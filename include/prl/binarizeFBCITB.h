// binarizeFBCITB.h - drop-in for PRLib's header of the same name (src/binarizations/binarizeFBCITB.h): declares prl::binarizeFBCITB
// with the reference's signature, defaults (both stages, CLAHE, the bilateral filter, the morphology and Canny on the variances on;
// varianceMapThreshold = 200, CLAHEClipLimit = 2, gaussianBlurKernelSize = 9, the Canny coefficients 0.6 and 0.4,
// boundingRectangleMaxArea = 0.3, bilateralKernelSize = 5, both bilateral sigmas 150) and CV_EXPORTS linkage.  A caller that includes
// "binarizeFBCITB.h" builds against this repository with only its include path changed to include/prl; the declaration itself
// lives in prl.h.  The reference's OPERATIONS and FBCITB_ParamsCodes enumerations belong to a call form it has commented out and
// are not provided.
#ifndef PRLIB_HIP_DROPIN_binarizeFBCITB_h
#define PRLIB_HIP_DROPIN_binarizeFBCITB_h
#include "prl.h"
#endif  // PRLIB_HIP_DROPIN_binarizeFBCITB_h
