// balanceSimpleWhite.h - drop-in for PRLib's header of the same name (src/balance/balanceSimpleWhite.h:33): declares prl::simpleWhiteBalance with the
// reference's signature (no default arguments there).  A caller that includes "balanceSimpleWhite.h" builds against this repository
// with only its include path changed to include/prl; the declarations themselves live in prl.h.
#ifndef PRLIB_HIP_DROPIN_balanceSimpleWhite_h
#define PRLIB_HIP_DROPIN_balanceSimpleWhite_h
#include "prl.h"
#endif  // PRLIB_HIP_DROPIN_balanceSimpleWhite_h
