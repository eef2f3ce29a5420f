// What the two halves of the C ABI share: capi.cpp holds the handle API and the library's initialisation, capi_stage.cpp the
// handle-free calls, which refuse to touch a device before init_ratelib has succeeded.  No state crosses between them but this.
#pragma once

namespace rsmp {

// true from a successful init_ratelib to close_ratelib (capi.cpp).  Hidden: the library exports its C ABI, not this.
__attribute__((visibility("hidden"))) bool ratelib_initialized();

} // namespace rsmp
