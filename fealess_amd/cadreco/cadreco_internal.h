// cadreco_internal.h -- what cadreco_train.cpp and cadreco_c.cpp need from the facade class, which stays private to
// obj_reco_lmicp_hip.cpp.  Not for callers: nothing declared here is exported from libcadreco_hip.so.
#ifndef FEALESS_CADRECO_INTERNAL_H
#define FEALESS_CADRECO_INTERNAL_H

#include "fealess_cadreco.h"
#include "../../include/fealess_hip.h"

#include <cstdio>

#define CADRECO_LOCAL __attribute__((visibility("hidden")))

// false: not a handle of this library.  *ctx: the handle's context, nullptr when it found no GPU
CADRECO_LOCAL bool cadreco_context(CObjRecoCAD *handle, fl_context **ctx);
// false: not a handle of this library
CADRECO_LOCAL bool cadreco_set_recognition_params(CObjRecoCAD *handle, const fl_recognition_params &params);

// the library's message for the call that just failed goes to stderr; returns `code`, the facade's code for that failure
static inline int fl_fail(fl_context *ctx, int code)
{
  fprintf(stderr, "[fealess_hip] %s\n", fl_last_error(ctx));
  return code;
}

#endif  // FEALESS_CADRECO_INTERNAL_H
