// What the units of the C ABI (api.hip, api_lg.hip, api_geometry.hip, api_retrieval.hip, api_cameras.hip) share: the error setter and the launch and workspace checks -- each
// defined once, in api.hip -- and the limits that the argument checks and the *_workspace_bytes guards name.  Internal: in namespace xfh, so
// the exported xfh_* symbols are those of include/xfeat_hip.h and include/xfeat_hip_cameras.h alone.
#pragma once
#include "../../include/xfeat_hip.h"      // (size_t)

namespace xfh {
int fail(int code, const char* fmt, ...);                        // sets the thread's xfh_last_error() text (printf style); returns code
int check_launch(const char* what);                              // XFH_OK, or XFH_ERR_HIP with hipGetLastError()'s text
int check_ws(const void* ws, size_t have, size_t need);          // XFH_OK, or XFH_ERR_WORKSPACE: NULL, not 256-byte aligned, too small

constexpr int MAX_BATCH = 65535;          // pairs or scenes of one call: they are a grid dimension
constexpr int MAX_VIEWS = 32;             // views of a scene: a view set is the bits of one word
constexpr int MAX_ROWS = 1 << 24;         // rows of a key-point table, entries of a match list, tracks of a scene
constexpr int MAX_RANSAC_ITERS = 16384;   // hypotheses of one RANSAC call (the homography's own limit is lower)
}  // namespace xfh
