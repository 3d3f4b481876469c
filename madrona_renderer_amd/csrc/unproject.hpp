// The unprojection stage of a renderer with the position output: the depth tensor the caller
// sees -> one xyzw point per pixel, in view or in world space.  One launch per step behind the render (and the
// resolve, where there is one) on the same stream (unproject.hip).
#pragma once

#include <cstdint>

#include <hip/hip_runtime_api.h>

#include "raster.hpp"

namespace mrx {

enum UnprojectFrame : int32_t { kFrameNone = 0, kFrameWorld = 1, kFrameView = 2 };   // mrx_positions' values

// depth is [views][nslow][nfast] floats, pos [views][nslow][nfast][4], both NATIVE (on a supersampled renderer the
// resolved depth); sx ox sz oz / viewProj are the constants the render used, those of the SAMPLE image, and a native
// pixel (x, y) stands for sample (s * x + half, s * y + half).  Pose and projection are read when the kernel runs.
struct UnprojectParams {
    const float *depth;
    float *pos;                     // 16-byte aligned
    const float *camPos;            // [views][3]
    const float *camRot;            // [views][4] w, x, y, z
    const ViewProj *viewProj;       // [views], or null: the uniform constants below
    float sx, ox, sz, oz;
    uint32_t numViews, nfast, nslow;
    uint32_t s, half;               // supersampling factor (1 without) and s / 2
    int32_t frame;                  // kFrameWorld or kFrameView
    int32_t transposed;             // Raytracer-mode [x][y] storage
    uint32_t numCUs;
};

// how many native pixels the stage can address (its work items are counted in 32 bits)
constexpr uint64_t kUnprojectMaxPixels = 0xFFFFFFFFull;

// Enqueues one kernel on `stream`.  hipErrorInvalidValue for a frame other than the two, a factor outside 1 ... 4, an
// unaligned position tensor or more pixels than kUnprojectMaxPixels -- there is no other path.
hipError_t launchUnproject(const UnprojectParams &p, hipStream_t stream);

}  // namespace mrx
