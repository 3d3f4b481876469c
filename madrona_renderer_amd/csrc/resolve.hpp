// The resolve stage of a supersampled renderer: s x s samples per native pixel -> the tensors
// the caller sees.  One launch per step for every selected output (resolve.hip).
#pragma once

#include <cstdint>

#include <hip/hip_runtime_api.h>

namespace mrx {

// The sample tensors are [rows * s][nfast * s] dwords, the native ones [rows][nfast]; rows = views * storage_slow (a
// view's sample rows follow one another, so native row r owns sample rows s * r ... s * r + s - 1 whatever its view).
// A null pair = an output that is not rendered.  Depth, ids and normals travel as their bit patterns.
struct ResolveParams {
    const uint32_t *rgbIn, *depthIn, *idsIn, *normalIn;
    uint32_t *rgbOut, *depthOut, *idsOut, *normalOut;
    uint32_t rows;      // native rows of all views
    uint32_t nfast;     // native pixels per row
    uint32_t numCUs;
};

// how many native pixels the resolve can address (its work items are counted in 32 bits)
constexpr uint64_t kResolveMaxPixels = 0xFFFFFFFFull;

// s = 2, 3, 4; anything else is hipErrorInvalidValue -- there is no other path.  Enqueues one kernel on `stream`.
hipError_t launchResolve(const ResolveParams &p, int s, hipStream_t stream);

}  // namespace mrx
