// The observation stage of a renderer with the packed observation output: the rgb and depth
// tensors the caller sees -> one channel-first tensor [views][S * C][H][W] in the precision a policy runs in, with
// optional luma, optional depth normalisation and an optional stack of the last S frames.  One launch per step behind
// the render, the resolve, the unprojection and the boxes on the same stream, and a clear of the reset column behind
// it (observe.hip).
#pragma once

#include <cstdint>

#include <hip/hip_runtime_api.h>

namespace mrx {

// the layout field's values (mrx.h MRX_OBS_*): C = 3, 4, 1, 1, 2
enum ObserveLayout : uint32_t { kObsNone = 0, kObsRgb = 1, kObsRgbd = 2, kObsD = 3, kObsY = 4, kObsYd = 5 };
// the dtype field's values
enum ObserveDtype : uint32_t { kObsF32 = 0, kObsF16 = 1, kObsBf16 = 2, kObsU8 = 3 };
// the kernel's forms: x-fast storage one pixel per lane, x-fast storage four pixels per lane, x-slow storage through LDS
enum ObserveForm : uint32_t { kObsNarrow = 0, kObsWide = 1, kObsTile = 2 };

constexpr uint32_t kObsMaxStack = 8;

// channels of a layout, 0 for a value that is none; whether it reads rgb / depth; bytes of an element
constexpr uint32_t observeChannels(uint32_t layout)
{
    return layout == kObsRgb ? 3u : layout == kObsRgbd ? 4u : layout == kObsD || layout == kObsY ? 1u
         : layout == kObsYd ? 2u : 0u;
}
constexpr bool observeReadsColour(uint32_t layout) { return layout != kObsD && observeChannels(layout) != 0; }
constexpr bool observeReadsDepth(uint32_t layout) { return layout == kObsRgbd || layout == kObsD || layout == kObsYd; }
constexpr uint32_t observeElemBytes(uint32_t dtype) { return dtype == kObsF32 ? 4u : dtype == kObsU8 ? 1u : 2u; }

// rgb is [views][nslow][nfast] RGBA8 words, depth [views][nslow][nfast] floats, both NATIVE (on a supersampled renderer
// the resolved tensors); obs is [views][S * C][H][W] elements with (H, W) = (nslow, nfast), or (nfast, nslow) on
// transposed storage, where the stage undoes the transposition.
struct ObserveParams {
    const uint32_t *rgb;            // null when the layout has no colour
    const float *depth;             // null when the layout has no depth
    void *obs;                      // 16-byte aligned
    uint8_t *reset;                 // [views], null when stack == 1; cleared behind the kernel
    uint32_t numViews, nfast, nslow;
    uint32_t layout, dtype, stack;
    int32_t hasRange;               // depth is normalised: (d - lo) * inv clamped to 0 ... 1, background 1
    float lo, inv;
    int32_t transposed;             // Raytracer-mode [x][y] storage
    uint32_t numCUs;
};

// how many native pixels the stage can address (its work items are counted in 32 bits)
constexpr uint64_t kObserveMaxPixels = 0xFFFFFFFFull;

// The form launchObserve picks: kObsTile on transposed storage; otherwise kObsWide when a view's pixel count is a
// multiple of 4 and the three tensors are 16-byte aligned, kObsNarrow for everything else.
uint32_t observeForm(const ObserveParams &p);

// Enqueues the kernel on `stream` and, with a reset column, the memset that clears it.  hipErrorInvalidValue for a
// layout, dtype or stack outside the fields' ranges, a missing tensor or more pixels than kObserveMaxPixels -- there
// is no other path.
hipError_t launchObserve(const ObserveParams &p, hipStream_t stream);

}  // namespace mrx
