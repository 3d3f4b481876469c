// The names of the packed observation output's channel layouts and element types, indexed by their codes in the
// MRX_FLAG_OBSERVATIONS field (include/mrx.h: MRX_OBS_*, and the dtype 0 ... 3), as the Python binding and
// renderer_headless both spell them.  For the host-side front ends only: nothing here is device code.
#pragma once

#include <cstdint>
#include <string>

namespace madRender {

constexpr uint32_t kNumObsLayouts = 5, kNumObsDtypes = 4;
inline const char *const kObsChannels[kNumObsLayouts + 1] = { "", "rgb", "rgbd", "d", "y", "yd" };   // ([0]: no output)
inline const char *const kObsDtypes[kNumObsDtypes] = { "float32", "float16", "bfloat16", "uint8" };

// the layout code of a channels name, 0 where there is none
inline uint32_t obsLayoutOf(const std::string &name)
{
    for (uint32_t i = 1; i <= kNumObsLayouts; ++i)
        if (name == kObsChannels[i])
            return i;
    return 0;
}

// the code of an element type's name, kNumObsDtypes where there is none
inline uint32_t obsDtypeOf(const std::string &name)
{
    for (uint32_t i = 0; i < kNumObsDtypes; ++i)
        if (name == kObsDtypes[i])
            return i;
    return kNumObsDtypes;
}

}  // namespace madRender
