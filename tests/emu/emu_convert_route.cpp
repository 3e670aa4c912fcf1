// TEST INFRASTRUCTURE — not part of the product; nothing in smelter_amd/ builds, links or loads this.
//
// The input converter's classifier (smelter_amd/csrc/smr_convert_route.h: conv_route, conv_rgb12_ok) compiled for the CPU, so that
// tests/test_convert_route.py can ask it about frames described by numbers: no plane is ever read, a plane is an address, a pitch and who owns it.
#include <hip/hip_runtime.h>

#include "smr_convert_route.h"

// A frame of `format` (base format | matrix << 8), width x height; plane k (k < nplanes; the others are absent) at address ptr[k] with pitch[k]
// bytes per row, owned by the library or not.  node16: the node takes 16-byte stores.  Returns the ConvRoute, rgb12_out = conv_rgb12_ok.
extern "C" int emu_conv_route(unsigned convert_impl, unsigned format, unsigned width, unsigned height, int nplanes, const unsigned long long *ptr,
                              const unsigned long long *pitch, const int *owned, int node16, int *rgb12_out) {
    smr_ctx ctx;
    ctx.convert_impl = convert_impl;
    smr_surface s[3];
    smr_frame f;
    f.format = format; f.width = width; f.height = height;
    for (int k = 0; k < 3; k++) {
        f.planes[k] = k < nplanes ? &s[k] : nullptr;
        if (k >= nplanes) continue;
        s[k].ptr = (void *)(uintptr_t)ptr[k];
        s[k].pitch = (size_t)pitch[k];
        s[k].owned = owned[k] != 0;
    }
    if (rgb12_out) *rgb12_out = conv_rgb12_ok(&ctx, &f) ? 1 : 0;
    return (int)conv_route(&ctx, &f, node16 != 0);
}
// the enum's values by name, so that the test's table cannot drift from the header's order unnoticed
extern "C" int emu_conv_route_value(int which) {
    static const int v[] = {CONV_GENERAL, CONV_BATCH_4X2, CONV_420_PLANAR, CONV_420_NV12, CONV_420_PLANAR_TIGHT, CONV_420_NV12_TIGHT, CONV_HI420_PLANAR,
                            CONV_HI420_P010, CONV_HI422_PLANAR, CONV_HI422_P210, CONV_HI422_V210, CONV_420_PLANAR_601, CONV_420_NV12_601,
                            CONV_420_PLANAR_TIGHT_601, CONV_420_NV12_TIGHT_601, CONV_420_PLANAR_2020, CONV_420_NV12_2020, CONV_420_PLANAR_TIGHT_2020,
                            CONV_420_NV12_TIGHT_2020, CONV_ROUTES};
    return which >= 0 && which < (int)(sizeof(v) / sizeof(v[0])) ? v[which] : -100;
}
