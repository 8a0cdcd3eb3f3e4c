// Host-only: how an order object of the curved kernels (sw2d_curved_order.hip) tells the C ABI (sw2d_curved_device.hip) which
// kernel instance its launch path picks. Beside the launch table, whose declaration is shared with the device code.
#pragma once

namespace bdg_dev {

// form, streamed, image_in_lds, fb, live_steps, waves, mapm, lds_bytes (bdg_sw2d_curved_kernel_info in include/blitzdg_hip.h)
constexpr int kCurvedKernelInfoFields = 8;
// false: no compiled kernel serves these sizes. Launches nothing.
typedef bool (*CurvedKernelInfoFn)(bool nodalTrace, int ncb, int ng, int fb, bool mapm, bool filter, int out[kCurvedKernelInfoFields]);

} // namespace bdg_dev
