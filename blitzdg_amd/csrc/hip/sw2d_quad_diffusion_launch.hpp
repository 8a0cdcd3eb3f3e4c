// Per-order launch table of the tracer's diffusion passes on quadrilaterals (sw2d_quad_diffusion_kernel.hpp), compiled in
// translation units of its own (sw2d_quad_diffusion_order.hip with -DBDG_ORDER=N): the per-order objects of sw2d_quad_order.hip,
// sw2d_quadb_order.hip and sw2d_quadb4_order.hip, and with them every kernel instance that existed before the passes, stay as
// they are.
#pragma once
#include "sw2d_quad_diffusion_kernel.hpp"

namespace bdg_dev {

struct QuadDiffusionKernelTable {
    int order;
    // First pass: fx, fy of p.qin into dp.flux. general: per-node geometry (p.geo, p.fgeo), else p.ageo.
    hipError_t (*gradient)(bool general, const QuadParams& p, const QuadDiffusionParams& dp, hipStream_t stream);
    // Second pass: T (filter: p.filt T) from dp.flux, added to plane 3 of the stage of `mode`: RHS and COMBINE plain and filtered,
    // LSERK plain, HEUN plain and filtered; anything else is hipErrorInvalidValue.
    hipError_t (*divergence)(int mode, bool filter, bool general, const QuadParams& p, const QuadDiffusionParams& dp,
                             hipStream_t stream);
};

const QuadDiffusionKernelTable* quad_diffusion_kernel_table(int order); // nullptr if the order is not compiled in

} // namespace bdg_dev
