// Per-order launch table of the tracer's diffusion passes (sw2d_diffusion_kernel.hpp), compiled in translation units of its own
// (sw2d_diffusion_order.hip with -DBDG_ORDER=N): the per-order objects of sw2d_order.hip and sw2d_vb4_order.hip, and with them
// every kernel instance that existed before the passes, stay as they are.
#pragma once
#include "sw2d_diffusion_kernel.hpp"

namespace bdg_dev {

struct DiffusionKernelTable {
    int order;
    // First pass: fx, fy of p.qin into dp.flux. ops: plain VnOps image. nodal: per-node geometry (p.geo, p.fgeo), else p.ageo.
    hipError_t (*gradient)(bool nodal, const StageParams& p, const DiffusionParams& dp, const double* ops, hipStream_t stream);
    // Second pass: T from dp.flux, added to plane 3 of the stage of `mode`. ops: VnOps image -- pre-filtered only on straight-sided
    // elements with dp.source == nullptr and dp.decay == 0. raw: the unfiltered T goes to dp.raw instead (mode is then not used).
    hipError_t (*divergence)(int mode, bool nodal, bool raw, const StageParams& p, const DiffusionParams& dp, const double* ops,
                             hipStream_t stream);
    // Last step of a filtered evaluation in two steps: Filter rows `filt` on dp.raw, then the update of `mode`.
    hipError_t (*filter)(int mode, const StageParams& p, const DiffusionParams& dp, const double* filt, hipStream_t stream);
};

const DiffusionKernelTable* diffusion_kernel_table(int order); // nullptr if the order is not compiled in

} // namespace bdg_dev
