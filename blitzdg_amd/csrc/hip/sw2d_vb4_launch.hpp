// Per-order launch table of variant B's tracer pass (sw2d_vb_tracer_kernel.hpp), compiled in translation units of its own
// (sw2d_vb4_order.hip with -DBDG_ORDER=N): the per-order objects of sw2d_order.hip, and with them every kernel instance
// that existed before the pass, stay as they are.
#pragma once
#include "sw2d_vb_tracer_kernel.hpp"

namespace bdg_dev {

struct Vb4KernelTable {
    int order;
    // 1: the unrolled form exists at this order (N <= 4)
    int unrolled;
    // Unrolled form, straight-sided elements: p.opsAffine = AffineOps image, plain or pre-filtered. hipErrorNotSupported where
    // `unrolled` is 0.
    hipError_t (*tracerUnrolled)(int mode, const StageParams& p, const VbParams& vb, const VbTracerParams& tp, hipStream_t stream);
    // General form. ops: VnOps image (pre-filtered: straight-sided elements only). nodal: per-node geometry (p.geo, p.fgeo), else
    // p.ageo. filt != nullptr (per-node geometry): the filtered evaluation in two passes, unfiltered rows to plane 3 of `raw`,
    // then the Filter rows `filt` and the update.
    hipError_t (*tracerGeneral)(int mode, bool nodal, const StageParams& p, const VbParams& vb, const VbTracerParams& tp,
                                const double* ops, const double* filt, double* raw, hipStream_t stream);
};

const Vb4KernelTable* vb4_kernel_table(int order); // nullptr if the order is not compiled in

} // namespace bdg_dev
