// Instantiates variant B's tracer pass (sw2d_vb_tracer_kernel.hpp) for one polynomial order (-DBDG_ORDER=N).
#include "sw2d_vb4_launch.hpp"
#include "sw2d_launch_host.hpp"

#ifndef BDG_ORDER
#error "compile with -DBDG_ORDER=<polynomial order>"
#endif

namespace bdg_dev {
namespace {

static_assert(TriModes::RHS == MODE_RHS && TriModes::LSERK == MODE_LSERK && TriModes::COMBINE == MODE_COMBINE, "sw2d_dispatch.hpp");

constexpr int kN = BDG_ORDER;
// the unrolled form up to the order the other unrolled source-term kernels go to (bdg_sw2d::kUnrolledSourcesMaxOrder)
constexpr bool kUnrolled = BDG_ORDER <= 4;

bool emptyRange(const StageParams& p) { return p.kend <= p.kbegin; }
// one-wave workgroups of 64 elements, both forms
dim3 waveGrid(const StageParams& p) { return dim3(static_cast<unsigned>((p.kend - p.kbegin + 63) / 64)); }

template <int MODE>
hipError_t launchUnrolled(const StageParams& p, const VbParams& vb, const VbTracerParams& tp, hipStream_t stream) {
    if constexpr (!kUnrolled) return hipErrorNotSupported;
    else {
    if (emptyRange(p)) return hipSuccess;
    hipLaunchKernelGGL((sw2d_stage_vb_tracer_unrolled_kernel<kN, MODE>), waveGrid(p), dim3(64), 0, stream, p, vb, tp);
    return hipGetLastError();
    }
}

hipError_t tracerUnrolled(int mode, const StageParams& p, const VbParams& vb, const VbTracerParams& tp, hipStream_t stream) {
    return forMode(mode, [&](auto m) { return launchUnrolled<decltype(m)::value>(p, vb, tp, stream); });
}

template <int MODE>
hipError_t launchGeneral(bool nodal, const StageParams& p, const VbParams& vb, const VbTracerParams& tp, const double* ops,
                         const double* filt, double* raw, hipStream_t stream) {
    if (emptyRange(p)) return hipSuccess;
    const dim3 grid = waveGrid(p), blk(64);
    if (!nodal) { // the filter, if any, rides in the operator rows
        if (filt) return hipErrorInvalidValue;
        hipLaunchKernelGGL((sw2d_stage_vb_tracer_kernel<kN, MODE, false>), grid, blk, 0, stream, p, vb, tp, ops);
    } else if (!filt) {
        hipLaunchKernelGGL((sw2d_stage_vb_tracer_kernel<kN, MODE, true>), grid, blk, 0, stream, p, vb, tp, ops);
    } else {
        StageParams pr = p;
        pr.rhs = raw;
        hipLaunchKernelGGL((sw2d_stage_vb_tracer_kernel<kN, MODE_RHS, true>), grid, blk, 0, stream, pr, vb, tp, ops);
        hipLaunchKernelGGL((sw2d_vb_tracer_filter_kernel<kN, MODE>), grid, blk, 0, stream, p, raw, filt);
    }
    return hipGetLastError();
}

hipError_t tracerGeneral(int mode, bool nodal, const StageParams& p, const VbParams& vb, const VbTracerParams& tp, const double* ops,
                         const double* filt, double* raw, hipStream_t stream) {
    return forMode(mode, [&](auto m) { return launchGeneral<decltype(m)::value>(nodal, p, vb, tp, ops, filt, raw, stream); });
}

} // namespace

const Vb4KernelTable* BDG_CAT(vb4_kernel_table_order, BDG_ORDER)() {
    static const Vb4KernelTable table = {kN, kUnrolled ? 1 : 0, &tracerUnrolled, &tracerGeneral};
    return &table;
}

} // namespace bdg_dev
