// One polynomial order of the quadrilateral sw2d kernel (compiled once per order with -DBDG_ORDER=N, as
// sw2d_order.hip): every (mode, filter, geometry form) instance of sw2d_quad_stage_kernel<N>.
#include "sw2d_quad_kernel.hpp"

#ifndef BDG_ORDER
#error "compile with -DBDG_ORDER=N"
#endif

namespace bdg_dev {

namespace {
template <int N, int MODE, bool FILT>
hipError_t launchForm(bool general, const QuadParams& p, hipStream_t stream) {
    using Q = QuadElem<N>;
    if (p.kEnd <= p.kBegin) return hipSuccess; // (an empty range: a share without interior elements)
    const dim3 grid((p.kEnd - p.kBegin + Q::E - 1) / Q::E), block(Q::THREADS);
    if (general)
        hipLaunchKernelGGL((sw2d_quad_stage_kernel<N, MODE, FILT, true>), grid, block, 0, stream, p);
    else
        hipLaunchKernelGGL((sw2d_quad_stage_kernel<N, MODE, FILT, false>), grid, block, 0, stream, p);
    return hipGetLastError();
}
} // namespace

template <>
hipError_t sw2d_quad_launch<BDG_ORDER>(int mode, bool filter, bool general, const QuadParams& p, hipStream_t stream) {
    constexpr int N = BDG_ORDER;
    switch (mode) {
    case QMODE_RHS:
        return filter ? launchForm<N, QMODE_RHS, true>(general, p, stream) : launchForm<N, QMODE_RHS, false>(general, p, stream);
    case QMODE_COMBINE:
        return filter ? launchForm<N, QMODE_COMBINE, true>(general, p, stream)
                      : launchForm<N, QMODE_COMBINE, false>(general, p, stream);
    case QMODE_LSERK:
        if (filter) return hipErrorInvalidValue; // LSERK4 stages are unfiltered
        return launchForm<N, QMODE_LSERK, false>(general, p, stream);
    default:
        return hipErrorInvalidValue;
    }
}

} // namespace bdg_dev
