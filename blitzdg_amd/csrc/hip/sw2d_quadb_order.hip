// One polynomial order of the variant-B quadrilateral sw2d kernel (compiled once per order with -DBDG_ORDER=N, as
// sw2d_quad_order.hip): every (mode, filter, geometry form) instance of sw2d_quadb_stage_kernel<N>: RHS, COMBINE and
// HEUN plain and filtered, LSERK plain.
#include "sw2d_quadb_kernel.hpp"

#ifndef BDG_ORDER
#error "compile with -DBDG_ORDER=N"
#endif

namespace bdg_dev {

namespace {
template <int N, int MODE, bool FILT>
hipError_t launchFormB(bool general, const QuadBParams& p, hipStream_t stream) {
    using Q = QuadBElem<N>;
    if (p.q.kEnd <= p.q.kBegin) return hipSuccess; // (an empty range: a share without interior elements)
    const dim3 grid((p.q.kEnd - p.q.kBegin + Q::E - 1) / Q::E), block(Q::THREADS);
    if (general)
        hipLaunchKernelGGL((sw2d_quadb_stage_kernel<N, MODE, FILT, true>), grid, block, 0, stream, p);
    else
        hipLaunchKernelGGL((sw2d_quadb_stage_kernel<N, MODE, FILT, false>), grid, block, 0, stream, p);
    return hipGetLastError();
}
} // namespace

template <>
hipError_t sw2d_quadb_launch<BDG_ORDER>(int mode, bool filter, bool general, const QuadBParams& p, hipStream_t stream) {
    constexpr int N = BDG_ORDER;
    switch (mode) {
    case QMODE_RHS:
        return filter ? launchFormB<N, QMODE_RHS, true>(general, p, stream) : launchFormB<N, QMODE_RHS, false>(general, p, stream);
    case QMODE_COMBINE:
        return filter ? launchFormB<N, QMODE_COMBINE, true>(general, p, stream)
                      : launchFormB<N, QMODE_COMBINE, false>(general, p, stream);
    case QMODE_LSERK:
        if (filter) return hipErrorInvalidValue; // LSERK4 stages are unfiltered
        return launchFormB<N, QMODE_LSERK, false>(general, p, stream);
    case QMODE_HEUN:
        return filter ? launchFormB<N, QMODE_HEUN, true>(general, p, stream) : launchFormB<N, QMODE_HEUN, false>(general, p, stream);
    default:
        return hipErrorInvalidValue;
    }
}

} // namespace bdg_dev
