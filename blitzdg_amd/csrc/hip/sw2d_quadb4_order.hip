// One polynomial order of the four-field variant-B quadrilateral sw2d kernel (compiled once per order with -DBDG_ORDER=N, as
// sw2d_quadb_order.hip): every (mode, filter, geometry form) instance of sw2d_quadb4_stage_kernel<N>: RHS, COMBINE and
// HEUN plain and filtered, LSERK plain.
#include "sw2d_quadb4_kernel.hpp"

#ifndef BDG_ORDER
#error "compile with -DBDG_ORDER=N"
#endif

namespace bdg_dev {

namespace {
template <int N, int MODE, bool FILT>
hipError_t launchFormB4(bool general, const QuadB4Params& p, hipStream_t stream) {
    using Q = QuadB4Elem<N>;
    const QuadParams& q = p.b.q;
    if (q.kEnd <= q.kBegin) return hipSuccess; // (an empty range: a share without interior elements)
    const dim3 grid((q.kEnd - q.kBegin + Q::E - 1) / Q::E), block(Q::THREADS);
    if (general)
        hipLaunchKernelGGL((sw2d_quadb4_stage_kernel<N, MODE, FILT, true>), grid, block, 0, stream, p);
    else
        hipLaunchKernelGGL((sw2d_quadb4_stage_kernel<N, MODE, FILT, false>), grid, block, 0, stream, p);
    return hipGetLastError();
}
} // namespace

template <>
hipError_t sw2d_quadb4_launch<BDG_ORDER>(int mode, bool filter, bool general, const QuadB4Params& p, hipStream_t stream) {
    constexpr int N = BDG_ORDER;
    switch (mode) {
    case QMODE_RHS:
        return filter ? launchFormB4<N, QMODE_RHS, true>(general, p, stream) : launchFormB4<N, QMODE_RHS, false>(general, p, stream);
    case QMODE_COMBINE:
        return filter ? launchFormB4<N, QMODE_COMBINE, true>(general, p, stream)
                      : launchFormB4<N, QMODE_COMBINE, false>(general, p, stream);
    case QMODE_LSERK:
        if (filter) return hipErrorInvalidValue; // LSERK4 stages are unfiltered
        return launchFormB4<N, QMODE_LSERK, false>(general, p, stream);
    case QMODE_HEUN:
        return filter ? launchFormB4<N, QMODE_HEUN, true>(general, p, stream) : launchFormB4<N, QMODE_HEUN, false>(general, p, stream);
    default:
        return hipErrorInvalidValue;
    }
}

} // namespace bdg_dev
