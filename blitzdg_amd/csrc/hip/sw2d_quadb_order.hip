// One polynomial order of the variant-B quadrilateral sw2d kernel (compiled once per order with -DBDG_ORDER=N, as
// sw2d_quad_order.hip): every (mode, filter, geometry form) instance of sw2d_quadb_stage_kernel<N>: RHS, COMBINE and
// HEUN plain and filtered, LSERK plain.
#include "sw2d_quadb_kernel.hpp"
#include "sw2d_dispatch.hpp"

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
    return quadForMode<true>(mode, filter, [&](auto m, auto f) {
        return launchFormB<BDG_ORDER, decltype(m)::value, decltype(f)::value>(general, p, stream);
    });
}

} // namespace bdg_dev
