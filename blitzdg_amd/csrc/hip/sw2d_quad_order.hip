// One polynomial order of the quadrilateral sw2d kernel (compiled once per order with -DBDG_ORDER=N, as
// sw2d_order.hip): every (mode, filter, geometry form) instance of sw2d_quad_stage_kernel<N>, and every
// (mode, filter, geometry form, sources) instance of the four-field sw2d_quad4_stage_kernel<N>; and the output step
// sw2d_quad_output_kernel<N> for three and four fields, with and without the lattice interpolation.
#include "sw2d_quad4_kernel.hpp"
#include "sw2d_dispatch.hpp"
#include "sw2d_quad_output_kernel.hpp"

#ifndef BDG_ORDER
#error "compile with -DBDG_ORDER=N"
#endif

namespace bdg_dev {

static_assert(QuadModes::RHS == QMODE_RHS && QuadModes::COMBINE == QMODE_COMBINE && QuadModes::LSERK == QMODE_LSERK &&
              QuadModes::HEUN == QMODE_HEUN, "sw2d_dispatch.hpp");

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
    return quadForMode<false>(mode, filter, [&](auto m, auto f) {
        return launchForm<BDG_ORDER, decltype(m)::value, decltype(f)::value>(general, p, stream);
    });
}

namespace {
template <int N, int MODE, bool FILT>
hipError_t launchForm4(bool general, bool sources, const Quad4Params& p, hipStream_t stream) {
    using Q = Quad4Elem<N>;
    if (p.q.kEnd <= p.q.kBegin) return hipSuccess;
    const dim3 grid((p.q.kEnd - p.q.kBegin + Q::E - 1) / Q::E), block(Q::THREADS);
    if (general && sources)
        hipLaunchKernelGGL((sw2d_quad4_stage_kernel<N, MODE, FILT, true, true>), grid, block, 0, stream, p);
    else if (general)
        hipLaunchKernelGGL((sw2d_quad4_stage_kernel<N, MODE, FILT, true, false>), grid, block, 0, stream, p);
    else if (sources)
        hipLaunchKernelGGL((sw2d_quad4_stage_kernel<N, MODE, FILT, false, true>), grid, block, 0, stream, p);
    else
        hipLaunchKernelGGL((sw2d_quad4_stage_kernel<N, MODE, FILT, false, false>), grid, block, 0, stream, p);
    return hipGetLastError();
}
} // namespace

template <>
hipError_t sw2d_quad4_launch<BDG_ORDER>(int mode, bool filter, bool general, bool sources, const Quad4Params& p,
                                        hipStream_t stream) {
    return quadForMode<false>(mode, filter, [&](auto m, auto f) {
        return launchForm4<BDG_ORDER, decltype(m)::value, decltype(f)::value>(general, sources, p, stream);
    });
}

namespace {
template <int N, int NF>
hipError_t launchOutput(const QuadOutParams& p, hipStream_t stream) {
    if (p.kEnd <= 0) return hipSuccess;
    const dim3 grid((p.kEnd + 63) / 64), block(64 * (N + 1));
    if (p.I1)
        hipLaunchKernelGGL((sw2d_quad_output_kernel<N, NF, true>), grid, block, 0, stream, p.q, p.H, p.I1, p.out, p.ld, p.kEnd, p.mask);
    else
        hipLaunchKernelGGL((sw2d_quad_output_kernel<N, NF, false>), grid, block, 0, stream, p.q, p.H, p.I1, p.out, p.ld, p.kEnd,
                           p.mask);
    return hipGetLastError();
}
} // namespace

template <>
hipError_t sw2d_quad_output_launch<BDG_ORDER>(int fields, const QuadOutParams& p, hipStream_t stream) {
    if (fields == 3) return launchOutput<BDG_ORDER, 3>(p, stream);
    if (fields == 4) return launchOutput<BDG_ORDER, 4>(p, stream);
    return hipErrorInvalidValue;
}

} // namespace bdg_dev
