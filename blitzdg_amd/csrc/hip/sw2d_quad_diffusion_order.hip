// Instantiates the tracer's diffusion passes on quadrilaterals (sw2d_quad_diffusion_kernel.hpp) for one polynomial order
// (-DBDG_ORDER=N): the gradient pass on both geometry forms, the divergence pass for RHS, COMBINE and HEUN plain and filtered
// and LSERK plain, each on both geometry forms.
#include "sw2d_quad_diffusion_launch.hpp"
#include "sw2d_dispatch.hpp"

#ifndef BDG_ORDER
#error "compile with -DBDG_ORDER=N"
#endif

#define BDG_QD_CAT2(a, b) a##b
#define BDG_QD_CAT(a, b) BDG_QD_CAT2(a, b)

namespace bdg_dev {

static_assert(QuadModes::RHS == QMODE_RHS && QuadModes::COMBINE == QMODE_COMBINE && QuadModes::LSERK == QMODE_LSERK &&
              QuadModes::HEUN == QMODE_HEUN, "sw2d_dispatch.hpp");

namespace {

constexpr int kN = BDG_ORDER;
using Q = QuadDiffElem<kN>;

dim3 tileGrid(const QuadParams& p) { return dim3(static_cast<unsigned>((p.kEnd - p.kBegin + Q::E - 1) / Q::E)); }

hipError_t gradient(bool general, const QuadParams& p, const QuadDiffusionParams& dp, hipStream_t stream) {
    if (p.kEnd <= p.kBegin) return hipSuccess;
    if (!dp.flux) return hipErrorInvalidValue;
    if (general)
        hipLaunchKernelGGL((sw2d_quad_tracer_gradient_kernel<kN, true>), tileGrid(p), dim3(Q::THREADS), 0, stream, p, dp);
    else
        hipLaunchKernelGGL((sw2d_quad_tracer_gradient_kernel<kN, false>), tileGrid(p), dim3(Q::THREADS), 0, stream, p, dp);
    return hipGetLastError();
}

template <int MODE, bool FILT>
hipError_t launchDivergence(bool general, const QuadParams& p, const QuadDiffusionParams& dp, hipStream_t stream) {
    if (general)
        hipLaunchKernelGGL((sw2d_quad_tracer_divergence_kernel<kN, MODE, FILT, true>), tileGrid(p), dim3(Q::THREADS), 0, stream, p, dp);
    else
        hipLaunchKernelGGL((sw2d_quad_tracer_divergence_kernel<kN, MODE, FILT, false>), tileGrid(p), dim3(Q::THREADS), 0, stream, p, dp);
    return hipGetLastError();
}

hipError_t divergence(int mode, bool filter, bool general, const QuadParams& p, const QuadDiffusionParams& dp, hipStream_t stream) {
    if (p.kEnd <= p.kBegin) return hipSuccess;
    if (!dp.flux || (filter && !p.filt)) return hipErrorInvalidValue;
    return quadForMode<true>(mode, filter, [&](auto m, auto f) {
        return launchDivergence<decltype(m)::value, decltype(f)::value>(general, p, dp, stream);
    });
}

} // namespace

const QuadDiffusionKernelTable* BDG_QD_CAT(quad_diffusion_kernel_table_order, BDG_ORDER)() {
    static const QuadDiffusionKernelTable table = {kN, &gradient, &divergence};
    return &table;
}

} // namespace bdg_dev
