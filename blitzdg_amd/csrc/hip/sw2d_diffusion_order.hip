// Instantiates the tracer's diffusion passes (sw2d_diffusion_kernel.hpp) for one polynomial order (-DBDG_ORDER=N).
#include "sw2d_diffusion_launch.hpp"
#include "sw2d_launch_host.hpp"

#ifndef BDG_ORDER
#error "compile with -DBDG_ORDER=<polynomial order>"
#endif

namespace bdg_dev {
namespace {

static_assert(TriModes::RHS == MODE_RHS && TriModes::LSERK == MODE_LSERK && TriModes::COMBINE == MODE_COMBINE, "sw2d_dispatch.hpp");

constexpr int kN = BDG_ORDER;

bool emptyRange(const StageParams& p) { return p.kend <= p.kbegin; }
// one-wave workgroups of 64 elements
dim3 waveGrid(const StageParams& p) { return dim3(static_cast<unsigned>((p.kend - p.kbegin + 63) / 64)); }

hipError_t gradient(bool nodal, const StageParams& p, const DiffusionParams& dp, const double* ops, hipStream_t stream) {
    if (emptyRange(p)) return hipSuccess;
    if (nodal) hipLaunchKernelGGL((sw2d_tracer_gradient_kernel<kN, true>), waveGrid(p), dim3(64), 0, stream, p, dp, ops);
    else hipLaunchKernelGGL((sw2d_tracer_gradient_kernel<kN, false>), waveGrid(p), dim3(64), 0, stream, p, dp, ops);
    return hipGetLastError();
}

template <int MODE>
hipError_t launchDivergence(bool nodal, const StageParams& p, const DiffusionParams& dp, const double* ops, hipStream_t stream) {
    if (nodal) hipLaunchKernelGGL((sw2d_tracer_diffusion_kernel<kN, MODE, true>), waveGrid(p), dim3(64), 0, stream, p, dp, ops);
    else hipLaunchKernelGGL((sw2d_tracer_diffusion_kernel<kN, MODE, false>), waveGrid(p), dim3(64), 0, stream, p, dp, ops);
    return hipGetLastError();
}

hipError_t divergence(int mode, bool nodal, bool raw, const StageParams& p, const DiffusionParams& dp, const double* ops,
                      hipStream_t stream) {
    if (emptyRange(p)) return hipSuccess;
    if (raw) {
        if (!dp.raw) return hipErrorInvalidValue;
        if (nodal) hipLaunchKernelGGL((sw2d_tracer_diffusion_kernel<kN, MODE_RHS, true, true>), waveGrid(p), dim3(64), 0, stream, p, dp, ops);
        else hipLaunchKernelGGL((sw2d_tracer_diffusion_kernel<kN, MODE_RHS, false, true>), waveGrid(p), dim3(64), 0, stream, p, dp, ops);
        return hipGetLastError();
    }
    return forMode(mode, [&](auto m) { return launchDivergence<decltype(m)::value>(nodal, p, dp, ops, stream); });
}

template <int MODE>
hipError_t launchFilter(const StageParams& p, const DiffusionParams& dp, const double* filt, hipStream_t stream) {
    hipLaunchKernelGGL((sw2d_tracer_diffusion_filter_kernel<kN, MODE>), waveGrid(p), dim3(64), 0, stream, p, dp, filt);
    return hipGetLastError();
}

hipError_t filter(int mode, const StageParams& p, const DiffusionParams& dp, const double* filt, hipStream_t stream) {
    if (emptyRange(p)) return hipSuccess;
    if (!dp.raw || !filt) return hipErrorInvalidValue;
    return forMode(mode, [&](auto m) { return launchFilter<decltype(m)::value>(p, dp, filt, stream); });
}

} // namespace

const DiffusionKernelTable* BDG_CAT(diffusion_kernel_table_order, BDG_ORDER)() {
    static const DiffusionKernelTable table = {kN, &gradient, &divergence, &filter};
    return &table;
}

} // namespace bdg_dev
