// Instantiates the eddy-viscosity passes (sw2d_viscosity_kernel.hpp) for one polynomial order (-DBDG_ORDER=N).
#include "sw2d_viscosity_launch.hpp"
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

hipError_t gradient(bool nodal, const StageParams& p, const ViscosityParams& vp, const double* ops, hipStream_t stream) {
    if (emptyRange(p)) return hipSuccess;
    if (!vp.flux) return hipErrorInvalidValue;
    if (nodal) hipLaunchKernelGGL((sw2d_viscosity_gradient_kernel<kN, true>), waveGrid(p), dim3(64), 0, stream, p, vp, ops);
    else hipLaunchKernelGGL((sw2d_viscosity_gradient_kernel<kN, false>), waveGrid(p), dim3(64), 0, stream, p, vp, ops);
    return hipGetLastError();
}

template <int MODE>
hipError_t launchDivergence(bool nodal, const StageParams& p, const ViscosityParams& vp, const double* ops, hipStream_t stream) {
    if (nodal) hipLaunchKernelGGL((sw2d_viscosity_divergence_kernel<kN, MODE, true>), waveGrid(p), dim3(64), 0, stream, p, vp, ops);
    else hipLaunchKernelGGL((sw2d_viscosity_divergence_kernel<kN, MODE, false>), waveGrid(p), dim3(64), 0, stream, p, vp, ops);
    return hipGetLastError();
}

hipError_t divergence(int mode, bool nodal, bool raw, const StageParams& p, const ViscosityParams& vp, const double* ops,
                      hipStream_t stream) {
    if (emptyRange(p)) return hipSuccess;
    if (raw) {
        if (!vp.raw) return hipErrorInvalidValue;
        if (nodal) hipLaunchKernelGGL((sw2d_viscosity_divergence_kernel<kN, MODE_RHS, true, true>), waveGrid(p), dim3(64), 0, stream, p, vp, ops);
        else hipLaunchKernelGGL((sw2d_viscosity_divergence_kernel<kN, MODE_RHS, false, true>), waveGrid(p), dim3(64), 0, stream, p, vp, ops);
        return hipGetLastError();
    }
    return forMode(mode, [&](auto m) { return launchDivergence<decltype(m)::value>(nodal, p, vp, ops, stream); });
}

template <int MODE>
hipError_t launchFilter(const StageParams& p, const ViscosityParams& vp, const double* filt, hipStream_t stream) {
    hipLaunchKernelGGL((sw2d_viscosity_filter_kernel<kN, MODE>), waveGrid(p), dim3(64), 0, stream, p, vp, filt);
    return hipGetLastError();
}

hipError_t filter(int mode, const StageParams& p, const ViscosityParams& vp, const double* filt, hipStream_t stream) {
    if (emptyRange(p)) return hipSuccess;
    if (!vp.raw || !filt) return hipErrorInvalidValue;
    return forMode(mode, [&](auto m) { return launchFilter<decltype(m)::value>(p, vp, filt, stream); });
}

hipError_t maxOf(const double* in, long long n, double* part, double* out, hipStream_t stream) {
    if (!in || !part || !out || n <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sw2d_viscosity_max_kernel<kN>, dim3(kViscosityMaxBlocks), dim3(256), 0, stream, in, n, part);
    hipLaunchKernelGGL(sw2d_viscosity_max_kernel<kN>, dim3(1), dim3(256), 0, stream, part, static_cast<long long>(kViscosityMaxBlocks), out);
    return hipGetLastError();
}

} // namespace

const ViscosityKernelTable* BDG_CAT(viscosity_kernel_table_order, BDG_ORDER)() {
    static const ViscosityKernelTable table = {kN, &gradient, &divergence, &filter, &maxOf};
    return &table;
}

} // namespace bdg_dev
