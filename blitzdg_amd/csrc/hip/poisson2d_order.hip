// Instantiates the elliptic operator's passes and the mass product (poisson2d_kernel.hpp) for one polynomial order (-DBDG_ORDER=N).
#include "poisson2d_launch.hpp"
#include "sw2d_launch_host.hpp"

#ifndef BDG_ORDER
#error "compile with -DBDG_ORDER=<polynomial order>"
#endif

namespace bdg_dev {
namespace {

constexpr int kN = BDG_ORDER;

// one-wave workgroups of 64 elements
dim3 waveGrid(int kbegin, int kend) { return dim3(static_cast<unsigned>((kend - kbegin + 63) / 64)); }

int fmaskOf(int f, int n) { return Elem<kN>::fmask(f, n); }

template <bool DATA, bool FUSED>
hipError_t launchGradient(const PoissonParams& p, const double* ops, hipStream_t stream) {
    hipLaunchKernelGGL((poisson2d_gradient_kernel<kN, DATA, FUSED>), waveGrid(p.kbegin, p.kend), dim3(64), 0, stream, p, ops);
    return hipGetLastError();
}

hipError_t gradient(bool data, bool fused, const PoissonParams& p, const double* ops, hipStream_t stream) {
    if (p.kend <= p.kbegin) return hipSuccess;
    if (data && (!p.g || !p.qn)) return hipErrorInvalidValue;
    if (fused && (!p.pold || !p.pnew || !p.scal || p.pold == p.pnew || data)) return hipErrorInvalidValue;
    if (fused) return launchGradient<false, true>(p, ops, stream);
    return data ? launchGradient<true, false>(p, ops, stream) : launchGradient<false, false>(p, ops, stream);
}

hipError_t divergence(bool data, const PoissonParams& p, const double* u, const double* ops, hipStream_t stream) {
    if (p.kend <= p.kbegin) return hipSuccess;
    if (data && (!p.g || !p.qn)) return hipErrorInvalidValue;
    if (data) hipLaunchKernelGGL((poisson2d_divergence_kernel<kN, true>), waveGrid(p.kbegin, p.kend), dim3(64), 0, stream, p, u, ops);
    else hipLaunchKernelGGL((poisson2d_divergence_kernel<kN, false>), waveGrid(p.kbegin, p.kend), dim3(64), 0, stream, p, u, ops);
    return hipGetLastError();
}

hipError_t mass(const double* u, const double* v, double* w, const double* massRows, const double* jac, double* partial,
                long long ld, int kbegin, int kend, hipStream_t stream) {
    if (kend <= kbegin) return hipSuccess;
    hipLaunchKernelGGL((poisson2d_mass_kernel<kN>), waveGrid(kbegin, kend), dim3(64), 0, stream, u, v, w, massRows, jac, partial, ld,
                       kbegin, kend);
    return hipGetLastError();
}

} // namespace

const PoissonKernelTable* BDG_CAT(poisson_kernel_table_order, BDG_ORDER)() {
    static const PoissonKernelTable table = {kN, Elem<kN>::Np, Elem<kN>::Nfp, &fmaskOf, &gradient, &divergence, &mass};
    return &table;
}

} // namespace bdg_dev
