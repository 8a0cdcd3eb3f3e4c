// Instantiates the elliptic operator's passes and the mass product on quadrilaterals (poisson2d_quad_kernel.hpp) for one polynomial
// order (-DBDG_ORDER=N): the gradient pass plain, with data and with the direction update fused in, the divergence pass with and
// without data, the mass product. Parallelogram geometry only: no per-node-geometry instance exists.
#include "poisson2d_quad_launch.hpp"
#include "poisson2d_quad_kernel.hpp"

#ifndef BDG_ORDER
#error "compile with -DBDG_ORDER=<polynomial order>"
#endif

#define BDG_PQ_CAT2(a, b) a##b
#define BDG_PQ_CAT(a, b) BDG_PQ_CAT2(a, b)

namespace bdg_dev {
namespace {

constexpr int kN = BDG_ORDER;
using Q = QuadPoissonElem<kN>;

// one 256-thread workgroup per tile of E elements
dim3 tileGrid(int kbegin, int kend) { return dim3(static_cast<unsigned>((kend - kbegin + Q::E - 1) / Q::E)); }

int fmaskOf(int f, int n) { return Q::fmask(f, n); }

template <bool DATA, bool FUSED>
hipError_t launchGradient(const PoissonParams& p, const double* ops, hipStream_t stream) {
    hipLaunchKernelGGL((poisson2d_quad_gradient_kernel<kN, DATA, FUSED>), tileGrid(p.kbegin, p.kend), dim3(Q::THREADS), 0, stream, p,
                       ops);
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
    if (data)
        hipLaunchKernelGGL((poisson2d_quad_divergence_kernel<kN, true>), tileGrid(p.kbegin, p.kend), dim3(Q::THREADS), 0, stream, p, u,
                           ops);
    else
        hipLaunchKernelGGL((poisson2d_quad_divergence_kernel<kN, false>), tileGrid(p.kbegin, p.kend), dim3(Q::THREADS), 0, stream, p, u,
                           ops);
    return hipGetLastError();
}

hipError_t mass(const double* u, const double* v, double* w, const double* mass1, const double* jac, double* partial, long long ld,
                int kbegin, int kend, hipStream_t stream) {
    if (kend <= kbegin) return hipSuccess;
    hipLaunchKernelGGL((poisson2d_quad_mass_kernel<kN>), tileGrid(kbegin, kend), dim3(Q::THREADS), 0, stream, u, v, w, mass1, jac,
                       partial, ld, kbegin, kend);
    return hipGetLastError();
}

} // namespace

const PoissonKernelTable* BDG_PQ_CAT(poisson_quad_kernel_table_order, BDG_ORDER)() {
    static const PoissonKernelTable table = {kN, Q::Np, Q::Nq, &fmaskOf, &gradient, &divergence, &mass};
    return &table;
}

int BDG_PQ_CAT(poisson_quad_tile_elements_order, BDG_ORDER)() { return Q::E; }

} // namespace bdg_dev
