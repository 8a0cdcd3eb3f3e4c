// Per-order launch table of the elliptic operator's passes and of the mass product (poisson2d_kernel.hpp), compiled in translation
// units of its own (poisson2d_order.hip with -DBDG_ORDER=N): every per-order object that existed before stays as it is.
#pragma once
#include "poisson2d_kernel.hpp"

namespace bdg_dev {

struct PoissonKernelTable {
    int order, Np, Nfp;
    int (*fmask)(int f, int n);
    // First pass: qx, qy of p.u (fused: of p = p.u + beta p.pold, stored to p.pnew) into p.q. ops: plain VnOps image.
    hipError_t (*gradient)(bool data, bool fused, const PoissonParams& p, const double* ops, hipStream_t stream);
    // Second pass: A u from p.q and u (what the first pass differentiated) into p.out.
    hipError_t (*divergence)(bool data, const PoissonParams& p, const double* u, const double* ops, hipStream_t stream);
    // w = J M v where w is not nullptr, partial[tile] = u . (J M v) over the tile's elements: ceil((kend - kbegin) / 64) partials.
    hipError_t (*mass)(const double* u, const double* v, double* w, const double* mass, const double* jac, double* partial,
                       long long ld, int kbegin, int kend, hipStream_t stream);
};

const PoissonKernelTable* poisson_kernel_table(int order); // nullptr if the order is not compiled in

} // namespace bdg_dev
