// Per-order launch table of the eddy-viscosity passes (sw2d_viscosity_kernel.hpp), compiled in translation units of its own
// (sw2d_viscosity_order.hip with -DBDG_ORDER=N): the per-order objects of sw2d_order.hip, sw2d_vb4_order.hip and
// sw2d_diffusion_order.hip, and with them every kernel instance that existed before the passes, stay as they are.
#pragma once
#include "sw2d_viscosity_kernel.hpp"

namespace bdg_dev {

struct ViscosityKernelTable {
    int order;
    // First pass: nu h grad u, nu h grad v of p.qin into vp.flux (and nu into vp.nuOut if set). ops: plain VnOps image. nodal:
    // per-node geometry (p.geo, p.fgeo), else p.ageo.
    hipError_t (*gradient)(bool nodal, const StageParams& p, const ViscosityParams& vp, const double* ops, hipStream_t stream);
    // Second pass: T_u, T_v from vp.flux, added to planes 1 and 2 of the stage of `mode`. ops: VnOps image -- pre-filtered only on
    // straight-sided elements. raw: the unfiltered terms go to vp.raw instead (mode is then not used).
    hipError_t (*divergence)(int mode, bool nodal, bool raw, const StageParams& p, const ViscosityParams& vp, const double* ops,
                             hipStream_t stream);
    // Last step of a filtered evaluation in two steps: Filter rows `filt` on vp.raw, then the update of `mode`.
    hipError_t (*filter)(int mode, const StageParams& p, const ViscosityParams& vp, const double* filt, hipStream_t stream);
    // out[0] = max of the n entries of `in` (all >= 0), through `part` (at least kViscosityMaxBlocks doubles), in a fixed order.
    hipError_t (*maxOf)(const double* in, long long n, double* part, double* out, hipStream_t stream);
};

constexpr int kViscosityMaxBlocks = 256;

const ViscosityKernelTable* viscosity_kernel_table(int order); // nullptr if the order is not compiled in

} // namespace bdg_dev
