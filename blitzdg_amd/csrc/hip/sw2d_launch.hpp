// Per-order launch table: each polynomial order is compiled in its own
// translation unit (sw2d_order.hip with -DBDG_ORDER=N) so the fully unrolled
// kernels build in parallel; the solver picks the table at run time.
#pragma once
#include "sw2d_affine_kernel.hpp"
#include "sw2d_affine_lean_kernel.hpp"
#include "sw2d_vd_kernel.hpp"
#include "sw2d_tracer_kernel.hpp"
#include "sw2d_vb_kernel.hpp"
#include "sw2d_vn_kernel.hpp"
#include "sw2d_mfma_kernel.hpp"
#include "sw2d_mfma3_kernel.hpp"
#include "sw2d_mfma3src_kernel.hpp"
#include "sw2d_affine_xchg_kernel.hpp"
#include "sw2d_kernels.hpp"

namespace bdg_dev {

// ---- the kernel forms a table entry chooses between, by name

// stageAffine: the families of the straight three-field stage. The numbers are the values of BDG_SW2D_AFFINE_VARIANT
// (DESIGN.md); Mfma, Mfma2 and Mfma3 have table entries of their own (stageMfma, stageMfma2, stageMfma3) and are the
// solver's to route -- stageAffine runs Unrolled for them.
enum class AffineVariant : int {
    Unrolled = 0,   // fully unrolled, register-resident state, one wave per SIMD
    FieldSplit = 1, // rolled, one field per wave (every order)
    Stream2 = 2,    // unrolled, streamed state at two waves per SIMD (N <= 5; above: FieldSplit)
    Stream3 = 3,    // ... at three waves per SIMD
    Rolled = 4,     // rolled, three fields per lane (N <= 6; above: FieldSplit)
    Mfma = 5,       // matrix cores, whole tile unrolled
    Mfma2 = 6,      // matrix cores, face-by-face schedule at two waves per SIMD
    Mfma3 = 7,      // matrix cores, state-once schedule
    Lean = 8,       // state-resident at two waves per SIMD, LSERK stages (N <= 5; other modes and orders: Unrolled)
    Xchg = 9        // in-wave neighbour traces through LDS, LSERK stages (N <= 5; other modes and orders: Unrolled)
};

// stageMfma2Src (N >= 5): what the matrix-core kernel with sources computes, and on which schedule. The image in p.opsAffine is
// MfmaOps2 + MT*KV tiles of F' (identity or Filter), except for TracerPass (plain MfmaOps2 image). The Once* forms are the
// state-once schedule (sw2d_mfma3src_kernel.hpp); they exist where KernelTable::mfma3SrcFields / mfma3TracerPhase say so and
// the state fits one buffer descriptor, hipErrorNotSupported otherwise.
enum class SrcForm {
    Sources,           // momentum sources of variants C / D, three fields, two waves per SIMD
    TracerPass,        // the tracer equation alone (field 3 of a four-field state)
    VariantB,          // variant B's surface term and sources, two waves per SIMD
    SourcesTracer,     // sources + tracer in one pass (MT <= 2, i.e. N <= 6)
    OnceSources,       // state-once: sources, three fields
    OnceSourcesTracer, // state-once: sources + tracer, four fields (mfma3SrcFields = 4)
    OnceVariantB,      // state-once: variant B
    OnceTracerPhase    // state-once: three fields with sources, the tracer as a second phase of every tile (mfma3TracerPhase)
};

// stageVb: the stage kernel that follows variant B's speed pass
enum class VbStage {
    None,    // speed pass alone (the stage runs on another entry: stageMfma2Src, or none at all)
    Rolled,  // rolled kernel, VdOps image (plain or filtered) in p.opsAffine
    Unrolled // unrolled kernel (N <= 4), plain AffineOps in p.opsAffine, the filter applied at the end
};

struct KernelTable {
    int order, Np, Nfp, ldsDoubles;
    // mode: StageMode; launches one fused RHS(+stage update) pass over K elements (per-node geometry, vector kernel).
    hipError_t (*stage)(int mode, bool filter, const StageParams& p, hipStream_t stream);
    // affine-geometry fast path (no FILTER template: the filter is folded into the operators)
    int affineOpsDoubles;
    hipError_t (*stageAffine)(int mode, AffineVariant variant, const StageParams& p, hipStream_t stream);
    // matrix-core path (v_mfma_f64_16x16x4_f64), straight-sided elements; needs ldsBytes of dynamic LDS
    int mfmaOpsDoubles, mfmaMT, mfmaKV, mfmaKS;
    hipError_t (*stageMfma)(int mode, const StageParams& p, hipStream_t stream);
    // MODE_LSERK on partition-boundary elements with pack / unpack folded in (StageParams::halo*)
    hipError_t (*stageMfmaHalo)(const StageParams& p, hipStream_t stream);
    hipError_t (*stageMfma2Halo)(const StageParams& p, hipStream_t stream); // the same on the face-by-face kernel (N >= 5)
    int mfma2OpsDoubles, mfma2KF; // face-by-face schedule (lift tiles padded per face)
    hipError_t (*stageMfma2)(int mode, const StageParams& p, hipStream_t stream);
    // state-once schedule, one wave per SIMD with software-pipelined loads (same MfmaOps2 image; three fields, no
    // sources, no halo staging): sw2d_mfma3_kernel.hpp
    hipError_t (*stageMfma3)(int mode, const StageParams& p, hipStream_t stream);
    hipError_t (*stageMfma3Halo)(const StageParams& p, hipStream_t stream); // MODE_LSERK with the halo staging folded in
    // per-node geometry (geo / fgeo planes); filter: plain operators + MT*KV Filter tiles in the image
    hipError_t (*stageMfma3Nodal)(int mode, bool filter, const StageParams& p, hipStream_t stream);
    // N >= 5: the matrix-core kernels with sources, one SrcForm each. identity (Once* forms only): the image's F' tiles are the
    // identity (no filter) -- the instance that adds the sources pointwise instead of multiplying by them
    hipError_t (*stageMfma2Src)(int mode, const StageParams& p, const PhysParams& ph, SrcForm form, bool identity, hipStream_t stream);
    int mfma3SrcFields; // 0: no state-once kernel with sources at this order; else the number of fields it takes (up to)
    int mfma3TracerPhase; // 1: SrcForm::OnceTracerPhase exists (N = 8)
    // variant D (tracer + sources), straight-sided elements, nf = 3 or 4 waves per 64 elements
    int vdOpsDoubles;
    hipError_t (*stageVd)(int mode, const StageParams& p, const VdParams& vp, hipStream_t stream);
    // unrolled affine kernel + momentum sources (N <= 4), the fast path of variants C / D; tracer: four-field state, the tracer
    // equation in the same pass
    hipError_t (*stageAffineSrc)(int mode, const StageParams& p, const PhysParams& ph, bool tracer, hipStream_t stream);
    // tracer equation alone (field 3 of a four-field state), unrolled; N <= 4
    hipError_t (*stageTracer)(int mode, const StageParams& p, hipStream_t stream);
    // variant B (depth, star states, open boundary, global Lax-Friedrichs speed, sources). speedPass: the speed of the state over
    // [kbegin, kend) is reduced into partials (one double per 256 elements) and *lam first (else vp.lam is current: accumulated by
    // the launch that wrote the state, or reduced over all ranks beforehand); then the `then` kernel. filterT (Unrolled only):
    // [m][i] = F[i][m], or nullptr
    hipError_t (*stageVb)(int mode, const StageParams& p, const VbParams& vp, double* partials, double* lam, bool speedPass,
                          VbStage then, const double* filterT, hipStream_t stream);
    // variant B (variantB) and variants C / D (else) on per-node geometry (sw2d_vn_kernel.hpp): ops = VnOps image; filt != nullptr:
    // the filtered RHS in two passes (unfiltered rows to raw, nf planes; then Filter and the update); speedPass: variant B's
    // global speed of this state is reduced into *lam first (else vb.lam is current)
    int vnOpsDoubles;
    hipError_t (*stageVn)(int mode, bool variantB, const StageParams& p, const VdParams& vd, const VbParams& vb, const double* ops,
                          const double* filt, double* raw, double* partials, double* lam, bool speedPass, hipStream_t stream);
    // per-block partial maxima (2 doubles per block of 256 elements)
    hipError_t (*dt)(const double* q, const double* fscale, const double* H, long long ld, int K, double g,
                     double* partials, hipStream_t stream);
    // output step: which = 0 eta (h - H or h), 1 u, 2 v; M = (Np, Np) lattice interpolation or nullptr
    hipError_t (*output)(const double* q, const double* H, const double* M, double* out, long long ld, int K, int which,
                         hipStream_t stream);
    // volume node index of face node (f, n), for validating the caller's vmapM
    int (*fmask)(int f, int n);
};

const KernelTable* kernel_table(int order); // nullptr if the order is not compiled in

} // namespace bdg_dev
