// Instantiates the sw2d kernels for one polynomial order (-DBDG_ORDER=N).
#include "sw2d_launch.hpp"
#include "sw2d_launch_host.hpp"
#include <hip/hip_ext.h>
#include <algorithm>
#include <cstdlib>

#ifndef BDG_ORDER
#error "compile with -DBDG_ORDER=<polynomial order>"
#endif

// A launch that records p.stopEvent (when set) through the dispatch's own completion signal: one packet instead of two on the
// queue, which is what the dependent launch on the other stream of a partitioned stage waits behind (sw2d_device.hip).
#define BDG_LAUNCH_EV(kern, grid, block, lds, stream, p, ...)                                                          \
    do {                                                                                                                \
        if ((p).stopEvent) {                                                                                            \
            hipExtLaunchKernelGGL(kern, grid, block, lds, stream, nullptr, (p).stopEvent, 0, p, ##__VA_ARGS__);         \
            if ((p).stopEventUsed) *(p).stopEventUsed = true;                                                           \
        } else {                                                                                                        \
            hipLaunchKernelGGL(kern, grid, block, lds, stream, p, ##__VA_ARGS__);                                       \
        }                                                                                                               \
    } while (0)

namespace bdg_dev {
namespace {

static_assert(TriModes::RHS == MODE_RHS && TriModes::LSERK == MODE_LSERK && TriModes::COMBINE == MODE_COMBINE, "sw2d_dispatch.hpp");

constexpr int kN = BDG_ORDER;
constexpr int kBlock = 256;
// The unrolled kernels run one wave per SIMD (their registers fill a SIMD's file). With one-wave workgroups
// every SIMD takes its next wave the moment its own finishes; with four-wave workgroups the CU waits for the
// slowest of the four (C3, N=4: 0.345 ms against 0.384 ms; 250 k elements: 0.102 against 0.111 ms).
constexpr int kUnrolledBlock = 64;
// Orders above this use the field-split kernels only (3*Np accumulators exceed the VGPR file).
constexpr bool kHighOrder = BDG_ORDER > 6;
// The unrolled source-term / tracer / variant-B kernels are the default only up to N = 4 (createSolver:
// kUnrolledSourcesMaxOrder); above it they are not instantiated (each costs minutes of compile time).
constexpr bool kNoUnrolledSources = BDG_ORDER > 4;
// The streamed unrolled A/B variants (BDG_SW2D_AFFINE_VARIANT = 2, 3) exist up to N = 5.
constexpr bool kNoStream = BDG_ORDER > 5;
// The matrix-core source-term / tracer / variant-B kernels exist from this order up.
constexpr bool kMfmaSources = BDG_ORDER >= 5;
// state-once kernel with sources (sw2d_mfma3src_kernel.hpp): with the tracer too at N = 5, 6, 7 (N = 7 with tracer: 501-512
// registers, 3 spilled in the combine form and still 1.9 times the two-wave kernels); three fields at N = 8, without the
// next-tile prefetch (registers) -- four fields' state tiles + operators + F' tiles would exceed 160 KB of LDS there
constexpr int kMfma3SrcFields = (BDG_ORDER >= 5 && BDG_ORDER <= 7) ? 4 : (BDG_ORDER == 8 ? 3 : 0);
// ... and at N = 8 the tracer equation as a second phase of every tile of that three-field kernel (TPHASE, sw2d_mfma3src_kernel.hpp)
constexpr bool kTracerPhase = BDG_ORDER == 8;

// ---- launch arithmetic
bool emptyRange(const StageParams& p) { return p.kend <= p.kbegin; }
// workgroups that take `per` elements each
unsigned blocksOf(const StageParams& p, int per) { return static_cast<unsigned>((p.kend - p.kbegin + per - 1) / per); }
// the unrolled kernels' one-wave workgroups (N <= 6: above, none of them exists)
[[maybe_unused]] unsigned unrolledGrid(const StageParams& p) { return blocksOf(p, kUnrolledBlock); }
// Matrix-core kernels: 16-element tiles, four to a four-wave workgroup; the waves loop over their tiles, so a launch has at
// most `cap` workgroups.
unsigned tileWorkgroups(unsigned ntiles, unsigned cap) { return std::min((ntiles + 3u) / 4u, cap); }
// ... with the cap from what a CU holds: up to `waves` workgroups (waves per SIMD) as far as 160 KB of LDS allow
struct TileGrid { unsigned ntiles, perCu, grid; };
TileGrid tileGrid(const StageParams& p, size_t ldsBytes, size_t waves) {
    const unsigned ntiles = blocksOf(p, 16);
    const unsigned perCu = static_cast<unsigned>(std::min<size_t>(waves, std::max<size_t>(1, (160u * 1024u) / ldsBytes)));
    return {ntiles, perCu, tileWorkgroups(ntiles, 256u * perCu)};
}

// Rolled kernels. FIELDS = 1 (three waves per 64 elements, one field each) exists for every
// order; FIELDS = 3 (all fields per lane) only where 3*Np accumulators fit (N <= 6).
template <int MODE, int FIELDS>
hipError_t launchRolled(const StageParams& p, hipStream_t stream) {
    if (emptyRange(p)) return hipSuccess;
    hipLaunchKernelGGL((sw2d_stage_affine_rolled_kernel<kN, MODE, FIELDS>), dim3(blocksOf(p, FIELDS == 3 ? 256 : 64)),
                       dim3(FIELDS == 3 ? 256 : 192), 0, stream, p);
    return hipGetLastError();
}

template <int FIELDS>
hipError_t stageRolled(int mode, const StageParams& p, hipStream_t stream) {
    return forMode(mode, [&](auto m) { return launchRolled<decltype(m)::value, FIELDS>(p, stream); });
}

hipError_t stageFieldSplit(int mode, const StageParams& p, hipStream_t stream) { return stageRolled<1>(mode, p, stream); }

template <int MODE, bool FILTER>
hipError_t launchStage(const StageParams& p, hipStream_t stream) {
    if constexpr (kHighOrder) return hipErrorNotSupported;
    else {
    if (emptyRange(p)) return hipSuccess;
    hipLaunchKernelGGL((sw2d_stage_kernel<kN, MODE, FILTER>), dim3(blocksOf(p, kBlock)), dim3(kBlock), 0, stream, p);
    return hipGetLastError();
    }
}

hipError_t stage(int mode, bool filter, const StageParams& p, hipStream_t stream) {
    return forModeFilter(mode, filter, [&](auto m, auto f) { return launchStage<decltype(m)::value, decltype(f)::value>(p, stream); });
}

template <int MODE>
hipError_t launchAffine(const StageParams& p, hipStream_t stream) {
    if constexpr (kHighOrder) return stageFieldSplit(MODE, p, stream);
    else {
    if (emptyRange(p)) return hipSuccess;
    const dim3 grid(unrolledGrid(p)), blk(kUnrolledBlock);
    if constexpr (MODE == MODE_COMBINE) {
        if (p.sponge != 0.0) {
            hipLaunchKernelGGL((sw2d_stage_affine_kernel<kN, MODE, 0, false, true>), grid, blk, 0, stream, p, PhysParams{});
            return hipGetLastError();
        }
    }
    if (p.syncSignal) return hipErrorNotSupported; // (no SYNC instance of the unrolled kernel: see flagSyncUsable in sw2d_device.hip)
    if constexpr (MODE == MODE_LSERK && kN <= 4) {
        if (p.faceLink) { // gathers through the face links; the residual rows only where the stage needs them
            switch (p.stageKind) {
            case STAGE_FIRST:
                BDG_LAUNCH_EV((sw2d_stage_affine_kernel<kN, MODE, 0, false, false, STAGE_FIRST>), grid, blk, 0, stream, p, PhysParams{});
                break;
            case STAGE_MID:
                BDG_LAUNCH_EV((sw2d_stage_affine_kernel<kN, MODE, 0, false, false, STAGE_MID>), grid, blk, 0, stream, p, PhysParams{});
                break;
            case STAGE_LAST:
                BDG_LAUNCH_EV((sw2d_stage_affine_kernel<kN, MODE, 0, false, false, STAGE_LAST>), grid, blk, 0, stream, p, PhysParams{});
                break;
            default: return hipErrorInvalidValue;
            }
            return hipGetLastError();
        }
    }
    BDG_LAUNCH_EV((sw2d_stage_affine_kernel<kN, MODE>), grid, blk, 0, stream, p, PhysParams{});
    return hipGetLastError();
    }
}

// unrolled kernel with the momentum sources (orders where it exists: N <= 4)
template <int MODE>
hipError_t launchAffineSrc(const StageParams& p, const PhysParams& ph, bool tracer, hipStream_t stream) {
    if constexpr (kNoUnrolledSources) return hipErrorNotSupported;
    else {
    if (emptyRange(p)) return hipSuccess;
    const dim3 grid(unrolledGrid(p)), blk(kUnrolledBlock);
    if constexpr (MODE == MODE_COMBINE) {
        if (p.sponge != 0.0) { // the instances with the momentum relaxation
            if (tracer) {
                if (ph.fmat) hipLaunchKernelGGL((sw2d_stage_affine_kernel<kN, MODE, 2, true, true>), grid, blk, 0, stream, p, ph);
                else hipLaunchKernelGGL((sw2d_stage_affine_kernel<kN, MODE, 1, true, true>), grid, blk, 0, stream, p, ph);
            } else {
                if (ph.fmat) hipLaunchKernelGGL((sw2d_stage_affine_kernel<kN, MODE, 2, false, true>), grid, blk, 0, stream, p, ph);
                else hipLaunchKernelGGL((sw2d_stage_affine_kernel<kN, MODE, 1, false, true>), grid, blk, 0, stream, p, ph);
            }
            return hipGetLastError();
        }
    }
    if (tracer) {
        if (ph.fmat) hipLaunchKernelGGL((sw2d_stage_affine_kernel<kN, MODE, 2, true>), grid, blk, 0, stream, p, ph);
        else hipLaunchKernelGGL((sw2d_stage_affine_kernel<kN, MODE, 1, true>), grid, blk, 0, stream, p, ph);
    } else {
        if (ph.fmat) hipLaunchKernelGGL((sw2d_stage_affine_kernel<kN, MODE, 2>), grid, blk, 0, stream, p, ph);
        else hipLaunchKernelGGL((sw2d_stage_affine_kernel<kN, MODE, 1>), grid, blk, 0, stream, p, ph);
    }
    return hipGetLastError();
    }
}

template <int MODE>
hipError_t launchTracer(const StageParams& p, hipStream_t stream) {
    if constexpr (kNoUnrolledSources) return hipErrorNotSupported;
    else {
    if (emptyRange(p)) return hipSuccess;
    hipLaunchKernelGGL((sw2d_stage_tracer_kernel<kN, MODE>), dim3(unrolledGrid(p)), dim3(kUnrolledBlock), 0, stream, p);
    return hipGetLastError();
    }
}

hipError_t stageTracer(int mode, const StageParams& p, hipStream_t stream) {
    return forMode(mode, [&](auto m) { return launchTracer<decltype(m)::value>(p, stream); });
}

hipError_t stageAffineSrc(int mode, const StageParams& p, const PhysParams& ph, bool tracer, hipStream_t stream) {
    return forMode(mode, [&](auto m) { return launchAffineSrc<decltype(m)::value>(p, ph, tracer, stream); });
}

template <int MODE, int WAVES>
hipError_t launchStream(const StageParams& p, hipStream_t stream) {
    if constexpr (kNoStream) return stageFieldSplit(MODE, p, stream); // A/B variant, N <= 5 only
    else {
    if (emptyRange(p)) return hipSuccess;
    hipLaunchKernelGGL((sw2d_stage_affine_stream_kernel<kN, MODE, WAVES>), dim3(blocksOf(p, kBlock)), dim3(kBlock), 0, stream, p);
    return hipGetLastError();
    }
}

hipError_t stageAffine(int mode, AffineVariant variant, const StageParams& p, hipStream_t stream) {
    if (variant == AffineVariant::FieldSplit) return stageFieldSplit(mode, p, stream);
    if (variant == AffineVariant::Xchg) { // A/B (sw2d_affine_xchg_kernel.hpp), LSERK stages; other modes: Unrolled
        if constexpr (!kNoStream) {
            if (mode == MODE_LSERK && fitsOneDescriptor(3, Elem<kN>::Np, p.ld)) {
                if (emptyRange(p)) return hipSuccess;
                const unsigned magic = static_cast<unsigned>((0x100000000ull + static_cast<unsigned long long>(p.ld) - 1ull) / static_cast<unsigned long long>(p.ld));
                hipLaunchKernelGGL((sw2d_stage_affine_xchg_kernel<kN>), dim3(unrolledGrid(p)), dim3(kUnrolledBlock), 0, stream, p, magic);
                return hipGetLastError();
            }
        }
    }
    if (variant == AffineVariant::Lean) { // A/B (sw2d_affine_lean_kernel.hpp), LSERK stages; other modes: Unrolled
        if constexpr (!kNoStream) {
            if (mode == MODE_LSERK) {
                if (emptyRange(p)) return hipSuccess;
                hipLaunchKernelGGL((sw2d_stage_affine_lean_kernel<kN>), dim3(unrolledGrid(p)), dim3(kUnrolledBlock), 0, stream, p);
                return hipGetLastError();
            }
        }
    }
    return forMode(mode, [&](auto m) {
        constexpr int MODE = decltype(m)::value;
        switch (variant) {
        case AffineVariant::Rolled:
            if constexpr (kHighOrder) return stageFieldSplit(MODE, p, stream);
            else return launchRolled<MODE, 3>(p, stream);
        case AffineVariant::Stream2: return launchStream<MODE, 2>(p, stream);
        case AffineVariant::Stream3: return launchStream<MODE, 3>(p, stream);
        default: return launchAffine<MODE>(p, stream);
        }
    });
}

template <int MODE>
hipError_t launchMfma(const StageParams& p, hipStream_t stream) {
    if (emptyRange(p)) return hipSuccess;
    const size_t ldsBytes = sizeof(double) * MfmaOps<kN>::DOUBLES;
    const TileGrid g = tileGrid(p, ldsBytes, 8);
    if (p.syncSignal) { // interior launch of a partitioned stage with in-kernel dependencies: one signal per ring tile
        if constexpr (MODE == MODE_LSERK) {
            if (p.syncSignalsOut) *p.syncSignalsOut = g.ntiles - std::min(g.ntiles, static_cast<unsigned>(p.syncFirstTile));
            hipLaunchKernelGGL((sw2d_stage_mfma_kernel<kN, MODE_LSERK, false, true>), dim3(g.grid), dim3(256), ldsBytes, stream, p);
            return hipGetLastError();
        } else return hipErrorNotSupported;
    }
    hipLaunchKernelGGL((sw2d_stage_mfma_kernel<kN, MODE>), dim3(g.grid), dim3(256), ldsBytes, stream, p);
    return hipGetLastError();
}

// one LSERK4 stage of the partition-boundary elements with the halo staging folded in
hipError_t stageMfmaHalo(const StageParams& p, hipStream_t stream) {
    if (emptyRange(p)) return hipSuccess;
    const size_t ldsBytes = sizeof(double) * MfmaOps<kN>::DOUBLES;
    const TileGrid g = tileGrid(p, ldsBytes, 8);
    if (p.syncSignal) { // waits for the previous interior launch's ring tiles in the kernel, one signal per workgroup
        if (p.syncSignalsOut) *p.syncSignalsOut = g.grid;
        hipLaunchKernelGGL((sw2d_stage_mfma_kernel<kN, MODE_LSERK, true, true>), dim3(g.grid), dim3(256), ldsBytes, stream, p);
        return hipGetLastError();
    }
    // event form (2- and 4-way splits of N <= 4: the interior share runs on the unrolled kernel): one-wave workgroups, one tile each, so that
    // the launch finds room beside the interior launch (sw2d_stage_mfma_kernel, THREADS); BDG_SW2D_STRIP_WORKGROUP=256 restores the four-wave form
    static const bool fourWaves = [] { const char* e = std::getenv("BDG_SW2D_STRIP_WORKGROUP"); return e && std::atoi(e) == 256; }();
    if (!fourWaves && kN <= 4) {
        BDG_LAUNCH_EV((sw2d_stage_mfma_kernel<kN, MODE_LSERK, true, false, 64>), dim3(std::min(g.ntiles, 2048u * g.perCu)), dim3(64), ldsBytes, stream, p);
        return hipGetLastError();
    }
    BDG_LAUNCH_EV((sw2d_stage_mfma_kernel<kN, MODE_LSERK, true>), dim3(g.grid), dim3(256), ldsBytes, stream, p);
    return hipGetLastError();
}

// the same for the face-by-face matrix-core kernel (the boundary strip's kernel at N >= 5)
hipError_t stageMfma2Halo(const StageParams& p, hipStream_t stream) {
    if (emptyRange(p)) return hipSuccess;
    const size_t ldsBytes = sizeof(double) * MfmaOps2<kN>::DOUBLES;
    hipLaunchKernelGGL((sw2d_stage_mfma2_kernel<kN, MODE_LSERK, 0, false, true>), dim3(tileGrid(p, ldsBytes, BDG_MFMA2_WAVES).grid), dim3(256),
                       ldsBytes, stream, p, PhysParams{});
    return hipGetLastError();
}

hipError_t stageMfma(int mode, const StageParams& p, hipStream_t stream) {
    return forMode(mode, [&](auto m) { return launchMfma<decltype(m)::value>(p, stream); });
}

template <int MODE>
hipError_t launchMfma2(const StageParams& p, hipStream_t stream) {
    if (emptyRange(p)) return hipSuccess;
    const size_t ldsBytes = sizeof(double) * MfmaOps2<kN>::DOUBLES;
    hipLaunchKernelGGL((sw2d_stage_mfma2_kernel<kN, MODE>), dim3(tileGrid(p, ldsBytes, BDG_MFMA2_WAVES).grid), dim3(256), ldsBytes, stream, p,
                       PhysParams{});
    return hipGetLastError();
}

template <int MODE, bool NODAL = false, bool NFILT = false>
hipError_t launchMfma3(const StageParams& p, hipStream_t stream) {
    if (emptyRange(p)) return hipSuccess;
    const size_t ldsBytes = sizeof(double) * (Mfma3Lds<kN>::DOUBLES + (NFILT ? MfmaOps2<kN>::MT * MfmaOps2<kN>::KV * 64 : 0));
    auto kern = sw2d_stage_mfma3_kernel<kN, MODE, false, NODAL, NFILT>;
    if (const hipError_t e = allowDynamicLds(kern, ldsBytes); e != hipSuccess) return e;
    const unsigned ntiles = blocksOf(p, 16);
    // one four-wave workgroup per CU, one wave per SIMD
    const dim3 grid(tileWorkgroups(ntiles, p.gridCap > 0 ? static_cast<unsigned>(p.gridCap) : 256u));
    static const int interleave = [] { const char* e = std::getenv("BDG_SW2D_TILE_INTERLEAVE"); return e ? std::atoi(e) : 1; }();
    static const int stagger = [] { const char* e = std::getenv("BDG_SW2D_STAGGER"); return e ? std::atoi(e) : 0; }();
    StageParams pi = p;
    pi.tileInterleave = interleave;
    pi.stagger = stagger;
#ifdef BDG_PHASE_CLOCK
    pi.phaseClock = phaseClockBuffer<1024, 16>(); // per wave
    if (!pi.phaseClock) return hipErrorOutOfMemory;
    hipLaunchKernelGGL(kern, grid, dim3(256), ldsBytes, stream, pi);
    return hipGetLastError();
#else
    if (p.syncSignal) { // interior launch of a partitioned stage with in-kernel dependencies: one signal per ring tile
        if constexpr (MODE == MODE_LSERK && !NODAL && !NFILT) {
            auto kernSync = sw2d_stage_mfma3_kernel<kN, MODE_LSERK, false, false, false, true>;
            if (const hipError_t e = allowDynamicLds(kernSync, ldsBytes); e != hipSuccess) return e;
            if (p.syncSignalsOut) *p.syncSignalsOut = ntiles - std::min(ntiles, static_cast<unsigned>(p.syncFirstTile));
            hipLaunchKernelGGL(kernSync, grid, dim3(256), ldsBytes, stream, pi);
            return hipGetLastError();
        } else return hipErrorNotSupported;
    }
    BDG_LAUNCH_EV(kern, grid, dim3(256), ldsBytes, stream, pi);
    return hipGetLastError();
#endif
}

// per-node geometry (StageParams::geo / fgeo) on the same schedule
// filter: the image in p.opsAffine carries the Filter tiles behind the plain operators
hipError_t stageMfma3Nodal(int mode, bool filter, const StageParams& p, hipStream_t stream) {
    return forModeFilter(mode, filter, [&](auto m, auto f) { return launchMfma3<decltype(m)::value, true, decltype(f)::value>(p, stream); });
}

// one LSERK4 stage of the partition-boundary elements with the halo staging folded in, state-once schedule
hipError_t stageMfma3Halo(const StageParams& p, hipStream_t stream) {
    if (emptyRange(p)) return hipSuccess;
    const size_t ldsBytes = sizeof(double) * Mfma3Lds<kN>::DOUBLES;
    auto kern = sw2d_stage_mfma3_kernel<kN, MODE_LSERK, true>;
    if (const hipError_t e = allowDynamicLds(kern, ldsBytes); e != hipSuccess) return e;
    const unsigned ntiles = blocksOf(p, 16);
    // Strips (up to a few thousand elements): the latency form, a tile shared by three waves (one field each). Larger
    // boundary sets: the throughput form.
    if (ntiles <= 1024u && !std::getenv("BDG_SW2D_STRIP_THROUGHPUT")) {
        const size_t stripLds = sizeof(double) * MfmaOps2<kN>::DOUBLES;
        if (p.syncSignal) { // waits for the previous interior launch's ring tiles in the kernel, one signal per workgroup
            if (p.syncSignalsOut) *p.syncSignalsOut = ntiles;
            hipLaunchKernelGGL((sw2d_strip_mfma3_kernel<kN, true>), dim3(ntiles), dim3(192), stripLds, stream, p);
            return hipGetLastError();
        }
        BDG_LAUNCH_EV((sw2d_strip_mfma3_kernel<kN>), dim3(ntiles), dim3(192), stripLds, stream, p);
        return hipGetLastError();
    }
    if (p.syncSignal) return hipErrorNotSupported; // (the throughput form has no in-kernel dependencies: the caller keeps the events)
    BDG_LAUNCH_EV(kern, dim3(tileWorkgroups(ntiles, 256u)), dim3(256), ldsBytes, stream, p);
    return hipGetLastError();
}

hipError_t stageMfma3(int mode, const StageParams& p, hipStream_t stream) {
    return forMode(mode, [&](auto m) { return launchMfma3<decltype(m)::value>(p, stream); });
}

// The matrix-core kernels with sources (SrcForm, sw2d_launch.hpp). Orders above the unrolled kernels' range only.
template <int MODE>
hipError_t launchMfma2Src(const StageParams& p, const PhysParams& ph, SrcForm form, bool identity, hipStream_t stream) {
    if constexpr (!kMfmaSources) return hipErrorNotSupported;
    else {
    if (emptyRange(p)) return hipSuccess;
    using O = MfmaOps2<kN>;
    const bool tracerPass = form == SrcForm::TracerPass;
    const size_t ldsBytes = sizeof(double) * (O::DOUBLES + (tracerPass ? 0 : O::MT * O::KV * 64));
    const dim3 grid(tileGrid(p, ldsBytes, tracerPass ? 3 : BDG_MFMA2_WAVES).grid), blk(256);
    switch (form) {
    case SrcForm::Sources: hipLaunchKernelGGL((sw2d_stage_mfma2_kernel<kN, MODE, 1>), grid, blk, ldsBytes, stream, p, ph); break;
    case SrcForm::TracerPass: hipLaunchKernelGGL((sw2d_stage_mfma2_tracer_kernel<kN, MODE>), grid, blk, ldsBytes, stream, p); break;
    case SrcForm::VariantB: hipLaunchKernelGGL((sw2d_stage_mfma2_kernel<kN, MODE, 2>), grid, blk, ldsBytes, stream, p, ph); break;
    case SrcForm::SourcesTracer:
        if constexpr (O::MT <= 2) hipLaunchKernelGGL((sw2d_stage_mfma2_kernel<kN, MODE, 1, true>), grid, blk, ldsBytes, stream, p, ph);
        else return hipErrorNotSupported;
        break;
    default: { // the state-once schedule
        if constexpr (kMfma3SrcFields == 0) return hipErrorNotSupported;
        else {
            const bool four = form == SrcForm::OnceSourcesTracer || form == SrcForm::OnceTracerPhase;
            if (!fitsOneDescriptor(four ? 4 : 3, Elem<kN>::Np, p.ld)) return hipErrorNotSupported;
            auto launch = [&](auto kern, size_t lds) -> hipError_t {
                if (const hipError_t e = allowDynamicLds(kern, lds); e != hipSuccess) return e;
                hipLaunchKernelGGL(kern, dim3(tileWorkgroups(blocksOf(p, 16), 256u)), blk, lds, stream, p, ph); // one four-wave workgroup per CU
                return hipGetLastError();
            };
            constexpr size_t lds3 = sizeof(double) * Mfma3SrcLds<kN, false>::DOUBLES, lds4 = sizeof(double) * Mfma3SrcLds<kN, true>::DOUBLES;
            if (form == SrcForm::OnceSourcesTracer) {
                if constexpr (kMfma3SrcFields >= 4)
                    return identity ? launch(sw2d_stage_mfma3src_kernel<kN, MODE, true, 1, false, true>, lds4)
                                    : launch(sw2d_stage_mfma3src_kernel<kN, MODE, true>, lds4);
                else return hipErrorNotSupported;
            }
            if (form == SrcForm::OnceTracerPhase) {
                if constexpr (kTracerPhase)
                    return identity ? launch(sw2d_stage_mfma3src_kernel<kN, MODE, false, 1, true, true>, lds4)
                                    : launch(sw2d_stage_mfma3src_kernel<kN, MODE, false, 1, true>, lds4);
                else return hipErrorNotSupported;
            }
            if (form == SrcForm::OnceVariantB)
                return identity ? launch(sw2d_stage_mfma3src_kernel<kN, MODE, false, 2, false, true>, lds3)
                                : launch(sw2d_stage_mfma3src_kernel<kN, MODE, false, 2>, lds3);
            return identity ? launch(sw2d_stage_mfma3src_kernel<kN, MODE, false, 1, false, true>, lds3)
                            : launch(sw2d_stage_mfma3src_kernel<kN, MODE, false>, lds3);
        }
    }
    }
    return hipGetLastError();
    }
}

hipError_t stageMfma2Src(int mode, const StageParams& p, const PhysParams& ph, SrcForm form, bool identity, hipStream_t stream) {
    return forMode(mode, [&](auto m) { return launchMfma2Src<decltype(m)::value>(p, ph, form, identity, stream); });
}

hipError_t stageMfma2(int mode, const StageParams& p, hipStream_t stream) {
    return forMode(mode, [&](auto m) { return launchMfma2<decltype(m)::value>(p, stream); });
}

template <int MODE>
hipError_t launchVd(const StageParams& p, const VdParams& vp, hipStream_t stream) {
    if (emptyRange(p)) return hipSuccess;
    hipLaunchKernelGGL((sw2d_stage_vd_kernel<kN, MODE>), dim3(blocksOf(p, 64)), dim3(64 * (vp.nf - vp.cbase)), 0, stream, p, vp);
    return hipGetLastError();
}

hipError_t stageVd(int mode, const StageParams& p, const VdParams& vp, hipStream_t stream) {
    return forMode(mode, [&](auto m) { return launchVd<decltype(m)::value>(p, vp, stream); });
}

// variant B's global speed of the state in p.qin: per-block partial maxima, then their maximum into *lam
template <class SpeedKernel>
void launchSpeed(SpeedKernel kern, const StageParams& p, const VbParams& vb, double* partials, double* lam, hipStream_t stream) {
    const unsigned nblocks = blocksOf(p, 256);
    hipLaunchKernelGGL(kern, dim3(nblocks), dim3(256), 0, stream, p, vb, partials);
    hipLaunchKernelGGL((sw2d_vb_speed_reduce_kernel<kN>), dim3(1), dim3(256), 0, stream, partials, static_cast<int>(nblocks), lam);
}

template <int MODE>
hipError_t launchVb(const StageParams& p, const VbParams& vp, double* partials, double* lam, bool speedPass, VbStage then,
                    const double* filterT, hipStream_t stream) {
    if (emptyRange(p)) return hipSuccess;
    // (a solver on per-node geometry has no affine table: its speed alone is asked for here by the partitioned steppers,
    // and comes from the kernel its own stage launches run in front of them, launchVn)
    if (speedPass && p.ageo) launchSpeed(sw2d_vb_speed_kernel<kN>, p, vp, partials, lam, stream);
    else if (speedPass) launchSpeed(sw2d_vn_speed_kernel<kN>, p, vp, partials, lam, stream);
    if (then == VbStage::None) return hipGetLastError();
    if constexpr (!kNoUnrolledSources) {
        if (then == VbStage::Unrolled) {
            const dim3 grid(unrolledGrid(p)), blk(kUnrolledBlock);
            if (filterT) hipLaunchKernelGGL((sw2d_stage_vb_unrolled_kernel<kN, MODE, true>), grid, blk, 0, stream, p, vp, filterT);
            else hipLaunchKernelGGL((sw2d_stage_vb_unrolled_kernel<kN, MODE, false>), grid, blk, 0, stream, p, vp, filterT);
            return hipGetLastError();
        }
    }
    hipLaunchKernelGGL((sw2d_stage_vb_kernel<kN, MODE>), dim3(blocksOf(p, 64)), dim3(192), 0, stream, p, vp);
    return hipGetLastError();
}

hipError_t stageVb(int mode, const StageParams& p, const VbParams& vp, double* partials, double* lam, bool speedPass, VbStage then,
                   const double* filterT, hipStream_t stream) {
    return forMode(mode, [&](auto m) { return launchVb<decltype(m)::value>(p, vp, partials, lam, speedPass, then, filterT, stream); });
}

// ---- variants B / C / D on per-node geometry (sw2d_vn_kernel.hpp); PHYS = 2: variant B, 1: variants C / D
template <int MODE, int PHYS>
hipError_t launchVn(const StageParams& p, const VdParams& vd, const VbParams& vb, const double* ops, const double* filt, double* raw,
                    double* partials, double* lam, bool speedPass, hipStream_t stream) {
    if (emptyRange(p)) return hipSuccess;
    if (PHYS == 2 && speedPass) launchSpeed(sw2d_vn_speed_kernel<kN>, p, vb, partials, lam, stream);
    const dim3 grid(blocksOf(p, 64)), blk(64 * (PHYS == 2 ? 3 : vd.nf));
    if (!filt) {
        hipLaunchKernelGGL((sw2d_stage_vn_kernel<kN, MODE, PHYS>), grid, blk, 0, stream, p, vd, vb, ops);
    } else {
        StageParams pr = p;
        pr.rhs = raw;
        hipLaunchKernelGGL((sw2d_stage_vn_kernel<kN, MODE_RHS, PHYS>), grid, blk, 0, stream, pr, vd, vb, ops);
        hipLaunchKernelGGL((sw2d_filter_rows_kernel<kN, MODE, PHYS>), grid, blk, 0, stream, p, raw, filt, vb.sponge, 0);
    }
    return hipGetLastError();
}

hipError_t stageVn(int mode, bool variantB, const StageParams& p, const VdParams& vd, const VbParams& vb, const double* ops,
                   const double* filt, double* raw, double* partials, double* lam, bool speedPass, hipStream_t stream) {
    return forMode(mode, [&](auto m) {
        constexpr int MODE = decltype(m)::value;
        return variantB ? launchVn<MODE, 2>(p, vd, vb, ops, filt, raw, partials, lam, speedPass, stream)
                        : launchVn<MODE, 1>(p, vd, vb, ops, filt, raw, partials, lam, speedPass, stream);
    });
}

hipError_t dt(const double* q, const double* fscale, const double* H, long long ld, int K, double g, double* partials,
              hipStream_t stream) {
    const unsigned grid = static_cast<unsigned>((K + kBlock - 1) / kBlock);
    hipLaunchKernelGGL((sw2d_dt_kernel<kN>), dim3(grid), dim3(kBlock), 0, stream, q, fscale, H, ld, K, g, partials);
    return hipGetLastError();
}

hipError_t output(const double* q, const double* H, const double* M, double* out, long long ld, int K, int which,
                  hipStream_t stream) {
    const unsigned grid = static_cast<unsigned>((K + kBlock - 1) / kBlock);
    hipLaunchKernelGGL((sw2d_output_kernel<kN>), dim3(grid), dim3(kBlock), 0, stream, q, H, M, out, ld, K, which);
    return hipGetLastError();
}

int fmaskOf(int f, int n) { return Elem<kN>::fmask(f, n); }

} // namespace

// A host function (not a namespace-scope constant, which hipcc would also emit for
// the device and then fail to resolve the host function pointers in).
const KernelTable* BDG_CAT(kernel_table_order, BDG_ORDER)() {
    static const KernelTable table = {kN, Elem<kN>::Np, Elem<kN>::Nfp, kHighOrder ? 0 : Elem<kN>::LDS_DOUBLES, &stage,
                                      AffineOps<kN>::DOUBLES, &stageAffine, MfmaOps<kN>::DOUBLES, MfmaOps<kN>::MT,
                                      MfmaOps<kN>::KV, MfmaOps<kN>::KS, &stageMfma, &stageMfmaHalo, &stageMfma2Halo, MfmaOps2<kN>::DOUBLES, MfmaOps2<kN>::KF,
                                      &stageMfma2, &stageMfma3, &stageMfma3Halo, &stageMfma3Nodal, &stageMfma2Src, kMfma3SrcFields, kTracerPhase ? 1 : 0, VdOps<kN>::DOUBLES, &stageVd, &stageAffineSrc, &stageTracer, &stageVb, VnOps<kN>::DOUBLES, &stageVn, &dt, &output,
                                      &fmaskOf};
    return &table;
}

} // namespace bdg_dev
