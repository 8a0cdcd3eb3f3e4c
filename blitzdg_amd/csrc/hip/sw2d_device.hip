// sw2d_device.hip -- device-resident sw2d solver behind the C ABI
// (include/blitzdg_hip.h, group 2). Owns the HBM image of the DG tables and the
// state, launches the fused stage kernels (sw2d_kernels.hpp) on its own stream.
//
// HBM layout (fp64 planes of `ld` = K rounded up to 64 elements per nodal row):
//   qA, qB      3*Np*ld   state (h, hu, hv), double-buffered across stages
//   res         3*Np*ld   LSERK4 residual
//   aux         3*Np*ld   RHS output / RK2 intermediate stage
//   geo         4*Np*ld   rx, sx, ry, sy
//   fgeo        9*Nfp*ld  nx, ny, Fscale
//   vmapP       3*Nfp*ld  int32 gather offsets (wall flag in the sign bit)
//   ops         Dr|Ds interleaved, Lift, Filter (copied to LDS by every workgroup)
// Elements may be renumbered internally (BDG_SW2D_REORDER); all I/O is in the
// caller's numbering.
// After bdg_sw2d_enable_variant_b4 a four-field solver evaluates variant B with the tracer as a fourth equation: the three-field
// variant-B launches, each followed by the tracer pass of sw2d_vb_tracer_kernel.hpp (per-order objects sw2d_vb4_order.hip).
// After bdg_sw2d_enable_tracer_diffusion every evaluation of a four-field solver is followed by the two passes of
// sw2d_diffusion_kernel.hpp (per-order objects sw2d_diffusion_order.hip), which add the tracer's diffusion, source and decay.
// After bdg_sw2d_enable_viscosity every evaluation is also followed by the two passes of sw2d_viscosity_kernel.hpp (per-order objects
// sw2d_viscosity_order.hip), which add the eddy viscosity's terms to the momentum planes and make the Heun step's sponge division.
// After bdg_sw2d_enable_monitor the stepping calls record diagnostics and gauges on the device (sw2d_monitor_kernel.hpp).
// After bdg_sw2d_enable_drifters they also advance Lagrangian drifters after every completed step (sw2d_drifter_kernel.hpp).
#include "../host/capi_internal.hpp"
#include "../host/element_order.hpp"
#include "../host/element_tables.hpp"
#include "../host/parallel_for.hpp"
#include "blitzdg/LSERK4.hpp"
#include "row_transfer.hpp"
#include "run_records.hpp"
#include "sw2d_launch.hpp"
#include "sw2d_launch_host.hpp"
#include "sw2d_vb4_launch.hpp"
#include "sw2d_diffusion_launch.hpp"
#include "sw2d_viscosity_launch.hpp"
#include "sw2d_drifter_kernel.hpp"
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <queue>
#include <stdexcept>
#include <string>
#include <vector>

namespace bdg_dev {

const KernelTable* kernel_table_order1();
const KernelTable* kernel_table_order2();
const KernelTable* kernel_table_order3();
const KernelTable* kernel_table_order4();
const KernelTable* kernel_table_order5();
const KernelTable* kernel_table_order6();
const KernelTable* kernel_table_order7();
const KernelTable* kernel_table_order8();

const KernelTable* kernel_table(int order) {
    switch (order) {
    case 1: return kernel_table_order1();
    case 2: return kernel_table_order2();
    case 3: return kernel_table_order3();
    case 4: return kernel_table_order4();
    case 5: return kernel_table_order5();
    case 6: return kernel_table_order6();
    case 7: return kernel_table_order7();
    case 8: return kernel_table_order8();
    default: return nullptr;
    }
}

const Vb4KernelTable* vb4_kernel_table_order1();
const Vb4KernelTable* vb4_kernel_table_order2();
const Vb4KernelTable* vb4_kernel_table_order3();
const Vb4KernelTable* vb4_kernel_table_order4();
const Vb4KernelTable* vb4_kernel_table_order5();
const Vb4KernelTable* vb4_kernel_table_order6();
const Vb4KernelTable* vb4_kernel_table_order7();
const Vb4KernelTable* vb4_kernel_table_order8();

const Vb4KernelTable* vb4_kernel_table(int order) {
    switch (order) {
    case 1: return vb4_kernel_table_order1();
    case 2: return vb4_kernel_table_order2();
    case 3: return vb4_kernel_table_order3();
    case 4: return vb4_kernel_table_order4();
    case 5: return vb4_kernel_table_order5();
    case 6: return vb4_kernel_table_order6();
    case 7: return vb4_kernel_table_order7();
    case 8: return vb4_kernel_table_order8();
    default: return nullptr;
    }
}

const DiffusionKernelTable* diffusion_kernel_table_order1();
const DiffusionKernelTable* diffusion_kernel_table_order2();
const DiffusionKernelTable* diffusion_kernel_table_order3();
const DiffusionKernelTable* diffusion_kernel_table_order4();
const DiffusionKernelTable* diffusion_kernel_table_order5();
const DiffusionKernelTable* diffusion_kernel_table_order6();
const DiffusionKernelTable* diffusion_kernel_table_order7();
const DiffusionKernelTable* diffusion_kernel_table_order8();

const DiffusionKernelTable* diffusion_kernel_table(int order) {
    switch (order) {
    case 1: return diffusion_kernel_table_order1();
    case 2: return diffusion_kernel_table_order2();
    case 3: return diffusion_kernel_table_order3();
    case 4: return diffusion_kernel_table_order4();
    case 5: return diffusion_kernel_table_order5();
    case 6: return diffusion_kernel_table_order6();
    case 7: return diffusion_kernel_table_order7();
    case 8: return diffusion_kernel_table_order8();
    default: return nullptr;
    }
}

const ViscosityKernelTable* viscosity_kernel_table_order1();
const ViscosityKernelTable* viscosity_kernel_table_order2();
const ViscosityKernelTable* viscosity_kernel_table_order3();
const ViscosityKernelTable* viscosity_kernel_table_order4();
const ViscosityKernelTable* viscosity_kernel_table_order5();
const ViscosityKernelTable* viscosity_kernel_table_order6();
const ViscosityKernelTable* viscosity_kernel_table_order7();
const ViscosityKernelTable* viscosity_kernel_table_order8();

const ViscosityKernelTable* viscosity_kernel_table(int order) {
    switch (order) {
    case 1: return viscosity_kernel_table_order1();
    case 2: return viscosity_kernel_table_order2();
    case 3: return viscosity_kernel_table_order3();
    case 4: return viscosity_kernel_table_order4();
    case 5: return viscosity_kernel_table_order5();
    case 6: return viscosity_kernel_table_order6();
    case 7: return viscosity_kernel_table_order7();
    case 8: return viscosity_kernel_table_order8();
    default: return nullptr;
    }
}

// Final reduction of the per-block partials of sw2d_dt_kernel (single block).
__global__ __launch_bounds__(256) void sw2d_reduce_kernel(const double* __restrict__ part, int nblocks,
                                                          double* __restrict__ out2) {
    __shared__ double sA[256], sB[256];
    __shared__ int sBad;
    if (threadIdx.x == 0) sBad = 0;
    __syncthreads();
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += blockDim.x) {
        const double x = part[2 * i], y = part[2 * i + 1];
        if (x != x || y != y) sBad = 1;
        a = fmax(a, x);
        b = fmax(b, y);
    }
    sA[threadIdx.x] = a;
    sB[threadIdx.x] = b;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (static_cast<int>(threadIdx.x) < s) {
            sA[threadIdx.x] = fmax(sA[threadIdx.x], sA[threadIdx.x + s]);
            sB[threadIdx.x] = fmax(sB[threadIdx.x], sB[threadIdx.x + s]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double nan = __builtin_nan("");
        out2[0] = sBad ? nan : sA[0];
        out2[1] = sBad ? nan : sB[0];
    }
}

// ---- bandwidth probes (measurement aids, not part of the solver)
// STREAM triad a = b + s*c on 16-byte lanes: the practical HBM roof of this device.
__global__ __launch_bounds__(256) void triad_kernel(double2* __restrict__ a, const double2* __restrict__ b,
                                                    const double2* __restrict__ c, double s, size_t n2) {
    const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
    for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n2; i += stride) {
        const double2 x = b[i], y = c[i];
        a[i] = make_double2(x.x + s * y.x, x.y + s * y.y);
    }
}

// Same rows, same 8-byte-per-lane accesses and same read/write mix as one fused LSERK stage of
// the affine kernel (reads: state 3Np rows, residual 3Np rows, 13 geometry rows, 3Nfp index rows;
// writes: residual and state, 6Np rows), with no gathers and almost no arithmetic: the time of
// this launch is the memory-system floor for the stage kernel's own access pattern. With face
// links: 3 index rows, no residual read (readRes = 0, first stage of a step) or no residual
// write (writeRes = 0, last stage). back = 1: the blocks from the high end, as the stage launches alternate (bdg_sw2d::nextSweep).
__global__ __launch_bounds__(256) void stage_traffic_probe_kernel(const double* __restrict__ qin, double* __restrict__ qout,
                                                                 double* __restrict__ res, const double* __restrict__ ageo,
                                                                 const int* __restrict__ vmapP, int rows, int idxRows,
                                                                 long long ld, int K, int readRes, int writeRes, int back) {
    const unsigned k = (back ? gridDim.x - 1u - blockIdx.x : blockIdx.x) * blockDim.x + threadIdx.x;
    if (k >= static_cast<unsigned>(K)) return;
    double acc = 0.0;
    for (int r = 0; r < 13; ++r) acc += ageo[r * ld + k];
    for (int r = 0; r < idxRows; ++r) acc += vmapP[r * ld + k];
    for (int r = 0; r < rows; ++r) {
        const double q = qin[r * ld + k], o = readRes ? res[r * ld + k] : 0.0;
        const double n = 0.5 * o + 1e-300 * (q + acc);
        if (writeRes) res[r * ld + k] = n;
        qout[r * ld + k] = q + 1e-300 * n;
    }
}

} // namespace bdg_dev

using bdg_detail::arg_error;
using bdg_detail::guard;
using bdg_detail::hip_error;
using bdg_detail::unstable_error;

using bdg_dev::DevBuf;
using bdg_dev::hipCheck;
using bdg_rccl::ncclCheck;
using bdg_rccl::rccl;

namespace {
std::vector<double> matmulHost(const double* A, const double* B, int n, int c);

// ---- run-time switches (A/B measurements and cross-checks; DESIGN.md section 3 lists them). Every name is read here and nowhere
// else, and WHEN it is read is part of its meaning: once per process (the first call fixes the value: set it before the process
// starts), when a solver is set up (the caller keeps the answer), or per call (the tests flip these within one process).
namespace env {
// -- once per process
// =n pins the crossover to the one-tile-per-wave kernel of whole-mesh and interior launches (default: kSmallLaunch[N])
int smallLaunchPinned() {
    static const int v = [] { const char* e = std::getenv("BDG_SW2D_SMALL_LAUNCH"); return e ? std::atoi(e) : -1; }();
    return v;
}
// =n pins the workgroup cap of the interior launch of a partitioned run (default: interiorGridCap)
int interiorCapPinned() {
    static const int v = [] { const char* e = std::getenv("BDG_SW2D_INTERIOR_CAP"); return e ? std::atoi(e) : 0; }();
    return v;
}
// =0: a stage's `done` event is recorded by a packet behind the launch instead of by the launch itself
bool extLaunch() {
    static const bool v = [] { const char* e = std::getenv("BDG_SW2D_EXT_LAUNCH"); return !e || e[0] != '0'; }();
    return v;
}
// -- when a solver is created (bdg_sw2d_create*)
const char* affineVariantPin() { return std::getenv("BDG_SW2D_AFFINE_VARIANT"); } // =0..9: one kernel family, no small-launch crossover
bool nodalVector() { return std::getenv("BDG_SW2D_NODAL_VECTOR") != nullptr; }      // per-node geometry on the vector kernel (N <= 6)
bool fullStageTraffic() {                                                            // no face links, residual read and written at every stage
    const char* e = std::getenv("BDG_SW2D_FULL_STAGE_TRAFFIC");
    return e && e[0] != '0';
}
// =forward: every whole-mesh stage launch walks the tiles from the low end (default: alternating, bdg_sw2d::nextSweep)
bool sweepForward() {
    const char* e = std::getenv("BDG_SW2D_SWEEP");
    return e && std::string(e) == "forward";
}
// ... and again when variant B is enabled: variants B/C/D on the rolled kernels
bool rolledSources() { return std::getenv("BDG_SW2D_ROLLED_SOURCES") != nullptr; }
// -- when the communicator is set up (bdg_sw2d_comm_init)
bool eventFence() { // =1 (older spelling: NOFENCE=0): the stage events keep their system-scope fence
    const char* on = std::getenv("BDG_SW2D_EVENT_FENCE");
    const char* off = std::getenv("BDG_SW2D_EVENT_NOFENCE");
    return (on && on[0] == '1') || (off && off[0] == '0');
}
bool noCommWarmup() { return std::getenv("BDG_SW2D_NO_COMM_WARMUP") != nullptr; }
// -- per call
bool eventSync() { // =1: the two chains of an exchanged stage meet through events, not inside the kernels
    const char* e = std::getenv("BDG_SW2D_EVENT_SYNC");
    return e && e[0] != '0';
}
bool sourcesProduct() { // =1: unfiltered evaluations with sources keep the products with the identity tiles (bit-identical)
    const char* e = std::getenv("BDG_SW2D_SOURCES_PRODUCT");
    return e && e[0] != '0';
}
bool speedPass() { return std::getenv("BDG_SW2D_SPEED_PASS") != nullptr; }             // variant B always runs its separate speed pass
bool tracerPass() { return std::getenv("BDG_SW2D_TRACER_PASS") != nullptr; }           // the tracer in a pass of its own
bool sourcesTwoWave() { return std::getenv("BDG_SW2D_SOURCES_TWO_WAVE") != nullptr; }  // variants B/C/D off the state-once schedule
bool haloKernels() { return std::getenv("BDG_SW2D_HALO_KERNELS") != nullptr; }         // separate pack / unpack kernels
bool stripThroughput() { return std::getenv("BDG_SW2D_STRIP_THROUGHPUT") != nullptr; } // (its boundary strips have no SYNC instance)
// ="6": the boundary strip of N >= 5 on the two-waves schedule. Two read times, both kept: flagSyncUsable asks per call,
// launchBoundaryStageFolded keeps the answer of its first launch for the rest of the process
const char* haloVariant() { return std::getenv("BDG_SW2D_HALO_VARIANT"); }
} // namespace env
} // namespace

struct bdg_sw2d {
    const bdg_dev::KernelTable* kt = nullptr;
    int N = 0, Np = 0, Nfp = 0, NFN = 0, K = 0, device = 0;
    long long ld = 0;
    double g = 9.81;
    bool hasFilter = false, hasH = false;
    hipStream_t stream = nullptr;
    size_t bytes = 0;
    DevBuf<double> qA, qB, res, aux, geo, fgeo, ops, Hbuf, stage, partials, red2;
    DevBuf<double> ageo, opsAffine, opsAffineFiltered; // affine-geometry fast path
    DevBuf<double> opsMfma, opsMfmaFiltered;           // same operators in MFMA A-operand layout
    DevBuf<double> opsMfma2, opsMfma2Filtered;         // ... with the lift tiles padded per face
    DevBuf<double> opsMfma2Src, opsMfma2SrcFiltered;   // ... followed by the source-term tiles F' (variants C/D, N >= 6)
    DevBuf<double> opsMfma2NodalFilter; // plain MfmaOps2 image + MT*KV Filter tiles
    bool mfmaSources = false;
    bool affine = false;
    bool nodalMfma = false;   // non-affine tables: matrix-core kernel (default) instead of the N <= 6 vector kernel
    bool fastSources = false; // variants B/C/D on the unrolled kernels instead of the rolled ones
    // up to this order the unrolled source-term kernels are used, above it the matrix-core ones
    static constexpr int kUnrolledSourcesMaxOrder = 4;
    DevBuf<double> filterT;   // [m][i] = Filter[i][m], for filtered source terms
    // variant D (reference swhelpers/rhs.py:178-311): optional tracer field and source terms
    int nf = 3;
    bool variantD = false;
    bdg_dev::VdParams vd{};
    DevBuf<double> zxBuf, zyBuf, fcorBuf, opsVd, opsVdFiltered;
    DevBuf<double> opsVn, filterRows, vnRaw; // variants B / C / D on per-node geometry (sw2d_vn_kernel.hpp)
    // variant B (reference src/sw2d/main.cpp:279-484): depth + star states, open boundary, global LF speed, sources
    bool variantB = false;
    bdg_dev::VbParams vb{};
    DevBuf<double> HxBuf, HyBuf, spongeBuf, lamBuf, vbPartials;
    DevBuf<double> outM; // (Np, Np) lattice interpolation of the output step
    DevBuf<int> obcBuf;
    double tideAmp = 0.0, tidePeriod = 1.0, tideRamp = 0.0;
    double timeNow = 0.0;  // model time of the resident state (tide phase)
    bool lamExternal = false; // variant B, partitioned: lamBuf holds the all-rank speed of the state about to be evaluated
    // variant B with the tracer (bdg_sw2d_enable_variant_b4): the tracer pass of sw2d_vb_tracer_kernel.hpp behind every three-field
    // variant-B launch, and the concentration the open boundary feeds (a scalar, or a table per open-boundary node in device slots)
    bool variantB4 = false;
    bool evaluated = false; // a stage kernel or a speed pass has been launched
    const bdg_dev::Vb4KernelTable* kt4 = nullptr;
    bdg_dev::VbTracerParams vb4{};
    DevBuf<int> openBase;
    DevBuf<double> openN, opsRow, opsRowFiltered; // VnOps images of the tracer pass's general form (straight-sided elements)
    // tracer diffusion, sources and decay (bdg_sw2d_enable_tracer_diffusion): the passes of sw2d_diffusion_kernel.hpp behind the
    // last launch of every evaluation. difOps / difOpsFiltered: VnOps images (the second on straight-sided elements with a Filter),
    // difFilter: the Filter's rows, difScratch: the flux planes fx, fy and, with a Filter, the plane of the unfiltered term
    bool diffusion = false;
    const bdg_dev::DiffusionKernelTable* ktd = nullptr;
    bdg_dev::DiffusionParams dif{};
    DevBuf<double> difKappa, difSource, difScratch, difOps, difOpsFiltered, difFilter;
    double difDt = 0.0;                // c / (max kappa (N+1)^4 max(Fscale)^2), kDiffusionDtConstant below
    // dt_diff <= 2 / rho(operator) at every order with this constant: the smallest bound measured is 4.30 (N = 1)
    static constexpr double kDiffusionDtConstant = 4.0;
    // eddy viscosity (bdg_sw2d_enable_viscosity): the passes of sw2d_viscosity_kernel.hpp behind the last launch of every evaluation
    // (behind the tracer's diffusion where both are on). visOps / visOpsFiltered: VnOps images (the second on straight-sided
    // elements with a Filter), visFilter: the Filter's rows (per-node geometry), visScratch: the four flux planes, the plane of nu
    // and, per-node geometry with a Filter, the two planes of the unfiltered terms; visRed: partials and result of max nu
    bool viscosity = false;
    const bdg_dev::ViscosityKernelTable* ktv = nullptr;
    bdg_dev::ViscosityParams vis{};
    DevBuf<double> visNu0, visScratch, visOps, visOpsFiltered, visFilter, visRed;
    double* visNuPlane = nullptr;
    bool visSmagorinsky = false;
    double visNu0Max = 0.0;            // max nu0, on the host at set-up
    double visDtScale = 0.0;           // c / ((N+1)^4 max(Fscale)^2): dt_visc = visDtScale / max nu
    // dt_visc <= 2 / rho(operator) at every order with this constant, nu a nodal field (tests/test_triviscosity_reference.py,
    // DESIGN.md 3.7)
    static constexpr double kViscosityDtConstant = 4.0;
    DevBuf<double> lamPair;            // two accumulators for the fused next-evaluation speed (alternating)
    int lamSlot = 0;
    // Direction of the tile sweep of whole-mesh stage launches (StageParams::sweepBack, sw2d_stage_tile.hpp): it alternates from
    // one launch to the next, so that a launch starts on the tiles the launch before it touched last, whose rows are still in
    // the Infinity Cache. BDG_SW2D_SWEEP=forward, read at creation: always forward.
    bool sweepAlternates = true;
    unsigned long long sweepLaunches = 0, backwardLaunches = 0;
    // the next whole-mesh launch's direction into p; partitioned launches (wholeMesh = false) keep 0
    void nextSweep(bdg_dev::StageParams& p, bool wholeMesh) {
        p.sweepBack = (wholeMesh && sweepAlternates) ? static_cast<int>(sweepLaunches++ & 1ull) : 0;
        backwardLaunches += static_cast<unsigned long long>(p.sweepBack);
    }
    const double* lamStateFor = nullptr; // state buffer the accumulated speed belongs to (nullptr: none)
    double lamTideFor = 0.0;
    double nextEvalTime = 0.0;         // model time of the evaluation that will follow the current launch
    // kept for operator images built after creation; the last three are Filter * (Dr, Ds, Lift): the filtered RHS of an affine
    // element is linear in these (empty without a Filter)
    std::vector<double> hostDr, hostDs, hostLift, hostFilter, hostFDr, hostFDs, hostFLift;
    using AffineVariant = bdg_dev::AffineVariant;
    AffineVariant affineVariant = AffineVariant::Unrolled; // kernel family of the straight three-field stage (sw2d_launch.hpp)
    bool variantForced = false;                 // BDG_SW2D_AFFINE_VARIANT given
    // elements below which the matrix-core kernel is the faster one, per order (measured crossovers:
    // N=2 near 10 k, N=3 near 125 k, N=4 between 125 k and 250 k; N=1 never ahead; N=5 runs on
    // the matrix cores at every size)
    // (round 4, after the matrix-core kernel of N <= 4 got all its requests ahead of its first product -- kernel ms, unrolled / matrix cores,
    // profiles/r04_rehearsal_experiments.txt: N=4 125 k elements 0.0543 / 0.0452, 250 k 0.1009 / 0.1142; N=3 125 k 0.0365 / 0.0313, 250 k 0.0612 /
    // 0.0704; N=2 125 k 0.0189 / 0.0283: N=3's crossover moves up to where N=4's is)
    static constexpr int kSmallLaunch[6] = {0, 4000, 10000, 160000, 160000, 0};
    // resident-workgroup kernels, interior launch of a partitioned run: CUs left to the boundary kernel (a strip of a few
    // hundred elements = 4..8 four-wave workgroups); N=8, 8-way rehearsal: 0.087 -> see profiles/r02_rehearsal.txt
    static constexpr int kInteriorGridCap = 244;
    DevBuf<int> vmapP, perm, istage, sendSlots, haloSendOf;
    // (3, ld) face links (bdg_dev::FaceLink) of the LSERK stages on the unrolled kernel; empty when the switch
    // BDG_SW2D_FULL_STAGE_TRAFFIC is set, when that kernel does not serve the solver, or when a face's vmapP rows are not
    // a neighbour face (or the face itself) in Fmask order
    DevBuf<int> faceLink;
    bool haloFusable = false;  // every sent element is a partition-boundary element with at most three records
    int numInterior = 0, numOwned = 0, numSend = 0; // element partition: [interior | boundary | ghost]
    // native halo exchange (RCCL over xGMI): one send and one receive range per neighbour rank
    bdg_halo::Transport halo;
    hipEvent_t evA[2] = {nullptr, nullptr}, evB[2] = {nullptr, nullptr};
    hipEvent_t evPacked[2] = {nullptr, nullptr}, evCopied[2] = {nullptr, nullptr}; // in-process group transport
    bool localGroup = false;
    // In-kernel dependencies between the two chains of an exchanged stage (round 4): two device counters --
    // [0] ring tiles of interior launches finished, [1] workgroups of boundary launches finished, [2] a word a bounded wait
    // sets when it gives up -- and what the host expects them to reach after the launches issued so far
    DevBuf<unsigned long long> syncBuf;
    unsigned long long expectRing = 0, expectStrip = 0;
    int ringBegin = 0;   // first interior element that has a partition-boundary neighbour (elements are ordered [deep | ring | boundary | ghost]
                         // by halo.build_plan; any other order only makes more tiles wait)
    double* fscaleNodal = nullptr; // (NFN, ld) per-node Fscale plane (time-step reduction)
    double* qcur = nullptr;  // current state
    double* qalt = nullptr;  // the other buffer
    long long stageCount = 0; // LSERK stage counter (stage index = count % 5)
    double dtStage = 0.0;
    std::vector<int> permHost; // caller element -> device slot (empty = identity)
    // run monitor (bdg_sw2d_enable_monitor): sw2d_monitor_kernel.hpp
    struct Monitor : bdg_records::MonitorState {
        DevBuf<double> row;     // (numGauges, Np): the nodal basis at each gauge
        DevBuf<double> scratch; // the record bdg_sw2d_monitor_time writes
    } mon;
    // drifters (bdg_sw2d_enable_drifters): sw2d_drifter_kernel.hpp; elements and neighbours in device slots
    struct Drifters : bdg_records::DrifterState {
        DevBuf<double> vert, vinvT, jac;
        std::vector<int> callerOf; // device slot -> caller element (empty = identity)
    } drf;
    // field statistics (bdg_sw2d_enable_field_stats): sw2d_stats_kernel.hpp
    bdg_records::FieldStatsState fst;
    bool partitionSet = false; // bdg_sw2d_set_partition has been called

    ~bdg_sw2d() {
        for (hipEvent_t e : {evA[0], evA[1], evB[0], evB[1], evPacked[0], evPacked[1], evCopied[0], evCopied[1]})
            if (e) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
    }

    void use() const { hipCheck(hipSetDevice(device), "hipSetDevice"); }
    size_t planeSize() const { return static_cast<size_t>(Np) * static_cast<size_t>(ld); }
    const int* permDev() const { return perm.p; }

    // host (rows, K) caller order <-> device planes (padded / renumbered): row_transfer.hpp
    bdg_dev::RowLayout rowLayout() const { return {K, ld, permDev(), stream}; }
    void uploadRows(const double* host, double* dev, int rows) { bdg_dev::uploadRows(rowLayout(), host, dev, stage.p, rows); }
    void downloadRows(const double* dev, double* host, int rows) { bdg_dev::downloadRows(rowLayout(), dev, host, stage.p, rows); }
    // one (Np, K) host array per field, to / from the nf consecutive device planes at `dev`
    void uploadFields(const double* const* host, double* dev) {
        for (int c = 0; c < nf; ++c) uploadRows(host[c], dev + c * planeSize(), Np);
    }
    void downloadFields(const double* dev, double* const* host) {
        for (int c = 0; c < nf; ++c) downloadRows(dev + c * planeSize(), host[c], Np);
    }
    const double* uploadPlane(const double* host, DevBuf<double>& buf) {
        if (!host) return nullptr;
        if (!buf.p) buf.alloc(planeSize(), bytes);
        hipCheck(hipMemsetAsync(buf.p, 0, buf.n * sizeof(double), stream), "hipMemset");
        uploadRows(host, buf.p, Np);
        return buf.p;
    }

    // ---- the field calls (bdg_sw2d_set_state / _get_state / _rhs and their four-field twins), nf fields each
    void setFields(const double* const* f) {
        uploadFields(f, qcur);
        hipCheck(hipMemsetAsync(res.p, 0, res.n * sizeof(double), stream), "hipMemset");
        stageCount = 0;
        mon.steps = 0;
        fst.steps = 0;
        lamStateFor = nullptr; // a speed accumulated for the previous contents of this buffer is void
        drifterResample();
        hipCheck(hipStreamSynchronize(stream), "set_state sync");
    }
    void getFields(double* const* f) {
        downloadFields(qcur, f);
        checkSyncError();
    }
    void rhsFields(const double* const* in, double* const* out, bool filter) {
        uploadFields(in, qalt); // the inactive state buffer is scratch between steps
        launchRhs(qalt, aux.p, filter);
        downloadFields(aux.p, out);
    }
    // the (Np, Np) lattice interpolation of an output call, staged for the launches that follow on the stream (nullptr: none)
    const double* stageOutputMatrix(const double* IM) {
        if (!IM) return nullptr;
        if (!outM.p) outM.alloc(static_cast<size_t>(Np) * Np, bytes);
        hipCheck(hipMemcpyAsync(outM.p, IM, outM.n * sizeof(double), hipMemcpyHostToDevice, stream), "H2D copy");
        return outM.p;
    }

    bdg_dev::StageParams baseParams() const {
        bdg_dev::StageParams p{};
        p.geo = geo.p;
        p.fgeo = fgeo.p;
        p.vmapP = vmapP.p;
        p.ops = ops.p;
        p.ageo = ageo.p;
        p.opsAffine = opsAffine.p;
        p.ld = ld;
        p.kbegin = 0;
        p.kend = numOwned;
        p.g = g;
        p.one = 1.0;
        return p;
    }

    // :352  hP = HM + amp cos(om t) 1/2 (tanh(ramp (t - T)) + 1)
    double tideAt(double t) const {
        const double om = 2.0 * M_PI / tidePeriod;
        return tideAmp * std::cos(om * t) * 0.5 * (std::tanh(tideRamp * (t - tidePeriod)) + 1);
    }
    // variant B's surface term and sources for the matrix-core source kernels (src/sw2d/main.cpp:461-478), at the tide in vb.tide
    bdg_dev::PhysParams physB() const {
        bdg_dev::PhysParams ph{};
        ph.sx = vb.Hx; ph.sy = vb.Hy; ph.fconst = vb.fcor; ph.cd = vb.cd;
        ph.slope = 1.0; ph.dragSign = -1.0;
        ph.H = vb.H; ph.obc = vb.obc; ph.lam = lamBuf.p; ph.spongeField = vb.sponge; ph.tide = vb.tide;
        return ph;
    }
    // variants C / D: the sources of swhelpers/rhs.py:300-309, if the solver has any
    bdg_dev::PhysParams physD() const {
        bdg_dev::PhysParams ph{};
        if (vd.sources) {
            ph.sx = vd.zx; ph.sy = vd.zy; ph.fcor = vd.fcor;
            ph.fconst = vd.fconst; ph.cd = vd.cd;
            ph.slope = -1.0; ph.dragSign = 1.0;
        }
        return ph;
    }
    // variant B's stage kernel on the state-once schedule where it exists (sw2d_mfma3src_kernel.hpp, PHYS = 2);
    // BDG_SW2D_SOURCES_TWO_WAVE=1 keeps the two-waves-per-SIMD kernel
    bool variantBStateOnce() const { return kt->mfma3SrcFields >= 3 && !env::sourcesTwoWave() && fitsOneDescriptor(3); }
    // unfiltered evaluation on a state-once kernel with sources: F' is the identity, the sources are added pointwise (IDF instance;
    // BDG_SW2D_SOURCES_PRODUCT=1 keeps the products with the identity tiles for A/B runs and cross-checks -- bit-identical)
    static bool srcIdentity(bool filter) { return !filter && !env::sourcesProduct(); }
    // the state-once kernels address an array of `fields` planes through ONE buffer descriptor
    bool fitsOneDescriptor(int fields) const { return bdg_dev::fitsOneDescriptor(fields, Np, ld); }
    // ... and at N >= 5 the strip kernel's workgroups (one 16-element tile each, three waves; two fit a CU, none fits beside an
    // interior workgroup's 120 KB of LDS) need free CUs, or the strip -- which sits on the exchange chain -- runs in many rounds.
    // Round 3 left one CU per strip tile (cap 218-232). Round 4, with the chains meeting inside the kernels, swept the cap in
    // the 8-way rehearsal (profiles/r04_rehearsal_experiments.txt; ms per stage): N=5 244: 0.0580, 250: 0.0521; N=6 244: 0.0486,
    // 248: 0.0464, 252: 0.0584 (four free CUs: the strip's 32 tiles take four rounds); N=7 240: 0.0473, 246: 0.0401, 250: 0.0400;
    // N=8 238: 0.0606 (1930 tiles are three rounds of a tile per wave on 952 waves, two on 968 and more), 242: 0.0546,
    // 244: 0.0540, 246: 0.0542. The interior wants every CU it can get; the strip needs about a round's worth of slots for its
    // tiles and RCCL's kernel a CU: eight free CUs, twelve at N = 8 (its strip tiles carry three row blocks).
    // BDG_SW2D_INTERIOR_CAP=n pins the cap.
    int interiorGridCap() const {
        if (env::interiorCapPinned() > 0) return env::interiorCapPinned();
        if (N < 5) return kInteriorGridCap;
        return N >= 8 ? 244 : 248;
    }

    // One fused pass. The affine path takes the filter through pre-multiplied operators.
    // `on`: stream to launch on (default: the compute stream).
    // `wholeMesh`: every kernel launched here takes the next direction of the alternating tile sweep (nextSweep). False for the
    // two launches of a partitioned stage: the interior launch orders its ring tiles last because they wait in the kernel for
    // the previous boundary launch -- walked backwards, the waiting tiles would come first and hold their CUs.
    void launchStage(int mode, bool filter, bdg_dev::StageParams& p, const char* what, hipStream_t on = nullptr, bool wholeMesh = true) {
        if (filter && !hasFilter) throw arg_error("filter requested but the solver was created without a Filter matrix");
        hipStream_t st = on ? on : stream;
        auto sweep = [&] { nextSweep(p, wholeMesh); };
        evaluated = true;
        // Eddy viscosity and the Heun step's sponge: q1 = sponge(q + dt (R + T)), and T cannot be added behind a store that has
        // divided already. The stage launches run with the sponge off (a coefficient of 0 divides by exactly 1, or takes the
        // instance without the division) and the viscosity's update divides planes 1 and 2 after adding T.
        struct SpongeHandOver {
            bdg_dev::StageParams& p;
            bdg_dev::VbParams& vb;
            double scalar;
            const double* field;
            bool on;
            ~SpongeHandOver() {
                if (on) { p.sponge = scalar; vb.sponge = field; }
            }
        } handOver{p, vb, p.sponge, vb.sponge, viscosity && mode == bdg_dev::MODE_COMBINE};
        if (handOver.on) {
            vis.sponge = p.sponge;
            vis.spongeField = variantB ? vb.sponge : nullptr;
            p.sponge = 0.0;
            vb.sponge = nullptr;
        }
        // Small launches (a rank's share of a many-way split, its partition-boundary strip) are bound by
        // the latency of one wavefront, not by HBM: the matrix-core kernel gives each wave 16 elements
        // instead of 64 (measured at N=4: 750 elements 7 us vs 19 us; 125 k elements 48 us vs 56 us;
        // 250 k elements 136 us vs 109 us -- DESIGN.md section 4).
        AffineVariant variant = affineVariant;
        // BDG_SW2D_SMALL_LAUNCH=n pins the crossover (A/B runs; the partition-boundary strip keeps the table's value: halosFold)
        const int smallPinned = env::smallLaunchPinned();
        const int smallLaunch = (smallPinned >= 0 && p.kbegin == 0) ? smallPinned : kSmallLaunch[N];
        if (!variantForced && affine && N <= 5 && p.kend - p.kbegin < smallLaunch) variant = AffineVariant::Mfma;
        if (p.syncSignal && !(affine && !variantB && !variantD && (variant == AffineVariant::Mfma || variant == AffineVariant::Mfma3)))
            throw std::logic_error("in-kernel stage dependencies were requested for a launch whose kernel has no SYNC instance");
        if (!affine && (variantB || variantD)) {
            // per-node geometry tables: the general (rolled) form of variants B / C / D
            buildNodalVariantOps();
            const double* filt = filter ? filterRows.p : nullptr;
            if (variantB) {
                vb.tide = tideAt(timeNow);
                vb.lam = lamBuf.p;
                vb.lamNext = nullptr;
                lamStateFor = nullptr;
                hipCheck(kt->stageVn(mode, true, p, vd, vb, opsVn.p, filt, vnRaw.p, vbPartials.p, lamBuf.p, !lamExternal, st), what);
                if (variantB4) launchTracerB(mode, filter, p, what, st);
            } else {
                bdg_dev::VdParams v = vd;
                v.cbase = 0;
                hipCheck(kt->stageVn(mode, false, p, v, vb, opsVn.p, filt, vnRaw.p, nullptr, nullptr, false, st), what);
            }
        } else if (variantB) {
            using bdg_dev::SrcForm;
            using bdg_dev::VbStage;
            vb.tide = tideAt(timeNow);
            // Where the global speed of this state comes from. Reduced: over all ranks of a partitioned run, into lamBuf
            // beforehand (globalSpeedOf). Reused: the unrolled kernel also reduces the speed of the state it writes (for the tide
            // value the next evaluation is expected to see); a launch that reads exactly that state at exactly that tide over
            // the whole mesh finds it in lamPair. OwnPass: a speed pass into lamBuf in front of the stage kernel.
            enum class Speed { Reduced, Reused, OwnPass };
            const bool whole = p.kbegin == 0 && p.kend == numOwned;
            const bool reusable = fastSources && whole && lamStateFor == p.qin && lamTideFor == vb.tide && !env::speedPass();
            const Speed speed = lamExternal ? Speed::Reduced : (reusable ? Speed::Reused : Speed::OwnPass);
            const bool ownPass = speed == Speed::OwnPass;
            const int cur = lamSlot, nxt = lamSlot ^ 1;
            vb.lam = speed == Speed::Reused ? lamPair.p + cur : lamBuf.p;
            vb.lamNext = nullptr;
            lamStateFor = nullptr;
            if (fastSources && !lamExternal && whole && mode != bdg_dev::MODE_RHS) { // ... and this launch leaves the next one its speed
                hipCheck(hipMemsetAsync(lamPair.p + nxt, 0, sizeof(double), st), "hipMemset");
                vb.lamNext = reinterpret_cast<unsigned long long*>(lamPair.p + nxt);
                vb.tideNext = tideAt(nextEvalTime);
                lamStateFor = p.qout;
                lamTideFor = vb.tideNext;
                lamSlot = nxt;
            }
            // the speed pass is a launch of its own over the same elements: it takes a direction, the stage kernel the other
            if (ownPass) {
                sweep();
                hipCheck(kt->stageVb(mode, p, vb, vbPartials.p, lamBuf.p, true, VbStage::None, nullptr, st), what);
            }
            sweep();
            if (fastSources) {
                p.opsAffine = opsAffine.p;
                hipCheck(kt->stageVb(mode, p, vb, vbPartials.p, lamBuf.p, false, VbStage::Unrolled, filter ? filterT.p : nullptr, st), what);
            } else if (mfmaSources) {
                // N >= 5: the matrix-core kernel with variant B's surface term and sources
                p.opsAffine = filter ? opsMfma2SrcFiltered.p : opsMfma2Src.p;
                hipCheck(kt->stageMfma2Src(mode, p, physB(), variantBStateOnce() ? SrcForm::OnceVariantB : SrcForm::VariantB, srcIdentity(filter), st), what);
            } else {
                p.opsAffine = filter ? opsVdFiltered.p : opsVd.p;
                hipCheck(kt->stageVb(mode, p, vb, vbPartials.p, lamBuf.p, false, VbStage::Rolled, nullptr, st), what);
            }
            if (variantB4) { // the tracer pass walks the tiles against the launch before it, as every whole-mesh launch does
                sweep();
                launchTracerB(mode, filter, p, what, st);
            }
        } else if (variantD && fastSources) {
            // three conserved fields on the unrolled kernel with the sources folded in, the tracer (if
            // any) by its own one-field-per-wave launch reading the same input state
            bdg_dev::PhysParams ph = physD();
            // filtered RHS: plain operators, Filter applied to flux terms + sources at the end
            ph.fmat = filter ? filterT.p : nullptr;
            p.opsAffine = opsAffine.p;
            sweep();
            if (nf == 4 && !env::tracerPass()) {
                hipCheck(kt->stageAffineSrc(mode, p, ph, true, st), what);    // the tracer rides in the same pass
            } else {
                hipCheck(kt->stageAffineSrc(mode, p, ph, false, st), what);
                if (nf == 4) { // own pass; the tracer has no sources: pre-filtered operators as in variant A
                    p.opsAffine = filter ? opsAffineFiltered.p : opsAffine.p;
                    sweep();
                    hipCheck(kt->stageTracer(mode, p, st), what);
                }
            }
        } else if (variantD && mfmaSources) {
            // N >= 6: three conserved fields with sources on the matrix cores, then the tracer pass
            using bdg_dev::SrcForm;
            const bdg_dev::PhysParams ph = physD();
            const bool identity = srcIdentity(filter);
            p.opsAffine = filter ? opsMfma2SrcFiltered.p : opsMfma2Src.p;
            // state-once schedule where it exists (sw2d_mfma3src_kernel.hpp: N = 5, 6, 7 with and without the tracer, N = 8 three fields;
            // BDG_SW2D_SOURCES_TWO_WAVE=1 keeps the two-waves-per-SIMD kernels below for A/B runs and cross-checks)
            const bool stateOnceSrc = !env::sourcesTwoWave();
            sweep();
            if (stateOnceSrc && kt->mfma3SrcFields >= nf && !env::tracerPass() && fitsOneDescriptor(nf)) {
                hipCheck(kt->stageMfma2Src(mode, p, ph, nf == 4 ? SrcForm::OnceSourcesTracer : SrcForm::OnceSources, identity, st), what);
            } else if (stateOnceSrc && kt->mfma3TracerPhase && nf == 4 && !env::tracerPass() && fitsOneDescriptor(4)) {
                // N = 8: the tracer equation as a second phase of every tile, from the state tile still in LDS (one launch, state read once)
                hipCheck(kt->stageMfma2Src(mode, p, ph, SrcForm::OnceTracerPhase, identity, st), what);
            } else if (stateOnceSrc && kt->mfma3SrcFields == 3 && nf == 4 && fitsOneDescriptor(3)) {
                // N = 8: three conserved fields with sources on the state-once schedule, the tracer in its own pass
                hipCheck(kt->stageMfma2Src(mode, p, ph, SrcForm::OnceSources, identity, st), what);
                p.opsAffine = filter ? opsMfma2Filtered.p : opsMfma2.p;
                sweep();
                hipCheck(kt->stageMfma2Src(mode, p, ph, SrcForm::TracerPass, false, st), what);
            } else if (nf == 4 && kt->mfmaMT <= 2 && !env::tracerPass()) {
                hipCheck(kt->stageMfma2Src(mode, p, ph, SrcForm::SourcesTracer, false, st), what); // N <= 6: the tracer rides in the same pass
            } else {
                hipCheck(kt->stageMfma2Src(mode, p, ph, SrcForm::Sources, false, st), what);
                if (nf == 4) {
                    p.opsAffine = filter ? opsMfma2Filtered.p : opsMfma2.p;
                    sweep();
                    hipCheck(kt->stageMfma2Src(mode, p, ph, SrcForm::TracerPass, false, st), what);
                }
            }
        } else if (variantD) {
            p.opsAffine = filter ? opsVdFiltered.p : opsVd.p;
            sweep();
            hipCheck(kt->stageVd(mode, p, vd, st), what);
        } else if (affine && variant == AffineVariant::Mfma) {
            p.opsAffine = filter ? opsMfmaFiltered.p : opsMfma.p;
            sweep();
            hipCheck(kt->stageMfma(mode, p, st), what);
        } else if (affine && variant == AffineVariant::Mfma3) {
            p.opsAffine = filter ? opsMfma2Filtered.p : opsMfma2.p;
            sweep();
            hipCheck(kt->stageMfma3(mode, p, st), what);
        } else if (affine && variant == AffineVariant::Mfma2) {
            p.opsAffine = filter ? opsMfma2Filtered.p : opsMfma2.p;
            sweep();
            hipCheck(kt->stageMfma2(mode, p, st), what);
        } else if (affine) {
            p.opsAffine = filter ? opsAffineFiltered.p : opsAffine.p;
            sweep();
            hipCheck(kt->stageAffine(mode, variant, p, st), what);
        } else if (nodalMfma) {
            // per-node geometry on the matrix cores (state-once schedule), every order
            p.opsAffine = filter ? opsMfma2NodalFilter.p : opsMfma2.p;
            sweep();
            hipCheck(kt->stageMfma3Nodal(mode, filter, p, st), what);
        } else {
            sweep();
            hipCheck(kt->stage(mode, filter, p, st), what);
        }
        if (diffusion) launchDiffusion(mode, filter, p, sweep, st);
        if (viscosity) launchViscosity(mode, filter, p, sweep, st);
    }

    // The tracer's diffusion, source and decay of the evaluation whose launches were just issued on `st`: T of p.qin -- which
    // those launches read and did not write -- added to plane 3 of what they wrote. Each launch takes the next direction of the
    // alternating sweep. A filtered evaluation: pre-filtered rows where T is linear in the fluxes and the metric is one per
    // element; else the unfiltered T into a scratch plane and the Filter's rows over all of it in a third launch.
    template <class Sweep>
    void launchDiffusion(int mode, bool filter, bdg_dev::StageParams& p, Sweep&& sweep, hipStream_t st) {
        const bool nodal = !affine;
        // what the scheme rests on: the evaluation's own launches have not written the state they read
        if (mode == bdg_dev::MODE_RHS ? p.qin == p.rhs : (p.qin == p.qout || p.qin == p.res))
            throw std::logic_error("tracer diffusion: the stage's input state is one of its output buffers");
        sweep();
        hipCheck(ktd->gradient(nodal, p, dif, difOps.p, st), "sw2d_tracer_gradient_kernel");
        sweep();
        const char* what = "sw2d_tracer_diffusion_kernel";
        if (!filter) {
            hipCheck(ktd->divergence(mode, nodal, false, p, dif, difOps.p, st), what);
        } else if (!nodal && !dif.source && dif.decay == 0.0) {
            hipCheck(ktd->divergence(mode, false, false, p, dif, difOpsFiltered.p, st), what);
        } else {
            hipCheck(ktd->divergence(mode, nodal, true, p, dif, difOps.p, st), what);
            sweep();
            hipCheck(ktd->filter(mode, p, dif, difFilter.p, st), "sw2d_tracer_diffusion_filter_kernel");
        }
    }

    // The eddy viscosity's terms of the evaluation whose launches were just issued on `st`: T_u, T_v of p.qin -- which those
    // launches read and did not write -- added to planes 1 and 2 of what they wrote, then (a Heun stage) the sponge division the
    // stage launch left out. Each launch takes the next direction of the alternating sweep. A filtered evaluation: pre-filtered
    // rows on straight-sided elements (T is linear in the fluxes); per-node geometry: the unfiltered terms into two scratch
    // planes and the Filter's rows over them in a third launch.
    template <class Sweep>
    void launchViscosity(int mode, bool filter, bdg_dev::StageParams& p, Sweep&& sweep, hipStream_t st) {
        const bool nodal = !affine;
        if (mode == bdg_dev::MODE_RHS ? p.qin == p.rhs : (p.qin == p.qout || p.qin == p.res))
            throw std::logic_error("eddy viscosity: the stage's input state is one of its output buffers");
        bdg_dev::ViscosityParams v = vis;
        v.nuOut = nullptr;
        if (mode != bdg_dev::MODE_COMBINE) { v.sponge = 0.0; v.spongeField = nullptr; }
        sweep();
        hipCheck(ktv->gradient(nodal, p, v, visOps.p, st), "sw2d_viscosity_gradient_kernel");
        sweep();
        const char* what = "sw2d_viscosity_divergence_kernel";
        if (!filter) {
            hipCheck(ktv->divergence(mode, nodal, false, p, v, visOps.p, st), what);
        } else if (!nodal) {
            hipCheck(ktv->divergence(mode, false, false, p, v, visOpsFiltered.p, st), what);
        } else {
            hipCheck(ktv->divergence(mode, true, true, p, v, visOps.p, st), what);
            sweep();
            hipCheck(ktv->filter(mode, p, v, visFilter.p, st), "sw2d_viscosity_filter_kernel");
        }
        // variant B's unrolled stage kernel reduced the speed of the state it wrote for the next evaluation: that state's momentum
        // has changed since, so the next evaluation runs its own speed pass
        if (mode != bdg_dev::MODE_RHS) lamStateFor = nullptr;
    }
    // nu of the resident state into visNuPlane: the first pass alone (its fluxes are scratch between evaluations)
    void launchEddyViscosity() {
        bdg_dev::StageParams p = baseParams();
        p.qin = qcur;
        nextSweep(p, true);
        bdg_dev::ViscosityParams v = vis;
        v.nuOut = visNuPlane;
        hipCheck(ktv->gradient(!affine, p, v, visOps.p, stream), "sw2d_viscosity_gradient_kernel");
    }
    // dt_visc = c / (max nu (N+1)^4 max(Fscale)^2), max nu of the resident state (Smagorinsky: a launch and a fixed-order reduction)
    double viscosityDt() {
        double numax = visNu0Max;
        if (visSmagorinsky) {
            launchEddyViscosity();
            hipCheck(ktv->maxOf(visNuPlane, static_cast<long long>(planeSize()), visRed.p, visRed.p + bdg_dev::kViscosityMaxBlocks, stream),
                     "sw2d_viscosity_max_kernel");
            hipCheck(hipMemcpyAsync(&numax, visRed.p + bdg_dev::kViscosityMaxBlocks, sizeof(double), hipMemcpyDeviceToHost, stream), "D2H copy");
            hipCheck(hipStreamSynchronize(stream), "sync");
        }
        return numax > 0.0 ? visDtScale / numax : std::numeric_limits<double>::infinity();
    }
    // max |Fscale| over the mesh, from the plane the time-step reduction reads (padding columns are zero)
    double maxFscale() {
        std::vector<double> fs(static_cast<size_t>(NFN) * ld);
        hipCheck(hipMemcpyAsync(fs.data(), fscaleNodal, fs.size() * sizeof(double), hipMemcpyDeviceToHost, stream), "D2H copy");
        hipCheck(hipStreamSynchronize(stream), "sync");
        double fmax = 0.0;
        for (double v : fs) fmax = std::max(fmax, std::fabs(v));
        return fmax;
    }

    // Variant B with the tracer: plane 3 of the evaluation whose three-field launch(es) were just issued on `st` -- same input
    // state, same tide (vb.tide) and the speed that launch read (vb.lam; the speed it leaves for the next evaluation is in the
    // other accumulator). The tracer has no source: the filter rides in the operators on straight-sided elements.
    void launchTracerB(int mode, bool filter, bdg_dev::StageParams& p, const char* what, hipStream_t st) {
        if (!affine) {
            hipCheck(kt4->tracerGeneral(mode, true, p, vb, vb4, opsVn.p, filter ? filterRows.p : nullptr, vnRaw.p, st), what);
        } else if (fastSources && kt4->unrolled) {
            p.opsAffine = filter ? opsAffineFiltered.p : opsAffine.p;
            hipCheck(kt4->tracerUnrolled(mode, p, vb, vb4, st), what);
        } else {
            hipCheck(kt4->tracerGeneral(mode, false, p, vb, vb4, filter ? opsRowFiltered.p : opsRow.p, nullptr, nullptr, st), what);
        }
    }

    void launchRhs(const double* qin, double* out, bool filter) {
        bdg_dev::StageParams p = baseParams();
        p.qin = qin;
        p.rhs = out;
        launchStage(bdg_dev::MODE_RHS, filter, p, "sw2d stage kernel <RHS>");
    }

    // ---- one LSERK4 stage. What its two launches (launchLserkStage, launchBoundaryStageFolded) share: the stage index (returned),
    // buffers and coefficients of the stage, and `done` -- an event to record when the launch has finished -- through the launch
    // itself where its helper can (one packet on the queue instead of two; *recorded says whether it did)
    int lserkStageParams(bdg_dev::StageParams& p, hipEvent_t done, bool* recorded) const {
        const int s = static_cast<int>(stageCount % blitzdg::LSERK4::numStages);
        const bool extLaunch = env::extLaunch();
        if (done && extLaunch) { p.stopEvent = done; p.stopEventUsed = recorded; }
        p.qin = qcur;
        p.qout = qalt;
        p.res = res.p;
        p.ca = blitzdg::LSERK4::rk4a[s];
        p.cb = blitzdg::LSERK4::rk4b[s];
        p.cc = dtStage;
        return s;
    }
    // ... and what follows them: the buffers swap roles; model time (the tide phase of variant B) is frozen over the five
    // stages and moves on after the last
    void lserkStageAdvance(int s) {
        std::swap(qcur, qalt);
        ++stageCount;
        if (s == blitzdg::LSERK4::numStages - 1) timeNow += dtStage;
    }
    // part: 0 = interior elements only (no ghost dependency; state not advanced),
    //       1 = partition-boundary elements, then advance; 2 = all owned elements, then advance.
    void launchLserkStage(int part = 2, hipStream_t on = nullptr, bool advance = true, hipEvent_t done = nullptr, bool flagSync = false) {
        bdg_dev::StageParams p = baseParams();
        bool recorded = false;
        unsigned signals = 0;
        if (flagSync && part == 0) { // ring tiles wait for every boundary launch issued so far and signal for themselves
            p.syncWait = syncBuf.p + 1; p.syncWaitValue = expectStrip;
            p.syncSignal = syncBuf.p; p.syncError = reinterpret_cast<unsigned int*>(syncBuf.p + 2);
            p.syncFirstTile = ringBegin / 16;
            p.syncSignalsOut = &signals;
        }
        const int s = lserkStageParams(p, done, &recorded);
        if (part == 0) {
            p.kend = numInterior;
            p.gridCap = interiorGridCap(); // the boundary kernel runs beside this launch (exchange stream)
        }
        if (part == 1) p.kbegin = numInterior;
        const bool lastOfStep = s == blitzdg::LSERK4::numStages - 1;
        // the unrolled kernel's face-link instances (launchAffine, sw2d_order.hip); every other kernel ignores both
        p.faceLink = faceLink.p;
        p.stageKind = p.ca == 0.0 ? bdg_dev::STAGE_FIRST : (lastOfStep ? bdg_dev::STAGE_LAST : bdg_dev::STAGE_MID);
        nextEvalTime = lastOfStep ? timeNow + dtStage : timeNow;
        launchStage(bdg_dev::MODE_LSERK, false, p, "sw2d stage kernel <LSERK>", on, part == 2);
        expectRing += signals;
        if (done && !recorded) hipCheck(hipEventRecord(done, on ? on : stream), "hipEventRecord");
        if (part != 0 && advance) lserkStageAdvance(s);
    }

    // `state`: the planes whose boundary elements are packed / whose ghost columns are filled (default: the current state)
    void launchPack(double* buf, hipStream_t on = nullptr, const double* state = nullptr) {
        bdg_halo::pack(state ? state : qcur, ld, nf * Np, sendSlots.p, numSend, buf, on ? on : stream);
    }
    void launchUnpack(const double* buf, hipStream_t on = nullptr, double* state = nullptr) {
        bdg_halo::unpack(state ? state : qcur, ld, nf * Np, numOwned, K - numOwned, buf, on ? on : stream);
    }

    // ---- plain (not overlapped) exchange for the steppers whose RHS needs more than the neighbours' traces of the
    //      previous stage: every evaluation of the midpoint / Heun schemes reads another state, and variant B also
    //      needs ONE Lax-Friedrichs speed over all ranks (reference src/sw2d/main.cpp:414) before any element starts.
    void exchangeGhostsOf(double* state) {
        if (!halo.comm) throw arg_error("no communicator: call bdg_sw2d_comm_init first");
        launchPack(halo.sendBuf.p, stream, state);
        halo.sendRecv(stream, nf * Np);
        launchUnpack(halo.recvBuf.p, stream, state);
    }
    // variant B: speed of `state` over this rank's owned elements (their '+' traces include the ghosts just received),
    // then the maximum over all ranks, left in lamBuf on the device: one 8-byte all-reduce per RHS evaluation
    void globalSpeedOf(const double* state) {
        bdg_dev::StageParams p = baseParams();
        p.qin = state;
        vb.tide = tideAt(timeNow);
        vb.lam = lamBuf.p;
        evaluated = true;
        hipCheck(kt->stageVb(bdg_dev::MODE_RHS, p, vb, vbPartials.p, lamBuf.p, true, bdg_dev::VbStage::None, nullptr, stream), "sw2d_vb_speed_kernel");
        if (halo.comm && halo.world > 1)
            ncclCheck(rccl().AllReduce(lamBuf.p, lamBuf.p, 1, ncclDouble, ncclMax, halo.comm, stream), "ncclAllReduce");
    }
    // one evaluation of a partitioned run: ghosts of `state`, the all-rank speed (variant B), then fn launches the stage
    template <typename Fn>
    void evaluateExchanged(double* state, Fn&& fn) {
        exchangeGhostsOf(state);
        if (variantB) {
            globalSpeedOf(state);
            lamExternal = true;
        }
        try {
            fn();
        } catch (...) {
            lamExternal = false;
            throw;
        }
        lamExternal = false;
    }

    // True when the partition-boundary launch of an exchanged stage can do the halo staging itself (three-field
    // straight-sided solver whose boundary strip runs on a matrix-core kernel).
    bool halosFold() const {
        if (!haloFusable || !affine || variantB || variantD || variantForced || env::haloKernels()) return false;
        return N >= 5 || numOwned - numInterior < kSmallLaunch[N]; // the strip runs on a matrix-core kernel
    }
    // True when the two chains of an exchanged stage can meet through device counters polled inside the kernels instead of
    // through events on the queues (BDG_SW2D_EVENT_SYNC=1 keeps the events): folded halo staging, and both launches of a stage
    // on kernels that have a SYNC instance -- the interior on the matrix-core kernel of its order, the strip on the latency form.
    bool flagSyncUsable() const {
        if (env::eventSync() || !syncBuf.p || !halosFold()) return false;
        if (env::stripThroughput() || env::haloVariant()) return false;
        if (N >= 5) return affineVariant == AffineVariant::Mfma3 && (numOwned - numInterior + 15) / 16 <= 1024;
        // N <= 4: only while the interior share is small enough for the matrix-core kernel (8-way split of C3). A SYNC instance of
        // the unrolled kernel (the wait in front of its one big basic block, ring waves storing write-through) was built and
        // measured in the 2- and 4-way rehearsal: 0.332 / 0.164 ms per stage against 0.220 / 0.121 with the events -- the branch
        // at the top costs that kernel its load batching (profiles/r04_rehearsal_experiments.txt); larger shares keep the events.
        const int smallPinned = env::smallLaunchPinned();
        return numInterior > 0 && affineVariant == AffineVariant::Unrolled && numInterior < (smallPinned >= 0 ? smallPinned : kSmallLaunch[N]);
    }
    // a bounded in-kernel wait that gave up (sync_wait) left a mark: report it the next time the host looks at the device
    bool takeSyncMark() { // true (and the mark cleared) if a wait of this device gave up since the last look
        if (!syncBuf.p) return false;
        unsigned long long mark = 0;
        hipCheck(hipMemcpy(&mark, syncBuf.p + 2, sizeof(mark), hipMemcpyDeviceToHost), "sync word download");
        if (mark != 0) hipCheck(hipMemset(syncBuf.p + 2, 0, sizeof(mark)), "hipMemset");
        return mark != 0;
    }
    static const char* syncErrorText() {
        return "an in-kernel wait between the interior and the partition-boundary launch of an exchanged stage "
               "timed out: the results of this run are not valid (BDG_SW2D_EVENT_SYNC=1 restores event waits)";
    }
    void checkSyncError() {
        if (takeSyncMark()) throw std::runtime_error(syncErrorText());
    }
    // LSERK4 stage of the partition-boundary elements: reads ghost traces from recv, writes send records
    // ringExpected (flagSync): the ring-tile count the interior launch of the PREVIOUS stage brings the counter to
    void launchBoundaryStageFolded(hipStream_t on, const double* recv, double* send, hipEvent_t done = nullptr, bool flagSync = false,
                                   unsigned long long ringExpected = 0) {
        bdg_dev::StageParams p = baseParams();
        bool recorded = false;
        unsigned signals = 0;
        if (flagSync) {
            p.syncWait = syncBuf.p; p.syncWaitValue = ringExpected;
            p.syncSignal = syncBuf.p + 1; p.syncError = reinterpret_cast<unsigned int*>(syncBuf.p + 2);
            p.syncFirstTile = 0;
            p.syncSignalsOut = &signals;
        }
        const int s = lserkStageParams(p, done, &recorded);
        p.kbegin = numInterior;
        p.haloRecv = recv; p.haloSend = send; p.haloSendOf = haloSendOf.p;
        p.haloOwned = numOwned; p.haloRows = nf * Np;
        if (N >= 5) { // the kernel family the interior (and a single-domain run) uses: bit-identical arithmetic
            p.opsAffine = opsMfma2.p;
            static const char* haloVariant = env::haloVariant(); // A/B switch: "6" = two-waves schedule
            const bool two = affineVariant == AffineVariant::Mfma2 || (haloVariant && haloVariant[0] == '6');
            hipCheck(two ? kt->stageMfma2Halo(p, on) : kt->stageMfma3Halo(p, on), "sw2d boundary stage kernel <LSERK, halo>");
        } else {
            p.opsAffine = opsMfma.p;
            hipCheck(kt->stageMfmaHalo(p, on), "sw2d boundary stage kernel <LSERK, halo>");
        }
        expectStrip += signals;
        if (done && !recorded) hipCheck(hipEventRecord(done, on), "hipEventRecord");
        lserkStageAdvance(s);
    }

    // LSERK4 stages of a partitioned run, all on the device, as two concurrent chains:
    //   compute stream  A:  wait B(s-1) -> [interior elements of stage s] -> signal A(s)
    //   exchange stream B:  pack(s) -> grouped ncclSend/ncclRecv with every neighbour -> unpack(s)
    //                       -> wait A(s-1) -> [partition-boundary elements of stage s] -> signal B(s)
    // The only true dependency loop is boundary -> transfer -> boundary on chain B; the interior
    // elements (99 % of the work) run beside it and only meet it one stage later:
    //   interior(s) reads boundary elements' state of stage s-1 and overwrites the buffer boundary(s-1)
    //   read, hence waits for B(s-1); boundary(s) reads interior neighbours' state of stage s-1 and
    //   overwrites slots interior(s-1) read, hence waits for A(s-1). Within B, stream order protects
    //   the send / receive buffers and the ghost slots. Events alternate by stage parity so that a
    //   wait issued for stage s-1 is not re-armed by the record of stage s.
    void launchLserkStagesExchanged(double dt, int numStages) {
        if (!halo.comm) throw arg_error("no communicator: call bdg_sw2d_comm_init first");
        if (numStages <= 0) return;
        const int rows = nf * Np;
        dtStage = dt;
        if (variantB) { // the all-rank speed has to exist before any element of the stage starts: no overlap to be had
            for (int i = 0; i < numStages; ++i) evaluateExchanged(qcur, [&] { launchLserkStage(2); });
            return;
        }
        // chain B starts after everything already queued on A (state upload, earlier steps)
        hipCheck(hipEventRecord(evA[1], stream), "hipEventRecord");
        hipCheck(hipStreamWaitEvent(halo.stream, evA[1], 0), "hipStreamWaitEvent");
        bool haveA = false, haveB = false;
        // With the staging folded into the boundary kernel, chain B is: exchange -> boundary kernel (which reads
        // the received records and writes the next send records); only the very first exchange needs a pack.
        const bool fold = halosFold();
        // Round 4: where both launches of a stage have a SYNC instance the two chains meet INSIDE the kernels. The elements are
        // ordered [deep interior | ring | boundary | ghost]; only the ring -- the interior elements next to the partition
        // boundary -- reads what boundary(s-1) wrote and overwrites what it read, and only the boundary elements read what the ring
        // tiles of interior(s-1) wrote. So interior(s)'s ring tiles (its last ones) poll a counter that boundary(s-1)'s workgroups
        // raise, boundary(s) polls the counter interior(s-1)'s ring tiles raise, and neither queue carries a wait or a record
        // for the other any more: the interior launches run back to back on A, exchange and boundary launch back to back on B.
        // No deadlock: a launch only ever waits for a launch that was queued earlier on the other stream and whose own waits
        // are for launches queued earlier still (down to counts that already hold when the loop starts); the waiting ring tiles
        // are a few dozen waves, so the boundary launch and RCCL's kernel always find free compute units (interiorGridCap keeps
        // them free at N >= 5), and every wait is bounded (sync_wait) -- a wave that gives up marks the run invalid.
        const bool flags = fold && flagSyncUsable();
        if (fold) launchPack(halo.sendBuf.p, halo.stream);
        for (int i = 0; i < numStages; ++i) {
            const int cur = i & 1, prev = cur ^ 1;
            const bool last = i == numStages - 1;
            const unsigned long long ringBefore = expectRing; // what interior(i-1) and everything before it brings the counter to
            // ---- chain A
            if (!flags && haveB) hipCheck(hipStreamWaitEvent(stream, evB[prev], 0), "hipStreamWaitEvent");
            launchLserkStage(0, nullptr, true, flags ? nullptr : evA[cur], flags);
            // ---- chain B
            if (!fold) launchPack(halo.sendBuf.p, halo.stream);
            halo.sendRecv(halo.stream, rows);
            if (!fold) launchUnpack(halo.recvBuf.p, halo.stream);
            if (!flags && haveA) hipCheck(hipStreamWaitEvent(halo.stream, evA[prev], 0), "hipStreamWaitEvent");
            if (fold) launchBoundaryStageFolded(halo.stream, halo.recvBuf.p, halo.sendBuf.p, (!flags || last) ? evB[cur] : nullptr, flags, ringBefore);
            else launchLserkStage(1, halo.stream, true, evB[cur]); // partition-boundary elements, advance
            haveA = haveB = true;
        }
        // later work on A (dt reduction, downloads, plain stages) sees the last boundary update
        hipCheck(hipStreamWaitEvent(stream, evB[(numStages - 1) & 1], 0), "hipStreamWaitEvent");
    }

    // max (or min) of one double over all ranks, through the device
    double allReduceScalar(double v, bool takeMax, bool sum = false) {
        if (!halo.comm || halo.world == 1) return v;
        hipCheck(hipMemcpyAsync(halo.scalarBuf.p, &v, sizeof(double), hipMemcpyHostToDevice, stream), "H2D copy");
        ncclCheck(rccl().AllReduce(halo.scalarBuf.p, halo.scalarBuf.p + 1, 1, ncclDouble, sum ? ncclSum : (takeMax ? ncclMax : ncclMin),
                                   halo.comm, stream), "ncclAllReduce");
        double out = 0.0;
        hipCheck(hipMemcpyAsync(&out, halo.scalarBuf.p + 1, sizeof(double), hipMemcpyDeviceToHost, stream), "D2H copy");
        hipCheck(hipStreamSynchronize(stream), "allreduce sync");
        return out;
    }

    // ---- the two-evaluation steppers. How an evaluation is issued: over the whole mesh, or -- a partitioned run -- exchanged:
    // the ghost columns of the state it reads refreshed first and, variant B, the Lax-Friedrichs speed reduced over all ranks
    enum class Eval { Whole, Exchanged };
    // out = ca base + cb in + cc R(in), base = the current state; `next`: model time of the evaluation that will follow this one
    void combine(Eval how, bool filter, bdg_dev::StageParams& p, double* in, double* out, double ca, double cb, double cc, double next) {
        p.qin = in; p.qbase = qcur; p.qout = out;
        p.ca = ca; p.cb = cb; p.cc = cc;
        nextEvalTime = next;
        auto launch = [&] { launchStage(bdg_dev::MODE_COMBINE, filter, p, "sw2d stage kernel <COMBINE>"); };
        if (how == Eval::Exchanged) evaluateExchanged(in, launch);
        else launch();
    }
    // q1 = q + dt/2 R(q);  q = q + dt R(q1)   (reference src/sw2d-simple/main.cpp:132-151)
    void rk2Step(double dt, bool filter, Eval how) {
        // (ahead of the first exchange of a partitioned run. The Heun step below leaves the check to launchStage, which in a
        // partitioned run comes after that exchange and its communicator check: what a caller sees first differs, and stays)
        if (filter && !hasFilter) throw arg_error("filter requested but the solver was created without a Filter matrix");
        bdg_dev::StageParams p = baseParams();
        combine(how, filter, p, qcur, aux.p, 1.0, 0.0, 0.5 * dt, timeNow);
        combine(how, filter, p, aux.p, qalt, 1.0, 0.0, dt, timeNow + dt);
        std::swap(qcur, qalt);
        timeNow += dt;
    }
    // SSP-RK2 (Heun) of the reference's variant-B driver (src/sw2d/main.cpp:211-235), sponge optional:
    //   q1 = sponge(q + dt R(q));   q = sponge(1/2 (q + q1 + dt R(q1)))
    void sspRk2Step(double dt, bool filter, double spongeCoeff, Eval how) {
        bdg_dev::StageParams p = baseParams();
        p.sponge = spongeCoeff;
        combine(how, filter, p, qcur, aux.p, 1.0, 0.0, dt, timeNow);                  // second evaluation: same time level (:225)
        combine(how, filter, p, aux.p, qalt, 0.5, 0.5, 0.5 * dt, timeNow + dt);       // then the first evaluation of the next step
        std::swap(qcur, qalt);
        timeNow += dt;
    }

    // ---- operator images built when a variant first needs them
    // Row-wise operator image of the per-node-geometry form of variants B / C / D (VnOps: row i = Dr[i][.], Ds[i][.] interleaved,
    // then Lift[i][.]), the Filter rows of its second pass and the scratch planes of the unfiltered rows
    void buildNodalVariantOps() {
        if (opsVn.p) return;
        const int row = 2 * Np + NFN;
        std::vector<double> img(static_cast<size_t>(row) * Np);
        for (int i = 0; i < Np; ++i) {
            for (int m = 0; m < Np; ++m) {
                img[static_cast<size_t>(i) * row + 2 * m] = hostDr[static_cast<size_t>(i) * Np + m];
                img[static_cast<size_t>(i) * row + 2 * m + 1] = hostDs[static_cast<size_t>(i) * Np + m];
            }
            for (int j = 0; j < NFN; ++j) img[static_cast<size_t>(i) * row + 2 * Np + j] = hostLift[static_cast<size_t>(i) * NFN + j];
        }
        opsVn.upload(img, bytes, "nodal variant ops upload");
        if (!hostFilter.empty()) {
            filterRows.upload(hostFilter, bytes, "filter upload");
            vnRaw.alloc(static_cast<size_t>(nf) * planeSize(), bytes);
        }
    }

    // [m][i]{Dr'[i][m], Ds'[i][m], F'[i][m]} + Lift' images (F' = I or Filter) for the rolled
    // one-field-per-wave kernels (variants B and D)
    void buildSourceOps() {
        if (opsVd.p) return;
        auto image = [&](const double* Dr, const double* Ds, const double* F, const double* Lift) {
            std::vector<double> img(static_cast<size_t>(3) * Np * Np + static_cast<size_t>(NFN) * Np);
            for (int m = 0; m < Np; ++m)
                for (int i = 0; i < Np; ++i) {
                    const size_t o = 3 * (static_cast<size_t>(m) * Np + i);
                    img[o] = Dr[i * Np + m];
                    img[o + 1] = Ds[i * Np + m];
                    img[o + 2] = F ? F[i * Np + m] : (i == m ? 1.0 : 0.0);
                }
            for (int j = 0; j < NFN; ++j)
                for (int i = 0; i < Np; ++i)
                    img[static_cast<size_t>(3) * Np * Np + static_cast<size_t>(j) * Np + i] = Lift[i * NFN + j];
            return img;
        };
        opsVd.upload(image(hostDr.data(), hostDs.data(), nullptr, hostLift.data()), bytes, "source ops upload");
        if (!hostFilter.empty())
            opsVdFiltered.upload(image(hostFDr.data(), hostFDs.data(), hostFilter.data(), hostFLift.data()), bytes,
                                 "filtered source ops upload");
    }

    // Operator image of the matrix-core kernel with source terms (variants B/C/D at N >= 6): MfmaOps2 layout --
    // Dr tiles [r][t], Ds tiles, lift tiles [r][f][tf] -- followed by MT*KV tiles of F' (identity, or Filter with
    // the other operators pre-multiplied by it). Lane l of a tile holds A[16r + (l&15)][4t + (l>>4)].
    void buildMfma2SourceOps() {
        if (opsMfma2Src.p) return;
        const int MT = kt->mfmaMT, KV = kt->mfmaKV, KF = kt->mfma2KF;
        auto image = [&](const double* Dr, const double* Ds, const double* Lift, const double* F) {
            const size_t tilesD = static_cast<size_t>(MT) * KV * 64, offF = static_cast<size_t>(kt->mfma2OpsDoubles);
            std::vector<double> img(offF + tilesD, 0.0);
            for (int r = 0; r < MT; ++r)
                for (int l = 0; l < 64; ++l) {
                    const int i = 16 * r + (l & 15);
                    if (i >= Np) continue;
                    for (int t = 0; t < KV; ++t) {
                        const int k = 4 * t + (l >> 4);
                        if (k >= Np) continue;
                        const size_t at = (static_cast<size_t>(r) * KV + t) * 64 + l;
                        img[at] = Dr[i * Np + k];
                        img[tilesD + at] = Ds[i * Np + k];
                        img[offF + at] = F ? F[i * Np + k] : (i == k ? 1.0 : 0.0);
                    }
                    for (int f = 0; f < 3; ++f)
                        for (int tf = 0; tf < KF; ++tf) {
                            const int n = 4 * tf + (l >> 4);
                            if (n < Nfp)
                                img[2 * tilesD + ((static_cast<size_t>(r) * 3 + f) * KF + tf) * 64 + l] = Lift[i * NFN + f * Nfp + n];
                        }
                }
            return img;
        };
        opsMfma2Src.upload(image(hostDr.data(), hostDs.data(), hostLift.data(), nullptr), bytes, "mfma2 source ops upload");
        if (!hostFilter.empty())
            opsMfma2SrcFiltered.upload(image(hostFDr.data(), hostFDs.data(), hostFLift.data(), hostFilter.data()), bytes,
                                       "filtered mfma2 source ops upload");
    }
    // the transposed Filter of the unrolled source kernels' filtered evaluations
    void buildFilterT() {
        if (filterT.p || hostFilter.empty()) return;
        std::vector<double> ft(static_cast<size_t>(Np) * Np);
        for (int m = 0; m < Np; ++m)
            for (int i = 0; i < Np; ++i) ft[static_cast<size_t>(m) * Np + i] = hostFilter[static_cast<size_t>(i) * Np + m];
        filterT.upload(ft, bytes, "filter upload");
    }

    // ---- run monitor and drifters (run_records.hpp)
    // records a stepping call of `steps` further completed steps would take; refused before anything is launched
    void monitorReserve(long long steps, const char* fn) const { mon.reserve(steps, fn, "bdg_sw2d"); }
    void drifterReserve(long long steps, const char* fn) const { drf.reserve(steps, fn, "bdg_sw2d"); }
    // completed LSERK4 steps among the next `stages` stages
    long long lserkSteps(long long stages) const { return bdg_records::lserkSteps(stageCount, stages, blitzdg::LSERK4::numStages); }
    // one record of the resident state into rec[column * capacity + slot], two launches on the solver's stream. The range
    // reduced is the owned device slots [0, numOwned); H: the monitor's own, else the solver's resident one, else none
    void monitorLaunch(double* rec, int capacity, int slot) {
        const double* Hm = mon.H.p ? mon.H.p : (hasH ? Hbuf.p : nullptr);
        mon.launch({qcur, Hm, ld, Np, nf, numOwned, g, timeNow}, rec, capacity, slot, bdg_dev::sw2d_monitor_finish_kernel,
                   "sw2d_monitor_finish_kernel launch", bdg_dev::MonRowGauges{mon.row.p}, stream);
    }
    void monitorSample() { monitorLaunch(mon.rec.p, mon.capacity, mon.count++); }
    // one launch of the drifter kernel on the solver's stream, reading the current state; slot < 0: no record
    void drifterLaunch(int mode, double dt, int slot) {
        drf.launch(bdg_dev::sw2d_drifter_kernel, "sw2d_drifter_kernel launch",
                   bdg_dev::TriDriftTables{drf.vert.p, drf.neigh.p, drf.vinvT.p, drf.jac.p}, qcur, ld, N, mode, dt, slot, stream);
    }
    // one advance in the resident state, with the record of time drf.t if one is due (room was reserved by the caller)
    void drifterAdvance(double dt, bool record = true) { drifterLaunch(bdg_dev::kDriftAdvance, dt, drf.takeSlot(record)); }
    // (u0, v0) again after the state under the drifters has been replaced
    void drifterResample() {
        if (drf.on) drifterLaunch(bdg_dev::kDriftSample, 0.0, -1);
    }
    // what a sample of the field statistics reads: the owned device slots; H by the monitor's rule: the statistics' own, else
    // the solver's resident one, else none
    bdg_records::StatsView statsView() const {
        const double* Hm = fst.H.p ? fst.H.p : (hasH ? Hbuf.p : nullptr);
        return {qcur, Hm, ld, Np, numOwned, timeNow};
    }
    void statsSample() { fst.sample(statsView(), stream); }
    // after every completed step (of size dt) of a stepping call whose launches are all on the solver's stream (room was reserved
    // by the caller): the monitor's sample, the sample of the field statistics, then the drifters' advance (statistics and
    // drifters exist on unpartitioned solvers only)
    void stepDone(double dt) {
        if (mon.on && ++mon.steps % mon.stride == 0) monitorSample();
        if (fst.on && ++fst.steps % fst.stride == 0) statsSample();
        if (drf.on) {
            drf.t = timeNow;
            drifterAdvance(dt);
        }
    }
    // `numStages` LSERK4 stages on the whole mesh, a record after every stride-th completed step
    void lserkStagesMonitored(int numStages) {
        for (int i = 0; i < numStages; ++i) {
            launchLserkStage();
            if (stageCount % blitzdg::LSERK4::numStages == 0) stepDone(dtStage);
        }
    }
    // ... of a partitioned run. The two-chain schedule is issued in pieces that end where a record is due: a piece starts
    // behind everything queued on the solver's stream (the sample) and ends with that stream behind its last boundary launch
    void lserkStagesExchangedMonitored(double dt, int numStages) {
        if (!mon.on) {
            launchLserkStagesExchanged(dt, numStages);
            return;
        }
        int left = numStages;
        while (left > 0) {
            // stages up to and including the one that completes the next step at which a record is due
            const int toStep = blitzdg::LSERK4::numStages - static_cast<int>(stageCount % blitzdg::LSERK4::numStages);
            const long long stepsToDue = mon.stride - mon.steps % mon.stride;
            const long long want = toStep + (stepsToDue - 1) * blitzdg::LSERK4::numStages;
            const int piece = static_cast<int>(std::min<long long>(left, want));
            const long long done = lserkSteps(piece);
            launchLserkStagesExchanged(dt, piece);
            left -= piece;
            if (done > 0) {
                mon.steps += done - 1;
                stepDone(dt);
            }
        }
    }

    // Returns {max |Fscale|*spd, max |eta|}; NaN if any entry is NaN.
    void reduceDt(double out[2]) {
        const int nblocks = (numOwned + 255) / 256;
        hipCheck(kt->dt(qcur, fscaleNodal, hasH ? Hbuf.p : nullptr, ld, numOwned, g, partials.p,
                        stream), "sw2d_dt_kernel");
        hipLaunchKernelGGL(bdg_dev::sw2d_reduce_kernel, dim3(1), dim3(256), 0, stream, partials.p, nblocks, red2.p);
        hipCheck(hipGetLastError(), "sw2d_reduce_kernel");
        hipCheck(hipMemcpyAsync(out, red2.p, 2 * sizeof(double), hipMemcpyDeviceToHost, stream), "D2H copy");
        hipCheck(hipStreamSynchronize(stream), "reduce sync");
    }
};

namespace {

// C = A (n x n) * B (n x c), row-major.
std::vector<double> matmulHost(const double* A, const double* B, int n, int c) {
    std::vector<double> C(static_cast<size_t>(n) * c, 0.0);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < c; ++j) {
            double s = 0.0;
            for (int k = 0; k < n; ++k) s += A[i * n + k] * B[k * c + j];
            C[static_cast<size_t>(i) * c + j] = s;
        }
    return C;
}

// AffineOps<N> image: [m][i]{Dr[i][m], Ds[i][m]} then [j][i] Lift[i][j].
std::vector<double> affineOpsImage(const double* Dr, const double* Ds, const double* Lift, int Np, int NFN) {
    std::vector<double> img(static_cast<size_t>(2) * Np * Np + static_cast<size_t>(NFN) * Np);
    for (int m = 0; m < Np; ++m)
        for (int i = 0; i < Np; ++i) {
            img[2 * (static_cast<size_t>(m) * Np + i)] = Dr[i * Np + m];
            img[2 * (static_cast<size_t>(m) * Np + i) + 1] = Ds[i * Np + m];
        }
    for (int j = 0; j < NFN; ++j)
        for (int i = 0; i < Np; ++i) img[static_cast<size_t>(2) * Np * Np + static_cast<size_t>(j) * Np + i] = Lift[i * NFN + j];
    return img;
}

bdg_sw2d* createSolver(const bdg_sw2d_desc& d) {
    if (d.order < 1 || d.order > BDG_SW2D_MAX_ORDER)
        throw arg_error("bdg_sw2d_create: order must be 1.." + std::to_string(BDG_SW2D_MAX_ORDER) +
                        " for the register-resident kernels");
    if (d.num_elements < 1) throw arg_error("bdg_sw2d_create: num_elements must be >= 1");
    if (!d.Dr || !d.Ds || !d.Lift || !d.rx || !d.sx || !d.ry || !d.sy || !d.nx || !d.ny || !d.Fscale || !d.vmapP)
        throw arg_error("bdg_sw2d_create: a required table pointer is NULL");
    if (d.num_wall < 0 || (d.num_wall > 0 && !d.mapW)) throw arg_error("bdg_sw2d_create: bad wall-node list");

    const bdg_dev::KernelTable* kt = bdg_dev::kernel_table(d.order);
    if (!kt) throw arg_error("bdg_sw2d_create: no kernels compiled for this order");

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        throw hip_error("bdg_sw2d_create: no HIP device available (the sw2d path has no CPU fallback)");
    if (d.device < 0 || d.device >= ndev) throw arg_error("bdg_sw2d_create: device ordinal out of range");

    auto s = std::unique_ptr<bdg_sw2d>(new bdg_sw2d());
    s->kt = kt;
    s->N = d.order; s->Np = kt->Np; s->Nfp = kt->Nfp; s->NFN = 3 * kt->Nfp; s->K = d.num_elements;
    s->device = d.device;
    s->g = d.g;
    if (d.num_fields != 0 && d.num_fields != 3 && d.num_fields != 4)
        throw arg_error("bdg_sw2d_create: num_fields must be 3 or 4");
    s->nf = d.num_fields == 4 ? 4 : 3;
    s->variantD = s->nf == 4 || d.sources != 0;
    s->ld = (static_cast<long long>(s->K) + 63) / 64 * 64;
    s->numInterior = s->numOwned = s->K;
    const int Np = s->Np, Nfp = s->Nfp, NFN = s->NFN, K = s->K;
    const long long ld = s->ld;
    // Lane addresses are a wave-uniform row pointer plus a 32-bit unsigned BYTE offset (8 * node offset).
    if (static_cast<long long>(Np) * ld * 8 > 4294967295LL)
        throw arg_error("bdg_sw2d_create: Np*K exceeds 2^29 nodes (32-bit byte offsets within a field): partition the "
                        "mesh over more devices");

    // ---- validate the index tables on the host before anything touches the GPU
    const size_t nFaceNodes = static_cast<size_t>(NFN) * K;
    if (d.vmapM)
        for (int k = 0; k < K; ++k)
            for (int f = 0; f < 3; ++f)
                for (int n = 0; n < Nfp; ++n)
                    if (d.vmapM[(static_cast<size_t>(k) * 3 + f) * Nfp + n] != kt->fmask(f, n) + Np * k)
                        throw arg_error("bdg_sw2d_create: vmapM does not follow the warp&blend face-node ordering "
                                        "(Fmask) these kernels are specialised for");
    const long long totalNodes = static_cast<long long>(Np) * K;
    for (size_t i = 0; i < nFaceNodes; ++i)
        if (d.vmapP[i] < 0 || d.vmapP[i] >= totalNodes) throw arg_error("bdg_sw2d_create: vmapP entry out of range");
    for (int i = 0; i < d.num_wall; ++i)
        if (d.mapW[i] < 0 || static_cast<size_t>(d.mapW[i]) >= nFaceNodes)
            throw arg_error("bdg_sw2d_create: wall-node index out of range");

    // Element numbering: the trace gather is cheap only when face neighbours sit within an L2-sized
    // window of slots. Forced by BDG_SW2D_REORDER, suppressed by BDG_SW2D_KEEP_ORDER, otherwise decided
    // from the neighbour distances (element_order.hpp): mean above 4 sqrt(K), as on a shuffled mesh
    // (10^6-triangle box: 1.06 ms as given, 0.32 ms renumbered), or, at N <= 4, over a tenth of the faces
    // beyond 1 MiB of stage traffic on a mesh larger than one XCD's L2, as in the row-by-row order of a
    // wide box (0.306 ms as given, 0.300 renumbered). The numbering is breadth-first;
    // BDG_SW2D_ORDER_PATCH=n makes it compact patches of n elements instead (measured, not kept).
    namespace eo = blitzdg::element_order;
    const bool reorder = (d.flags & BDG_SW2D_REORDER) != 0 ||
                         (!(d.flags & BDG_SW2D_KEEP_ORDER) && eo::renumberingWanted(d.vmapP, K, Np, Nfp, d.order));
    if (reorder) s->permHost = eo::renumbering(d.vmapP, K, Np, Nfp, eo::patchSetting());
    // Affine: the metric terms are constant per element and the face terms constant per face (straight-sided elements), to
    // round-off: then one value per element/face suffices. The tables themselves carry round-off from Dr*x on small elements
    // (relative ~1e-16 * |Dr| / h: 5e-11 at N=8 on a 500x250-cell box), so the test (element_tables.hpp) is 1e-8: far above
    // that noise, far below any real curvature. J is not held to it here.
    s->affine = !(d.flags & BDG_SW2D_NODAL_GEOMETRY) &&
                blitzdg::element_tables::trianglesAreAffine({d.rx, d.sx, d.ry, d.sy, nullptr, d.nx, d.ny, d.Fscale}, Np, Nfp, K);
    // Non-affine tables: the matrix-core kernel with per-node geometry (every order). BDG_SW2D_NODAL_VECTOR=1 keeps the
    // round-1 vector kernel (one lane per element, N <= 6) for A/B measurements and cross-checks.
    s->nodalMfma = !s->affine && !(env::nodalVector() && kt->ldsDoubles != 0);

    s->use();
    hipCheck(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking), "hipStreamCreate");

    const size_t plane3 = static_cast<size_t>(s->nf) * s->planeSize();
    s->qA.alloc(plane3, s->bytes);
    s->qB.alloc(plane3, s->bytes);
    s->res.alloc(plane3, s->bytes);
    s->aux.alloc(plane3, s->bytes);
    // Per-node geometry planes and the LDS operator image belong to the nodal kernels; the affine
    // path keeps 13 values per element (below) plus the per-node Fscale plane, which only the
    // time-step reduction reads (so that dt stays bit-identical to the reference formula).
    const size_t fplane = static_cast<size_t>(NFN) * ld;
    if (!s->affine) {
        s->geo.alloc(4 * s->planeSize(), s->bytes);
        s->fgeo.alloc(3 * fplane, s->bytes);
        s->ops.alloc(kt->ldsDoubles, s->bytes);
    } else {
        s->fgeo.alloc(fplane, s->bytes);
    }
    s->fscaleNodal = s->affine ? s->fgeo.p : s->fgeo.p + 2 * fplane;
    s->vmapP.alloc(static_cast<size_t>(NFN) * ld, s->bytes);
    s->stage.alloc(static_cast<size_t>(std::max(Np, NFN)) * K, s->bytes);
    s->istage.alloc(static_cast<size_t>(NFN) * K, s->bytes);
    s->partials.alloc(2 * static_cast<size_t>((K + 255) / 256), s->bytes);
    s->red2.alloc(2, s->bytes);
    if (!s->permHost.empty()) s->perm.upload(s->permHost, s->bytes, "perm upload");
    for (auto* b : {&s->qA, &s->qB, &s->res, &s->aux, &s->geo, &s->fgeo})
        if (b->p) hipCheck(hipMemsetAsync(b->p, 0, b->n * sizeof(double), s->stream), "hipMemset");
    hipCheck(hipMemsetAsync(s->vmapP.p, 0, s->vmapP.n * sizeof(int), s->stream), "hipMemset");
    s->qcur = s->qA.p;
    s->qalt = s->qB.p;

    s->hasFilter = d.Filter != nullptr;
    if (!s->affine && kt->ldsDoubles > 0) { // (orders 7, 8 have no vector kernel: matrix cores only)
        // ---- operator image for the nodal kernels: [Dr,Ds interleaved | Lift | Filter]
        std::vector<double> img(kt->ldsDoubles, 0.0);
        for (int i = 0; i < Np * Np; ++i) {
            img[2 * i] = d.Dr[i];
            img[2 * i + 1] = d.Ds[i];
        }
        std::copy(d.Lift, d.Lift + static_cast<size_t>(Np) * NFN, img.begin() + 2 * Np * Np);
        if (d.Filter) std::copy(d.Filter, d.Filter + static_cast<size_t>(Np) * Np, img.begin() + 2 * Np * Np + Np * NFN);
        hipCheck(hipMemcpyAsync(s->ops.p, img.data(), img.size() * sizeof(double), hipMemcpyHostToDevice, s->stream),
                 "ops upload");
        hipCheck(hipStreamSynchronize(s->stream), "ops sync");
    }

    // ---- geometry planes
    if (!s->affine) {
        const size_t pl = s->planeSize();
        s->uploadRows(d.rx, s->geo.p, Np);
        s->uploadRows(d.sx, s->geo.p + pl, Np);
        s->uploadRows(d.ry, s->geo.p + 2 * pl, Np);
        s->uploadRows(d.sy, s->geo.p + 3 * pl, Np);
        s->uploadRows(d.nx, s->fgeo.p, NFN);
        s->uploadRows(d.ny, s->fgeo.p + fplane, NFN);
    }
    s->uploadRows(d.Fscale, s->fscaleNodal, NFN);

    // ---- affine fast path: one metric value per element, one normal/scale per face
    // Measured on MI355X: the fully unrolled vector kernel wins up to N=4; from
    // N=5 on its basic block outgrows the register files and the matrix-core kernel is fastest
    // (N=5, 640 k elements: 0.454 ms unrolled, 0.405 ms matrix cores).
    // From N = 5 the default is the state-once matrix-core schedule (variant 7; measured against variant 6 at
    // 640 k / 500 k / 250 k / 250 k elements: N=5 0.36 vs 0.42 ms, N=6 0.33 vs 0.40, N=7 0.24 vs 0.28, N=8 0.30 vs 0.39).
    s->affineVariant = s->N <= 4 ? bdg_dev::AffineVariant::Unrolled : bdg_dev::AffineVariant::Mfma3;
    s->sweepAlternates = !env::sweepForward();
    if (const char* e = env::affineVariantPin()) {
        const int v = std::atoi(e);
        if (v >= 0 && v <= 9) {
            s->affineVariant = static_cast<bdg_dev::AffineVariant>(v);
            s->variantForced = true;
        }
    }
    // host copies for the operator images built after creation; Filter * (Dr, Ds, Lift) for every pre-filtered image
    s->hostDr.assign(d.Dr, d.Dr + static_cast<size_t>(Np) * Np);
    s->hostDs.assign(d.Ds, d.Ds + static_cast<size_t>(Np) * Np);
    s->hostLift.assign(d.Lift, d.Lift + static_cast<size_t>(Np) * NFN);
    if (d.Filter) {
        s->hostFilter.assign(d.Filter, d.Filter + static_cast<size_t>(Np) * Np);
        s->hostFDr = matmulHost(d.Filter, d.Dr, Np, Np);
        s->hostFDs = matmulHost(d.Filter, d.Ds, Np, Np);
        s->hostFLift = matmulHost(d.Filter, d.Lift, Np, NFN);
    }
    // the same operators as zero-padded 16x4 MFMA A tiles: lane l of tile (r, t) holds A[16r + (l&15)][4t + (l>>4)]
    auto mfmaImage = [&](const double* Dr, const double* Ds, const double* Lift) {
        const int MT = kt->mfmaMT, KV = kt->mfmaKV, KS = kt->mfmaKS;
        std::vector<double> img(static_cast<size_t>(kt->mfmaOpsDoubles), 0.0);
        auto fill = [&](size_t off, const double* A, int cols, int KT) {
            for (int r = 0; r < MT; ++r)
                for (int t = 0; t < KT; ++t)
                    for (int l = 0; l < 64; ++l) {
                        const int i = 16 * r + (l & 15), k = 4 * t + (l >> 4);
                        if (i < Np && k < cols) img[off + (static_cast<size_t>(r) * KT + t) * 64 + l] = A[i * cols + k];
                    }
        };
        fill(0, Dr, Np, KV);
        fill(static_cast<size_t>(MT) * KV * 64, Ds, Np, KV);
        fill(static_cast<size_t>(2) * MT * KV * 64, Lift, NFN, KS);
        return img;
    };
    // face-by-face variant: lift tile (r, f, tf), lane l = Lift[16r + (l&15)][f*Nfp + 4tf + (l>>4)]
    auto mfma2Image = [&](const double* Dr, const double* Ds, const double* Lift) {
        const int MT = kt->mfmaMT, KV = kt->mfmaKV, KF = kt->mfma2KF;
        std::vector<double> img(static_cast<size_t>(kt->mfma2OpsDoubles), 0.0);
        const std::vector<double> first = mfmaImage(Dr, Ds, Lift);
        std::copy(first.begin(), first.begin() + static_cast<size_t>(2) * MT * KV * 64, img.begin());
        const size_t off = static_cast<size_t>(2) * MT * KV * 64;
        for (int r = 0; r < MT; ++r)
            for (int f = 0; f < 3; ++f)
                for (int tf = 0; tf < KF; ++tf)
                    for (int l = 0; l < 64; ++l) {
                        const int i = 16 * r + (l & 15), n = 4 * tf + (l >> 4);
                        if (i < Np && n < Nfp)
                            img[off + ((static_cast<size_t>(r) * 3 + f) * KF + tf) * 64 + l] = Lift[i * NFN + f * Nfp + n];
                    }
        return img;
    };
    if (s->nodalMfma) { // per-node geometry on the matrix cores: the MfmaOps2 image, plain and pre-filtered
        const std::vector<double> img2 = mfma2Image(d.Dr, d.Ds, d.Lift);
        s->opsMfma2.upload(img2, s->bytes, "mfma2 ops upload");
        if (d.Filter) { // the filter follows the metric terms: plain operators, then the Filter's own tiles (r, t)
            std::vector<double> imgF = img2;
            const int MT = kt->mfmaMT, KV = kt->mfmaKV;
            imgF.resize(img2.size() + static_cast<size_t>(MT) * KV * 64, 0.0);
            for (int r = 0; r < MT; ++r)
                for (int t = 0; t < KV; ++t)
                    for (int l = 0; l < 64; ++l) {
                        const int i = 16 * r + (l & 15), k = 4 * t + (l >> 4);
                        if (i < Np && k < Np) imgF[img2.size() + (static_cast<size_t>(r) * KV + t) * 64 + l] = d.Filter[i * Np + k];
                    }
            s->opsMfma2NodalFilter.upload(imgF, s->bytes, "nodal filter ops upload");
        }
    }
    if (s->affine) {
        s->ageo.alloc(13 * static_cast<size_t>(ld), s->bytes);
        hipCheck(hipMemsetAsync(s->ageo.p, 0, s->ageo.n * sizeof(double), s->stream), "hipMemset");
        s->uploadRows(d.rx, s->ageo.p, 1);           // row 0 of each (Np, K) table
        s->uploadRows(d.sx, s->ageo.p + ld, 1);
        s->uploadRows(d.ry, s->ageo.p + 2 * ld, 1);
        s->uploadRows(d.sy, s->ageo.p + 3 * ld, 1);
        for (int f = 0; f < 3; ++f) {                 // first node of each face
            const size_t row = static_cast<size_t>(f) * Nfp * K;
            s->uploadRows(d.nx + row, s->ageo.p + (4 + f) * ld, 1);
            s->uploadRows(d.ny + row, s->ageo.p + (7 + f) * ld, 1);
            s->uploadRows(d.Fscale + row, s->ageo.p + (10 + f) * ld, 1);
        }
        s->opsAffine.upload(affineOpsImage(d.Dr, d.Ds, d.Lift, Np, NFN), s->bytes, "affine ops upload");
        s->opsMfma2.upload(mfma2Image(d.Dr, d.Ds, d.Lift), s->bytes, "mfma2 ops upload");
        s->opsMfma.upload(mfmaImage(d.Dr, d.Ds, d.Lift), s->bytes, "mfma ops upload");
        if (d.Filter) {
            const double *FDr = s->hostFDr.data(), *FDs = s->hostFDs.data(), *FL = s->hostFLift.data();
            s->opsMfma2Filtered.upload(mfma2Image(FDr, FDs, FL), s->bytes, "filtered mfma2 ops upload");
            s->opsMfmaFiltered.upload(mfmaImage(FDr, FDs, FL), s->bytes, "filtered mfma ops upload");
            s->opsAffineFiltered.upload(affineOpsImage(FDr, FDs, FL, Np, NFN), s->bytes, "filtered affine ops upload");
        }
    }

    // ---- variant D: operator image with a third row per (m, i) (identity or Filter) + source tables
    if (s->variantD) {
        s->buildSourceOps();
        if (s->N > bdg_sw2d::kUnrolledSourcesMaxOrder) {
            s->buildMfma2SourceOps();
            s->mfmaSources = !env::rolledSources();
        }
        s->vd.nf = s->nf;
        s->vd.sources = d.sources ? 1 : 0;
        s->vd.fconst = d.coriolis_const;
        s->vd.cd = d.drag;
        if (d.sources) {
            s->vd.zx = s->uploadPlane(d.zx, s->zxBuf);
            s->vd.zy = s->uploadPlane(d.zy, s->zyBuf);
            s->vd.fcor = s->uploadPlane(d.coriolis, s->fcorBuf);
        }
        // Measured at C3 (10^6 triangles, N=4): rolled kernel 0.87 ms (3 fields) / 1.16 ms (4 fields) per
        // stage; unrolled kernel + tracer launch: see DESIGN.md section 3.
        s->fastSources = s->N <= bdg_sw2d::kUnrolledSourcesMaxOrder && !env::rolledSources();
        if (s->fastSources) s->buildFilterT();
    }

    // ---- gather offsets: reference numbering (n' + Np*k') -> n'*ld + slot(k'), as (NFN, K) rows;
    //      wall nodes are stored as -(offset+1).
    {
        std::vector<int> rows(nFaceNodes);
        const int* perm = s->permHost.empty() ? nullptr : s->permHost.data();
        for (int k = 0; k < K; ++k)
            for (int j = 0; j < NFN; ++j) {
                const int v = d.vmapP[static_cast<size_t>(k) * NFN + j];
                const int n2 = v % Np, k2 = v / Np;
                rows[static_cast<size_t>(j) * K + k] = static_cast<int>(n2 * ld + (perm ? perm[k2] : k2));
            }
        for (int i = 0; i < d.num_wall; ++i) {
            const int w = d.mapW[i], k = w / NFN, j = w % NFN;
            int& e = rows[static_cast<size_t>(j) * K + k];
            if (e >= 0) e = -(e + 1);
        }
        bdg_dev::uploadRows(s->rowLayout(), rows.data(), s->vmapP.p, s->istage.p, NFN);

        // ---- face links: every face of every element must reproduce its Nfp rows above exactly (address and wall
        //      flag); one face that does not (periodic maps, non-conforming meshes, hand-made tables) keeps the whole
        //      solver on the vmapP gather
        const bool full = env::fullStageTraffic();
        if (s->affine && s->N <= 4 && !s->variantD && !full) {
            int fm[3][5]; // (N <= 4)
            for (int f = 0; f < 3; ++f)
                for (int n = 0; n < Nfp; ++n) fm[f][n] = kt->fmask(f, n);
            std::vector<int> links(static_cast<size_t>(3) * K);
            std::atomic<bool> ok{true};
            blitzdg::detail::parallelChunks(K, [&](int kBegin, int kEnd) {
                for (int k = kBegin; k < kEnd && ok.load(std::memory_order_relaxed); ++k)
                    for (int f = 0; f < 3; ++f) {
                        const int k2 = d.vmapP[static_cast<size_t>(k) * NFN + f * Nfp] / Np;
                        const long long slot = perm ? perm[k2] : k2;
                        const bool wall = rows[static_cast<size_t>(f * Nfp) * K + k] < 0;
                        int code = -1;
                        for (int c = 0; c < 6 && code < 0; ++c) {
                            const int f2 = c % 3;
                            const bool rev = c >= 3;
                            bool same = true;
                            for (int n = 0; n < Nfp && same; ++n) {
                                const long long off = fm[f2][rev ? Nfp - 1 - n : n] * ld + slot;
                                same = rows[static_cast<size_t>(f * Nfp + n) * K + k] == (wall ? -(off + 1) : off);
                            }
                            if (same) code = f2 | (rev ? 4 : 0);
                        }
                        if (code < 0) {
                            ok = false;
                            break;
                        }
                        links[static_cast<size_t>(f) * K + k] = static_cast<int>(
                            bdg_dev::FaceLink::make(static_cast<unsigned>(slot), code & 3, code >= 4, wall));
                    }
            });
            if (ok) {
                s->faceLink.alloc(static_cast<size_t>(3) * ld, s->bytes);
                hipCheck(hipMemsetAsync(s->faceLink.p, 0, s->faceLink.n * sizeof(int), s->stream), "hipMemset");
                bdg_dev::uploadRows(s->rowLayout(), links.data(), s->faceLink.p, s->istage.p, 3);
            }
        }
    }
    s->istage.release();
    return s.release();
}

void requireSolver(const bdg_sw2d* s, const char* fn) {
    if (!s) throw arg_error(std::string(fn) + ": solver handle is NULL");
}

// prologue of the six field calls: a solver of `count` fields (`other`: what the refusal says otherwise) and no NULL field
void requireFields(const bdg_sw2d* s, const char* fn, int count, const char* other, std::initializer_list<const void*> fields) {
    requireSolver(s, fn);
    if (s->nf != count) throw arg_error(std::string(fn) + ": " + other);
    for (const void* f : fields)
        if (!f) throw arg_error(std::string(fn) + ": NULL field");
    s->use();
}

// the four bdg_sw2d_step_*rk2* calls: their prologue, then `step()` num_steps times
template <class Step>
int stepCall(bdg_sw2d* s, const char* fn, double dt, int num_steps, Step&& step) {
    return guard([&] {
        requireSolver(s, fn);
        if (num_steps < 0) throw arg_error(std::string(fn) + ": num_steps < 0");
        s->monitorReserve(num_steps, fn);
        s->drifterReserve(num_steps, fn);
        s->use();
        for (int i = 0; i < num_steps; ++i) {
            step();
            s->stepDone(dt);
        }
    });
}

} // namespace

extern "C" {

int bdg_device_count(void) {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

int bdg_sw2d_create(const bdg_sw2d_desc* desc, bdg_sw2d** out) {
    return guard([&] {
        if (!desc || !out) throw arg_error("bdg_sw2d_create: NULL argument");
        *out = createSolver(*desc);
    });
}

int bdg_sw2d_create_from_nodes(const bdg_trinodes* nodes, double g, int device, int flags, bdg_sw2d** out) {
    return guard([&] {
        if (!nodes || !out) throw arg_error("bdg_sw2d_create_from_nodes: NULL argument");
        const blitzdg::TriangleNodesProvisioner& p = nodes->prov;
        bdg_sw2d_desc d{};
        d.order = p.get_NOrder();
        d.num_elements = p.get_NumElements();
        d.Dr = p.get_Dr().data(); d.Ds = p.get_Ds().data(); d.Lift = p.get_Lift().data();
        d.Filter = nodes->hasFilter ? p.get_Filter().data() : nullptr;
        d.rx = p.get_rx().data(); d.sx = p.get_sx().data(); d.ry = p.get_ry().data(); d.sy = p.get_sy().data();
        d.nx = p.get_nx().data(); d.ny = p.get_ny().data(); d.Fscale = p.get_Fscale().data();
        d.vmapM = p.get_vmapM().data(); d.vmapP = p.get_vmapP().data();
        const auto& bc = p.get_bcMap();
        const auto it = bc.find(blitzdg::BCTag::Wall);
        if (it != bc.end()) { d.mapW = it->second.data(); d.num_wall = static_cast<int>(it->second.size()); }
        d.g = g; d.device = device; d.flags = flags;
        *out = createSolver(d);
    });
}

void bdg_sw2d_destroy(bdg_sw2d* s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    delete s;
}

int bdg_sw2d_set_state(bdg_sw2d* s, const double* h, const double* hu, const double* hv) {
    return guard([&] {
        requireFields(s, "bdg_sw2d_set_state", 3, "this solver has 4 fields, use bdg_sw2d_set_state4", {h, hu, hv});
        const double* f[] = {h, hu, hv};
        s->setFields(f);
    });
}

int bdg_sw2d_get_state(bdg_sw2d* s, double* h, double* hu, double* hv) {
    return guard([&] {
        requireFields(s, "bdg_sw2d_get_state", 3, "this solver has 4 fields, use bdg_sw2d_get_state4", {h, hu, hv});
        double* f[] = {h, hu, hv};
        s->getFields(f);
    });
}

int bdg_sw2d_output_fields(bdg_sw2d* s, const double* IM, double* eta, double* u, double* v) {
    return guard([&] {
        requireSolver(s, "bdg_sw2d_output_fields");
        s->use();
        const double* M = s->stageOutputMatrix(IM);
        double* targets[3] = {eta, u, v};
        for (int which = 0; which < 3; ++which) {
            if (!targets[which]) continue;
            // aux is scratch between steps (RHS output / RK2 intermediate)
            hipCheck(s->kt->output(s->qcur, s->hasH ? s->Hbuf.p : nullptr, M, s->aux.p, s->ld, s->numOwned, which, s->stream),
                     "sw2d_output_kernel");
            s->downloadRows(s->aux.p, targets[which], s->Np);
        }
    });
}

int bdg_sw2d_output_tracer(bdg_sw2d* s, const double* IM, double* tracer) {
    return guard([&] {
        requireSolver(s, "bdg_sw2d_output_tracer");
        if (s->nf != 4) throw arg_error("bdg_sw2d_output_tracer: the solver has no tracer field");
        if (!tracer) throw arg_error("bdg_sw2d_output_tracer: NULL output");
        s->use();
        // which = 3: field 3 divided by h, i.e. the concentration N = hN / h the reference script writes out
        hipCheck(s->kt->output(s->qcur, nullptr, s->stageOutputMatrix(IM), s->aux.p, s->ld, s->numOwned, 3, s->stream),
                 "sw2d_output_kernel");
        s->downloadRows(s->aux.p, tracer, s->Np);
    });
}

int bdg_sw2d_set_bathymetry(bdg_sw2d* s, const double* H) {
    return guard([&] {
        requireSolver(s, "bdg_sw2d_set_bathymetry");
        s->use();
        if (!H) { s->hasH = false; return; }
        if (!s->Hbuf.p) s->Hbuf.alloc(s->planeSize(), s->bytes);
        hipCheck(hipMemsetAsync(s->Hbuf.p, 0, s->Hbuf.n * sizeof(double), s->stream), "hipMemset");
        s->uploadRows(H, s->Hbuf.p, s->Np);
        s->hasH = true;
    });
}

} // extern "C"

namespace {

// what bdg_sw2d_enable_variant_b and _b4 share: the checks on the descriptor (`fn` names the caller in the messages) ...
void checkVariantB(const bdg_sw2d* s, const bdg_sw2d_vb_desc* d, const std::string& fn) {
    // partitioned solvers: allowed -- their steppers are the *_exchanged ones, which reduce the global speed over all
    // ranks before each evaluation (evaluateExchanged); the in-process group transport has no such reduction
    if (s->localGroup) throw arg_error(fn + ": not available with the in-process group transport");
    if (d->num_out < 0 || (d->num_out > 0 && !d->mapO)) throw arg_error(fn + ": bad open-boundary list");
    if (!(d->tide_period > 0.0) && d->num_out > 0) throw arg_error(fn + ": tide_period must be > 0");
    const size_t nFaceNodes = static_cast<size_t>(s->NFN) * s->K;
    for (int i = 0; i < d->num_out; ++i)
        if (d->mapO[i] < 0 || static_cast<size_t>(d->mapO[i]) >= nFaceNodes)
            throw arg_error(fn + ": open-boundary node index out of range");
}

// ... and the set-up: operator images of the source-term kernels, the bed, the sponge, the open-boundary bit masks, the tide
void enableVariantB(bdg_sw2d* s, const bdg_sw2d_vb_desc* d) {
    s->buildSourceOps();
    s->fastSources = s->N <= bdg_sw2d::kUnrolledSourcesMaxOrder && !env::rolledSources();
    if (s->N > bdg_sw2d::kUnrolledSourcesMaxOrder && !env::rolledSources()) {
        s->buildMfma2SourceOps();
        s->mfmaSources = true;
    }
    if (s->fastSources) s->buildFilterT();
    if (!s->Hbuf.p) s->Hbuf.alloc(s->planeSize(), s->bytes);
    hipCheck(hipMemsetAsync(s->Hbuf.p, 0, s->Hbuf.n * sizeof(double), s->stream), "hipMemset");
    // padding lanes are never computed, but give them a positive depth anyway
    s->uploadRows(d->H, s->Hbuf.p, s->Np);
    s->hasH = true;
    s->vb.H = s->Hbuf.p;
    s->vb.Hx = s->uploadPlane(d->Hx, s->HxBuf);
    s->vb.Hy = s->uploadPlane(d->Hy, s->HyBuf);
    s->vb.sponge = s->uploadPlane(d->sponge, s->spongeBuf);
    // open-boundary face nodes as one bit mask per element, in device slots
    std::vector<int> mask(static_cast<size_t>(s->ld), 0);
    for (int i = 0; i < d->num_out; ++i) {
        const int k = d->mapO[i] / s->NFN, j = d->mapO[i] % s->NFN;
        mask[s->permHost.empty() ? k : s->permHost[k]] |= 1 << j;
    }
    if (!s->obcBuf.p) s->obcBuf.alloc(static_cast<size_t>(s->ld), s->bytes);
    hipCheck(hipMemcpy(s->obcBuf.p, mask.data(), mask.size() * sizeof(int), hipMemcpyHostToDevice), "open-boundary upload");
    s->vb.obc = s->obcBuf.p;
    if (!s->lamBuf.p) s->lamBuf.alloc(1, s->bytes);
    if (!s->lamPair.p) s->lamPair.alloc(2, s->bytes);
    s->lamStateFor = nullptr;
    if (!s->vbPartials.p) s->vbPartials.alloc(static_cast<size_t>((s->K + 255) / 256), s->bytes);
    s->vb.lam = s->lamBuf.p;
    s->vb.fcor = d->coriolis;
    s->vb.cd = d->drag;
    s->tideAmp = d->tide_amplitude;
    s->tidePeriod = d->tide_period > 0.0 ? d->tide_period : 1.0;
    s->tideRamp = d->tide_ramp;
    s->variantB = true;
}

// VnOps image (row i = {Dr[i][m], Ds[i][m]} interleaved, then Lift[i][j]) of the tracer pass's general form
std::vector<double> rowOpsImage(const double* Dr, const double* Ds, const double* Lift, int Np, int NFN) {
    const int row = 2 * Np + NFN;
    std::vector<double> img(static_cast<size_t>(row) * Np);
    for (int i = 0; i < Np; ++i) {
        for (int m = 0; m < Np; ++m) {
            img[static_cast<size_t>(i) * row + 2 * m] = Dr[static_cast<size_t>(i) * Np + m];
            img[static_cast<size_t>(i) * row + 2 * m + 1] = Ds[static_cast<size_t>(i) * Np + m];
        }
        for (int j = 0; j < NFN; ++j) img[static_cast<size_t>(i) * row + 2 * Np + j] = Lift[static_cast<size_t>(i) * NFN + j];
    }
    return img;
}

} // namespace

extern "C" {

int bdg_sw2d_enable_variant_b(bdg_sw2d* s, const bdg_sw2d_vb_desc* d) {
    return guard([&] {
        requireSolver(s, "bdg_sw2d_enable_variant_b");
        if (!d || !d->H || !d->Hx || !d->Hy) throw arg_error("bdg_sw2d_enable_variant_b: H, Hx and Hy are required");
        if (s->nf != 3 || s->variantD)
            throw arg_error("bdg_sw2d_enable_variant_b: the solver was created with tracer / variant-D sources");
        checkVariantB(s, d, "bdg_sw2d_enable_variant_b");
        s->use();
        enableVariantB(s, d);
    });
}

int bdg_sw2d_enable_variant_b4(bdg_sw2d* s, const bdg_sw2d_vb_desc* d, const double* n_open, int n_open_count) {
    return guard([&] {
        const std::string fn = "bdg_sw2d_enable_variant_b4";
        requireSolver(s, fn.c_str());
        if (!d || !d->H || !d->Hx || !d->Hy) throw arg_error(fn + ": H, Hx and Hy are required");
        if (s->nf != 4) throw arg_error(fn + ": the solver was created with three fields; the tracer needs four (num_fields = 4)");
        if (s->vd.sources) throw arg_error(fn + ": the solver was created with variant-D sources; variant B brings its own");
        if (s->variantB) throw arg_error(fn + ": variant B is already enabled on this solver; the call is made once");
        if (s->evaluated)
            throw arg_error(fn + ": the solver has evaluated a right-hand side already; variant B is enabled before the first evaluation");
        checkVariantB(s, d, fn);
        // (without an open-boundary node no concentration is read: a count of 0 is then num_out, and n_open may be NULL)
        const bool none = d->num_out == 0 && n_open_count == 0;
        if (!none && (!n_open || (n_open_count != 1 && n_open_count != d->num_out)))
            throw arg_error(fn + ": n_open must hold 1 value or one per open-boundary node (num_out)");
        const bdg_dev::Vb4KernelTable* kt4 = bdg_dev::vb4_kernel_table(s->N);
        if (!kt4) throw arg_error(fn + ": no tracer-pass kernels compiled for this order");
        s->use();
        bdg_dev::VbTracerParams tp{};
        if (none || n_open_count == 1) { // (also a single open node given per node)
            tp.nOpenC = none ? 0.0 : n_open[0];
        } else {
            // per element in DEVICE slots (as the bit masks of the open boundary are stored): the values of its open nodes in the
            // order of its face nodes, from base[slot] on; the last entry of a node listed twice wins, as an assignment through
            // mapO does
            struct Entry { int slot, node, at; };
            std::vector<Entry> entries(static_cast<size_t>(d->num_out));
            for (int i = 0; i < d->num_out; ++i) {
                const int k = d->mapO[i] / s->NFN;
                entries[static_cast<size_t>(i)] = {s->permHost.empty() ? k : s->permHost[k], d->mapO[i] % s->NFN, i};
            }
            std::sort(entries.begin(), entries.end(), [](const Entry& a, const Entry& b) {
                return a.slot != b.slot ? a.slot < b.slot : (a.node != b.node ? a.node < b.node : a.at < b.at);
            });
            std::vector<int> base(static_cast<size_t>(s->ld), 0);
            std::vector<double> vals;
            for (size_t e = 0; e < entries.size(); ++e) {
                const bool again = e > 0 && entries[e - 1].slot == entries[e].slot && entries[e - 1].node == entries[e].node;
                if (again) { vals.back() = n_open[entries[e].at]; continue; }
                if (e == 0 || entries[e - 1].slot != entries[e].slot) base[static_cast<size_t>(entries[e].slot)] = static_cast<int>(vals.size());
                vals.push_back(n_open[entries[e].at]);
            }
            if (vals.empty()) vals.push_back(0.0);
            s->openBase.upload(base, s->bytes, "open-boundary tracer index upload");
            s->openN.upload(vals, s->bytes, "open-boundary tracer upload");
            tp.openBase = s->openBase.p;
            tp.openN = s->openN.p;
        }
        if (s->affine && !(s->N <= bdg_sw2d::kUnrolledSourcesMaxOrder && !env::rolledSources() && kt4->unrolled)) {
            s->opsRow.upload(rowOpsImage(s->hostDr.data(), s->hostDs.data(), s->hostLift.data(), s->Np, s->NFN), s->bytes, "tracer row ops upload");
            if (!s->hostFilter.empty())
                s->opsRowFiltered.upload(rowOpsImage(s->hostFDr.data(), s->hostFDs.data(), s->hostFLift.data(), s->Np, s->NFN), s->bytes,
                                         "filtered tracer row ops upload");
        }
        enableVariantB(s, d);
        // from here on the solver is variant B with a tracer: the three-field variant-B launches, each followed by the tracer pass
        s->variantD = false;
        s->kt4 = kt4;
        s->vb4 = tp;
        s->variantB4 = true;
    });
}

int bdg_sw2d_enable_tracer_diffusion(bdg_sw2d* s, const bdg_sw2d_diffusion_desc* d) {
    return guard([&] {
        const std::string fn = "bdg_sw2d_enable_tracer_diffusion";
        requireSolver(s, fn.c_str());
        if (!d) throw arg_error(fn + ": NULL descriptor");
        if (s->nf != 4) throw arg_error(fn + ": the solver was created with three fields; the tracer needs four (num_fields = 4)");
        if (s->diffusion) throw arg_error(fn + ": tracer diffusion is already enabled on this solver; the call is made once");
        if (s->evaluated)
            throw arg_error(fn + ": the solver has evaluated a right-hand side already; diffusion is enabled before the first evaluation");
        if (s->partitionSet) throw arg_error(fn + ": the solver has a partition set; the diffusion passes cover a single domain only");
        if (!(d->decay >= 0.0) || !std::isfinite(d->decay)) throw arg_error(fn + ": decay must be finite and >= 0");
        const size_t nodesTotal = static_cast<size_t>(s->Np) * s->K;
        double kmax = d->kappa;
        if (d->kappa_field) {
            kmax = 0.0;
            for (size_t i = 0; i < nodesTotal; ++i) {
                const double v = d->kappa_field[i];
                if (!(v >= 0.0) || !std::isfinite(v)) throw arg_error(fn + ": kappa must be finite and >= 0 at every node");
                kmax = std::max(kmax, v);
            }
        } else if (!(d->kappa >= 0.0) || !std::isfinite(d->kappa)) {
            throw arg_error(fn + ": kappa must be finite and >= 0");
        }
        if (d->source)
            for (size_t i = 0; i < nodesTotal; ++i)
                if (!std::isfinite(d->source[i])) throw arg_error(fn + ": the source must be finite at every node");
        const bdg_dev::DiffusionKernelTable* ktd = bdg_dev::diffusion_kernel_table(s->N);
        if (!ktd) throw arg_error(fn + ": no diffusion kernels compiled for this order");
        s->use();
        bdg_dev::DiffusionParams dp{};
        dp.kappa = d->kappa;
        dp.decay = d->decay;
        dp.kappaField = s->uploadPlane(d->kappa_field, s->difKappa);
        dp.source = s->uploadPlane(d->source, s->difSource);
        const size_t pl = s->planeSize();
        s->difScratch.alloc((s->hasFilter ? 3 : 2) * pl, s->bytes);
        hipCheck(hipMemsetAsync(s->difScratch.p, 0, s->difScratch.n * sizeof(double), s->stream), "hipMemset");
        dp.flux = s->difScratch.p;
        dp.raw = s->hasFilter ? s->difScratch.p + 2 * pl : nullptr;
        s->difOps.upload(rowOpsImage(s->hostDr.data(), s->hostDs.data(), s->hostLift.data(), s->Np, s->NFN), s->bytes, "diffusion row ops upload");
        if (s->hasFilter) {
            s->difFilter.upload(s->hostFilter, s->bytes, "diffusion filter upload");
            if (s->affine)
                s->difOpsFiltered.upload(rowOpsImage(s->hostFDr.data(), s->hostFDs.data(), s->hostFLift.data(), s->Np, s->NFN), s->bytes,
                                         "filtered diffusion row ops upload");
        }
        const double fmax = s->maxFscale();
        const double n1 = static_cast<double>(s->N + 1);
        s->difDt = kmax > 0.0 ? bdg_sw2d::kDiffusionDtConstant / (kmax * n1 * n1 * n1 * n1 * fmax * fmax) : std::numeric_limits<double>::infinity();
        s->ktd = ktd;
        s->dif = dp;
        s->diffusion = true;
    });
}

int bdg_sw2d_diffusion_dt(const bdg_sw2d* s, double* dt_diff) {
    return guard([&] {
        requireSolver(s, "bdg_sw2d_diffusion_dt");
        if (!dt_diff) throw arg_error("bdg_sw2d_diffusion_dt: NULL argument");
        if (!s->diffusion) throw arg_error("bdg_sw2d_diffusion_dt: tracer diffusion is not enabled");
        *dt_diff = s->difDt;
    });
}

int bdg_sw2d_enable_viscosity(bdg_sw2d* s, const bdg_sw2d_viscosity_desc* d) {
    return guard([&] {
        const std::string fn = "bdg_sw2d_enable_viscosity";
        requireSolver(s, fn.c_str());
        if (!d) throw arg_error(fn + ": NULL descriptor");
        if (s->viscosity) throw arg_error(fn + ": eddy viscosity is already enabled on this solver; the call is made once");
        if (s->evaluated)
            throw arg_error(fn + ": the solver has evaluated a right-hand side already; viscosity is enabled before the first evaluation");
        if (s->partitionSet) throw arg_error(fn + ": the solver has a partition set; the viscosity passes cover a single domain only");
        if (!(d->smagorinsky >= 0.0) || !std::isfinite(d->smagorinsky)) throw arg_error(fn + ": smagorinsky must be finite and >= 0");
        const size_t nodesTotal = static_cast<size_t>(s->Np) * s->K;
        double numax = d->nu;
        if (d->nu_field) {
            numax = 0.0;
            for (size_t i = 0; i < nodesTotal; ++i) {
                const double v = d->nu_field[i];
                if (!(v >= 0.0) || !std::isfinite(v)) throw arg_error(fn + ": nu must be finite and >= 0 at every node");
                numax = std::max(numax, v);
            }
        } else if (!(d->nu >= 0.0) || !std::isfinite(d->nu)) {
            throw arg_error(fn + ": nu must be finite and >= 0");
        }
        if (numax == 0.0 && d->smagorinsky == 0.0) throw arg_error(fn + ": nu and smagorinsky are both zero: there is no viscosity to enable");
        const bdg_dev::ViscosityKernelTable* ktv = bdg_dev::viscosity_kernel_table(s->N);
        if (!ktv) throw arg_error(fn + ": no viscosity kernels compiled for this order");
        s->use();
        const double n1 = static_cast<double>(s->N + 1);
        bdg_dev::ViscosityParams vp{};
        vp.nu = d->nu_field ? 0.0 : d->nu;
        vp.cs2d2 = d->smagorinsky * d->smagorinsky * 2.0 / (n1 * n1);
        vp.nuField = s->uploadPlane(d->nu_field, s->visNu0);
        const size_t pl = s->planeSize();
        const bool rawPlanes = s->hasFilter && !s->affine;
        s->visScratch.alloc((rawPlanes ? 7 : 5) * pl, s->bytes);
        hipCheck(hipMemsetAsync(s->visScratch.p, 0, s->visScratch.n * sizeof(double), s->stream), "hipMemset");
        vp.flux = s->visScratch.p;
        s->visNuPlane = s->visScratch.p + 4 * pl;
        vp.raw = rawPlanes ? s->visScratch.p + 5 * pl : nullptr;
        s->visRed.alloc(bdg_dev::kViscosityMaxBlocks + 1, s->bytes);
        s->visOps.upload(rowOpsImage(s->hostDr.data(), s->hostDs.data(), s->hostLift.data(), s->Np, s->NFN), s->bytes, "viscosity row ops upload");
        if (s->hasFilter) {
            if (s->affine)
                s->visOpsFiltered.upload(rowOpsImage(s->hostFDr.data(), s->hostFDs.data(), s->hostFLift.data(), s->Np, s->NFN), s->bytes,
                                         "filtered viscosity row ops upload");
            else
                s->visFilter.upload(s->hostFilter, s->bytes, "viscosity filter upload");
        }
        const double fmax = s->maxFscale();
        s->visDtScale = bdg_sw2d::kViscosityDtConstant / (n1 * n1 * n1 * n1 * fmax * fmax);
        s->visNu0Max = numax;
        s->visSmagorinsky = d->smagorinsky > 0.0;
        s->ktv = ktv;
        s->vis = vp;
        s->viscosity = true;
    });
}

int bdg_sw2d_viscosity_dt(bdg_sw2d* s, double* dt_visc) {
    return guard([&] {
        requireSolver(s, "bdg_sw2d_viscosity_dt");
        if (!dt_visc) throw arg_error("bdg_sw2d_viscosity_dt: NULL argument");
        if (!s->viscosity) throw arg_error("bdg_sw2d_viscosity_dt: eddy viscosity is not enabled");
        s->use();
        *dt_visc = s->viscosityDt();
    });
}

int bdg_sw2d_eddy_viscosity(bdg_sw2d* s, double* nu) {
    return guard([&] {
        requireSolver(s, "bdg_sw2d_eddy_viscosity");
        if (!nu) throw arg_error("bdg_sw2d_eddy_viscosity: NULL argument");
        if (!s->viscosity) throw arg_error("bdg_sw2d_eddy_viscosity: eddy viscosity is not enabled");
        s->use();
        s->launchEddyViscosity();
        s->downloadRows(s->visNuPlane, nu, s->Np);
    });
}

int bdg_sw2d_set_time(bdg_sw2d* s, double t) {
    return guard([&] {
        requireSolver(s, "bdg_sw2d_set_time");
        s->timeNow = t;
    });
}

int bdg_sw2d_get_time(const bdg_sw2d* s, double* t) {
    return guard([&] {
        requireSolver(s, "bdg_sw2d_get_time");
        if (!t) throw arg_error("bdg_sw2d_get_time: NULL argument");
        *t = s->timeNow;
    });
}

int bdg_sw2d_global_speed(bdg_sw2d* s, double* lam) {
    return guard([&] {
        requireSolver(s, "bdg_sw2d_global_speed");
        if (!s->variantB || !lam) throw arg_error("bdg_sw2d_global_speed: variant B is not enabled");
        s->use();
        hipCheck(hipMemcpyAsync(lam, s->vb.lam ? s->vb.lam : s->lamBuf.p, sizeof(double), hipMemcpyDeviceToHost, s->stream),
                 "D2H copy");
        hipCheck(hipStreamSynchronize(s->stream), "sync");
    });
}

int bdg_sw2d_rhs(bdg_sw2d* s, const double* h, const double* hu, const double* hv, double* r1, double* r2,
                 double* r3, int filter) {
    return guard([&] {
        requireFields(s, "bdg_sw2d_rhs", 3, "this solver has 4 fields, use bdg_sw2d_rhs4", {h, hu, hv, r1, r2, r3});
        const double* in[] = {h, hu, hv};
        double* out[] = {r1, r2, r3};
        s->rhsFields(in, out, filter != 0);
    });
}

int bdg_sw2d_num_fields(const bdg_sw2d* s) { return s ? s->nf : -1; }

int bdg_sw2d_set_state4(bdg_sw2d* s, const double* h, const double* hu, const double* hv, const double* hN) {
    return guard([&] {
        requireFields(s, "bdg_sw2d_set_state4", 4, "the solver was created with 3 fields", {h, hu, hv, hN});
        const double* f[] = {h, hu, hv, hN};
        s->setFields(f);
    });
}

int bdg_sw2d_get_state4(bdg_sw2d* s, double* h, double* hu, double* hv, double* hN) {
    return guard([&] {
        requireFields(s, "bdg_sw2d_get_state4", 4, "the solver was created with 3 fields", {h, hu, hv, hN});
        double* f[] = {h, hu, hv, hN};
        s->getFields(f);
    });
}

int bdg_sw2d_rhs4(bdg_sw2d* s, const double* h, const double* hu, const double* hv, const double* hN, double* r1,
                  double* r2, double* r3, double* r4, int filter) {
    return guard([&] {
        requireFields(s, "bdg_sw2d_rhs4", 4, "the solver was created with 3 fields", {h, hu, hv, hN, r1, r2, r3, r4});
        const double* in[] = {h, hu, hv, hN};
        double* out[] = {r1, r2, r3, r4};
        s->rhsFields(in, out, filter != 0);
    });
}

int bdg_sw2d_lserk4_stages(bdg_sw2d* s, double dt, int num_stages) {
    return guard([&] {
        requireSolver(s, "bdg_sw2d_lserk4_stages");
        if (num_stages < 0) throw arg_error("bdg_sw2d_lserk4_stages: num_stages < 0");
        s->monitorReserve(s->lserkSteps(num_stages), "bdg_sw2d_lserk4_stages");
        s->drifterReserve(s->lserkSteps(num_stages), "bdg_sw2d_lserk4_stages");
        s->use();
        s->dtStage = dt;
        s->lserkStagesMonitored(num_stages);
    });
}

int bdg_sw2d_step_lserk4(bdg_sw2d* s, double dt, int num_steps) {
    return guard([&] {
        requireSolver(s, "bdg_sw2d_step_lserk4");
        if (num_steps < 0) throw arg_error("bdg_sw2d_step_lserk4: num_steps < 0");
        if (s->stageCount % blitzdg::LSERK4::numStages != 0)
            throw arg_error("bdg_sw2d_step_lserk4: a previous step was left part-way through its stages");
        s->monitorReserve(num_steps, "bdg_sw2d_step_lserk4");
        s->drifterReserve(num_steps, "bdg_sw2d_step_lserk4");
        s->use();
        s->dtStage = dt;
        s->lserkStagesMonitored(num_steps * blitzdg::LSERK4::numStages);
    });
}

int bdg_sw2d_step_rk2(bdg_sw2d* s, double dt, int num_steps, int filter) {
    return stepCall(s, "bdg_sw2d_step_rk2", dt, num_steps, [&] { s->rk2Step(dt, filter != 0, bdg_sw2d::Eval::Whole); });
}

int bdg_sw2d_step_ssprk2(bdg_sw2d* s, double dt, int num_steps, int filter, double sponge_coeff) {
    return stepCall(s, "bdg_sw2d_step_ssprk2", dt, num_steps,
                    [&] { s->sspRk2Step(dt, filter != 0, sponge_coeff, bdg_sw2d::Eval::Whole); });
}

int bdg_sw2d_step_rk2_exchanged(bdg_sw2d* s, double dt, int num_steps, int filter) {
    return stepCall(s, "bdg_sw2d_step_rk2_exchanged", dt, num_steps,
                    [&] { s->rk2Step(dt, filter != 0, bdg_sw2d::Eval::Exchanged); });
}

int bdg_sw2d_step_ssprk2_exchanged(bdg_sw2d* s, double dt, int num_steps, int filter, double sponge_coeff) {
    return stepCall(s, "bdg_sw2d_step_ssprk2_exchanged", dt, num_steps,
                    [&] { s->sspRk2Step(dt, filter != 0, sponge_coeff, bdg_sw2d::Eval::Exchanged); });
}

int bdg_sw2d_compute_dt(bdg_sw2d* s, double cfl, double* dt, double* eta_max) {
    return guard([&] {
        requireSolver(s, "bdg_sw2d_compute_dt");
        s->use();
        double r[2];
        s->reduceDt(r);
        if (eta_max) *eta_max = r[1];
        if (dt) *dt = cfl / ((s->N + 1) * (s->N + 1) * 0.5 * r[0]);
        if (dt && s->diffusion) *dt = std::min(*dt, cfl * s->difDt);
        if (dt && s->viscosity) *dt = std::min(*dt, cfl * s->viscosityDt());
        if (std::isnan(r[0]) || std::isnan(r[1]) || std::fabs(r[1]) > 1e8)
            throw unstable_error("A numerical instability has occurred!");
    });
}

int bdg_sw2d_run_adaptive(bdg_sw2d* s, double cfl, double final_time, int max_steps, int filter, double* t_inout,
                          double* dt_inout, int* steps_done) {
    int done = 0;
    const int rc = guard([&] {
        requireSolver(s, "bdg_sw2d_run_adaptive");
        if (!t_inout || !dt_inout) throw arg_error("bdg_sw2d_run_adaptive: NULL argument");
        s->use();
        double t = *t_inout, dt = *dt_inout;
        while (t < final_time && (max_steps <= 0 || done < max_steps)) {
            // the number of steps is not known in advance: room for this step's record is checked before the step is launched
            s->monitorReserve(1, "bdg_sw2d_run_adaptive");
            s->drifterReserve(1, "bdg_sw2d_run_adaptive");
            s->rk2Step(dt, filter != 0, bdg_sw2d::Eval::Whole);
            s->stepDone(dt);
            double r[2];
            s->reduceDt(r);
            if (std::isnan(r[0]) || std::isnan(r[1]) || std::fabs(r[1]) > 1e8)
                throw unstable_error("A numerical instability has occurred!");
            dt = cfl / ((s->N + 1) * (s->N + 1) * 0.5 * r[0]);
            if (s->diffusion) dt = std::min(dt, cfl * s->difDt);
            if (s->viscosity) dt = std::min(dt, cfl * s->viscosityDt());
            t += dt;
            ++done;
            *t_inout = t;
            *dt_inout = dt;
        }
    });
    if (steps_done) *steps_done = done;
    return rc;
}

int bdg_sw2d_synchronize(bdg_sw2d* s) {
    return guard([&] {
        requireSolver(s, "bdg_sw2d_synchronize");
        s->use();
        hipCheck(hipStreamSynchronize(s->stream), "hipStreamSynchronize");
        s->checkSyncError();
    });
}

int bdg_sw2d_time_lserk4_stages(bdg_sw2d* s, double dt, int num_stages, float* ms_per_launch) {
    return guard([&] {
        requireSolver(s, "bdg_sw2d_time_lserk4_stages");
        if (num_stages < 1 || !ms_per_launch) throw arg_error("bdg_sw2d_time_lserk4_stages: bad argument");
        s->use();
        s->dtStage = dt;
        *ms_per_launch = bdg_dev::timePerRun(s->stream, num_stages, [&] { s->launchLserkStage(); });
    });
}

int bdg_sw2d_set_partition(bdg_sw2d* s, int num_interior, int num_owned, const int* send_elements, int num_send) {
    return guard([&] {
        requireSolver(s, "bdg_sw2d_set_partition");
        if (s->diffusion)
            throw arg_error("bdg_sw2d_set_partition: the solver has tracer diffusion, whose passes cover a single domain only");
        if (s->viscosity)
            throw arg_error("bdg_sw2d_set_partition: the solver has eddy viscosity, whose passes cover a single domain only");
        if (s->drf.on)
            throw arg_error("bdg_sw2d_set_partition: the solver has drifters, which do not migrate between ranks (single domain only)");
        if (s->fst.on)
            throw arg_error("bdg_sw2d_set_partition: the solver has field statistics, which cover a single domain only");
        if (!s->permHost.empty())
            throw arg_error("bdg_sw2d_set_partition: the solver renumbered its elements; create it with BDG_SW2D_KEEP_ORDER");
        if (num_interior < 0 || num_interior > num_owned || num_owned > s->K || num_send < 0 ||
            (num_send > 0 && !send_elements))
            throw arg_error("bdg_sw2d_set_partition: need 0 <= num_interior <= num_owned <= K");
        for (int i = 0; i < num_send; ++i)
            if (send_elements[i] < 0 || send_elements[i] >= num_owned)
                throw arg_error("bdg_sw2d_set_partition: send element is not an owned element");
        s->use();
        s->sendSlots.release();
        if (num_send > 0) {
            s->sendSlots.alloc(num_send, s->bytes);
            hipCheck(hipMemcpy(s->sendSlots.p, send_elements, sizeof(int) * num_send, hipMemcpyHostToDevice),
                     "send list upload");
        }
        s->numInterior = num_interior;
        s->numOwned = num_owned;
        s->numSend = num_send;
        s->partitionSet = true;
        // the first interior element with a partition-boundary neighbour: interior tiles from there on read what the boundary
        // launch of the previous stage writes (and overwrite what it reads); tiles before it depend on interior elements only
        {
            const int NFN = s->NFN;
            std::vector<int> vm(static_cast<size_t>(NFN) * s->ld);
            hipCheck(hipMemcpy(vm.data(), s->vmapP.p, vm.size() * sizeof(int), hipMemcpyDeviceToHost), "gather table download");
            int ring = num_interior;
            for (int jf = 0; jf < NFN && ring > 0; ++jf) {
                const int* row = vm.data() + static_cast<size_t>(jf) * s->ld;
                for (int k = 0; k < ring; ++k) {
                    const int id = row[k];
                    const long long slot = static_cast<long long>(id < 0 ? -(id + 1) : id) % s->ld;
                    if (slot >= num_interior && slot < num_owned) { ring = k; break; }
                }
            }
            s->ringBegin = ring;
        }
        // for the boundary kernel with the halo staging folded in: the (up to three) send records of each
        // partition-boundary element
        const int nB = num_owned - num_interior;
        std::vector<int> of(static_cast<size_t>(3) * std::max(nB, 1), -1);
        bool ok = true;
        for (int r = 0; r < num_send && ok; ++r) {
            const int b = send_elements[r] - num_interior;
            if (b < 0) { ok = false; break; }
            int t = 0;
            while (t < 3 && of[3 * b + t] >= 0) ++t;
            if (t == 3) { ok = false; break; }
            of[3 * b + t] = r;
        }
        s->haloSendOf.release();
        s->haloFusable = ok && nB > 0;
        if (s->haloFusable) s->haloSendOf.upload(of, s->bytes, "send table upload");
    });
}

int bdg_sw2d_halo_doubles_per_element(const bdg_sw2d* s) { return s ? s->nf * s->Np : -1; }

int bdg_sw2d_halo_pack(bdg_sw2d* s, void* send_buffer) {
    return guard([&] {
        requireSolver(s, "bdg_sw2d_halo_pack");
        if (s->numSend == 0) return;
        if (!send_buffer) throw arg_error("bdg_sw2d_halo_pack: buffer is NULL");
        s->use();
        s->launchPack(static_cast<double*>(send_buffer));
    });
}

int bdg_sw2d_halo_unpack(bdg_sw2d* s, const void* recv_buffer) {
    return guard([&] {
        requireSolver(s, "bdg_sw2d_halo_unpack");
        if (s->K == s->numOwned) return;
        if (!recv_buffer) throw arg_error("bdg_sw2d_halo_unpack: buffer is NULL");
        s->use();
        s->launchUnpack(static_cast<const double*>(recv_buffer));
    });
}

int bdg_sw2d_lserk4_stage_part(bdg_sw2d* s, double dt, int part) {
    return guard([&] {
        requireSolver(s, "bdg_sw2d_lserk4_stage_part");
        if (part < 0 || part > 2) throw arg_error("bdg_sw2d_lserk4_stage_part: part must be 0, 1 or 2");
        s->use();
        s->dtStage = dt;
        s->launchLserkStage(part);
    });
}

int bdg_sw2d_rhs_resident(bdg_sw2d* s, double* r1, double* r2, double* r3) {
    return guard([&] {
        requireSolver(s, "bdg_sw2d_rhs_resident");
        if (s->nf != 3) throw arg_error("bdg_sw2d_rhs_resident: three-field solvers only");
        if (!r1 || !r2 || !r3) throw arg_error("bdg_sw2d_rhs_resident: NULL output");
        s->use();
        double* out[] = {r1, r2, r3};
        s->launchRhs(s->qcur, s->aux.p, false);
        s->downloadFields(s->aux.p, out);
    });
}

int bdg_comm_unique_id(void* id_out, int capacity) {
    return guard([&] {
        if (!id_out || capacity < static_cast<int>(sizeof(ncclUniqueId)))
            throw arg_error("bdg_comm_unique_id: need a buffer of at least 128 bytes");
        ncclUniqueId id;
        ncclCheck(rccl().GetUniqueId(&id), "ncclGetUniqueId");
        std::memcpy(id_out, &id, sizeof(id));
    });
}

int bdg_sw2d_comm_init(bdg_sw2d* s, int rank, int world, const void* unique_id, const int* peer_ranks,
                       const int* send_start, const int* send_count, const int* recv_start, const int* recv_count,
                       int num_peers) {
    return guard([&] {
        requireSolver(s, "bdg_sw2d_comm_init");
        if (!unique_id || world < 1 || rank < 0 || rank >= world || num_peers < 0 ||
            (num_peers > 0 && (!peer_ranks || !send_start || !send_count || !recv_start || !recv_count)))
            throw arg_error("bdg_sw2d_comm_init: bad argument");
        if (s->halo.comm) throw arg_error("bdg_sw2d_comm_init: communicator already initialised");
        if (s->fst.on) throw arg_error("bdg_sw2d_comm_init: the solver has field statistics, which cover a single domain only");
        const int ghosts = s->K - s->numOwned;
        std::vector<bdg_halo::Peer> peers = bdg_halo::parsePeers("bdg_sw2d", "comm_init", peer_ranks, send_start, send_count, recv_start,
                                                                 recv_count, num_peers, s->numSend, ghosts, world);
        s->use();
        const size_t rows = static_cast<size_t>(s->nf) * s->Np;
        s->halo.connect(unique_id, rank, world, rows, s->numSend, ghosts, s->bytes);
        s->halo.peers = peers;
        hipCheck(hipMemset(s->halo.sendBuf.p, 0, s->halo.sendBuf.n * sizeof(double)), "hipMemset");
        hipCheck(hipMemset(s->halo.recvBuf.p, 0, s->halo.recvBuf.n * sizeof(double)), "hipMemset");
        // These four events only order kernels of the two streams of THIS device against each other (a kernel's own
        // end-of-kernel release is device-wide, and data from another GPU is made visible by the RCCL kernel that received
        // it, on the stream that then runs the boundary kernel): the system-scope fence of a default event record is not
        // needed and costs 2-3 us per stage (8-way rehearsal, N=4: 0.056 ms per stage without, 0.058-0.059 with).
        // tests/test_dist_gpu.py::test_loopback_rccl_result_is_independent_of_event_flags_and_halo_staging compares both
        // settings bit for bit through real RCCL; BDG_SW2D_EVENT_FENCE=1 (or BDG_SW2D_EVENT_NOFENCE=0) restores the fence.
        const unsigned evFlags = hipEventDisableTiming | (env::eventFence() ? 0u : hipEventDisableSystemFence);
        for (hipEvent_t* e : {&s->evA[0], &s->evA[1], &s->evB[0], &s->evB[1]})
            hipCheck(hipEventCreateWithFlags(e, evFlags), "hipEventCreate");
        s->syncBuf.alloc(8, s->bytes);
        hipCheck(hipMemset(s->syncBuf.p, 0, 8 * sizeof(unsigned long long)), "hipMemset");
        s->expectRing = s->expectStrip = 0;
        // The first send / receive between two ranks sets their connection up (host side, inside ncclGroupEnd, and only as fast as the
        // slower of the two gets there). Do that HERE, where every rank is anyway and nothing is in flight: one double each way with
        // every neighbour, in the buffers and with the pairing of the stage exchange. Otherwise it would happen in the first exchanged
        // stage, behind interior launches whose ring tiles wait -- with a bound -- for the launches queued behind that exchange.
        if (!s->halo.peers.empty() && !env::noCommWarmup()) {
            s->halo.sendRecv(s->halo.stream, rows, 1);
            hipCheck(hipStreamSynchronize(s->halo.stream), "hipStreamSynchronize");
        }
    });
}

// ---- in-process group: every part of the split lives in this process (one per GPU of the node, or
// several on one GPU); the exchange is a device-to-device copy from the neighbour's send buffer. The
// schedule is the two-chain pipeline of launchLserkStagesExchanged with the RCCL group replaced by
//   B_r: wait packed(p) -> copy p.send[range towards r] -> r.recv[range from p]   for every neighbour p
// and the send buffer of a part protected by copied(r) of every neighbour before its next pack.
int bdg_sw2d_local_peers(bdg_sw2d* s, int rank, const int* peer_ranks, const int* send_start, const int* send_count,
                         const int* recv_start, const int* recv_count, int num_peers) {
    return guard([&] {
        requireSolver(s, "bdg_sw2d_local_peers");
        if (rank < 0 || num_peers < 0 ||
            (num_peers > 0 && (!peer_ranks || !send_start || !send_count || !recv_start || !recv_count)))
            throw arg_error("bdg_sw2d_local_peers: bad argument");
        if (s->halo.comm || s->localGroup) throw arg_error("bdg_sw2d_local_peers: a transport is already initialised");
        if (s->fst.on) throw arg_error("bdg_sw2d_local_peers: the solver has field statistics, which cover a single domain only");
        const int ghosts = s->K - s->numOwned;
        // (no world here: any other rank of the group)
        std::vector<bdg_halo::Peer> peers = bdg_halo::parsePeers("bdg_sw2d", "local_peers", peer_ranks, send_start, send_count, recv_start,
                                                                 recv_count, num_peers, s->numSend, ghosts, INT_MAX, rank);
        s->use();
        s->halo.rank = rank;
        s->halo.peers = peers;
        s->halo.open(static_cast<size_t>(s->nf) * s->Np, s->numSend, ghosts, s->bytes);
        for (hipEvent_t* e : {&s->evA[0], &s->evA[1], &s->evB[0], &s->evB[1], &s->evPacked[0], &s->evPacked[1],
                              &s->evCopied[0], &s->evCopied[1]})
            hipCheck(hipEventCreateWithFlags(e, hipEventDisableTiming), "hipEventCreate");
        s->localGroup = true;
    });
}

int bdg_sw2d_group_lserk4_stages(bdg_sw2d** parts, int num_parts, double dt, int num_stages) {
    return guard([&] {
        if (!parts || num_parts < 1 || num_stages < 0) throw arg_error("bdg_sw2d_group_lserk4_stages: bad argument");
        for (int r = 0; r < num_parts; ++r) {
            if (!parts[r] || !parts[r]->localGroup || parts[r]->halo.rank != r)
                throw arg_error("bdg_sw2d_group_lserk4_stages: parts[r] must be the part given rank r in bdg_sw2d_local_peers");
            for (const bdg_halo::Peer& pr : parts[r]->halo.peers) {
                if (pr.rank >= num_parts) throw arg_error("bdg_sw2d_group_lserk4_stages: peer rank outside the group");
                bool matched = false;
                for (const bdg_halo::Peer& back : parts[pr.rank]->halo.peers)
                    matched = matched || (back.rank == r && back.sendCount == pr.recvCount && back.recvCount == pr.sendCount);
                if (!matched) throw arg_error("bdg_sw2d_group_lserk4_stages: neighbour tables of two parts do not match");
            }
            if (parts[r]->nf != parts[0]->nf || parts[r]->Np != parts[0]->Np)
                throw arg_error("bdg_sw2d_group_lserk4_stages: parts differ in order / field count");
        }
        if (num_stages == 0) return;
        for (int r = 0; r < num_parts; ++r)          // direct access between the GPUs that exchange ghosts
            for (const bdg_halo::Peer& pr : parts[r]->halo.peers)
                if (parts[pr.rank]->device != parts[r]->device) {
                    parts[r]->use();
                    const hipError_t e = hipDeviceEnablePeerAccess(parts[pr.rank]->device, 0);
                    if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) hipCheck(e, "hipDeviceEnablePeerAccess");
                    (void)hipGetLastError();
                }
        const size_t rows = static_cast<size_t>(parts[0]->nf) * parts[0]->Np;
        for (int r = 0; r < num_parts; ++r) {
            bdg_sw2d* s = parts[r];
            s->use();
            s->dtStage = dt;
            hipCheck(hipEventRecord(s->evA[1], s->stream), "hipEventRecord");
            hipCheck(hipStreamWaitEvent(s->halo.stream, s->evA[1], 0), "hipStreamWaitEvent");
        }
        // pack / unpack folded into the boundary kernel where every part can do it (see launchLserkStagesExchanged)
        bool fold = true;
        for (int r = 0; r < num_parts; ++r) fold = fold && parts[r]->halosFold();
        for (int i = 0; i < num_stages; ++i) {
            const int cur = i & 1, prev = cur ^ 1;
            const bool first = i == 0;
            for (int r = 0; r < num_parts; ++r) {           // chain A + pack
                bdg_sw2d* s = parts[r];
                s->use();
                if (!first) hipCheck(hipStreamWaitEvent(s->stream, s->evB[prev], 0), "hipStreamWaitEvent");
                s->launchLserkStage(0);
                hipCheck(hipEventRecord(s->evA[cur], s->stream), "hipEventRecord");
                if (!fold || first) {
                    if (!first)                               // neighbours are done reading our send buffer
                        for (const bdg_halo::Peer& pr : s->halo.peers)
                            hipCheck(hipStreamWaitEvent(s->halo.stream, parts[pr.rank]->evCopied[prev], 0), "hipStreamWaitEvent");
                    s->launchPack(s->halo.sendBuf.p, s->halo.stream);
                }                                             // (folded: boundary(i-1) wrote the records, same stream)
                hipCheck(hipEventRecord(s->evPacked[cur], s->halo.stream), "hipEventRecord");
            }
            for (int r = 0; r < num_parts; ++r) {           // pull the ghosts
                bdg_sw2d* s = parts[r];
                s->use();
                for (const bdg_halo::Peer& pr : s->halo.peers) {
                    if (pr.recvCount == 0) continue;
                    bdg_sw2d* src = parts[pr.rank];
                    const bdg_halo::Peer* back = nullptr;
                    for (const bdg_halo::Peer& b : src->halo.peers)
                        if (b.rank == r) back = &b;
                    hipCheck(hipStreamWaitEvent(s->halo.stream, src->evPacked[cur], 0), "hipStreamWaitEvent");
                    double* dst = s->halo.recvBuf.p + static_cast<size_t>(pr.recvStart) * rows;
                    const double* from = src->halo.sendBuf.p + static_cast<size_t>(back->sendStart) * rows;
                    const size_t bytes = static_cast<size_t>(pr.recvCount) * rows * sizeof(double);
                    if (src->device == s->device)
                        hipCheck(hipMemcpyAsync(dst, from, bytes, hipMemcpyDeviceToDevice, s->halo.stream), "ghost copy");
                    else  // another GPU of the node: the copy engine pulls over xGMI
                        hipCheck(hipMemcpyPeerAsync(dst, s->device, from, src->device, bytes, s->halo.stream), "ghost peer copy");
                }
                hipCheck(hipEventRecord(s->evCopied[cur], s->halo.stream), "hipEventRecord");
            }
            for (int r = 0; r < num_parts; ++r) {           // chain B: unpack, boundary elements
                bdg_sw2d* s = parts[r];
                s->use();
                if (!fold) s->launchUnpack(s->halo.recvBuf.p, s->halo.stream);
                if (!first) hipCheck(hipStreamWaitEvent(s->halo.stream, s->evA[prev], 0), "hipStreamWaitEvent");
                if (fold) {
                    // the kernel overwrites the send records: every neighbour must have pulled this stage's first
                    for (const bdg_halo::Peer& pr : s->halo.peers)
                        hipCheck(hipStreamWaitEvent(s->halo.stream, parts[pr.rank]->evCopied[cur], 0), "hipStreamWaitEvent");
                    s->launchBoundaryStageFolded(s->halo.stream, s->halo.recvBuf.p, s->halo.sendBuf.p);
                } else {
                    s->launchLserkStage(1, s->halo.stream);
                }
                hipCheck(hipEventRecord(s->evB[cur], s->halo.stream), "hipEventRecord");
            }
        }
        for (int r = 0; r < num_parts; ++r) {
            bdg_sw2d* s = parts[r];
            s->use();
            hipCheck(hipStreamWaitEvent(s->stream, s->evB[(num_stages - 1) & 1], 0), "hipStreamWaitEvent");
            // the neighbours' last copies read this part's send buffer: order them before anything later on A
            for (const bdg_halo::Peer& pr : s->halo.peers)
                hipCheck(hipStreamWaitEvent(s->stream, parts[pr.rank]->evCopied[(num_stages - 1) & 1], 0), "hipStreamWaitEvent");
        }
    });
}

int bdg_sw2d_lserk4_stages_exchanged(bdg_sw2d* s, double dt, int num_stages) {
    return guard([&] {
        requireSolver(s, "bdg_sw2d_lserk4_stages_exchanged");
        if (num_stages < 0) throw arg_error("bdg_sw2d_lserk4_stages_exchanged: num_stages < 0");
        s->monitorReserve(s->lserkSteps(num_stages), "bdg_sw2d_lserk4_stages_exchanged");
        s->use();
        s->lserkStagesExchangedMonitored(dt, num_stages);
    });
}

int bdg_sw2d_compute_dt_global(bdg_sw2d* s, double cfl, double* dt, double* eta_max) {
    return guard([&] {
        requireSolver(s, "bdg_sw2d_compute_dt_global");
        s->use();
        double r[2];
        s->reduceDt(r);
        // NaN does not survive a max-reduction reliably: send it as +inf
        const double big = std::numeric_limits<double>::infinity();
        const double f = s->allReduceScalar(std::isnan(r[0]) ? big : r[0], true);
        const double e = s->allReduceScalar(std::isnan(r[1]) ? big : r[1], true);
        if (eta_max) *eta_max = e;
        if (dt) *dt = cfl / ((s->N + 1) * (s->N + 1) * 0.5 * f);
        if (std::isinf(f) || std::isinf(e) || std::fabs(e) > 1e8)
            throw unstable_error("A numerical instability has occurred!");
    });
}

int bdg_sw2d_allreduce_max(bdg_sw2d* s, double value, double* out) {
    return guard([&] {
        requireSolver(s, "bdg_sw2d_allreduce_max");
        if (!out) throw arg_error("bdg_sw2d_allreduce_max: out is NULL");
        s->use();
        *out = s->allReduceScalar(value, true);
    });
}

int bdg_sw2d_allreduce_sum(bdg_sw2d* s, double value, double* out) {
    return guard([&] {
        requireSolver(s, "bdg_sw2d_allreduce_sum");
        if (!out) throw arg_error("bdg_sw2d_allreduce_sum: out is NULL");
        s->use();
        *out = s->allReduceScalar(value, false, true);
    });
}

int bdg_sw2d_barrier(bdg_sw2d* s) {
    return guard([&] {
        requireSolver(s, "bdg_sw2d_barrier");
        s->use();
        hipCheck(hipStreamSynchronize(s->stream), "hipStreamSynchronize");
        if (s->halo.stream) hipCheck(hipStreamSynchronize(s->halo.stream), "hipStreamSynchronize");
        // every rank arrives before anyone leaves -- and a wait that gave up on ANY rank is reported by ALL of them here (a rank that
        // threw before the reduction would leave the others inside it), so that the callers can react together
        const bool mine = s->takeSyncMark();
        const double any = s->allReduceScalar(mine ? 1.0 : 0.0, true);
        hipCheck(hipDeviceSynchronize(), "hipDeviceSynchronize");
        if (mine) throw std::runtime_error(bdg_sw2d::syncErrorText());
        if (any != 0.0) throw std::runtime_error(std::string("on another rank: ") + bdg_sw2d::syncErrorText());
    });
}

// ---- run monitor (what the quadrilateral solver has too: run_records.hpp)
int bdg_sw2d_enable_monitor(bdg_sw2d* s, const bdg_sw2d_monitor_desc* d) {
    return guard([&] {
        const std::string fn = "bdg_sw2d_enable_monitor";
        requireSolver(s, fn.c_str());
        bdg_sw2d::Monitor& m = s->mon;
        m.checkEnable(fn, d, s->K);
        const int ng = d->num_gauges, Np = s->Np;
        if (ng > 0 && !d->gauge_row) throw arg_error(fn + ": bad gauge list");
        // the gauges' elements in device slots (the caller's numbering through the renumbering, if there is one)
        std::vector<int> slots(static_cast<size_t>(std::max(1, ng)), 0);
        for (int i = 0; i < ng; ++i) slots[i] = s->permHost.empty() ? d->gauge_element[i] : s->permHost[d->gauge_element[i]];
        s->use();
        m.enable(d->stride, d->capacity, ng, s->nf, slots.data(), {&m.row, &m.scratch}, &m.scratch, s->bytes, s->stream, [&] {
            // the weight plane (and H) zero-padded and through the solver's own upload, so that they follow the renumbering
            s->uploadPlane(d->weights, m.w);
            if (d->H) s->uploadPlane(d->H, m.H);
            m.row.alloc(static_cast<size_t>(std::max(1, ng)) * Np, s->bytes, s->stream);
            if (ng > 0)
                hipCheck(hipMemcpyAsync(m.row.p, d->gauge_row, static_cast<size_t>(ng) * Np * sizeof(double), hipMemcpyHostToDevice,
                                        s->stream), "hipMemcpy (gauge rows)");
        });
    });
}

namespace {
void requireMonitorOn(const bdg_sw2d* s, const char* fn) {
    requireSolver(s, fn);
    s->mon.requireOn(fn, "bdg_sw2d");
}
} // namespace

int bdg_sw2d_monitor_sample(bdg_sw2d* s) {
    return guard([&] {
        requireMonitorOn(s, "bdg_sw2d_monitor_sample");
        s->mon.requireFree("bdg_sw2d_monitor_sample", "bdg_sw2d");
        s->use();
        s->monitorSample();
    });
}

int bdg_sw2d_monitor_count(const bdg_sw2d* s, int* n) {
    return guard([&] {
        requireMonitorOn(s, "bdg_sw2d_monitor_count");
        if (!n) throw arg_error("bdg_sw2d_monitor_count: NULL argument");
        *n = s->mon.count;
    });
}

int bdg_sw2d_monitor_width(const bdg_sw2d* s, int* width) {
    return guard([&] {
        requireMonitorOn(s, "bdg_sw2d_monitor_width");
        if (!width) throw arg_error("bdg_sw2d_monitor_width: NULL argument");
        *width = s->mon.width;
    });
}

int bdg_sw2d_monitor_read(bdg_sw2d* s, int first, int count, double* records) {
    return guard([&] {
        requireMonitorOn(s, "bdg_sw2d_monitor_read");
        s->use();
        s->mon.read("bdg_sw2d_monitor_read", first, count, records, s->stream);
    });
}

int bdg_sw2d_monitor_reset(bdg_sw2d* s) {
    return guard([&] {
        requireMonitorOn(s, "bdg_sw2d_monitor_reset");
        s->mon.reset();
    });
}

int bdg_sw2d_monitor_reduce(bdg_sw2d* s) {
    return guard([&] {
        requireMonitorOn(s, "bdg_sw2d_monitor_reduce");
        bdg_halo::requireComm(s->halo, "bdg_sw2d", "bdg_sw2d_monitor_reduce");
        s->use();
        s->mon.allReduce(s->halo.comm, s->stream, s->nf, s->bytes);
    });
}

int bdg_sw2d_monitor_time(bdg_sw2d* s, int count, float* ms) {
    return guard([&] {
        requireMonitorOn(s, "bdg_sw2d_monitor_time");
        if (count < 1 || !ms) throw arg_error("bdg_sw2d_monitor_time: bad argument");
        s->use();
        s->monitorLaunch(s->mon.scratch.p, 1, 0); // once before the clock starts
        *ms = bdg_dev::timePerRun(s->stream, count, [&] { s->monitorLaunch(s->mon.scratch.p, 1, 0); });
    });
}

// ---- drifters
int bdg_sw2d_enable_drifters(bdg_sw2d* s, const bdg_sw2d_drifter_desc* d) {
    return guard([&] {
        using namespace bdg_dev;
        const std::string fn = "bdg_sw2d_enable_drifters";
        requireSolver(s, fn.c_str());
        if (!d || d->count < 1 || !d->element || !d->r || !d->s || !d->vertices || !d->neighbours || !d->vinv || !d->jacobi)
            throw arg_error(fn + ": the descriptor, at least one drifter and the tables of bdg_trinodes_drifter_tables are required");
        bdg_sw2d::Drifters& m = s->drf;
        m.checkEnable(fn, d->count, d->stride, d->capacity, s->partitionSet || s->numOwned != s->K || s->halo.comm || s->localGroup);
        const int n = d->count, K = s->K, Np = s->Np, Nq = s->N + 1;
        const int* perm = s->permHost.empty() ? nullptr : s->permHost.data();
        std::vector<int> slots(static_cast<size_t>(n));
        for (int i = 0; i < n; ++i) {
            const int e = d->element[i];
            if (e < 0 || e >= K) throw arg_error(fn + ": drifter " + std::to_string(i) + " names an element outside [0, K)");
            const double r = d->r[i], t = d->s[i];
            if (!(-1.0 - t <= 1e-10) || !(r + t <= 1e-10) || !(-1.0 - r <= 1e-10))
                throw arg_error(fn + ": drifter " + std::to_string(i) + " lies outside its element (r, s >= -1, r + s <= 0)");
            slots[i] = perm ? perm[e] : e;
        }
        // the tables in device slots; the kernel follows the neighbour entries without a further check
        std::vector<int> nb(static_cast<size_t>(4) * K, kDriftWall);
        std::vector<double> vert(static_cast<size_t>(8) * K);
        std::vector<int> callerOf(static_cast<size_t>(K));
        for (int k = 0; k < K; ++k) {
            const int slot = perm ? perm[k] : k;
            callerOf[slot] = k;
            const double* line = d->vertices + static_cast<size_t>(8) * k;
            std::copy(line, line + 8, vert.begin() + static_cast<size_t>(8) * slot);
            for (int f = 0; f < 3; ++f) {
                const int v = d->neighbours[static_cast<size_t>(f) * K + k];
                if (v < kDriftOpen || v >= K) throw arg_error(fn + ": neighbour entry out of range");
                nb[static_cast<size_t>(4) * slot + f] = v < 0 ? v : (perm ? perm[v] : v);
            }
        }
        std::vector<double> vinvT(static_cast<size_t>(Np) * Np);
        for (int r = 0; r < Np; ++r)
            for (int c = 0; c < Np; ++c) vinvT[static_cast<size_t>(c) * Np + r] = d->vinv[static_cast<size_t>(r) * Np + c];
        s->use();
        m.enable(n, d->stride, d->capacity, s->timeNow, nb, slots.data(), d->r, d->s, {&m.vert, &m.vinvT, &m.jac}, s->bytes, s->stream,
                 [&] {
                     m.put(m.vert, vert.data(), vert.size(), s->bytes, s->stream);
                     m.put(m.vinvT, vinvT.data(), vinvT.size(), s->bytes, s->stream);
                     m.put(m.jac, d->jacobi, static_cast<size_t>(Nq + 1) * Nq * 3, s->bytes, s->stream);
                 },
                 [&] { s->drifterLaunch(kDriftInit, 0.0, -1); });
        m.callerOf = perm ? std::move(callerOf) : std::vector<int>();
    });
}

namespace {
void requireDriftersOn(const bdg_sw2d* s, const char* fn) {
    requireSolver(s, fn);
    s->drf.requireOn(fn, "bdg_sw2d");
}
} // namespace

int bdg_sw2d_drifters_advance(bdg_sw2d* s, double dt, int num_steps) {
    return guard([&] {
        requireDriftersOn(s, "bdg_sw2d_drifters_advance");
        if (num_steps < 0) throw arg_error("bdg_sw2d_drifters_advance: num_steps < 0");
        s->drifterReserve(num_steps, "bdg_sw2d_drifters_advance");
        s->use();
        for (int i = 0; i < num_steps; ++i) {
            s->drf.t += dt;
            s->drifterAdvance(dt);
        }
    });
}

int bdg_sw2d_drifters_time(bdg_sw2d* s, double dt, int count, float* ms) {
    return guard([&] {
        requireDriftersOn(s, "bdg_sw2d_drifters_time");
        if (!ms || count < 1) throw arg_error("bdg_sw2d_drifters_time: bad argument");
        s->use();
        *ms = bdg_dev::timePerRun(s->stream, count, [&] { s->drifterAdvance(dt, false); });
    });
}

int bdg_sw2d_drifters_state(bdg_sw2d* s, double* x, double* y, int* element, double* r, double* sref, int* status) {
    return guard([&] {
        requireDriftersOn(s, "bdg_sw2d_drifters_state");
        s->use();
        s->drf.downloadState(x, y, element, r, sref, status, s->drf.callerOf, s->stream); // (device slots back to the caller's numbering)
    });
}

int bdg_sw2d_drifters_count(const bdg_sw2d* s, int* num_records, int* num_drifters) {
    return guard([&] {
        requireDriftersOn(s, "bdg_sw2d_drifters_count");
        if (num_records) *num_records = s->drf.count;
        if (num_drifters) *num_drifters = s->drf.n;
    });
}

int bdg_sw2d_drifters_read(bdg_sw2d* s, int first, int count, double* t, double* x, double* y, int* status) {
    return guard([&] {
        requireDriftersOn(s, "bdg_sw2d_drifters_read");
        s->use();
        s->drf.readTracks("bdg_sw2d_drifters_read", first, count, t, x, y, status, s->stream);
    });
}

int bdg_sw2d_drifters_reset(bdg_sw2d* s) {
    return guard([&] {
        requireDriftersOn(s, "bdg_sw2d_drifters_reset");
        s->drf.count = 0;
    });
}

// ---- field statistics (what the quadrilateral solver has too: run_records.hpp)
int bdg_sw2d_enable_field_stats(bdg_sw2d* s, const bdg_field_stats_desc* d) {
    return guard([&] {
        const std::string fn = "bdg_sw2d_enable_field_stats";
        requireSolver(s, fn.c_str());
        s->fst.checkEnable(fn, d, s->partitionSet || s->numOwned != s->K || s->halo.comm || s->localGroup);
        s->use();
        // H zero-padded and through the solver's own upload, so that it follows the renumbering
        s->fst.enable(*d, s->planeSize(), s->bytes, s->stream, [&] {
            if (d->H) s->uploadPlane(d->H, s->fst.H);
        });
    });
}

namespace {
void requireStatsOn(const bdg_sw2d* s, const char* fn) {
    requireSolver(s, fn);
    s->fst.requireOn(fn, "bdg_sw2d");
}
} // namespace

int bdg_sw2d_field_stats_sample(bdg_sw2d* s) {
    return guard([&] {
        requireStatsOn(s, "bdg_sw2d_field_stats_sample");
        s->use();
        s->statsSample();
    });
}

int bdg_sw2d_field_stats_count(const bdg_sw2d* s, int* samples, int* num_periods) {
    return guard([&] {
        requireStatsOn(s, "bdg_sw2d_field_stats_count");
        if (!samples || !num_periods) throw arg_error("bdg_sw2d_field_stats_count: NULL argument");
        *samples = s->fst.count();
        *num_periods = s->fst.m;
    });
}

int bdg_sw2d_field_stats_read(bdg_sw2d* s, int which, int index, double* plane) {
    return guard([&] {
        requireStatsOn(s, "bdg_sw2d_field_stats_read");
        if (!plane) throw arg_error("bdg_sw2d_field_stats_read: NULL argument");
        const double* dev = s->fst.planeOf("bdg_sw2d_field_stats_read", which, index);
        s->use();
        s->downloadRows(dev, plane, s->Np); // (device slots back to the caller's numbering)
    });
}

int bdg_sw2d_field_stats_samples(const bdg_sw2d* s, int first, int count, double* rows) {
    return guard([&] {
        requireStatsOn(s, "bdg_sw2d_field_stats_samples");
        s->fst.samples("bdg_sw2d_field_stats_samples", first, count, rows);
    });
}

int bdg_sw2d_field_stats_reset(bdg_sw2d* s) {
    return guard([&] {
        requireStatsOn(s, "bdg_sw2d_field_stats_reset");
        s->use();
        s->fst.reset(s->stream);
    });
}

int bdg_sw2d_field_stats_time(bdg_sw2d* s, int count, float* ms) {
    return guard([&] {
        requireStatsOn(s, "bdg_sw2d_field_stats_time");
        if (count < 1 || !ms) throw arg_error("bdg_sw2d_field_stats_time: bad argument");
        s->use();
        *ms = s->fst.time(s->statsView(), count, s->bytes, s->stream);
    });
}

int bdg_probe_stream_triad(int device, size_t bytes_per_array, int repeats, double* gbps) {
    return guard([&] {
        if (!gbps || repeats < 1 || bytes_per_array < (1u << 20)) throw arg_error("bdg_probe_stream_triad: bad argument");
        hipCheck(hipSetDevice(device), "hipSetDevice");
        const size_t n2 = bytes_per_array / sizeof(double2);
        size_t total = 0;
        DevBuf<double> a, b, c;
        a.alloc(2 * n2, total); b.alloc(2 * n2, total); c.alloc(2 * n2, total);
        hipCheck(hipMemset(a.p, 0, 2 * n2 * sizeof(double)), "hipMemset");
        hipCheck(hipMemset(b.p, 0, 2 * n2 * sizeof(double)), "hipMemset");
        hipCheck(hipMemset(c.p, 0, 2 * n2 * sizeof(double)), "hipMemset");
        auto launch = [&] {
            hipLaunchKernelGGL(bdg_dev::triad_kernel, dim3(256 * 8), dim3(256), 0, nullptr, reinterpret_cast<double2*>(a.p),
                               reinterpret_cast<const double2*>(b.p), reinterpret_cast<const double2*>(c.p), 0.5, n2);
        };
        launch();
        const float ms = bdg_dev::timePerRun(nullptr, repeats, launch);
        *gbps = 3.0 * static_cast<double>(n2) * sizeof(double2) / (ms * 1e-3) / 1e9;
    });
}

int bdg_sw2d_probe_stage_traffic(bdg_sw2d* s, int repeats, float* ms_per_launch) {
    return guard([&] {
        requireSolver(s, "bdg_sw2d_probe_stage_traffic");
        if (!ms_per_launch || repeats < 1) throw arg_error("bdg_sw2d_probe_stage_traffic: bad argument");
        if (!s->affine) throw arg_error("bdg_sw2d_probe_stage_traffic: affine geometry only");
        s->use();
        const unsigned grid = static_cast<unsigned>((s->K + 255) / 256);
        // with face links the launches cycle through the five stages of a step, as the stage kernel's do
        const bool links = s->faceLink.p != nullptr;
        unsigned launches = 0; // the direction alternates as the stage launches' does
        auto launch = [&](int stage) {
            const int last = blitzdg::LSERK4::numStages - 1;
            const int back = s->sweepAlternates ? static_cast<int>(launches++ & 1u) : 0;
            // aux / qalt are scratch here: the resident state is not modified
            hipLaunchKernelGGL(bdg_dev::stage_traffic_probe_kernel, dim3(grid), dim3(256), 0, s->stream, s->qcur, s->qalt,
                               s->aux.p, s->ageo.p, links ? s->faceLink.p : s->vmapP.p, 3 * s->Np, links ? 3 : s->NFN, s->ld,
                               s->K, !links || stage != 0 ? 1 : 0, !links || stage != last ? 1 : 0, back);
        };
        launch(1);
        int i = 0;
        *ms_per_launch = bdg_dev::timePerRun(s->stream, repeats, [&] { launch(i++ % blitzdg::LSERK4::numStages); });
    });
}

int bdg_sw2d_uses_affine_geometry(const bdg_sw2d* s) { return s ? (s->affine ? 1 : 0) : -1; }
int bdg_sw2d_is_renumbered(const bdg_sw2d* s) { return s ? (s->permHost.empty() ? 0 : 1) : -1; }

size_t bdg_sw2d_device_bytes(const bdg_sw2d* s) { return s ? s->bytes : 0; }
long long bdg_sw2d_backward_launches(const bdg_sw2d* s) { return s ? static_cast<long long>(s->backwardLaunches) : -1; }
unsigned bdg_stage_tile(unsigned block, unsigned grid, unsigned back) { return bdg_dev::stage_tile(block, grid, back); }
void* bdg_sw2d_stream(bdg_sw2d* s) { return s ? static_cast<void*>(s->stream) : nullptr; }

} // extern "C"
