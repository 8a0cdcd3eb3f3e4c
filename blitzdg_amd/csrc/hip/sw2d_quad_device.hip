// sw2d_quad_device.hip -- the device-resident quadrilateral sw2d solver behind the bdg_sw2dq_* C ABI
// (include/blitzdg_hip.h). Host side: checks that Dr, Ds and Lift have the Gauss-Lobatto tensor form and extracts
// their 1-D factors, chooses the geometry form (both: host/element_tables.hpp), builds the gather index; then launches sw2d_quad_stage_kernel
// (sw2d_quad_kernel.hpp) on its own stream. One device; results come back in the caller's numbering.
// Partitioned runs (bdg_sw2dq_set_partition / _comm_init) add the ghost exchange and the two-chain schedule of
// partition_schedule.hpp on a second stream. A solver created with four fields (bdg_sw2dq_create_fields) launches
// sw2d_quad4_stage_kernel (sw2d_quad4_kernel.hpp) instead, with the sources of bdg_sw2dq_set_sources if there are any.
// The output step (bdg_sw2dq_output_fields) is one launch of sw2d_quad_output_kernel (sw2d_quad_output_kernel.hpp).
// After bdg_sw2dq_enable_variant_b a three-field solver evaluates the tidal driver's right-hand side instead: the speed pass
// sw2d_quadb_speed_kernel, then sw2d_quadb_stage_kernel (sw2d_quadb_kernel.hpp), which reads the speed from device memory.
// After bdg_sw2dq_enable_variant_b4 a four-field solver does the same with the tracer as a fourth equation
// (sw2d_quadb4_stage_kernel, sw2d_quadb4_kernel.hpp; the speed pass is the three-field one).
// After bdg_sw2dq_enable_tracer_diffusion every evaluation of a four-field solver is followed on the same stream by the two passes
// of sw2d_quad_diffusion_kernel.hpp (per-order objects sw2d_quad_diffusion_order.hip), which add the tracer's diffusion, source
// and decay, evaluated from the stage's input state, to plane 3 of what the stage wrote. That state is never one of the stage's
// output buffers: rk2Step evaluates q into q1 and q1 into q, heunStep likewise, lserkStage q into q1 and res (then swaps), and
// computeRhs io into ioOut.
// After bdg_sw2dq_enable_monitor the stepping calls record diagnostics and gauges on the device (sw2d_monitor_kernel.hpp).
// After bdg_sw2dq_enable_drifters they also advance Lagrangian drifters after every completed step (sw2d_quad_drifter_kernel.hpp).
#include "../host/element_tables.hpp"
#include "device_buffer.hpp"
#include "partition_schedule.hpp"
#include "run_records.hpp"
#include "sw2d_quad4_kernel.hpp"
#include "sw2d_dispatch.hpp"
#include "sw2d_quad_diffusion_launch.hpp"
#include "sw2d_quad_drifter_kernel.hpp"
#include "sw2d_quad_output_kernel.hpp"
#include "sw2d_quadb4_kernel.hpp"
#include "sw2d_quadb_kernel.hpp"
#include "blitzdg/JacobiBuilders.hpp"
#include "blitzdg/LSERK4.hpp"
#include "blitzdg/MeshManager.hpp"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <limits>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

using bdg_detail::arg_error;
using bdg_detail::guard;
using bdg_detail::unstable_error;
using namespace bdg_dev;

namespace bdg_dev {

namespace {
// the per-order launchers exist for 1..BDG_SW2DQ_MAX_ORDER (the Makefile's QUAD_ORDERS)
template <class F>
hipError_t forQuadOrder(int order, F&& f) { return forOrder<BDG_SW2DQ_MAX_ORDER>(order, std::forward<F>(f)); }
} // namespace

hipError_t sw2d_quad_stage(int order, int mode, bool filter, bool general, const QuadParams& p, hipStream_t stream) {
    return forQuadOrder(order, [&](auto n) { return sw2d_quad_launch<decltype(n)::value>(mode, filter, general, p, stream); });
}

hipError_t sw2d_quad4_stage(int order, int mode, bool filter, bool general, bool sources, const Quad4Params& p,
                            hipStream_t stream) {
    return forQuadOrder(order, [&](auto n) { return sw2d_quad4_launch<decltype(n)::value>(mode, filter, general, sources, p, stream); });
}

hipError_t sw2d_quad_output(int order, int fields, const QuadOutParams& p, hipStream_t stream) {
    return forQuadOrder(order, [&](auto n) { return sw2d_quad_output_launch<decltype(n)::value>(fields, p, stream); });
}

hipError_t sw2d_quadb_stage(int order, int mode, bool filter, bool general, const QuadBParams& p, hipStream_t stream) {
    return forQuadOrder(order, [&](auto n) { return sw2d_quadb_launch<decltype(n)::value>(mode, filter, general, p, stream); });
}

hipError_t sw2d_quadb4_stage(int order, int mode, bool filter, bool general, const QuadB4Params& p, hipStream_t stream) {
    return forQuadOrder(order, [&](auto n) { return sw2d_quadb4_launch<decltype(n)::value>(mode, filter, general, p, stream); });
}

hipError_t sw2d_quadb_speed(int order, bool general, const QuadBParams& p, double* out, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(out, 0, sizeof(double), stream);
    if (e != hipSuccess || p.q.kEnd <= p.q.kBegin) return e;
    const long long items = 4LL * (order + 1) * (p.q.kEnd - p.q.kBegin);
    const dim3 grid(static_cast<unsigned>(std::min<long long>((items + 255) / 256, 2048))), block(256);
    unsigned long long* bits = reinterpret_cast<unsigned long long*>(out);
    if (general)
        hipLaunchKernelGGL((sw2d_quadb_speed_kernel<true>), grid, block, 0, stream, p, order, bits);
    else
        hipLaunchKernelGGL((sw2d_quadb_speed_kernel<false>), grid, block, 0, stream, p, order, bits);
    return hipGetLastError();
}

const QuadDiffusionKernelTable* quad_diffusion_kernel_table_order1();
const QuadDiffusionKernelTable* quad_diffusion_kernel_table_order2();
const QuadDiffusionKernelTable* quad_diffusion_kernel_table_order3();
const QuadDiffusionKernelTable* quad_diffusion_kernel_table_order4();
const QuadDiffusionKernelTable* quad_diffusion_kernel_table_order5();
const QuadDiffusionKernelTable* quad_diffusion_kernel_table_order6();
const QuadDiffusionKernelTable* quad_diffusion_kernel_table_order7();
const QuadDiffusionKernelTable* quad_diffusion_kernel_table_order8();
const QuadDiffusionKernelTable* quad_diffusion_kernel_table_order9();
const QuadDiffusionKernelTable* quad_diffusion_kernel_table_order10();
const QuadDiffusionKernelTable* quad_diffusion_kernel_table_order11();
const QuadDiffusionKernelTable* quad_diffusion_kernel_table_order12();
static_assert(BDG_SW2DQ_MAX_ORDER == 12, "one table per order of the Makefile's QUAD_ORDERS");

const QuadDiffusionKernelTable* quad_diffusion_kernel_table(int order) {
    switch (order) {
    case 1: return quad_diffusion_kernel_table_order1();
    case 2: return quad_diffusion_kernel_table_order2();
    case 3: return quad_diffusion_kernel_table_order3();
    case 4: return quad_diffusion_kernel_table_order4();
    case 5: return quad_diffusion_kernel_table_order5();
    case 6: return quad_diffusion_kernel_table_order6();
    case 7: return quad_diffusion_kernel_table_order7();
    case 8: return quad_diffusion_kernel_table_order8();
    case 9: return quad_diffusion_kernel_table_order9();
    case 10: return quad_diffusion_kernel_table_order10();
    case 11: return quad_diffusion_kernel_table_order11();
    case 12: return quad_diffusion_kernel_table_order12();
    default: return nullptr;
    }
}

int sw2d_quad_tile(int order) {
    switch (order) {
    case 1: return QuadElem<1>::E;
    case 2: return QuadElem<2>::E;
    case 9: case 10: case 11: case 12: return QuadElem<9>::E;
    default: return QuadElem<3>::E;
    }
}

} // namespace bdg_dev

namespace {

// |h| maximum and NaN count of plane 0 over [0, K): two doubles per block
__global__ __launch_bounds__(256) void sw2d_quad_hmax_kernel(const double* h, long long ld, int Np, int K, double* partials) {
    __shared__ double smax[256], snan[256];
    double mx = 0.0, nn = 0.0;
    const long long total = static_cast<long long>(Np) * K;
    for (long long t = blockIdx.x * 256LL + threadIdx.x; t < total; t += 256LL * gridDim.x) {
        const long long n = t / K, k = t % K;
        const double v = h[n * ld + k];
        if (v != v) nn += 1.0;
        else mx = fabs(v) > mx ? fabs(v) : mx;
    }
    smax[threadIdx.x] = mx;
    snan[threadIdx.x] = nn;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            smax[threadIdx.x] = fmax(smax[threadIdx.x], smax[threadIdx.x + s]);
            snan[threadIdx.x] += snan[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        partials[2 * blockIdx.x] = smax[0];
        partials[2 * blockIdx.x + 1] = snan[0];
    }
}

constexpr int kHmaxBlocks = 512;

// Face-node maximum of |Fscale| (sqrt(u^2 + v^2) + sqrt(g h)) over the elements [0, K), for the drivers' time step
// dt = CFL / ((N + 1)^2 / 2 * maximum); one partial per block, NaN if any value is NaN. Contraction is off, and division
// and square root are the correctly rounded ones, so the value is bit-identical to the host formula.
__global__ __launch_bounds__(256) void sw2d_quad_dt_kernel(const double* __restrict__ q, const double* __restrict__ fgeo,
                                                           const double* __restrict__ ageo, long long ld, int N, int K,
                                                           double g, double* __restrict__ partials) {
#pragma clang fp contract(off)
    const int Nq = N + 1, Np = Nq * Nq, NFN = 4 * Nq;
    const long long plane = static_cast<long long>(Np) * ld, total = static_cast<long long>(NFN) * K;
    double mx = 0.0;
    bool bad = false;
    for (long long t = blockIdx.x * 256LL + threadIdx.x; t < total; t += 256LL * gridDim.x) {
        const int fn = static_cast<int>(t / K), k = static_cast<int>(t % K), f = fn / Nq, n = fn % Nq;
        const int node = f == 0 ? Nq * n : (f == 1 ? Nq * N + n : (f == 2 ? Nq * n + N : n));
        const long long o = node * ld + k;
        const double h = q[o], u = q[plane + o] / h, v = q[2 * plane + o] / h;
        const double fsc = fgeo ? fgeo[(2LL * NFN + fn) * ld + k] : ageo[(12 + f) * ld + k];
        const double val = fabs(fsc) * (sqrt(u * u + v * v) + sqrt(g * h));
        if (val != val) bad = true;
        mx = fmax(mx, val);
    }
    __shared__ double smax[256];
    __shared__ int sBad;
    if (threadIdx.x == 0) sBad = 0;
    __syncthreads();
    if (bad) sBad = 1;
    smax[threadIdx.x] = mx;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (static_cast<int>(threadIdx.x) < s) smax[threadIdx.x] = fmax(smax[threadIdx.x], smax[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) partials[blockIdx.x] = sBad ? __builtin_nan("") : smax[0];
}

} // namespace

struct bdg_sw2dq {
    int N = 0, Np = 0, Nfp = 0, NFN = 0, K = 0, device = 0;
    int fields = 3;           // 4: the tracer plane hN and sw2d_quad4_stage_kernel
    bool hasSources = false;  // bdg_sw2dq_set_sources
    bool evaluated = false;   // a stage kernel has been launched: the sources are fixed from then on
    double fconst = 0.0, CD = 0.0;
    DevBuf<double> zx, zy, fcor;
    // variant B (bdg_sw2dq_enable_variant_b): sw2d_quadb_kernel.hpp
    bool variantB = false;
    DevBuf<double> vbH, vbHx, vbHy, vbSponge, lamBuf;
    DevBuf<int> gidxB;        // gidx with the open-boundary nodes marked
    // four fields (bdg_sw2dq_enable_variant_b4): the open-boundary concentration, sw2d_quadb4_kernel.hpp
    DevBuf<long long> openKey;
    DevBuf<double> openN;
    int numOpenN = 0;
    double nOpenC = 0.0;
    double vbF = 0.0, vbCD = 0.0, tideAmp = 0.0, tidePeriod = 1.0, tideRamp = 0.0;
    // tracer diffusion, sources and decay (bdg_sw2dq_enable_tracer_diffusion): the two passes of sw2d_quad_diffusion_kernel.hpp
    // behind the stage launch of every evaluation. difFlux: the planes fx, fy
    bool diffusion = false;
    const QuadDiffusionKernelTable* ktd = nullptr;
    QuadDiffusionParams dif{};
    DevBuf<double> difKappa, difSource, difFlux;
    double fscaleMax = 0.0;   // max|Fscale| of the mesh (createQuad)
    double difDt = 0.0;       // kDiffusionDtConstant / (max kappa (N+1)^4 max(Fscale)^2)
    // every eigenvalue z = dt_diff lambda of the operator stays inside the RK2 stability region with this constant: the smallest
    // bound measured is 4.02 (N = 1 on squares; DESIGN.md 3.8, tests/test_quaddiff_reference.py)
    static constexpr double kDiffusionDtConstant = 4.0;
    double timeNow = 0.0;     // model time of the resident state (tide phase); the steppers advance it
    double spongeC = 0.0;     // scalar sponge coefficient of the Heun step in flight
    long long ld = 0;
    double g = 9.81;
    bool general = true, hasFilter = false;
    hipStream_t stream = nullptr;
    size_t bytes = 0;
    long long stageCount = 0;
    DevBuf<double> q, q1, res, io, ioOut, geo, fgeo, ageo, ops, filt, partials;
    DevBuf<double> outH, outI1; // output step: the caller's H and I1
    DevBuf<int> gidx;
    std::vector<double> hostPartials;
    // partitioned runs (bdg_sw2dq_set_partition / _comm_init): partition_schedule.hpp
    std::vector<int> maxNeighbourHost; // largest element a face node of element k gathers from (from vmapP, kept for set_partition)
    bdg_halo::Partition part;
    bdg_halo::Transport halo;
    bdg_halo::TwoChains chains;
    // run monitor (bdg_sw2dq_enable_monitor): sw2d_monitor_kernel.hpp, the tensor gauge rule
    struct Monitor : bdg_records::MonitorState {
        DevBuf<double> lr, ls; // (numGauges, N+1): the 1-D basis at each gauge's r and s
    } mon;
    // drifters (bdg_sw2dq_enable_drifters): sw2d_quad_drifter_kernel.hpp
    struct Drifters : bdg_records::DrifterState {
        DevBuf<double> bil, r1d, bary;
    } drf;
    // field statistics (bdg_sw2dq_enable_field_stats): sw2d_stats_kernel.hpp
    bdg_records::FieldStatsState fst;

    void use() const { hipCheck(hipSetDevice(device), "hipSetDevice"); }
    long long plane() const { return static_cast<long long>(Np) * ld; }

    // host (rows, K) -> device planes of stride ld
    void upload(double* dst, const double* src, int rows) {
        hipCheck(hipMemcpy2DAsync(dst, ld * sizeof(double), src, K * sizeof(double), K * sizeof(double), rows,
                                  hipMemcpyHostToDevice, stream), "hipMemcpy2D (upload)");
    }
    void download(double* dst, const double* src, int rows) {
        hipCheck(hipMemcpy2DAsync(dst, K * sizeof(double), src, ld * sizeof(double), K * sizeof(double), rows,
                                  hipMemcpyDeviceToHost, stream), "hipMemcpy2D (download)");
    }

    QuadParams params() const {
        QuadParams p{};
        p.geo = geo.p; p.fgeo = fgeo.p; p.ageo = ageo.p; p.gidx = gidx.p; p.ops = ops.p; p.filt = filt.p;
        p.ld = ld; p.kBegin = 0; p.kEnd = K; p.g = g;
        return p;
    }
    double tideAt(double t) const { // main.cpp:352
        const double om = 2.0 * M_PI / tidePeriod;
        return tideAmp * std::cos(om * t) * 0.5 * (std::tanh(tideRamp * (t - tidePeriod)) + 1);
    }
    QuadBParams paramsB(const QuadParams& p) const {
        QuadBParams b{};
        b.q = p; b.q.gidx = gidxB.p;
        b.H = vbH.p; b.Hx = vbHx.p; b.Hy = vbHy.p; b.lam = lamBuf.p; b.sponge = vbSponge.p; b.spongeC = spongeC;
        b.tide = tideAt(timeNow); b.fcor = vbF; b.cd = vbCD;
        return b;
    }
    // variant B: the global speed of `state` over the columns [0, count) into lamBuf, on the solver's stream; with a
    // communicator the maximum over every rank (one 8-byte all-reduce). Needs no current ghosts (sw2d_quadb_kernel.hpp).
    void speedPass(const double* state, int count) {
        QuadParams p = params();
        p.qin = state; p.kEnd = count;
        hipCheck(sw2d_quadb_speed(N, general, paramsB(p), lamBuf.p, stream), "sw2d_quadb_speed_kernel launch");
        if (halo.comm)
            bdg_rccl::ncclCheck(bdg_rccl::rccl().AllReduce(lamBuf.p, lamBuf.p, 1, ncclDouble, ncclMax, halo.comm, stream),
                                "ncclAllReduce");
    }
    void launchOn(int mode, bool filter, const QuadParams& p, hipStream_t on) {
        evaluated = true;
        if (variantB && fields == 4) {
            const QuadB4Params p4{paramsB(p), openKey.p, openN.p, numOpenN, nOpenC};
            hipCheck(sw2d_quadb4_stage(N, mode, filter, general, p4, on), "sw2d_quadb4_stage_kernel launch");
        } else if (variantB) {
            hipCheck(sw2d_quadb_stage(N, mode, filter, general, paramsB(p), on), "sw2d_quadb_stage_kernel launch");
        } else if (fields == 4) {
            const Quad4Params p4{p, zx.p, zy.p, fcor.p, fconst, CD};
            hipCheck(sw2d_quad4_stage(N, mode, filter, general, hasSources, p4, on), "sw2d_quad4_stage_kernel launch");
        } else {
            hipCheck(sw2d_quad_stage(N, mode, filter, general, p, on), "sw2d_quad_stage_kernel launch");
        }
        if (diffusion) launchDiffusion(mode, filter, p, on);
    }
    // The tracer's diffusion, source and decay of the evaluation whose stage launch was just issued on `on`: T of p.qin -- which
    // that launch read and did not write -- added to plane 3 of what it wrote. p.gidx is the solver's first gather index (wall
    // flags only), for variant B too: a boundary node is one that gathers itself.
    void launchDiffusion(int mode, bool filter, const QuadParams& p, hipStream_t on) {
        // what the scheme rests on
        if (mode == QMODE_RHS ? p.qin == p.rhs : (p.qin == p.qout || (mode == QMODE_LSERK && p.qin == p.res)))
            throw std::logic_error("tracer diffusion: the stage's input state is one of its output buffers");
        hipCheck(ktd->gradient(general, p, dif, on), "sw2d_quad_tracer_gradient_kernel launch");
        hipCheck(ktd->divergence(mode, filter, general, p, dif, on), "sw2d_quad_tracer_divergence_kernel launch");
    }
    // ---- how one evaluation (reads p.qin, writes its outputs) is carried out
    enum class Eval {
        Whole,     // every element on the solver's stream
        Exchanged, // a partition: the ghost columns of p.qin refreshed, then every owned element, in stream order
        TwoChains  // a partition: the two-chain schedule of partition_schedule.hpp, interior elements beside the exchange
    };
    // Eval of the *_exchanged calls: the two chains unless there is no interior element or BDG_SW2DQ_NO_OVERLAP is set.
    // Variant B is never overlapped: the all-rank speed has to exist before any element of the evaluation starts.
    Eval exchangedEval() const {
        const bool two = !variantB && part.numInterior >= 1 && std::getenv("BDG_SW2DQ_NO_OVERLAP") == nullptr; // (A/B switch, read per call)
        return two ? Eval::TwoChains : Eval::Exchanged;
    }
    void exchangeOn(double* state, hipStream_t on) { bdg_halo::exchange(halo, part, state, ld, fields * Np, K, on); }
    // one evaluation of the elements [kBegin, kEnd) on `on`
    void evaluateRange(int mode, bool filter, QuadParams p, int kBegin, int kEnd, hipStream_t on) {
        p.kBegin = kBegin; p.kEnd = kEnd;
        launchOn(mode, filter, p, on);
    }
    void evaluate(Eval how, int mode, bool filter, const QuadParams& p) {
        double* in = const_cast<double*>(p.qin);
        switch (how) {
        case Eval::Whole:
            if (variantB) speedPass(in, K);
            launchOn(mode, filter, p, stream);
            return;
        case Eval::Exchanged:
            if (variantB) speedPass(in, part.numOwned);
            exchangeOn(in, stream);
            evaluateRange(mode, filter, p, 0, part.numOwned, stream);
            return;
        case Eval::TwoChains:
            // (the interior launch is the plain grid of one workgroup per tile: a capped grid of workgroups looping over tiles,
            // which leaves room for the boundary launch, measured slower at every split and order: DESIGN section 3.8)
            chains.eval(stream, halo.stream,
                        [&](hipStream_t a) { evaluateRange(mode, filter, p, 0, part.numInterior, a); },
                        [&](hipStream_t b) {
                            exchangeOn(in, b);
                            evaluateRange(mode, filter, p, part.numInterior, part.numOwned, b);
                        });
            return;
        }
    }

    // ---- the steppers: one RK2 or Heun step, or one LSERK4 stage, of the resident state
    enum class Stepper { Lserk, Rk2, Heun }; // (in the order of bdg_sw2dq_time's `kind`)
    // the script's midpoint RK2, both evaluations at the old time level
    void rk2Step(double dt, bool filter, Eval how) {
        QuadParams p = params();
        p.qin = q.p; p.qbase = q.p; p.qout = q1.p; p.cc = 0.5 * dt;        // predictor: q1 = q + dt/2 F R(q)
        evaluate(how, QMODE_COMBINE, filter, p);
        p.qin = q1.p; p.qbase = q.p; p.qout = q.p; p.cc = dt;              // corrector: q += dt F R(q1)
        evaluate(how, QMODE_COMBINE, filter, p);
        timeNow += dt;
    }
    // SSP-RK2 (Heun) of the tidal driver (main.cpp:211-236), the sponge division in the stage store:
    //   q1 = sp(q + dt R(q));  q = sp(1/2 (q + q1 + dt R(q1))), both evaluations at the old time level
    void heunStep(double dt, bool filter, Eval how) {
        QuadParams p = params();
        p.qin = q.p; p.qbase = q.p; p.qout = q1.p; p.ca = 1.0; p.cb = 0.0; p.cc = dt;
        evaluate(how, QMODE_HEUN, filter, p);
        p.qin = q1.p; p.qbase = q.p; p.qout = q.p; p.ca = 0.5; p.cb = 0.5; p.cc = 0.5 * dt;
        evaluate(how, QMODE_HEUN, filter, p);
        timeNow += dt;
    }
    // q and q1 swap roles after every stage (neighbours read the old traces during the launch: double-buffered; on a partition
    // the next stage's exchange refreshes the ghosts of the new q). The tide is frozen over the five stages of an LSERK4 step and
    // the model time moves on after the last
    void lserkStage(double dt, Eval how) {
        const int st = static_cast<int>(stageCount % blitzdg::LSERK4::numStages);
        QuadParams p = params();
        p.qin = q.p; p.qout = q1.p; p.res = res.p;
        p.ca = blitzdg::LSERK4::rk4a[st]; p.cb = blitzdg::LSERK4::rk4b[st]; p.cc = dt;
        evaluate(how, QMODE_LSERK, false, p);
        std::swap(q.p, q1.p);
        if (st == blitzdg::LSERK4::numStages - 1) timeNow += dt;
        ++stageCount;
    }
    // true when a step of size dt is complete (an LSERK4 stage: after the fifth)
    bool advance(Stepper kind, double dt, bool filter, Eval how) {
        switch (kind) {
        case Stepper::Rk2: rk2Step(dt, filter, how); return true;
        case Stepper::Heun: heunStep(dt, filter, how); return true;
        default: lserkStage(dt, how); return stageCount % blitzdg::LSERK4::numStages == 0;
        }
    }
    // the reference script's check after every step: max|h| > 1e8 or NaN, over the columns [0, count) of h. collective: the two
    // values are all-reduced (maximum) over every rank of the communicator first, so that all ranks raise together
    void checkBlowUp(int count = -1, bool collective = false) {
        hipLaunchKernelGGL(sw2d_quad_hmax_kernel, dim3(kHmaxBlocks), dim3(256), 0, stream, q.p, ld, Np, count < 0 ? K : count,
                           partials.p);
        hipCheck(hipGetLastError(), "sw2d_quad_hmax_kernel launch");
        hostPartials.resize(2 * kHmaxBlocks);
        hipCheck(hipMemcpyAsync(hostPartials.data(), partials.p, 2 * kHmaxBlocks * sizeof(double), hipMemcpyDeviceToHost,
                                stream), "hipMemcpy (partials)");
        hipCheck(hipStreamSynchronize(stream), "hipStreamSynchronize");
        double v[2] = {0.0, 0.0}; // max|h|, NaN count
        for (int b = 0; b < kHmaxBlocks; ++b) {
            v[0] = std::max(v[0], hostPartials[2 * b]);
            v[1] += hostPartials[2 * b + 1];
        }
        if (collective) {
            hipCheck(hipMemcpyAsync(halo.scalarBuf.p, v, sizeof(v), hipMemcpyHostToDevice, stream), "hipMemcpy (blow-up check)");
            bdg_rccl::ncclCheck(bdg_rccl::rccl().AllReduce(halo.scalarBuf.p, halo.scalarBuf.p, 2, ncclDouble, ncclMax, halo.comm, stream),
                                "ncclAllReduce");
            hipCheck(hipMemcpyAsync(v, halo.scalarBuf.p, sizeof(v), hipMemcpyDeviceToHost, stream), "hipMemcpy (blow-up check)");
            hipCheck(hipStreamSynchronize(stream), "hipStreamSynchronize");
        }
        if (v[1] > 0 || v[0] > 1e8) throw unstable_error("A numerical instability has occurred!");
    }

    // max over the face nodes of the columns [0, count) of |Fscale| (|u| + sqrt(g h)); NaN if any value is NaN
    double maxFaceSpeed(int count) {
        hipLaunchKernelGGL(sw2d_quad_dt_kernel, dim3(kHmaxBlocks), dim3(256), 0, stream, q.p, general ? fgeo.p : nullptr, ageo.p, ld,
                           N, count, g, partials.p);
        hipCheck(hipGetLastError(), "sw2d_quad_dt_kernel launch");
        hostPartials.resize(2 * kHmaxBlocks);
        hipCheck(hipMemcpyAsync(hostPartials.data(), partials.p, kHmaxBlocks * sizeof(double), hipMemcpyDeviceToHost, stream),
                 "hipMemcpy (partials)");
        hipCheck(hipStreamSynchronize(stream), "hipStreamSynchronize");
        double m = 0.0;
        for (int b = 0; b < kHmaxBlocks; ++b) {
            if (std::isnan(hostPartials[b])) return hostPartials[b];
            m = std::max(m, hostPartials[b]);
        }
        return m;
    }

    // ---- output step: q1 is written whole by every step and stage before it is read, so between steps it is free and
    // takes the output planes. Returns the number of columns computed (a partitioned run: the owned elements).
    // staged = false: H and I1 are on the device already (a repeated launch).
    int outputLaunch(const double* H, const double* lattice, int mask, bool staged = true) {
        const int count = part.numOwned > 0 ? part.numOwned : K;
        if (H && staged) {
            if (!outH.p) outH.alloc(plane(), bytes, stream);
            upload(outH.p, H, Np);
        }
        if (lattice && staged) {
            if (!outI1.p) outI1.alloc(static_cast<size_t>(Nfp) * Nfp, bytes);
            hipCheck(hipMemcpyAsync(outI1.p, lattice, static_cast<size_t>(Nfp) * Nfp * sizeof(double), hipMemcpyHostToDevice, stream),
                     "hipMemcpy (I1)");
        }
        const QuadOutParams p{q.p, H ? outH.p : nullptr, lattice ? outI1.p : nullptr, q1.p, ld, count, mask};
        hipCheck(sw2d_quad_output(N, fields, p, stream), "sw2d_quad_output_kernel launch");
        return count;
    }

    // ---- run monitor and drifters (run_records.hpp)
    // records a stepping call of `steps` further completed steps would take; refused before anything is launched
    void monitorReserve(long long steps, const char* fn) const { mon.reserve(steps, fn, "bdg_sw2dq"); }
    void drifterReserve(long long steps, const char* fn) const { drf.reserve(steps, fn, "bdg_sw2dq"); }
    // completed LSERK4 steps among the next `stages` stages
    long long lserkSteps(long long stages) const { return bdg_records::lserkSteps(stageCount, stages, blitzdg::LSERK4::numStages); }
    // one record of the resident state, two launches on the solver's stream; H: the monitor's own, else variant B's, else none
    void monitorSample() {
        const int count = part.numOwned > 0 ? part.numOwned : K;
        const double* Hm = mon.H.p ? mon.H.p : (variantB ? vbH.p : nullptr);
        mon.sample({q.p, Hm, ld, Np, fields, count, g, timeNow}, sw2d_quad_monitor_finish_kernel, "sw2d_quad_monitor_finish_kernel launch",
                   MonTensorGauges{mon.lr.p, mon.ls.p, N + 1}, stream);
    }
    // one launch of the drifter kernel on the solver's stream; slot < 0: no record
    void drifterLaunch(int mode, double dt, int slot) {
        drf.launch(sw2d_quad_drifter_kernel, "sw2d_quad_drifter_kernel launch",
                   QuadDriftTables{drf.bil.p, drf.neigh.p, drf.r1d.p, drf.bary.p}, q.p, ld, N, mode, dt, slot, stream);
    }
    // one advance in the resident state, with the record of time drf.t if one is due (room was reserved by the caller)
    void drifterAdvance(double dt, bool record = true) { drifterLaunch(kDriftAdvance, dt, drf.takeSlot(record)); }
    // (u0, v0) again after the state under the drifters has been replaced
    void drifterResample() {
        if (drf.on) drifterLaunch(kDriftSample, 0.0, -1);
    }
    // what a sample of the field statistics reads; H by the monitor's rule: the statistics' own, else variant B's, else none
    bdg_records::StatsView statsView() const {
        const double* Hm = fst.H.p ? fst.H.p : (variantB ? vbH.p : nullptr);
        return {q.p, Hm, ld, Np, K, timeNow};
    }
    void statsSample() { fst.sample(statsView(), stream); }
    // after every completed step (of size dt) of a stepping call: the monitor's sample, the sample of the field statistics, then
    // the drifters' advance. two: the call runs the two-chain schedule, whose chains are joined in front of the monitor's sample
    // and started again behind it (the sample reads columns the exchange stream wrote); statistics and drifters exist on
    // unpartitioned solvers only
    void stepDone(double dt, bool two = false) {
        if (mon.on && ++mon.steps % mon.stride == 0) {
            if (two) chains.end(stream, halo.stream);
            monitorSample();
            if (two) chains.begin(stream, halo.stream);
        }
        if (fst.on && ++fst.steps % fst.stride == 0) statsSample();
        if (drf.on) {
            drf.t = timeNow;
            drifterAdvance(dt);
        }
    }

    ~bdg_sw2dq() { // both streams drained before the members destroy the events, the communicator and the exchange stream
        if (!stream) return;
        (void)hipSetDevice(device);
        (void)hipStreamSynchronize(stream);
        if (halo.stream) (void)hipStreamSynchronize(halo.stream);
        (void)hipStreamDestroy(stream);
    }
};

namespace {

using Eval = bdg_sw2dq::Eval;
using Stepper = bdg_sw2dq::Stepper;

void requireSolver(const bdg_sw2dq* s, const char* fn) {
    if (!s) throw arg_error(std::string(fn) + ": solver handle is NULL");
}

// the three-field calls are for three-field solvers and the *4 calls for four-field ones
void requireFields(const bdg_sw2dq* s, int fields, const char* fn) {
    if (s->fields != fields)
        throw arg_error(std::string(fn) + ": the solver was created with " + std::to_string(s->fields) + " fields; use " +
                        (s->fields == 4 ? "the *4 calls (h, hu, hv, hN)" : "the three-field calls (h, hu, hv)"));
}

void requireComm(const bdg_sw2dq* s, const char* fn) {
    requireSolver(s, fn);
    bdg_halo::requireComm(s->halo, "bdg_sw2dq", fn);
}

double maxAbs(const double* a, size_t n) {
    double m = 0.0;
    for (size_t i = 0; i < n; ++i) m = std::max(m, std::fabs(a[i]));
    return m;
}

bdg_sw2dq* createQuad(const bdg_sw2dq_desc& d, int fields) {
    const int N = d.order, K = d.num_elements;
    if (fields != 3 && fields != 4) throw arg_error("bdg_sw2dq_create: num_fields must be 3 or 4");
    if (N < 1 || N > BDG_SW2DQ_MAX_ORDER)
        throw arg_error("bdg_sw2dq_create: order " + std::to_string(N) + " is outside 1.." + std::to_string(BDG_SW2DQ_MAX_ORDER));
    if (K < 1) throw arg_error("bdg_sw2dq_create: num_elements < 1");
    if (!d.Dr || !d.Ds || !d.Lift || !d.rx || !d.sx || !d.ry || !d.sy || !d.nx || !d.ny || !d.Fscale || !d.vmapP)
        throw arg_error("bdg_sw2dq_create: NULL table");
    if (d.num_wall < 0 || (d.num_wall > 0 && !d.mapW)) throw arg_error("bdg_sw2dq_create: bad wall list");
    const int Nq = N + 1, Np = Nq * Nq, NFN = 4 * Nq;
    if (static_cast<long long>(Np) * (K + 64) >= (1LL << 31)) throw arg_error("bdg_sw2dq_create: mesh too large for int32 gathers");
    std::vector<double> opsHost = blitzdg::element_tables::tensorOperators("bdg_sw2dq_create", N, d.Dr, d.Ds, d.Lift);

    if (d.vmapM) {
        for (int k = 0; k < K; ++k)
            for (int f = 0; f < 4; ++f)
                for (int n = 0; n < Nq; ++n) {
                    const int fm = f == 0 ? Nq * n : (f == 1 ? Nq * N + n : (f == 2 ? Nq * n + N : n));
                    if (d.vmapM[(static_cast<size_t>(k) * 4 + f) * Nq + n] != fm + Np * k)
                        throw arg_error("bdg_sw2dq_create: vmapM is not the Gauss-Lobatto face numbering (faces s=-1, r=+1, s=+1, r=-1)");
                }
    }

    std::unique_ptr<bdg_sw2dq> s(new bdg_sw2dq());
    s->N = N; s->Np = Np; s->Nfp = Nq; s->NFN = NFN; s->K = K; s->g = d.g; s->device = d.device; s->fields = fields;
    s->fscaleMax = maxAbs(d.Fscale, static_cast<size_t>(NFN) * K);
    s->ld = (static_cast<long long>(K) + 63) / 64 * 64;
    const long long ld = s->ld;

    // gather index, [fn][ld]: vmapP entry of face node fn of element k, wall nodes with the sign bit
    std::vector<int> gi(static_cast<size_t>(NFN) * ld, 0);
    std::vector<char> wall(static_cast<size_t>(NFN) * K, 0);
    for (int w = 0; w < d.num_wall; ++w) {
        if (d.mapW[w] < 0 || d.mapW[w] >= NFN * K) throw arg_error("bdg_sw2dq_create: mapW entry out of range");
        wall[d.mapW[w]] = 1;
    }
    s->maxNeighbourHost.assign(static_cast<size_t>(K), 0);
    for (int k = 0; k < K; ++k)
        for (int fn = 0; fn < NFN; ++fn) {
            const size_t g = static_cast<size_t>(k) * NFN + fn;
            const int v = d.vmapP[g];
            if (v < 0 || v >= Np * K) throw arg_error("bdg_sw2dq_create: vmapP entry out of range");
            const long long off = static_cast<long long>(v % Np) * ld + v / Np;
            gi[static_cast<size_t>(fn) * ld + k] = wall[g] ? static_cast<int>(-(off + 1)) : static_cast<int>(off);
            s->maxNeighbourHost[static_cast<size_t>(k)] = std::max(s->maxNeighbourHost[static_cast<size_t>(k)], v / Np);
        }

    // geometry form: parallelograms (metric terms constant per element, nx, ny, Fscale per face, to 1e-10 relative), else general
    bool para = (d.flags & BDG_SW2DQ_GENERAL_GEOMETRY) == 0;
    std::vector<double> ag;
    if (para) {
        ag.assign(static_cast<size_t>(16) * ld, 0.0);
        para = blitzdg::element_tables::parallelogramForm({d.rx, d.sx, d.ry, d.sy, nullptr, d.nx, d.ny, d.Fscale}, Np, Nq, K,
                                                          static_cast<size_t>(ld), ag.data(), nullptr);
    }
    s->general = !para;

    s->use();
    hipCheck(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking), "hipStreamCreate");
    const long long plane = s->plane();
    s->q.alloc(fields * plane, s->bytes, s->stream);
    s->q1.alloc(fields * plane, s->bytes, s->stream);
    s->res.alloc(fields * plane, s->bytes, s->stream);
    s->gidx.alloc(gi.size(), s->bytes);
    hipCheck(hipMemcpyAsync(s->gidx.p, gi.data(), gi.size() * sizeof(int), hipMemcpyHostToDevice, s->stream), "hipMemcpy (gidx)");
    s->ops.alloc(opsHost.size(), s->bytes);
    hipCheck(hipMemcpyAsync(s->ops.p, opsHost.data(), opsHost.size() * sizeof(double), hipMemcpyHostToDevice, s->stream),
             "hipMemcpy (ops)");
    if (d.Filter) {
        s->filt.alloc(static_cast<size_t>(Np) * Np, s->bytes);
        hipCheck(hipMemcpyAsync(s->filt.p, d.Filter, static_cast<size_t>(Np) * Np * sizeof(double), hipMemcpyHostToDevice,
                                s->stream), "hipMemcpy (Filter)");
        s->hasFilter = true;
    }
    if (para) {
        s->ageo.alloc(ag.size(), s->bytes);
        hipCheck(hipMemcpyAsync(s->ageo.p, ag.data(), ag.size() * sizeof(double), hipMemcpyHostToDevice, s->stream),
                 "hipMemcpy (ageo)");
    } else {
        s->geo.alloc(4 * plane, s->bytes, s->stream);
        s->fgeo.alloc(3LL * NFN * ld, s->bytes, s->stream);
        const double* met[4] = {d.rx, d.sx, d.ry, d.sy};
        for (int a = 0; a < 4; ++a) s->upload(s->geo.p + a * plane, met[a], Np);
        s->upload(s->fgeo.p, d.nx, NFN);
        s->upload(s->fgeo.p + static_cast<long long>(NFN) * ld, d.ny, NFN);
        s->upload(s->fgeo.p + 2LL * NFN * ld, d.Fscale, NFN);
    }
    s->partials.alloc(2 * kHmaxBlocks, s->bytes);
    hipCheck(hipStreamSynchronize(s->stream), "hipStreamSynchronize (create)"); // host staging vectors die here
    return s.release();
}

// ---- what the three-field calls and their *4 twins share: `nf` fields, `fn` names the caller in the messages
void setState(bdg_sw2dq* s, int nf, const double* const* in, const std::string& fn) {
    requireSolver(s, fn.c_str());
    requireFields(s, nf, fn.c_str());
    if (std::find(in, in + nf, nullptr) != in + nf) throw arg_error(fn + ": NULL field");
    s->use();
    for (int c = 0; c < nf; ++c) s->upload(s->q.p + c * s->plane(), in[c], s->Np);
    s->res.zero(s->stream);
    s->stageCount = 0;
    s->mon.steps = 0;
    s->fst.steps = 0;
    s->drifterResample();
    hipCheck(hipStreamSynchronize(s->stream), "hipStreamSynchronize");
}

void getState(bdg_sw2dq* s, int nf, double* const* out, const char* fn) {
    requireSolver(s, fn);
    requireFields(s, nf, fn);
    s->use();
    for (int c = 0; c < nf; ++c)
        if (out[c]) s->download(out[c], s->q.p + c * s->plane(), s->Np);
    hipCheck(hipStreamSynchronize(s->stream), "hipStreamSynchronize");
}

void computeRhs(bdg_sw2dq* s, int nf, const double* const* in, double* const* out, int filter, const std::string& fn) {
    requireSolver(s, fn.c_str());
    requireFields(s, nf, fn.c_str());
    if (std::find(in, in + nf, nullptr) != in + nf || std::find(out, out + nf, nullptr) != out + nf)
        throw arg_error(fn + ": NULL argument");
    if (filter && !s->hasFilter) throw arg_error(fn + ": filter requested but the solver has no Filter");
    s->use();
    const long long plane = s->plane();
    if (!s->io.p) {
        s->io.alloc(nf * plane, s->bytes, s->stream);
        s->ioOut.alloc(nf * plane, s->bytes, s->stream);
    }
    for (int c = 0; c < nf; ++c) s->upload(s->io.p + c * plane, in[c], s->Np);
    QuadParams p = s->params();
    p.qin = s->io.p; p.rhs = s->ioOut.p;
    s->evaluate(Eval::Whole, QMODE_RHS, filter != 0, p);
    for (int c = 0; c < nf; ++c) s->download(out[c], s->ioOut.p + c * plane, s->Np);
    hipCheck(hipStreamSynchronize(s->stream), "hipStreamSynchronize");
}

// ---- what the stepping calls share: `count` steps (Stepper::Lserk: stages) of size dt, on a partition (`exchanged`) with the
// ghost exchange in front of every evaluation. The schedule is chosen once per call and the two chains bracket the whole call.
void stepping(bdg_sw2dq* s, const std::string& fn, Stepper kind, bool exchanged, double dt, int count, int filter,
              double spongeCoeff = 0.0) {
    if (exchanged) requireComm(s, fn.c_str());
    else requireSolver(s, fn.c_str());
    if (count < 0) throw arg_error(fn + (kind == Stepper::Lserk ? ": num_stages < 0" : ": num_steps < 0"));
    if (kind == Stepper::Heun && !s->variantB)
        throw arg_error(fn + ": variant B is not enabled" + (exchanged ? "" : " (the Heun step is the tidal driver's)"));
    if (filter && !s->hasFilter) throw arg_error(fn + ": filter requested but the solver has no Filter");
    const long long steps = kind == Stepper::Lserk ? s->lserkSteps(count) : count;
    s->monitorReserve(steps, fn.c_str());
    if (!exchanged) s->drifterReserve(steps, fn.c_str()); // (drifters exist on unpartitioned solvers only)
    s->use();
    if (kind == Stepper::Heun) s->spongeC = spongeCoeff;
    const Eval how = exchanged ? s->exchangedEval() : Eval::Whole;
    const bool two = how == Eval::TwoChains;
    if (two) s->chains.begin(s->stream, s->halo.stream);
    for (int i = 0; i < count; ++i)
        if (s->advance(kind, dt, filter != 0, how)) s->stepDone(dt, two);
    if (two) s->chains.end(s->stream, s->halo.stream);
    if (exchanged) s->checkBlowUp(s->part.numOwned, true);
    else s->checkBlowUp();
}

} // namespace

extern "C" {

int bdg_sw2dq_create(const bdg_sw2dq_desc* desc, bdg_sw2dq** out) {
    return guard([&] {
        if (!desc || !out) throw arg_error("bdg_sw2dq_create: NULL argument");
        *out = createQuad(*desc, 3);
    });
}

int bdg_sw2dq_create_fields(const bdg_sw2dq_desc* desc, int num_fields, bdg_sw2dq** out) {
    return guard([&] {
        if (!desc || !out) throw arg_error("bdg_sw2dq_create_fields: NULL argument");
        *out = createQuad(*desc, num_fields);
    });
}

int bdg_sw2dq_create_from_nodes(const bdg_quadnodes* nodes, double g, int device, int flags, bdg_sw2dq** out) {
    return bdg_sw2dq_create_from_nodes_fields(nodes, g, device, flags, 3, out);
}

int bdg_sw2dq_create_from_nodes_fields(const bdg_quadnodes* nodes, double g, int device, int flags, int num_fields,
                                       bdg_sw2dq** out) {
    return guard([&] {
        if (!nodes || !out) throw arg_error("bdg_sw2dq_create_from_nodes: NULL argument");
        const blitzdg::QuadNodesProvisioner& p = nodes->prov;
        bdg_sw2dq_desc d{};
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
        *out = createQuad(d, num_fields);
    });
}

void bdg_sw2dq_destroy(bdg_sw2dq* s) { delete s; }

int bdg_sw2dq_set_state(bdg_sw2dq* s, const double* h, const double* hu, const double* hv) {
    return guard([&] {
        const double* in[] = {h, hu, hv};
        setState(s, 3, in, "bdg_sw2dq_set_state");
    });
}

int bdg_sw2dq_get_state(bdg_sw2dq* s, double* h, double* hu, double* hv) {
    return guard([&] {
        double* out[] = {h, hu, hv};
        getState(s, 3, out, "bdg_sw2dq_get_state");
    });
}

int bdg_sw2dq_rhs(bdg_sw2dq* s, const double* h, const double* hu, const double* hv, double* rhs1, double* rhs2,
                  double* rhs3, int filter) {
    return guard([&] {
        const double* in[] = {h, hu, hv};
        double* out[] = {rhs1, rhs2, rhs3};
        computeRhs(s, 3, in, out, filter, "bdg_sw2dq_rhs");
    });
}

int bdg_sw2dq_num_fields(const bdg_sw2dq* s) { return s ? s->fields : -1; }

int bdg_sw2dq_set_sources(bdg_sw2dq* s, const double* zx, const double* zy, double f_scalar, const double* f_array, double CD) {
    return guard([&] {
        requireSolver(s, "bdg_sw2dq_set_sources");
        requireFields(s, 4, "bdg_sw2dq_set_sources");
        if (s->variantB) throw arg_error("bdg_sw2dq_set_sources: variant B is enabled and brings its own sources");
        if (s->evaluated)
            throw arg_error("bdg_sw2dq_set_sources: the solver has evaluated a right-hand side already; sources are set before the "
                            "first evaluation");
        if (!zx || !zy) throw arg_error("bdg_sw2dq_set_sources: zx / zy is NULL");
        s->use();
        const long long plane = s->plane();
        s->zx.alloc(plane, s->bytes, s->stream);
        s->zy.alloc(plane, s->bytes, s->stream);
        s->upload(s->zx.p, zx, s->Np);
        s->upload(s->zy.p, zy, s->Np);
        if (f_array) {
            s->fcor.alloc(plane, s->bytes, s->stream);
            s->upload(s->fcor.p, f_array, s->Np);
        } else if (s->fcor.p) {
            s->fcor.alloc(0, s->bytes);
        }
        s->fconst = f_scalar;
        s->CD = CD;
        s->hasSources = true;
        hipCheck(hipStreamSynchronize(s->stream), "hipStreamSynchronize");
    });
}

namespace {

// what bdg_sw2dq_enable_variant_b and _b4 share: the checks on the descriptor (`fn` names the caller in the messages), the
// gather index with the open-boundary nodes marked, the bed, the sponge and the tide
void checkVariantB(const bdg_sw2dq* s, const bdg_sw2dq_vb_desc* d, const std::string& fn) {
    if (s->evaluated)
        throw arg_error(fn + ": the solver has evaluated a right-hand side already; variant B is enabled "
                        "before the first evaluation");
    if (d->num_out < 0 || (d->num_out > 0 && !d->mapO)) throw arg_error(fn + ": bad open-boundary list");
    if (!(d->tide_period > 0.0) && d->num_out > 0) throw arg_error(fn + ": tide_period must be > 0");
    const long long nFaceNodes = static_cast<long long>(s->NFN) * s->K;
    for (int i = 0; i < d->num_out; ++i)
        if (d->mapO[i] < 0 || d->mapO[i] >= nFaceNodes)
            throw arg_error(fn + ": open-boundary node index out of range");
}

void enableVariantB(bdg_sw2dq* s, const bdg_sw2dq_vb_desc* d) {
    const long long plane = s->plane();
    // the gather index again, open-boundary nodes as kQuadBOpen (they win over the wall flag where a node has both)
    std::vector<int> gi(s->gidx.n);
    hipCheck(hipMemcpyAsync(gi.data(), s->gidx.p, gi.size() * sizeof(int), hipMemcpyDeviceToHost, s->stream), "hipMemcpy (gidx)");
    hipCheck(hipStreamSynchronize(s->stream), "hipStreamSynchronize");
    for (int i = 0; i < d->num_out; ++i) {
        const int k = d->mapO[i] / s->NFN, fn = d->mapO[i] % s->NFN;
        gi[static_cast<size_t>(fn) * s->ld + k] = kQuadBOpen;
    }
    s->gidxB.alloc(gi.size(), s->bytes);
    hipCheck(hipMemcpyAsync(s->gidxB.p, gi.data(), gi.size() * sizeof(int), hipMemcpyHostToDevice, s->stream), "hipMemcpy (gidx)");
    s->vbH.alloc(plane, s->bytes, s->stream);
    s->vbHx.alloc(plane, s->bytes, s->stream);
    s->vbHy.alloc(plane, s->bytes, s->stream);
    s->upload(s->vbH.p, d->H, s->Np);
    s->upload(s->vbHx.p, d->Hx, s->Np);
    s->upload(s->vbHy.p, d->Hy, s->Np);
    if (d->sponge) {
        s->vbSponge.alloc(plane, s->bytes, s->stream);
        s->upload(s->vbSponge.p, d->sponge, s->Np);
    } else if (s->vbSponge.p) {
        s->vbSponge.alloc(0, s->bytes);
    }
    s->lamBuf.alloc(1, s->bytes, s->stream);
    s->vbF = d->coriolis;
    s->vbCD = d->drag;
    s->tideAmp = d->tide_amplitude;
    s->tidePeriod = d->tide_period > 0.0 ? d->tide_period : 1.0;
    s->tideRamp = d->tide_ramp;
    hipCheck(hipStreamSynchronize(s->stream), "hipStreamSynchronize"); // the host staging vector dies here
    s->variantB = true;
}

} // namespace

int bdg_sw2dq_enable_variant_b(bdg_sw2dq* s, const bdg_sw2dq_vb_desc* d) {
    return guard([&] {
        requireSolver(s, "bdg_sw2dq_enable_variant_b");
        if (!d || !d->H || !d->Hx || !d->Hy) throw arg_error("bdg_sw2dq_enable_variant_b: H, Hx and Hy are required");
        if (s->fields != 3)
            throw arg_error("bdg_sw2dq_enable_variant_b: the solver was created with four fields; variant B has three (h, hu, hv)");
        checkVariantB(s, d, "bdg_sw2dq_enable_variant_b");
        s->use();
        enableVariantB(s, d);
    });
}

int bdg_sw2dq_enable_variant_b4(bdg_sw2dq* s, const bdg_sw2dq_vb_desc* d, const double* n_open, int n_open_count) {
    return guard([&] {
        const std::string fn = "bdg_sw2dq_enable_variant_b4";
        requireSolver(s, fn.c_str());
        if (!d || !d->H || !d->Hx || !d->Hy) throw arg_error(fn + ": H, Hx and Hy are required");
        if (s->fields != 4)
            throw arg_error(fn + ": the solver was created with three fields; the tracer needs four (bdg_sw2dq_create_fields)");
        if (s->hasSources)
            throw arg_error(fn + ": the solver has sources of bdg_sw2dq_set_sources; variant B brings its own");
        if (s->variantB) throw arg_error(fn + ": variant B is already enabled on this solver; the call is made once");
        checkVariantB(s, d, fn);
        // (without an open-boundary node no concentration is read: a count of 0 is then num_out, and n_open may be NULL)
        const bool none = d->num_out == 0 && n_open_count == 0;
        if (!none && (!n_open || (n_open_count != 1 && n_open_count != d->num_out)))
            throw arg_error(fn + ": n_open must hold 1 value or one per open-boundary node (num_out)");
        s->use();
        if (none || n_open_count == 1) { // (also a single open node given per node)
            s->nOpenC = none ? 0.0 : n_open[0];
            s->numOpenN = 0;
            s->openKey.alloc(0, s->bytes);
            s->openN.alloc(0, s->bytes);
        } else {
            // positions fn * ld + k in the gather index, sorted; the last entry of a node listed twice wins, as an assignment
            // through mapO does
            std::vector<std::pair<long long, int>> slots(static_cast<size_t>(d->num_out));
            for (int i = 0; i < d->num_out; ++i)
                slots[static_cast<size_t>(i)] = {static_cast<long long>(d->mapO[i] % s->NFN) * s->ld + d->mapO[i] / s->NFN, i};
            std::sort(slots.begin(), slots.end());
            std::vector<long long> keys;
            std::vector<double> vals;
            for (const auto& kv : slots) {
                if (!keys.empty() && keys.back() == kv.first) vals.back() = n_open[kv.second];
                else { keys.push_back(kv.first); vals.push_back(n_open[kv.second]); }
            }
            s->openKey.alloc(keys.size(), s->bytes);
            s->openN.alloc(vals.size(), s->bytes);
            hipCheck(hipMemcpyAsync(s->openKey.p, keys.data(), keys.size() * sizeof(long long), hipMemcpyHostToDevice, s->stream),
                     "hipMemcpy (open-boundary slots)");
            hipCheck(hipMemcpyAsync(s->openN.p, vals.data(), vals.size() * sizeof(double), hipMemcpyHostToDevice, s->stream),
                     "hipMemcpy (open-boundary tracer)");
            hipCheck(hipStreamSynchronize(s->stream), "hipStreamSynchronize"); // the host staging vectors die here
            s->numOpenN = static_cast<int>(keys.size());
        }
        enableVariantB(s, d);
    });
}

int bdg_sw2dq_enable_tracer_diffusion(bdg_sw2dq* s, const bdg_sw2d_diffusion_desc* d) {
    return guard([&] {
        const std::string fn = "bdg_sw2dq_enable_tracer_diffusion";
        requireSolver(s, fn.c_str());
        if (!d) throw arg_error(fn + ": NULL descriptor");
        if (s->fields != 4)
            throw arg_error(fn + ": the solver was created with three fields; the tracer needs four (bdg_sw2dq_create_fields)");
        if (s->diffusion) throw arg_error(fn + ": tracer diffusion is already enabled on this solver; the call is made once");
        if (s->evaluated)
            throw arg_error(fn + ": the solver has evaluated a right-hand side already; diffusion is enabled before the first evaluation");
        if (s->part.numOwned > 0 || s->halo.comm)
            throw arg_error(fn + ": the solver has a partition set; the diffusion passes cover a single domain only");
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
                if (!(d->source[i] >= 0.0) || !std::isfinite(d->source[i]))
                    throw arg_error(fn + ": the source must be finite and >= 0 at every node");
        const QuadDiffusionKernelTable* ktd = quad_diffusion_kernel_table(s->N);
        if (!ktd) throw arg_error(fn + ": no diffusion kernels compiled for this order");
        s->use();
        const long long plane = s->plane();
        QuadDiffusionParams dp{};
        dp.kappa = d->kappa;
        dp.decay = d->decay;
        if (d->kappa_field) {
            s->difKappa.alloc(plane, s->bytes, s->stream);
            s->upload(s->difKappa.p, d->kappa_field, s->Np);
        }
        if (d->source) {
            s->difSource.alloc(plane, s->bytes, s->stream);
            s->upload(s->difSource.p, d->source, s->Np);
        }
        s->difFlux.alloc(2 * plane, s->bytes, s->stream);
        hipCheck(hipStreamSynchronize(s->stream), "hipStreamSynchronize"); // the caller's arrays are free again
        dp.kappaField = s->difKappa.p;
        dp.source = s->difSource.p;
        dp.flux = s->difFlux.p;
        const double n1 = static_cast<double>(s->N + 1);
        s->difDt = kmax > 0.0 ? bdg_sw2dq::kDiffusionDtConstant / (kmax * n1 * n1 * n1 * n1 * s->fscaleMax * s->fscaleMax)
                              : std::numeric_limits<double>::infinity();
        s->ktd = ktd;
        s->dif = dp;
        s->diffusion = true;
    });
}

int bdg_sw2dq_diffusion_dt(const bdg_sw2dq* s, double* dt_diff) {
    return guard([&] {
        requireSolver(s, "bdg_sw2dq_diffusion_dt");
        if (!dt_diff) throw arg_error("bdg_sw2dq_diffusion_dt: NULL argument");
        if (!s->diffusion) throw arg_error("bdg_sw2dq_diffusion_dt: tracer diffusion is not enabled");
        *dt_diff = s->difDt;
    });
}

int bdg_sw2dq_set_time(bdg_sw2dq* s, double t) {
    return guard([&] {
        requireSolver(s, "bdg_sw2dq_set_time");
        s->timeNow = t;
    });
}

int bdg_sw2dq_get_time(const bdg_sw2dq* s, double* t) {
    return guard([&] {
        requireSolver(s, "bdg_sw2dq_get_time");
        if (!t) throw arg_error("bdg_sw2dq_get_time: NULL argument");
        *t = s->timeNow;
    });
}

int bdg_sw2dq_global_speed(bdg_sw2dq* s, double* lam) {
    return guard([&] {
        requireSolver(s, "bdg_sw2dq_global_speed");
        if (!s->variantB || !lam) throw arg_error("bdg_sw2dq_global_speed: variant B is not enabled");
        s->use();
        hipCheck(hipMemcpyAsync(lam, s->lamBuf.p, sizeof(double), hipMemcpyDeviceToHost, s->stream), "hipMemcpy (speed)");
        hipCheck(hipStreamSynchronize(s->stream), "hipStreamSynchronize");
    });
}

int bdg_sw2dq_time_speed(bdg_sw2dq* s, int count, float* ms) {
    return guard([&] {
        requireSolver(s, "bdg_sw2dq_time_speed");
        if (!ms || count < 1) throw arg_error("bdg_sw2dq_time_speed: bad argument");
        if (!s->variantB) throw arg_error("bdg_sw2dq_time_speed: variant B is not enabled");
        s->use();
        const int owned = s->part.numOwned > 0 ? s->part.numOwned : s->K;
        *ms = timePerRun(s->stream, count, [&] { s->speedPass(s->q.p, owned); });
    });
}

int bdg_sw2dq_step_ssprk2(bdg_sw2dq* s, double dt, int num_steps, int filter, double sponge_coeff) {
    return guard([&] { stepping(s, "bdg_sw2dq_step_ssprk2", Stepper::Heun, false, dt, num_steps, filter, sponge_coeff); });
}

int bdg_sw2dq_set_state4(bdg_sw2dq* s, const double* h, const double* hu, const double* hv, const double* hN) {
    return guard([&] {
        const double* in[] = {h, hu, hv, hN};
        setState(s, 4, in, "bdg_sw2dq_set_state4");
    });
}

int bdg_sw2dq_get_state4(bdg_sw2dq* s, double* h, double* hu, double* hv, double* hN) {
    return guard([&] {
        double* out[] = {h, hu, hv, hN};
        getState(s, 4, out, "bdg_sw2dq_get_state4");
    });
}

int bdg_sw2dq_rhs4(bdg_sw2dq* s, const double* h, const double* hu, const double* hv, const double* hN, double* rhs1, double* rhs2,
                   double* rhs3, double* rhs4, int filter) {
    return guard([&] {
        const double* in[] = {h, hu, hv, hN};
        double* out[] = {rhs1, rhs2, rhs3, rhs4};
        computeRhs(s, 4, in, out, filter, "bdg_sw2dq_rhs4");
    });
}

int bdg_sw2dq_compute_dt(bdg_sw2dq* s, double cfl, double* dt, double* speed) {
    return guard([&] {
        requireSolver(s, "bdg_sw2dq_compute_dt");
        s->use();
        const bool collective = s->halo.comm != nullptr;
        double m = s->maxFaceSpeed(collective ? s->part.numOwned : s->K);
        if (collective) { // NaN does not survive a max-reduction reliably: send it as +inf
            double v[2] = {std::isnan(m) ? std::numeric_limits<double>::infinity() : m, 0.0};
            hipCheck(hipMemcpyAsync(s->halo.scalarBuf.p, v, sizeof(v), hipMemcpyHostToDevice, s->stream), "hipMemcpy (compute_dt)");
            bdg_rccl::ncclCheck(bdg_rccl::rccl().AllReduce(s->halo.scalarBuf.p, s->halo.scalarBuf.p, 2, ncclDouble, ncclMax,
                                                           s->halo.comm, s->stream), "ncclAllReduce");
            hipCheck(hipMemcpyAsync(v, s->halo.scalarBuf.p, sizeof(v), hipMemcpyDeviceToHost, s->stream), "hipMemcpy (compute_dt)");
            hipCheck(hipStreamSynchronize(s->stream), "hipStreamSynchronize");
            m = v[0];
        }
        if (speed) *speed = m;
        if (dt) *dt = cfl / ((s->N + 1) * (s->N + 1) * 0.5 * m);
        if (dt && s->diffusion) *dt = std::min(*dt, cfl * s->difDt);
        if (std::isnan(m) || std::isinf(m)) throw unstable_error("A numerical instability has occurred!");
    });
}

int bdg_sw2dq_output_fields(bdg_sw2dq* s, const double* H, const double* lattice, double* eta, double* u, double* v, double* N) {
    return guard([&] {
        requireSolver(s, "bdg_sw2dq_output_fields");
        if (N && s->fields != 4) throw arg_error("bdg_sw2dq_output_fields: N = hN / h needs a solver with four fields");
        double* out[4] = {eta, u, v, N};
        int mask = 0;
        for (int c = 0; c < 4; ++c) mask |= out[c] ? 1 << c : 0;
        if (!mask) return;
        s->use();
        const int count = s->outputLaunch(H, lattice, mask);
        const long long plane = s->plane();
        for (int c = 0; c < 4; ++c)
            if (out[c]) // the columns [0, count) of each row
                hipCheck(hipMemcpy2DAsync(out[c], s->K * sizeof(double), s->q1.p + c * plane, s->ld * sizeof(double),
                                          count * sizeof(double), s->Np, hipMemcpyDeviceToHost, s->stream), "hipMemcpy2D (download)");
        hipCheck(hipStreamSynchronize(s->stream), "hipStreamSynchronize");
    });
}

int bdg_sw2dq_time_output(bdg_sw2dq* s, const double* H, const double* lattice, int count, float* ms) {
    return guard([&] {
        requireSolver(s, "bdg_sw2dq_time_output");
        if (!ms || count < 1) throw arg_error("bdg_sw2dq_time_output: bad argument");
        s->use();
        const int mask = (1 << s->fields) - 1;
        s->outputLaunch(H, lattice, mask); // uploads H and I1; not timed
        *ms = timePerRun(s->stream, count, [&] { s->outputLaunch(H, lattice, mask, false); });
    });
}

int bdg_sw2dq_step_rk2(bdg_sw2dq* s, double dt, int num_steps, int filter) {
    return guard([&] { stepping(s, "bdg_sw2dq_step_rk2", Stepper::Rk2, false, dt, num_steps, filter); });
}

int bdg_sw2dq_lserk4_stages(bdg_sw2dq* s, double dt, int num_stages) {
    return guard([&] { stepping(s, "bdg_sw2dq_lserk4_stages", Stepper::Lserk, false, dt, num_stages, 0); });
}

int bdg_sw2dq_time(bdg_sw2dq* s, int kind, double dt, int count, float* ms) {
    return guard([&] {
        requireSolver(s, "bdg_sw2dq_time");
        if (!ms || count < 1 || kind < 0 || kind > 2) throw arg_error("bdg_sw2dq_time: bad argument");
        if (kind == 2 && !s->variantB) throw arg_error("bdg_sw2dq_time: the Heun step needs variant B");
        if (kind == 1 && !s->hasFilter) throw arg_error("bdg_sw2dq_time: RK2 + filter needs a Filter");
        s->use();
        // (steps without stepDone: nothing is recorded and no drifter moves; one check at the end)
        *ms = timePerRun(s->stream, count, [&] { s->advance(static_cast<Stepper>(kind), dt, kind == 1, Eval::Whole); });
        s->checkBlowUp();
    });
}

int bdg_sw2dq_synchronize(bdg_sw2dq* s) {
    return guard([&] {
        requireSolver(s, "bdg_sw2dq_synchronize");
        s->use();
        hipCheck(hipStreamSynchronize(s->stream), "hipStreamSynchronize");
    });
}

int bdg_sw2dq_set_partition(bdg_sw2dq* s, int num_interior, int num_owned, const int* send_elements, int num_send) {
    return guard([&] {
        requireSolver(s, "bdg_sw2dq_set_partition");
        if (s->diffusion)
            throw arg_error("bdg_sw2dq_set_partition: the solver has tracer diffusion, whose passes cover a single domain only");
        if (s->drf.on)
            throw arg_error("bdg_sw2dq_set_partition: the solver has drifters, which do not migrate between ranks (single domain only)");
        if (s->fst.on)
            throw arg_error("bdg_sw2dq_set_partition: the solver has field statistics, which cover a single domain only");
        s->use();
        s->part.set("bdg_sw2dq", s->K, s->maxNeighbourHost, num_interior, num_owned, send_elements, num_send, s->halo.comm != nullptr,
                    s->bytes, s->stream);
    });
}

int bdg_sw2dq_comm_init(bdg_sw2dq* s, int rank, int world, const void* unique_id, const int* peer_ranks, const int* send_start,
                        const int* send_count, const int* recv_start, const int* recv_count, int num_peers) {
    return guard([&] {
        requireSolver(s, "bdg_sw2dq_comm_init");
        if (s->fst.on) throw arg_error("bdg_sw2dq_comm_init: the solver has field statistics, which cover a single domain only");
        s->use();
        bdg_halo::commInit("bdg_sw2dq", s->halo, s->part, s->chains, s->K, static_cast<size_t>(s->fields) * s->Np, rank, world, unique_id,
                           peer_ranks, send_start, send_count, recv_start, recv_count, num_peers, s->bytes, s->stream);
    });
}

int bdg_sw2dq_exchange(bdg_sw2dq* s, int intermediate) {
    return guard([&] {
        requireComm(s, "bdg_sw2dq_exchange");
        s->use();
        s->exchangeOn(intermediate ? s->q1.p : s->q.p, s->stream);
    });
}

int bdg_sw2dq_step_rk2_exchanged(bdg_sw2dq* s, double dt, int num_steps, int filter) {
    return guard([&] { stepping(s, "bdg_sw2dq_step_rk2_exchanged", Stepper::Rk2, true, dt, num_steps, filter); });
}

int bdg_sw2dq_step_ssprk2_exchanged(bdg_sw2dq* s, double dt, int num_steps, int filter, double sponge_coeff) {
    return guard([&] { stepping(s, "bdg_sw2dq_step_ssprk2_exchanged", Stepper::Heun, true, dt, num_steps, filter, sponge_coeff); });
}

int bdg_sw2dq_lserk4_stages_exchanged(bdg_sw2dq* s, double dt, int num_stages) {
    return guard([&] { stepping(s, "bdg_sw2dq_lserk4_stages_exchanged", Stepper::Lserk, true, dt, num_stages, 0); });
}

int bdg_sw2dq_barrier(bdg_sw2dq* s) {
    return guard([&] {
        requireComm(s, "bdg_sw2dq_barrier");
        s->use();
        bdg_halo::barrier(s->halo, s->stream);
    });
}

// ---- run monitor (what the triangle solver has too: run_records.hpp)
int bdg_sw2dq_enable_monitor(bdg_sw2dq* s, const bdg_sw2dq_monitor_desc* d) {
    return guard([&] {
        const std::string fn = "bdg_sw2dq_enable_monitor";
        requireSolver(s, fn.c_str());
        bdg_sw2dq::Monitor& m = s->mon;
        m.checkEnable(fn, d, s->K);
        const int ng = d->num_gauges, Nq = s->N + 1;
        if (ng > 0 && (!d->gauge_r || !d->gauge_s)) throw arg_error(fn + ": bad gauge list");
        for (int i = 0; i < ng; ++i)
            if (!(std::fabs(d->gauge_r[i]) <= 1.0 + 1e-10) || !(std::fabs(d->gauge_s[i]) <= 1.0 + 1e-10))
                throw arg_error(fn + ": gauge " + std::to_string(i) + " lies outside its element (|r|, |s| <= 1)");
        // the 1-D basis at every gauge, on the solver's Gauss-Lobatto points
        blitzdg::real_vector_type r1d(Nq);
        blitzdg::JacobiBuilders().computeGaussLobottoPoints(0.0, 0.0, s->N, r1d);
        std::vector<double> lr(static_cast<size_t>(std::max(1, ng)) * Nq, 0.0), ls(lr.size(), 0.0);
        for (int i = 0; i < ng; ++i) {
            blitzdg::QuadNodesProvisioner::lagrangeBasis1D(r1d.data(), Nq, d->gauge_r[i], lr.data() + static_cast<size_t>(i) * Nq);
            blitzdg::QuadNodesProvisioner::lagrangeBasis1D(r1d.data(), Nq, d->gauge_s[i], ls.data() + static_cast<size_t>(i) * Nq);
        }
        s->use();
        m.enable(d->stride, d->capacity, ng, s->fields, d->gauge_element, {&m.lr, &m.ls}, nullptr, s->bytes, s->stream, [&] {
            const long long plane = s->plane();
            m.w.alloc(plane, s->bytes, s->stream);
            s->upload(m.w.p, d->weights, s->Np);
            if (d->H) {
                m.H.alloc(plane, s->bytes, s->stream);
                s->upload(m.H.p, d->H, s->Np);
            }
            m.lr.alloc(lr.size(), s->bytes);
            m.ls.alloc(ls.size(), s->bytes);
            hipCheck(hipMemcpyAsync(m.lr.p, lr.data(), lr.size() * sizeof(double), hipMemcpyHostToDevice, s->stream), "hipMemcpy (basis)");
            hipCheck(hipMemcpyAsync(m.ls.p, ls.data(), ls.size() * sizeof(double), hipMemcpyHostToDevice, s->stream), "hipMemcpy (basis)");
        });
    });
}

namespace {
void requireMonitor(const bdg_sw2dq* s, const char* fn) {
    requireSolver(s, fn);
    s->mon.requireOn(fn, "bdg_sw2dq");
}
} // namespace

int bdg_sw2dq_monitor_sample(bdg_sw2dq* s) {
    return guard([&] {
        requireMonitor(s, "bdg_sw2dq_monitor_sample");
        s->mon.requireFree("bdg_sw2dq_monitor_sample", "bdg_sw2dq");
        s->use();
        s->monitorSample();
    });
}

int bdg_sw2dq_monitor_count(const bdg_sw2dq* s, int* n) {
    return guard([&] {
        requireMonitor(s, "bdg_sw2dq_monitor_count");
        if (!n) throw arg_error("bdg_sw2dq_monitor_count: NULL argument");
        *n = s->mon.count;
    });
}

int bdg_sw2dq_monitor_width(const bdg_sw2dq* s, int* width) {
    return guard([&] {
        requireMonitor(s, "bdg_sw2dq_monitor_width");
        if (!width) throw arg_error("bdg_sw2dq_monitor_width: NULL argument");
        *width = s->mon.width;
    });
}

int bdg_sw2dq_monitor_read(bdg_sw2dq* s, int first, int count, double* records) {
    return guard([&] {
        requireMonitor(s, "bdg_sw2dq_monitor_read");
        s->use();
        s->mon.read("bdg_sw2dq_monitor_read", first, count, records, s->stream);
    });
}

int bdg_sw2dq_monitor_reset(bdg_sw2dq* s) {
    return guard([&] {
        requireMonitor(s, "bdg_sw2dq_monitor_reset");
        s->mon.reset();
    });
}

int bdg_sw2dq_monitor_reduce(bdg_sw2dq* s) {
    return guard([&] {
        requireMonitor(s, "bdg_sw2dq_monitor_reduce");
        bdg_halo::requireComm(s->halo, "bdg_sw2dq", "bdg_sw2dq_monitor_reduce");
        s->use();
        s->mon.allReduce(s->halo.comm, s->stream, s->fields, s->bytes);
    });
}

// ---- drifters
int bdg_sw2dq_enable_drifters(bdg_sw2dq* s, const bdg_sw2dq_drifter_desc* d) {
    return guard([&] {
        const std::string fn = "bdg_sw2dq_enable_drifters";
        requireSolver(s, fn.c_str());
        if (!d || d->count < 1 || !d->element || !d->r || !d->s || !d->bilinear || !d->neighbours || !d->bary)
            throw arg_error(fn + ": the descriptor, at least one drifter and the tables of bdg_quadnodes_drifter_tables are required");
        bdg_sw2dq::Drifters& m = s->drf;
        m.checkEnable(fn, d->count, d->stride, d->capacity, s->part.numOwned > 0 || s->halo.comm);
        const int n = d->count, K = s->K, Nq = s->N + 1;
        for (int i = 0; i < n; ++i) {
            if (d->element[i] < 0 || d->element[i] >= K)
                throw arg_error(fn + ": drifter " + std::to_string(i) + " names an element outside [0, K)");
            if (!(std::fabs(d->r[i]) <= 1.0 + 1e-10) || !(std::fabs(d->s[i]) <= 1.0 + 1e-10))
                throw arg_error(fn + ": drifter " + std::to_string(i) + " lies outside its element (|r|, |s| <= 1)");
        }
        // the kernel follows these entries without a further check
        std::vector<int> nb(static_cast<size_t>(4) * K);
        for (int f = 0; f < 4; ++f)
            for (int k = 0; k < K; ++k) {
                const int v = d->neighbours[static_cast<size_t>(f) * K + k];
                if (v < kDriftOpen || v >= K) throw arg_error(fn + ": neighbour entry out of range");
                nb[static_cast<size_t>(4) * k + f] = v;
            }
        blitzdg::real_vector_type r1d(Nq);
        blitzdg::JacobiBuilders().computeGaussLobottoPoints(0.0, 0.0, s->N, r1d);
        s->use();
        m.enable(n, d->stride, d->capacity, s->timeNow, nb, d->element, d->r, d->s, {&m.bil, &m.r1d, &m.bary}, s->bytes, s->stream,
                 [&] {
                     m.put(m.bil, d->bilinear, static_cast<size_t>(8) * K, s->bytes, s->stream);
                     m.put(m.r1d, r1d.data(), static_cast<size_t>(Nq), s->bytes, s->stream);
                     m.put(m.bary, d->bary, static_cast<size_t>(Nq), s->bytes, s->stream);
                 },
                 [&] { s->drifterLaunch(kDriftInit, 0.0, -1); });
    });
}

namespace {
void requireDrifters(const bdg_sw2dq* s, const char* fn) {
    requireSolver(s, fn);
    s->drf.requireOn(fn, "bdg_sw2dq");
}
} // namespace

int bdg_sw2dq_drifters_advance(bdg_sw2dq* s, double dt, int num_steps) {
    return guard([&] {
        requireDrifters(s, "bdg_sw2dq_drifters_advance");
        if (num_steps < 0) throw arg_error("bdg_sw2dq_drifters_advance: num_steps < 0");
        s->drifterReserve(num_steps, "bdg_sw2dq_drifters_advance");
        s->use();
        for (int i = 0; i < num_steps; ++i) {
            s->drf.t += dt;
            s->drifterAdvance(dt);
        }
    });
}

int bdg_sw2dq_drifters_time(bdg_sw2dq* s, double dt, int count, float* ms) {
    return guard([&] {
        requireDrifters(s, "bdg_sw2dq_drifters_time");
        if (!ms || count < 1) throw arg_error("bdg_sw2dq_drifters_time: bad argument");
        s->use();
        *ms = timePerRun(s->stream, count, [&] { s->drifterAdvance(dt, false); });
    });
}

int bdg_sw2dq_drifters_state(bdg_sw2dq* s, double* x, double* y, int* element, double* r, double* sref, int* status) {
    return guard([&] {
        requireDrifters(s, "bdg_sw2dq_drifters_state");
        s->use();
        s->drf.downloadState(x, y, element, r, sref, status, {}, s->stream);
    });
}

int bdg_sw2dq_drifters_count(const bdg_sw2dq* s, int* num_records, int* num_drifters) {
    return guard([&] {
        requireDrifters(s, "bdg_sw2dq_drifters_count");
        if (num_records) *num_records = s->drf.count;
        if (num_drifters) *num_drifters = s->drf.n;
    });
}

int bdg_sw2dq_drifters_read(bdg_sw2dq* s, int first, int count, double* t, double* x, double* y, int* status) {
    return guard([&] {
        requireDrifters(s, "bdg_sw2dq_drifters_read");
        s->use();
        s->drf.readTracks("bdg_sw2dq_drifters_read", first, count, t, x, y, status, s->stream);
    });
}

int bdg_sw2dq_drifters_reset(bdg_sw2dq* s) {
    return guard([&] {
        requireDrifters(s, "bdg_sw2dq_drifters_reset");
        s->drf.count = 0;
    });
}

// ---- field statistics (what the triangle solver has too: run_records.hpp)
int bdg_sw2dq_enable_field_stats(bdg_sw2dq* s, const bdg_field_stats_desc* d) {
    return guard([&] {
        const std::string fn = "bdg_sw2dq_enable_field_stats";
        requireSolver(s, fn.c_str());
        s->fst.checkEnable(fn, d, s->part.numOwned > 0 || s->halo.comm);
        s->use();
        s->fst.enable(*d, static_cast<size_t>(s->plane()), s->bytes, s->stream, [&] {
            if (!d->H) return;
            s->fst.H.alloc(static_cast<size_t>(s->plane()), s->bytes, s->stream);
            s->upload(s->fst.H.p, d->H, s->Np);
        });
    });
}

namespace {
void requireStats(const bdg_sw2dq* s, const char* fn) {
    requireSolver(s, fn);
    s->fst.requireOn(fn, "bdg_sw2dq");
}
} // namespace

int bdg_sw2dq_field_stats_sample(bdg_sw2dq* s) {
    return guard([&] {
        requireStats(s, "bdg_sw2dq_field_stats_sample");
        s->use();
        s->statsSample();
    });
}

int bdg_sw2dq_field_stats_count(const bdg_sw2dq* s, int* samples, int* num_periods) {
    return guard([&] {
        requireStats(s, "bdg_sw2dq_field_stats_count");
        if (!samples || !num_periods) throw arg_error("bdg_sw2dq_field_stats_count: NULL argument");
        *samples = s->fst.count();
        *num_periods = s->fst.m;
    });
}

int bdg_sw2dq_field_stats_read(bdg_sw2dq* s, int which, int index, double* plane) {
    return guard([&] {
        requireStats(s, "bdg_sw2dq_field_stats_read");
        if (!plane) throw arg_error("bdg_sw2dq_field_stats_read: NULL argument");
        const double* dev = s->fst.planeOf("bdg_sw2dq_field_stats_read", which, index);
        s->use();
        s->download(plane, dev, s->Np);
        hipCheck(hipStreamSynchronize(s->stream), "hipStreamSynchronize");
    });
}

int bdg_sw2dq_field_stats_samples(const bdg_sw2dq* s, int first, int count, double* rows) {
    return guard([&] {
        requireStats(s, "bdg_sw2dq_field_stats_samples");
        s->fst.samples("bdg_sw2dq_field_stats_samples", first, count, rows);
    });
}

int bdg_sw2dq_field_stats_reset(bdg_sw2dq* s) {
    return guard([&] {
        requireStats(s, "bdg_sw2dq_field_stats_reset");
        s->use();
        s->fst.reset(s->stream);
    });
}

int bdg_sw2dq_field_stats_time(bdg_sw2dq* s, int count, float* ms) {
    return guard([&] {
        requireStats(s, "bdg_sw2dq_field_stats_time");
        if (count < 1 || !ms) throw arg_error("bdg_sw2dq_field_stats_time: bad argument");
        s->use();
        *ms = s->fst.time(s->statsView(), count, s->bytes, s->stream);
    });
}

size_t bdg_sw2dq_device_bytes(const bdg_sw2dq* s) { return s ? s->bytes : 0; }

int bdg_sw2dq_uses_parallelogram_geometry(const bdg_sw2dq* s) { return s ? (s->general ? 0 : 1) : -1; }

} // extern "C"
