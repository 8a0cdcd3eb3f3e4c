// C ABI of the curved / over-integrated sw2d solver (include/blitzdg_hip.h, bdg_sw2d_curved_*): device layout, uploads of
// the host tables (host/curved_tables.cpp), launches. Kernels: sw2d_curved_kernel.hpp, sw2d_curved_nt_kernel.hpp; the driver's
// adaptive step, blow-up check and output fields (bdg_sw2d_curved_enable_driver): sw2d_curved_driver_kernel.hpp; the run monitor,
// the field statistics and the drifters: run_records.hpp with sw2d_curved_drifter_kernel.hpp.
// Reference: swhelpers/rhs.py:6-176 (the RHS), sw2d_curved.py:231-302 (the time loop).
#include "../host/capi_internal.hpp"
#include "../host/curved_tables.hpp"
#include "blitzdg/LSERK4.hpp"
#include "partition_schedule.hpp"
#include "run_records.hpp"
#include "sw2d_curved_drifter_kernel.hpp"
#include "sw2d_curved_driver_kernel.hpp"
#include "sw2d_curved_kernel.hpp"
#include "sw2d_curved_kernel_info.hpp"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

// ---- per-order objects (sw2d_curved_order.hip): the launch table, and which instance its launch path picks
#define BDG_CURVED_ORDERS(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8)
namespace bdg_dev {
static_assert(kCurvedKernelInfoFields == BDG_SW2D_CURVED_KERNEL_INFO_FIELDS, "the C ABI and the order objects disagree on the fields");
#define BDG_DECLARE(n) const CurvedKernelTable* curved_kernel_table_order##n(); CurvedKernelInfoFn curved_kernel_info_order##n();
BDG_CURVED_ORDERS(BDG_DECLARE)
#undef BDG_DECLARE
struct CurvedOrder { const CurvedKernelTable* (*table)(); CurvedKernelInfoFn (*info)(); };
#define BDG_ENTRY(n) {curved_kernel_table_order##n, curved_kernel_info_order##n},
const CurvedOrder kCurvedOrders[] = {BDG_CURVED_ORDERS(BDG_ENTRY)};
#undef BDG_ENTRY
const CurvedOrder* curvedOrder(int order) { // nullptr: not compiled in
    return order >= 1 && order <= static_cast<int>(sizeof(kCurvedOrders) / sizeof(kCurvedOrders[0])) ? &kCurvedOrders[order - 1] : nullptr;
}
const CurvedKernelTable* curved_kernel_table(int order) { return curvedOrder(order) ? curvedOrder(order)->table() : nullptr; }
} // namespace bdg_dev

using bdg_detail::arg_error;
using bdg_detail::guard;
using bdg_detail::hip_error;
using bdg_detail::unstable_error;

using bdg_dev::DevBuf;
using bdg_dev::hipCheck;
namespace tables = blitzdg::curved_tables;

namespace {
// ---- switches. Read when a solver is created (the first three by bdg_sw2d_curved_plan too: they decide
// tables; PRIO is handed to the kernel, and read once the nodal-trace form is chosen):
tables::Switches creationSwitches() {
    tables::Switches sw;
    sw.general = std::getenv("BDG_SW2D_CURVED_GENERAL") != nullptr;           // keep the general form (A/B, cross-check)
    sw.noAffine = std::getenv("BDG_SW2D_CURVED_NO_AFFINE") != nullptr;        // no straight-element compression
    sw.noTileOrder = std::getenv("BDG_SW2D_CURVED_NO_TILE_ORDER") != nullptr; // tiles in mesh order
    return sw;
}
int prioSwitch(int unset) { const char* e = std::getenv("BDG_SW2D_CURVED_PRIO"); return e ? std::atoi(e) : unset; } // (A/B: sw2d_curved_nt_kernel)
// once per process, by the first evaluation on the nodal-trace form:
int tileInterleave() {
    static const int v = [] { const char* e = std::getenv("BDG_SW2D_TILE_INTERLEAVE"); return e ? std::atoi(e) : 1; }();
    return v;
}
// per call:
bool noOverlap() { return std::getenv("BDG_SW2D_CURVED_NO_OVERLAP") != nullptr; } // (A/B: exchange, then every element, in stream order)

const char* const kNoFilter = "bdg_sw2d_curved: filter requested but the solver was created without a Filter matrix";

// `rows` rows of `width` bytes between pitched host and device arrays on `stream`, waited for
void copyRows(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t rows, hipMemcpyKind kind, hipStream_t stream) {
    const bool up = kind == hipMemcpyHostToDevice;
    hipCheck(hipMemcpy2DAsync(dst, dpitch, src, spitch, width, rows, kind, stream), up ? "H2D copy" : "D2H copy");
    hipCheck(hipStreamSynchronize(stream), up ? "upload sync" : "download sync");
}
} // namespace

struct bdg_sw2d_curved {
    const bdg_dev::CurvedKernelTable* kt = nullptr;
    int N = 0, Np = 0, K = 0, device = 0, ncub = 0, ncb = 0, ng = 0, fb = 0, numCurved = 0;
    long long ld = 0, sideLd = 0;
    bool hasFilter = false, identityM = true;
    hipStream_t stream = nullptr;
    size_t bytes = 0;
    DevBuf<double> qA, qB, res, rhs, gq, cubG, gaussG, coef, mmSide, minvSide, ops, filt;
    // nodal coefficient planes inside coef (one allocation: the stage kernel reaches all of them through one buffer
    // descriptor): 1 / J first, then whichever of zx, zy, f, CD the caller gave (nullptr: absent)
    double *rJ = nullptr, *zx = nullptr, *zy = nullptr, *fcor = nullptr, *cd = nullptr;
    DevBuf<int> gmapP, gmapM, curvedSlot, curvedEls, affineEl;
    DevBuf<double> cubAffine, cubWref;
    int numAffine = 0;
    // nodal-trace form (sw2d_curved_nt_kernel.hpp): used when the context has the structure it needs (useNT)
    bool useNT = false;
    DevBuf<double> opsNT, elAffine, gaussWref;
    DevBuf<double> cubWrefNT; // its reference weights when its reference element is not the general form's (else cubWref serves both)
    DevBuf<int> nodeP, faceFlags, faceNodesDev, tileOrder;
    int prioMode = 2;   // see sw2d_curved_nt_kernel (BDG_SW2D_CURVED_PRIO)
    double g = 9.81, fconst = 0.0, cdconst = 0.0;
    long long stageCount = 0;
    double bytesPerElement = 0.0;
    // partitioned runs (bdg_sw2d_curved_set_partition / _comm_init): partition_schedule.hpp. The two-chain schedule needs the
    // nodal-trace form; the curved elements of the interior and the partition-boundary range (columns of the side buffer) are
    // listed for the fix-up launches of either chain
    std::vector<int> curvedHost;          // element of each side-buffer column
    std::vector<int> maxNeighbourHost;    // largest element index a face of element k is paired with (from gmapP, kept for set_partition)
    DevBuf<int> slotsInterior, slotsBoundary;
    int numSlotsInterior = 0, numSlotsBoundary = 0;
    bdg_halo::Partition part;
    bdg_halo::Transport halo;
    bdg_halo::TwoChains chains;
    // the driver's tables (bdg_sw2d_curved_enable_driver; sw2d_curved_driver_kernel.hpp): the dt formula's Fscale and c planes
    // and face-node list, H, the derivative matrices (Dr, then Ds) and the metric planes (rx, sx, ry, sy) of the vorticity,
    // the lattice matrix of the latest output call, the six output planes, the reduction's partials and its three results
    struct Driver {
        bool on = false, hasC = false, hasH = false;
        int nFace = 0;
        double cConst = 0.0;
        DevBuf<double> fscale, c, H, deriv, metric, IM, out, partials, result;
        DevBuf<int> faceNodes;
    } drv;
    // the model time (bdg_sw2d_curved_set_time): + dt per completed step of step_rk2, lserk4_stages and run_adaptive
    double timeNow = 0.0;
    // run monitor, field statistics and drifters (run_records.hpp), single domain only. The columns are the caller's elements:
    // nothing is renumbered
    struct Monitor : bdg_records::MonitorState {
        DevBuf<double> row;     // (numGauges, Np): the nodal basis at each gauge
        DevBuf<double> scratch; // the record bdg_sw2d_curved_monitor_time writes
    } mon;
    bdg_records::FieldStatsState fst;
    struct Drifters : bdg_records::DrifterState {
        DevBuf<double> vert, vinvT, jac, modal;
        DevBuf<int> slot;       // per element: -1 or its row in modal
    } drf;

    ~bdg_sw2d_curved() { // both streams drained before the members destroy the events, the communicator and the exchange stream
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream);
        if (halo.stream) (void)hipStreamSynchronize(halo.stream);
        if (stream) (void)hipStreamDestroy(stream);
    }
    void use() const { hipCheck(hipSetDevice(device), "hipSetDevice"); }
    size_t plane() const { return static_cast<size_t>(Np) * static_cast<size_t>(ld); }

    // host (rows, K) row-major <-> device rows [row0, row0 + rows) of a (., ld) plane
    template <typename T>
    void uploadRows(const T* host, T* dev, int rows, int row0 = 0) {
        copyRows(dev + static_cast<size_t>(row0) * ld, static_cast<size_t>(ld) * sizeof(T), host, static_cast<size_t>(K) * sizeof(T),
                 static_cast<size_t>(K) * sizeof(T), rows, hipMemcpyHostToDevice, stream);
    }
    void downloadRows(const double* dev, double* host, int rows) {
        copyRows(host, static_cast<size_t>(K) * sizeof(double), dev, static_cast<size_t>(ld) * sizeof(double),
                 static_cast<size_t>(K) * sizeof(double), rows, hipMemcpyDeviceToHost, stream);
    }
    // a zeroed (rows, ld) buffer with the host's (rows, K) in it
    template <typename T>
    void uploadPadded(DevBuf<T>& buf, const std::vector<T>& host, int rows) {
        buf.alloc(static_cast<size_t>(rows) * ld, bytes, stream);
        uploadRows(host.data(), buf.p, rows);
    }

    // allocated to the size of `host` (not zeroed) and filled from it on the solver's stream. (Not DevBuf::upload: its blocking
    // hipMemcpy brings the null stream's queue to life beside the solver's, and every later launch of this process pays for
    // it -- 3 % of a step on an 18-element mesh, 1 % per evaluation on 2080 elements.) `host` must live until the stream is
    // waited for: upload() waits itself, creation queues its tables and waits once
    template <typename T>
    void queueUpload(DevBuf<T>& buf, const std::vector<T>& host, const char* what) {
        buf.alloc(host.size(), bytes);
        if (buf.p) hipCheck(hipMemcpyAsync(buf.p, host.data(), buf.n * sizeof(T), hipMemcpyHostToDevice, stream), what);
    }
    template <typename T>
    void upload(DevBuf<T>& buf, const std::vector<T>& host, const char* what) {
        queueUpload(buf, host, what);
        hipCheck(hipStreamSynchronize(stream), what);
    }

    // a zeroed (rows, ld) buffer with the host's (rows, K) in it, waited for
    void uploadPlanes(DevBuf<double>& buf, const double* host, int rows) {
        buf.alloc(static_cast<size_t>(rows) * ld, bytes, stream);
        uploadRows(host, buf.p, rows);
    }

    void requireFilter(bool filter) const { if (filter && !hasFilter) throw arg_error(kNoFilter); }

    // parameters of one evaluation: out = ca base + cb in + cc RHS(in), as `mode` reads them
    bdg_dev::CurvedParams params(bool filter, const double* qin, const double* qbase, double* qout, double ca, double cb, double cc) const {
        requireFilter(filter);
        bdg_dev::CurvedParams p{};
        p.gq = gq.p; p.cubG = cubG.p; p.gaussG = gaussG.p; p.gmapP = gmapP.p; p.gmapM = identityM ? nullptr : gmapM.p;
        p.rJ = rJ; p.zx = zx; p.zy = zy; p.fcor = fcor; p.cd = cd; p.fconst = fconst; p.cdconst = cdconst;
        p.curvedSlot = numCurved ? curvedSlot.p : nullptr;
        p.mmSide = mmSide.p; p.minvSide = minvSide.p; p.curvedEls = curvedEls.p; p.numCurved = numCurved; p.sideLd = sideLd;
        p.affineEl = numAffine ? affineEl.p : nullptr; p.cubAffine = numAffine ? cubAffine.p : nullptr; p.cubWref = cubWref.p;
        p.ops = ops.p; p.filt = filt.p; p.ld = ld; p.K = K; p.ncb = ncb; p.ncub = ncub; p.ng = ng; p.fb = fb; p.g = g;
        if (useNT) {
            p.opsNT = opsNT.p; p.nodeP = nodeP.p; p.faceFlags = faceFlags.p; p.faceNodes = faceNodesDev.p; p.gaussWref = gaussWref.p;
            p.affineEl = nullptr; p.elAffine = elAffine.p; // (the straight-element flag rides in faceFlags)
            if (cubWrefNT.p) p.cubWref = cubWrefNT.p;      // (elAffine holds ratios to THESE weights)
            p.tileInterleave = tileInterleave();
            p.tileOrder = tileOrder.p;
            p.prioMode = prioMode;
        }
        p.qin = qin; p.qbase = qbase; p.qout = qout; p.res = res.p; p.rhs = rhs.p; p.ca = ca; p.cb = cb; p.cc = cc;
        return p;
    }

    // One RHS evaluation fused with its update: Gauss traces of qin, stage kernel, curved-element kernel.
    // the same for the elements [kbegin, kend) and the listed columns of the side buffer only, on a given stream (nodal-trace form)
    void evaluateRange(int mode, bool filter, const double* qin, const double* qbase, double* qout, double ca, double cb, double cc,
                       int kbegin, int kend, const int* slotList, int numSlots, hipStream_t on, int gridReserve = 0) {
        bdg_dev::CurvedParams p = params(filter, qin, qbase, qout, ca, cb, cc);
        if (!useNT || qin == qout) throw arg_error("bdg_sw2d_curved: range evaluations need the nodal-trace form and two state buffers");
        p.kbegin = kbegin; p.K = kend; p.gridReserve = gridReserve;
        p.tileOrder = nullptr;  // (the list is built for the tiles of [0, K))
        hipCheck(kt->stageNT(mode, filter, p, on), "sw2d_curved_nt_kernel");
        p.slotList = slotList; p.numCurved = numSlots;
        hipCheck(kt->fixup(mode, filter, p, on), "sw2d_curved_fixup_kernel");
    }

    void evaluate(int mode, bool filter, const double* qin, const double* qbase, double* qout, double ca, double cb,
                  double cc) {
        const bdg_dev::CurvedParams p = params(filter, qin, qbase, qout, ca, cb, cc);
        if (useNT) { // one launch: the neighbours' traces are products of their nodal values (no Gauss-trace planes)
            if (qin == qout) throw arg_error("bdg_sw2d_curved: the nodal-trace kernel cannot update the state it gathers from in place");
            hipCheck(kt->stageNT(mode, filter, p, stream), "sw2d_curved_nt_kernel");
        } else {
            hipCheck(kt->gauss(p, stream), "sw2d_curved_gauss_kernel");
            hipCheck(kt->stage(mode, filter, p, stream), "sw2d_curved_stage_kernel");
        }
        hipCheck(kt->fixup(mode, filter, p, stream), "sw2d_curved_fixup_kernel");
    }

    void exchange(double* state) { exchangeOn(state, stream); }
    void exchangeOn(double* state, hipStream_t on) { bdg_halo::exchange(halo, part, state, ld, 4 * Np, K, on); }
    // one evaluation on both chains: reads `in` (ghost columns refreshed first), writes the owned columns of `out`
    void chainsEval(int mode, bool filter, double* in, const double* base, double* out, double ca, double cb, double cc) {
        // the interior launch is one resident round of workgroups that loop over their tiles: it leaves the slots the
        // partition-boundary launch needs (a workgroup per four tiles, rounded up to the eight XCDs), or that launch would wait
        const int boundaryWgs = (((part.numOwned - part.numInterior + 15) / 16 + 3) / 4 + 7) / 8 * 8;
        chains.eval(stream, halo.stream,
                    [&](hipStream_t a) {
                        evaluateRange(mode, filter, in, base, out, ca, cb, cc, 0, part.numInterior, slotsInterior.p, numSlotsInterior, a,
                                      boundaryWgs);
                    },
                    [&](hipStream_t b) {
                        exchangeOn(in, b);
                        evaluateRange(mode, filter, in, base, out, ca, cb, cc, part.numInterior, part.numOwned, slotsBoundary.p,
                                      numSlotsBoundary, b);
                    });
    }

    // ---- the steppers. How an evaluation is issued: over the whole mesh, or -- a partitioned run -- with an exchange of the
    // state it reads in front of it (stream order), or on the two chains of partition_schedule.hpp (nodal-trace form with
    // interior elements, unless BDG_SW2D_CURVED_NO_OVERLAP)
    enum class Eval { Whole, Exchanged, Chains };
    Eval exchangedEval() const { return useNT && part.numInterior >= 1 && !noOverlap() ? Eval::Chains : Eval::Exchanged; }
    void eval(Eval how, int mode, bool filter, double* in, const double* base, double* out, double ca, double cb, double cc) {
        if (how == Eval::Chains) return chainsEval(mode, filter, in, base, out, ca, cb, cc);
        if (how == Eval::Exchanged) exchange(in);
        evaluate(mode, filter, in, base, out, ca, cb, cc);
    }
    template <class Body>
    void run(Eval how, Body&& body) {
        if (how == Eval::Chains) chains.begin(stream, halo.stream);
        body();
        if (how == Eval::Chains) chains.end(stream, halo.stream);
    }
    // the driver's RK2 step in halves. phase 0, predictor: q1 = q + dt/2 RHS(q); phase 1, corrector: q += dt RHS(q1)
    void rk2Half(int phase, double dt, bool filter, Eval how) {
        if (phase == 0) eval(how, bdg_dev::CMODE_COMBINE, filter, qA.p, qA.p, qB.p, 1.0, 0.0, 0.5 * dt);
        else eval(how, bdg_dev::CMODE_COMBINE, filter, qB.p, qA.p, qA.p, 1.0, 0.0, dt);
    }
    void stepRk2(double dt, int steps, bool filter, Eval how) {
        run(how, [&] {
            for (int i = 0; i < 2 * steps; ++i) {
                rk2Half(i & 1, dt, filter, how);
                if (i & 1) stepDone(dt);
            }
        });
    }
    // LSERK4 stages (reference src/advec1d/main.cpp:92-102 per stage): res = a res + dt RHS(q); q += b res. The general form
    // updates q in place (it reads neighbours through the trace planes); the nodal-trace form reads neighbours' nodes from q,
    // so it writes the other buffer and the two swap roles.
    void lserkStages(double dt, int numStages, Eval how) {
        run(how, [&] {
            for (int i = 0; i < numStages; ++i, ++stageCount) {
                const int st = static_cast<int>(stageCount % blitzdg::LSERK4::numStages);
                eval(how, bdg_dev::CMODE_LSERK, false, qA.p, nullptr, useNT ? qB.p : qA.p, blitzdg::LSERK4::rk4a[st], blitzdg::LSERK4::rk4b[st], dt);
                if (useNT) std::swap(qA.p, qB.p);
                if ((stageCount + 1) % blitzdg::LSERK4::numStages == 0) stepDone(dt);
            }
        });
    }

    // ---- run monitor, field statistics and drifters (run_records.hpp). They exist on unpartitioned solvers only, whose stepping
    // calls launch everything on the solver's stream
    bool partitioned() const { return part.numOwned > 0 || halo.comm != nullptr; }
    // H of eta = h - H: the records' own if given, else the driver's, else none
    const double* recordsH(const DevBuf<double>& own) const { return own.p ? own.p : (drv.on && drv.hasH ? drv.H.p : nullptr); }
    // records that `steps` further completed steps would take; refused before anything is launched
    void reserveRecords(long long steps, const char* fn) const {
        mon.reserve(steps, fn, "bdg_sw2d_curved");
        drf.reserve(steps, fn, "bdg_sw2d_curved");
    }
    long long lserkSteps(long long stages) const { return bdg_records::lserkSteps(stageCount, stages, blitzdg::LSERK4::numStages); }
    void monitorLaunch(double* rec, int capacity, int slot) {
        mon.launch({qA.p, recordsH(mon.H), ld, Np, 4, K, g, timeNow}, rec, capacity, slot, bdg_dev::sw2d_monitor_finish_kernel,
                   "sw2d_monitor_finish_kernel launch", bdg_dev::MonRowGauges{mon.row.p}, stream);
    }
    void monitorSample() { monitorLaunch(mon.rec.p, mon.capacity, mon.count++); }
    bdg_records::StatsView statsView() const { return {qA.p, recordsH(fst.H), ld, Np, K, timeNow}; }
    void drifterLaunch(int mode, double dt, int slot) {
        drf.launch(bdg_dev::sw2d_curved_drifter_kernel, "sw2d_curved_drifter_kernel launch",
                   bdg_dev::CurvedTriDriftTables{{drf.vert.p, drf.neigh.p, drf.vinvT.p, drf.jac.p}, drf.slot.p, drf.modal.p, N}, qA.p, ld,
                   N, mode, dt, slot, stream);
    }
    void drifterAdvance(double dt, bool record = true) { drifterLaunch(bdg_dev::kDriftAdvance, dt, drf.takeSlot(record)); }
    // after every completed step of size dt: the model time, then the monitor's sample, the sample of the field statistics and
    // the drifters' advance (room was reserved by the caller). With nothing enabled: no launch
    void stepDone(double dt) {
        timeNow += dt;
        if (mon.on && ++mon.steps % mon.stride == 0) monitorSample();
        if (fst.on && ++fst.steps % fst.stride == 0) fst.sample(statsView(), stream);
        if (drf.on) {
            drf.t = timeNow;
            drifterAdvance(dt);
        }
    }

    // ---- the driver (sw2d_curved_driver_kernel.hpp). The elements its passes cover: the owned ones of a partitioned run
    int owned() const { return part.numOwned > 0 ? part.numOwned : K; }
    void dtPass() {
        bdg_dev::CurvedDtParams p{};
        p.q = qA.p; p.fscale = drv.fscale.p; p.c = drv.hasC ? drv.c.p : nullptr; p.faceNodes = drv.faceNodes.p;
        p.ld = ld; p.Np = Np; p.nFace = drv.nFace; p.count = owned();
        p.cConst = drv.cConst; p.fac = (N + 1) * (N + 1) * 0.5;
        const int nblocks = (p.count + bdg_dev::kCurvedDrvThreads - 1) / bdg_dev::kCurvedDrvThreads;
        hipLaunchKernelGGL(bdg_dev::sw2d_curved_dt_kernel, dim3(nblocks), dim3(bdg_dev::kCurvedDrvThreads), 0, stream, p, drv.partials.p);
        hipCheck(hipGetLastError(), "sw2d_curved_dt_kernel");
        hipLaunchKernelGGL(bdg_dev::sw2d_curved_dt_finish_kernel, dim3(1), dim3(bdg_dev::kCurvedDrvThreads), 0, stream, drv.partials.p,
                           nblocks, drv.result.p);
        hipCheck(hipGetLastError(), "sw2d_curved_dt_finish_kernel");
    }
    // {speed maximum, max|h|}; throws on the script's blow-up conditions (after `out` is filled)
    void reduceDt(double out[2]) {
        double r[3];
        dtPass();
        hipCheck(hipMemcpyAsync(r, drv.result.p, sizeof(r), hipMemcpyDeviceToHost, stream), "D2H copy");
        hipCheck(hipStreamSynchronize(stream), "reduce sync");
        out[0] = r[0]; out[1] = r[1];
        if (r[2] > 0.0 || std::isnan(r[0]) || std::isnan(r[1]) || r[1] > 1e8)
            throw unstable_error("A numerical instability has occurred.");
    }
    // one launch for the fields of `mask`; lattice: drv.IM holds the matrix
    void outputLaunch(int mask, bool lattice) {
        bdg_dev::CurvedOutParams p{};
        const size_t pl = plane(), mm = static_cast<size_t>(Np) * Np;
        p.q = qA.p; p.H = drv.hasH ? drv.H.p : nullptr; p.Dr = drv.deriv.p; p.Ds = drv.deriv.p + mm;
        p.rx = drv.metric.p; p.sx = drv.metric.p + pl; p.ry = drv.metric.p + 2 * pl; p.sy = drv.metric.p + 3 * pl;
        p.IM = lattice ? drv.IM.p : nullptr; p.out = drv.out.p; p.ld = ld; p.Np = Np; p.count = owned(); p.mask = mask;
        const dim3 grid((p.count + 63) / 64), block(64 * bdg_dev::kCurvedOutWaves);
        auto launch = [&](auto lat, auto cls) {
            hipLaunchKernelGGL((bdg_dev::sw2d_curved_output_kernel<decltype(lat)::value, decltype(cls)::value>), grid, block, 0, stream, p);
        };
        auto sized = [&](auto lat) { // the LDS size class of this order (curvedOutClass)
            switch (bdg_dev::curvedOutClass(Np)) {
            case 15: return launch(lat, std::integral_constant<int, 15>{});
            case 28: return launch(lat, std::integral_constant<int, 28>{});
            default: return launch(lat, std::integral_constant<int, bdg_dev::kCurvedDrvMaxNp>{});
            }
        };
        if (lattice) sized(std::true_type{});
        else sized(std::false_type{});
        hipCheck(hipGetLastError(), "sw2d_curved_output_kernel");
    }
    void stageLattice(const double* IM) { // queued on the stream: the caller's matrix must live until the stream is waited for
        hipCheck(hipMemcpyAsync(drv.IM.p, IM, drv.IM.n * sizeof(double), hipMemcpyHostToDevice, stream), "lattice upload");
    }
};

namespace {

void requireCurved(const bdg_sw2d_curved* s, const char* fn) {
    if (!s) throw arg_error(std::string(fn) + ": solver handle is NULL");
}

// the prologue of the calls on a solver: handle (and communicator when `comm`), a count that must not be negative (`countName`
// nullptr: none), device; then body()
template <class Body>
int prologue(bdg_sw2d_curved* s, const char* fn, bool comm, const char* countName, int count, Body&& body) {
    return guard([&] {
        requireCurved(s, fn);
        if (comm) bdg_halo::requireComm(s->halo, "bdg_sw2d_curved", fn);
        if (countName && count < 0) throw arg_error(std::string(fn) + ": " + countName + " < 0");
        s->use();
        body();
    });
}
template <class Body> int curvedCall(bdg_sw2d_curved* s, const char* fn, Body&& body) { return prologue(s, fn, false, nullptr, 0, body); }
template <class Body> int commCall(bdg_sw2d_curved* s, const char* fn, Body&& body) { return prologue(s, fn, true, nullptr, 0, body); }
// ... of the calls that need bdg_sw2d_curved_enable_driver first
template <class Body>
int driverCall(bdg_sw2d_curved* s, const char* fn, Body&& body) {
    return guard([&] {
        requireCurved(s, fn);
        if (!s->drv.on) throw arg_error(std::string(fn) + ": call bdg_sw2d_curved_enable_driver first");
        s->use();
        body();
    });
}

// The face-node list of the dt formula from ctx.vmapM: entry j of element k must be a node of element k, and the local part must
// be the same list in every element.
std::vector<int> driverFaceNodes(const int* vmapM, int Np, int nFace, int K) {
    std::vector<int> local(static_cast<size_t>(nFace));
    for (int k = 0; k < K; ++k)
        for (int j = 0; j < nFace; ++j) {
            const long long v = vmapM[j + static_cast<size_t>(nFace) * k], n = v - static_cast<long long>(Np) * k;
            if (n < 0 || n >= Np)
                throw arg_error("bdg_sw2d_curved_enable_driver: vmapM entry " + std::to_string(j) + " of element " + std::to_string(k) +
                                " is not a node of that element");
            if (k == 0) local[static_cast<size_t>(j)] = static_cast<int>(n);
            else if (local[static_cast<size_t>(j)] != n)
                throw arg_error("bdg_sw2d_curved_enable_driver: the face-node list of element " + std::to_string(k) +
                                " differs from element 0's");
        }
    return local;
}

// What the host tables need of the order's kernel table, for this descriptor's sizes.
tables::KernelSizes kernelSizes(const bdg_dev::CurvedKernelTable& kt, const bdg_sw2d_curved_desc& d) {
    const int ncb = (d.num_cub + 15) / 16, fb = (d.num_gauss + 15) / 16;
    tables::KernelSizes ks;
    ks.Np = kt.Np; ks.KV = kt.KV; ks.MT = kt.MT;
    ks.opsTiles = kt.opsTiles(ncb, fb);
    kt.opsOffsets(ncb, fb, ks.opsOff);
    ks.ntFits = kt.ntFits(ncb, fb, d.Filter != nullptr);
    ks.ntTiles = kt.ntTiles(ncb, fb);
    kt.ntOffsets(ncb, fb, ks.ntOff);
    return ks;
}

// The host half of creation, shared with bdg_sw2d_curved_plan: no HIP call. The cheap argument checks come first, so that
// creation can ask for a device between the two.
const bdg_dev::CurvedKernelTable* checkedTable(const bdg_sw2d_curved_desc& d) {
    const bdg_dev::CurvedKernelTable* kt = bdg_dev::curved_kernel_table(d.order);
    if (!kt) throw arg_error("bdg_sw2d_curved_create: order must be 1..8");
    tables::validate(d);
    return kt;
}
tables::Tables hostTables(const bdg_sw2d_curved_desc& d, const bdg_dev::CurvedKernelTable& kt) {
    return tables::build(d, kernelSizes(kt, d), creationSwitches());
}

bdg_sw2d_curved* createCurved(const bdg_sw2d_curved_desc& d) {
    const bdg_dev::CurvedKernelTable* kt = checkedTable(d);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        throw hip_error("bdg_sw2d_curved_create: no HIP device available (the sw2d path has no CPU fallback)");
    if (d.device < 0 || d.device >= ndev) throw arg_error("bdg_sw2d_curved_create: device ordinal out of range");
    tables::Tables t = hostTables(d, *kt); // every table, validated, before anything touches the GPU
    const std::vector<double> filter(d.Filter, d.Filter ? d.Filter + static_cast<size_t>(t.Np) * t.Np : d.Filter);
    // (t and filter outlive s: if creation throws, s drains its stream before the tables queued on it go)

    auto s = std::unique_ptr<bdg_sw2d_curved>(new bdg_sw2d_curved());
    s->kt = kt;
    s->N = t.N; s->Np = t.Np; s->K = t.K; s->device = d.device; s->g = d.g;
    s->ncub = t.ncub; s->ncb = t.ncb; s->ng = t.ng; s->fb = t.fb; s->ld = t.ld;
    s->identityM = t.identityM; s->numCurved = static_cast<int>(t.curved.size()); s->sideLd = t.sideLd;
    s->numAffine = t.numAffine; s->useNT = t.useNT; s->hasFilter = d.Filter != nullptr;
    s->fconst = d.coriolis_const; s->cdconst = d.drag_const;
    s->bytesPerElement = t.bytesPerElement;
    const int Np = t.Np, NG = t.ng, fb = t.fb, CR = 16 * t.ncb, GR = 48 * fb;
    const long long ld = t.ld;
    size_t& bytes = s->bytes;

    s->use();
    hipCheck(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking), "hipStreamCreate");
    hipStream_t st = s->stream;
    // ---- state and work planes; the Gauss-trace planes and maps belong to the general form only
    for (DevBuf<double>* b : {&s->qA, &s->qB, &s->res, &s->rhs}) b->alloc(4 * s->plane(), bytes, st);
    if (!t.useNT) {
        s->gq.alloc(static_cast<size_t>(4) * GR * ld, bytes, st);
        s->uploadPadded(s->gmapP, t.offP, GR);
        if (!t.identityM) s->uploadPadded(s->gmapM, t.offM, GR);
    }
    // ---- cubature geometry: W rx, W ry, W sx, W sy (the reference forms W (rx F + ry G); the products are folded here once,
    //      a rounding-level difference), rows padded to 16 ncb with zeros; Gauss geometry nx, ny, W, each face padded to 16 fb rows
    std::vector<double> plane;
    s->cubG.alloc(static_cast<size_t>(4) * CR * ld, bytes, st);
    for (int g = 0; g < 4; ++g) {
        tables::weightedGeometry(d, g, plane);
        s->uploadRows(plane.data(), s->cubG.p + static_cast<size_t>(g) * CR * ld, t.ncub);
    }
    s->gaussG.alloc(static_cast<size_t>(3) * GR * ld, bytes, st);
    const double* gaussGeo[3] = {d.gaussnx, d.gaussny, d.gaussW};
    for (int g = 0; g < 3; ++g)
        for (int f = 0; f < 3; ++f)
            s->uploadRows(gaussGeo[g] + static_cast<size_t>(f) * NG * t.K, s->gaussG.p + static_cast<size_t>(g) * GR * ld, NG, 16 * fb * f);
    // ---- nodal tables: 1 / J, then the sources the caller gave
    const double* given[4] = {d.zx, d.zy, d.coriolis, d.drag};
    double** slot[4] = {&s->zx, &s->zy, &s->fcor, &s->cd};
    s->coef.alloc((1 + static_cast<size_t>(std::count_if(given, given + 4, [](const double* p) { return p != nullptr; }))) * s->plane(), bytes, st);
    s->rJ = s->coef.p;
    tables::inverseJacobian(d, Np, plane);
    s->uploadRows(plane.data(), s->rJ, Np);
    for (int i = 0, next = 1; i < 4; ++i) {
        if (!given[i]) continue;
        *slot[i] = s->coef.p + static_cast<size_t>(next++) * s->plane();
        s->uploadRows(given[i], *slot[i], Np);
    }
    // ---- straight-sided elements of the general form, the elements of curvedEls, operator image
    if (t.numAffine) {
        s->queueUpload(s->affineEl, t.affineEl, "affine flags upload");
        s->uploadPadded(s->cubAffine, t.cubAffine, 4);
        s->queueUpload(s->cubWref, t.wref, "Wref upload");
    }
    if (s->numCurved) {
        s->queueUpload(s->curvedSlot, t.slotOf, "slot upload");
        s->queueUpload(s->curvedEls, t.curved, "curvedEls upload");
        s->queueUpload(s->minvSide, t.minv, "Minv upload");
        s->mmSide.alloc(static_cast<size_t>(4) * Np * t.curved.size(), bytes, st);
    }
    s->queueUpload(s->ops, t.ops, "ops upload");
    s->queueUpload(s->filt, filter, "filter upload");
    // ---- nodal-trace form. Its straight elements hold ratios to the weights of ITS reference element: the general form's
    //      buffer serves when that is the same element (or when there is none to serve), a buffer of its own otherwise
    if (t.useNT) {
        s->prioMode = prioSwitch(s->prioMode);
        s->uploadPadded(s->elAffine, t.elAffine, 14);
        if (!s->cubWref.p) s->queueUpload(s->cubWref, t.wrefNT, "Wref upload");
        else if (t.krefNT >= 0 && t.krefNT != t.kref) s->queueUpload(s->cubWrefNT, t.wrefNT, "Wref upload");
        s->queueUpload(s->gaussWref, t.gaussWref, "gauss Wref upload");
        s->queueUpload(s->faceFlags, t.faceFlags, "face flags upload");
        s->uploadPadded(s->nodeP, t.nodeP, t.rowsP);
        s->queueUpload(s->faceNodesDev, t.faceNodes, "face nodes upload");
        s->queueUpload(s->tileOrder, t.tileOrder, "tile order upload");
        s->queueUpload(s->opsNT, t.opsNT, "ops upload");
    }
    hipCheck(hipStreamSynchronize(st), "creation sync");
    s->curvedHost = std::move(t.curved);
    s->maxNeighbourHost = std::move(t.maxNeighbour);
    return s.release();
}

double* curvedBuffer(bdg_sw2d_curved* s, int which, int first, int count, const char* fn) {
    requireCurved(s, fn);
    if (which != 0 && which != 1) throw arg_error(std::string(fn) + ": which must be 0 (state) or 1 (intermediate)");
    if (first < 0 || count < 0 || static_cast<long long>(first) + count > s->K) throw arg_error(std::string(fn) + ": element range out of bounds");
    return (which == 0 ? s->qA.p : s->qB.p) + first;
}

// columns [first, first + count) of a state buffer <-> a host (4 Np, count) array: to the device when the host's is const
template <class Host>
int copyElements(bdg_sw2d_curved* s, int which, int first, int count, Host* host, const char* fn) {
    return guard([&] {
        double* dev = curvedBuffer(s, which, first, count, fn);
        if (count == 0) return;
        if (!host) throw arg_error(std::string(fn) + ": NULL buffer");
        s->use();
        const size_t width = static_cast<size_t>(count) * sizeof(double), pitch = static_cast<size_t>(s->ld) * sizeof(double);
        if constexpr (std::is_const<Host>::value) copyRows(dev, pitch, host, width, width, static_cast<size_t>(4) * s->Np, hipMemcpyHostToDevice, s->stream);
        else copyRows(host, width, dev, pitch, width, static_cast<size_t>(4) * s->Np, hipMemcpyDeviceToHost, s->stream);
    });
}

} // namespace

extern "C" {

int bdg_sw2d_curved_create(const bdg_sw2d_curved_desc* desc, bdg_sw2d_curved** out) {
    return guard([&] {
        if (!desc || !out) throw arg_error("bdg_sw2d_curved_create: NULL argument");
        *out = createCurved(*desc);
    });
}

int bdg_sw2d_curved_plan(const bdg_sw2d_curved_desc* desc, int* out, int n) {
    return guard([&] {
        if (!desc || !out || n < 0) throw arg_error("bdg_sw2d_curved_plan: bad argument");
        const tables::Tables t = hostTables(*desc, *checkedTable(*desc));
        const int v[BDG_SW2D_CURVED_PLAN_FIELDS] = {t.useNT ? 1 : 0, t.identityM ? 1 : 0, static_cast<int>(t.curved.size()), t.numAffine,
                                                    t.numAffineNT, t.kref, t.krefNT, static_cast<int>(t.tileOrder.size())};
        std::copy(v, v + std::min(n, BDG_SW2D_CURVED_PLAN_FIELDS), out);
    });
}

void bdg_sw2d_curved_destroy(bdg_sw2d_curved* s) { delete s; }

int bdg_sw2d_curved_rhs(bdg_sw2d_curved* s, const double* h, const double* hu, const double* hv, const double* hN,
                        double* r1, double* r2, double* r3, double* r4, int filter) {
    return curvedCall(s, "bdg_sw2d_curved_rhs", [&] {
        if (!h || !hu || !hv || !hN || !r1 || !r2 || !r3 || !r4) throw arg_error("bdg_sw2d_curved_rhs: NULL field pointer");
        const size_t pl = s->plane();
        const double* in[4] = {h, hu, hv, hN};
        double* outp[4] = {r1, r2, r3, r4};
        for (int c = 0; c < 4; ++c) s->uploadRows(in[c], s->qB.p + c * pl, s->Np); // the scratch state: qA stays untouched
        s->evaluate(bdg_dev::CMODE_RHS, filter != 0, s->qB.p, nullptr, nullptr, 0.0, 0.0, 0.0);
        for (int c = 0; c < 4; ++c) s->downloadRows(s->rhs.p + c * pl, outp[c], s->Np);
    });
}

int bdg_sw2d_curved_set_state(bdg_sw2d_curved* s, const double* h, const double* hu, const double* hv, const double* hN) {
    return curvedCall(s, "bdg_sw2d_curved_set_state", [&] {
        if (!h || !hu || !hv || !hN) throw arg_error("bdg_sw2d_curved_set_state: NULL field pointer");
        const double* in[4] = {h, hu, hv, hN};
        for (int c = 0; c < 4; ++c) s->uploadRows(in[c], s->qA.p + c * s->plane(), s->Np);
        s->res.zero(s->stream);
        s->stageCount = 0;
        s->mon.steps = 0;
        s->fst.steps = 0;
        if (s->drf.on) s->drifterLaunch(bdg_dev::kDriftSample, 0.0, -1); // (u0, v0) of the new state
    });
}

int bdg_sw2d_curved_get_state(bdg_sw2d_curved* s, double* h, double* hu, double* hv, double* hN) {
    return curvedCall(s, "bdg_sw2d_curved_get_state", [&] {
        if (!h || !hu || !hv || !hN) throw arg_error("bdg_sw2d_curved_get_state: NULL field pointer");
        double* outp[4] = {h, hu, hv, hN};
        for (int c = 0; c < 4; ++c) s->downloadRows(s->qA.p + c * s->plane(), outp[c], s->Np);
    });
}

int bdg_sw2d_curved_step_rk2(bdg_sw2d_curved* s, double dt, int num_steps, int filter) {
    return prologue(s, "bdg_sw2d_curved_step_rk2", false, "num_steps", num_steps, [&] {
        s->reserveRecords(num_steps, "bdg_sw2d_curved_step_rk2");
        s->stepRk2(dt, num_steps, filter != 0, bdg_sw2d_curved::Eval::Whole);
    });
}

int bdg_sw2d_curved_lserk4_stages(bdg_sw2d_curved* s, double dt, int num_stages) {
    return prologue(s, "bdg_sw2d_curved_lserk4_stages", false, "num_stages", num_stages, [&] {
        s->reserveRecords(s->lserkSteps(num_stages), "bdg_sw2d_curved_lserk4_stages");
        s->lserkStages(dt, num_stages, bdg_sw2d_curved::Eval::Whole);
    });
}

int bdg_sw2d_curved_time_rk2(bdg_sw2d_curved* s, double dt, int num_steps, int filter, float* ms_per_rhs) {
    return guard([&] {
        requireCurved(s, "bdg_sw2d_curved_time_rk2");
        if (num_steps < 1 || !ms_per_rhs) throw arg_error("bdg_sw2d_curved_time_rk2: bad argument");
        s->use();
        s->reserveRecords(num_steps, "bdg_sw2d_curved_time_rk2"); // (the steps are steps like any other: they feed the records)
        // (one run: all the steps, two evaluations each)
        const float ms = bdg_dev::timePerRun(s->stream, 1, [&] { s->stepRk2(dt, num_steps, filter != 0, bdg_sw2d_curved::Eval::Whole); });
        *ms_per_rhs = ms / (2.0f * static_cast<float>(num_steps));
    });
}

int bdg_sw2d_curved_get_elements(bdg_sw2d_curved* s, int which, int first, int count, double* out) {
    return copyElements(s, which, first, count, out, "bdg_sw2d_curved_get_elements");
}

int bdg_sw2d_curved_set_elements(bdg_sw2d_curved* s, int which, int first, int count, const double* in) {
    return copyElements(s, which, first, count, in, "bdg_sw2d_curved_set_elements");
}

int bdg_sw2d_curved_rk2_phase(bdg_sw2d_curved* s, double dt, int phase, int filter) {
    return guard([&] {
        requireCurved(s, "bdg_sw2d_curved_rk2_phase");
        if (phase != 0 && phase != 1) throw arg_error("bdg_sw2d_curved_rk2_phase: phase must be 0 (predictor) or 1 (corrector)");
        s->use();
        s->rk2Half(phase, dt, filter != 0, bdg_sw2d_curved::Eval::Whole);
    });
}

int bdg_sw2d_curved_set_partition(bdg_sw2d_curved* s, int num_interior, int num_owned, const int* send_elements, int num_send) {
    return curvedCall(s, "bdg_sw2d_curved_set_partition", [&] {
        if (s->mon.on || s->fst.on || s->drf.on)
            throw arg_error("bdg_sw2d_curved_set_partition: the solver has a monitor, field statistics or drifters, which cover a single domain only");
        s->part.set("bdg_sw2d_curved", s->K, s->maxNeighbourHost, num_interior, num_owned, send_elements, num_send,
                    s->halo.comm != nullptr, s->bytes, s->stream);
        std::vector<int> inner, outer; // columns of the side buffer whose element is an interior / a partition-boundary one
        for (size_t c = 0; c < s->curvedHost.size(); ++c) {
            const int k = s->curvedHost[c];
            if (k < num_interior) inner.push_back(static_cast<int>(c));
            else if (k < num_owned) outer.push_back(static_cast<int>(c));
        }
        s->numSlotsInterior = static_cast<int>(inner.size());
        s->numSlotsBoundary = static_cast<int>(outer.size());
        inner.resize(std::max<size_t>(1, inner.size())); // (a list is never an empty buffer)
        outer.resize(std::max<size_t>(1, outer.size()));
        s->upload(s->slotsInterior, inner, "slot list upload");
        s->upload(s->slotsBoundary, outer, "slot list upload");
    });
}

int bdg_sw2d_curved_comm_init(bdg_sw2d_curved* s, int rank, int world, const void* unique_id, const int* peer_ranks,
                              const int* send_start, const int* send_count, const int* recv_start, const int* recv_count,
                              int num_peers) {
    return curvedCall(s, "bdg_sw2d_curved_comm_init", [&] {
        if (s->mon.on || s->fst.on || s->drf.on)
            throw arg_error("bdg_sw2d_curved_comm_init: the solver has a monitor, field statistics or drifters, which cover a single domain only");
        bdg_halo::commInit("bdg_sw2d_curved", s->halo, s->part, s->chains, s->K, static_cast<size_t>(4) * s->Np, rank, world, unique_id,
                           peer_ranks, send_start, send_count, recv_start, recv_count, num_peers, s->bytes, s->stream);
    });
}

// the driver's RK2 step of a partitioned run: an exchange in front of EACH evaluation, of the state that evaluation reads
int bdg_sw2d_curved_step_rk2_exchanged(bdg_sw2d_curved* s, double dt, int num_steps, int filter) {
    return prologue(s, "bdg_sw2d_curved_step_rk2_exchanged", true, "num_steps", num_steps,
                    [&] { s->stepRk2(dt, num_steps, filter != 0, s->exchangedEval()); });
}

int bdg_sw2d_curved_lserk4_stages_exchanged(bdg_sw2d_curved* s, double dt, int num_stages) {
    return prologue(s, "bdg_sw2d_curved_lserk4_stages_exchanged", true, "num_stages", num_stages,
                    [&] { s->lserkStages(dt, num_stages, s->exchangedEval()); });
}

int bdg_sw2d_curved_exchange(bdg_sw2d_curved* s, int intermediate) {
    return commCall(s, "bdg_sw2d_curved_exchange", [&] { s->exchange(intermediate ? s->qB.p : s->qA.p); });
}

int bdg_sw2d_curved_barrier(bdg_sw2d_curved* s) {
    return commCall(s, "bdg_sw2d_curved_barrier", [&] { bdg_halo::barrier(s->halo, s->stream); });
}

int bdg_sw2d_curved_synchronize(bdg_sw2d_curved* s) {
    return curvedCall(s, "bdg_sw2d_curved_synchronize", [&] { hipCheck(hipStreamSynchronize(s->stream), "hipStreamSynchronize"); });
}

size_t bdg_sw2d_curved_device_bytes(const bdg_sw2d_curved* s) { return s ? s->bytes : 0; }
double bdg_sw2d_curved_bytes_per_element(const bdg_sw2d_curved* s) { return s ? s->bytesPerElement : 0.0; }
int bdg_sw2d_curved_form(const bdg_sw2d_curved* s) { return s ? (s->useNT ? 1 : 0) : -1; }

int bdg_sw2d_curved_kernel_info(const bdg_sw2d_curved* s, int filter, int* out, int n) {
    return guard([&] {
        requireCurved(s, "bdg_sw2d_curved_kernel_info");
        if (!out || n < 0) throw arg_error("bdg_sw2d_curved_kernel_info: bad output buffer");
        s->requireFilter(filter != 0);
        int v[BDG_SW2D_CURVED_KERNEL_INFO_FIELDS];
        const bdg_dev::CurvedOrder* order = bdg_dev::curvedOrder(s->N);
        if (!order || !order->info()(s->useNT, s->ncb, s->ng, s->fb, !s->identityM, filter != 0, v))
            throw arg_error("bdg_sw2d_curved_kernel_info: no compiled kernel serves this solver");
        std::copy(v, v + std::min(n, BDG_SW2D_CURVED_KERNEL_INFO_FIELDS), out);
    });
}

// ---- the driver's adaptive step, blow-up check and output fields (sw2d_curved.py:231-302)

int bdg_sw2d_curved_enable_driver(bdg_sw2d_curved* s, const bdg_sw2d_curved_driver_desc* d) {
    return curvedCall(s, "bdg_sw2d_curved_enable_driver", [&] {
        if (!d || !d->Fscale || !d->vmapM || !d->Dr || !d->Ds || !d->rx || !d->sx || !d->ry || !d->sy)
            throw arg_error("bdg_sw2d_curved_enable_driver: NULL argument (Fscale, vmapM, Dr, Ds, rx, sx, ry, sy are required)");
        const int Np = s->Np, nFace = 3 * (s->N + 1);
        const std::vector<int> faceNodes = driverFaceNodes(d->vmapM, Np, nFace, s->K); // nothing is changed before this passes
        bdg_sw2d_curved::Driver& v = s->drv;
        v.on = false;
        v.nFace = nFace;
        s->uploadPlanes(v.fscale, d->Fscale, nFace);
        v.hasC = d->c != nullptr;
        v.cConst = d->c_const;
        if (d->c) s->uploadPlanes(v.c, d->c, Np);
        v.hasH = d->H != nullptr;
        if (d->H) s->uploadPlanes(v.H, d->H, Np);
        const size_t mm = static_cast<size_t>(Np) * Np;
        std::vector<double> deriv(d->Dr, d->Dr + mm);
        deriv.insert(deriv.end(), d->Ds, d->Ds + mm);
        s->queueUpload(v.deriv, deriv, "Dr, Ds upload");
        s->queueUpload(v.faceNodes, faceNodes, "face-node list upload");
        v.metric.alloc(4 * s->plane(), s->bytes, s->stream);
        const double* metric[4] = {d->rx, d->sx, d->ry, d->sy};
        for (int i = 0; i < 4; ++i) s->uploadRows(metric[i], v.metric.p + i * s->plane(), Np); // (waits: deriv, faceNodes are up)
        v.IM.alloc(mm, s->bytes);
        v.out.alloc(bdg_dev::CURVED_OUT_FIELDS * s->plane(), s->bytes, s->stream);
        v.partials.alloc(static_cast<size_t>(3) * ((s->K + bdg_dev::kCurvedDrvThreads - 1) / bdg_dev::kCurvedDrvThreads), s->bytes);
        v.result.alloc(3, s->bytes);
        hipCheck(hipStreamSynchronize(s->stream), "driver tables sync");
        v.on = true;
    });
}

int bdg_sw2d_curved_compute_dt(bdg_sw2d_curved* s, double cfl, double* dt, double* h_max) {
    return driverCall(s, "bdg_sw2d_curved_compute_dt", [&] {
        double r[2] = {0.0, 0.0};
        try {
            s->reduceDt(r);
        } catch (const unstable_error&) { // the values are reported with the verdict
            if (h_max) *h_max = r[1];
            if (dt) *dt = cfl / r[0];
            throw;
        }
        if (h_max) *h_max = r[1];
        if (dt) *dt = cfl / r[0];
    });
}

int bdg_sw2d_curved_run_adaptive(bdg_sw2d_curved* s, double cfl, double final_time, int max_steps, int filter, double* t_inout,
                                 double* dt_inout, int* steps_done) {
    int done = 0;
    const int rc = driverCall(s, "bdg_sw2d_curved_run_adaptive", [&] {
        if (!t_inout || !dt_inout) throw arg_error("bdg_sw2d_curved_run_adaptive: NULL argument");
        if (s->halo.comm) throw arg_error("bdg_sw2d_curved_run_adaptive: not available on a solver with a communicator (no rank-global dt)");
        s->requireFilter(filter != 0);
        double t = *t_inout, dt = *dt_inout;
        s->timeNow = t;
        while (t < final_time && (max_steps <= 0 || done < max_steps)) { // the script's loop, in its order
            // the number of steps is not known in advance: room for this step's records is checked before the step is launched
            s->reserveRecords(1, "bdg_sw2d_curved_run_adaptive");
            s->stepRk2(dt, 1, filter != 0, bdg_sw2d_curved::Eval::Whole);
            t += dt; // (stepDone made the same sum)
            double r[2];
            s->reduceDt(r);
            dt = cfl / r[0];
            ++done;
            *t_inout = t;
            *dt_inout = dt;
        }
    });
    if (steps_done) *steps_done = done;
    return rc;
}

int bdg_sw2d_curved_output_fields(bdg_sw2d_curved* s, const double* IM, double* eta, double* u, double* v, double* B, double* h,
                                  double* vort) {
    return driverCall(s, "bdg_sw2d_curved_output_fields", [&] {
        double* target[bdg_dev::CURVED_OUT_FIELDS] = {eta, u, v, B, h, vort};
        int mask = 0;
        for (int c = 0; c < bdg_dev::CURVED_OUT_FIELDS; ++c) mask |= target[c] ? 1 << c : 0;
        if (!mask) return;
        if (IM) s->stageLattice(IM);
        s->outputLaunch(mask, IM != nullptr);
        // the owned columns of each row alone: the caller's ghost columns stay as they are
        const size_t width = static_cast<size_t>(s->owned()) * sizeof(double);
        for (int c = 0; c < bdg_dev::CURVED_OUT_FIELDS; ++c)
            if (target[c])
                copyRows(target[c], static_cast<size_t>(s->K) * sizeof(double), s->drv.out.p + c * s->plane(),
                         static_cast<size_t>(s->ld) * sizeof(double), width, static_cast<size_t>(s->Np), hipMemcpyDeviceToHost, s->stream);
    });
}

int bdg_sw2d_curved_time_driver(bdg_sw2d_curved* s, int which, const double* IM, int count, float* ms) {
    return driverCall(s, "bdg_sw2d_curved_time_driver", [&] {
        if (!ms || count < 1 || (which != 0 && which != 1)) throw arg_error("bdg_sw2d_curved_time_driver: bad argument");
        if (which == 1 && IM) s->stageLattice(IM);
        const int all = (1 << bdg_dev::CURVED_OUT_FIELDS) - 1;
        auto launch = [&] { which == 0 ? s->dtPass() : s->outputLaunch(all, IM != nullptr); };
        for (int i = 0; i < 10; ++i) launch(); // untimed
        *ms = bdg_dev::timePerRun(s->stream, count, launch);
    });
}

// ---- model time (the convention of bdg_sw2d_set_time)
int bdg_sw2d_curved_set_time(bdg_sw2d_curved* s, double t) {
    return guard([&] {
        requireCurved(s, "bdg_sw2d_curved_set_time");
        s->timeNow = t;
    });
}

int bdg_sw2d_curved_get_time(const bdg_sw2d_curved* s, double* t) {
    return guard([&] {
        requireCurved(s, "bdg_sw2d_curved_get_time");
        if (!t) throw arg_error("bdg_sw2d_curved_get_time: NULL argument");
        *t = s->timeNow;
    });
}

// ---- run monitor (run_records.hpp; the records of the triangle solver on four fields)
int bdg_sw2d_curved_enable_monitor(bdg_sw2d_curved* s, const bdg_sw2d_monitor_desc* d) {
    return guard([&] {
        const std::string fn = "bdg_sw2d_curved_enable_monitor";
        requireCurved(s, fn.c_str());
        bdg_sw2d_curved::Monitor& m = s->mon;
        m.checkEnable(fn, d, s->K);
        if (s->partitioned())
            throw arg_error(fn + ": the solver has a partition set; the monitor of a partitioned curved run is not recorded (single domain only)");
        const int ng = d->num_gauges, Np = s->Np;
        if (ng > 0 && !d->gauge_row) throw arg_error(fn + ": bad gauge list");
        s->use();
        m.enable(d->stride, d->capacity, ng, 4, d->gauge_element, {&m.row, &m.scratch}, &m.scratch, s->bytes, s->stream, [&] {
            s->uploadPlanes(m.w, d->weights, Np); // zero in the padding up to ld
            if (d->H) s->uploadPlanes(m.H, d->H, Np);
            m.row.alloc(static_cast<size_t>(std::max(1, ng)) * Np, s->bytes, s->stream);
            if (ng > 0)
                hipCheck(hipMemcpyAsync(m.row.p, d->gauge_row, static_cast<size_t>(ng) * Np * sizeof(double), hipMemcpyHostToDevice,
                                        s->stream), "hipMemcpy (gauge rows)");
        });
    });
}

namespace {
void requireCurvedMonitorOn(const bdg_sw2d_curved* s, const char* fn) {
    requireCurved(s, fn);
    s->mon.requireOn(fn, "bdg_sw2d_curved");
}
void requireCurvedStatsOn(const bdg_sw2d_curved* s, const char* fn) {
    requireCurved(s, fn);
    s->fst.requireOn(fn, "bdg_sw2d_curved");
}
void requireCurvedDriftersOn(const bdg_sw2d_curved* s, const char* fn) {
    requireCurved(s, fn);
    s->drf.requireOn(fn, "bdg_sw2d_curved");
}
} // namespace

int bdg_sw2d_curved_monitor_sample(bdg_sw2d_curved* s) {
    return guard([&] {
        requireCurvedMonitorOn(s, "bdg_sw2d_curved_monitor_sample");
        s->mon.requireFree("bdg_sw2d_curved_monitor_sample", "bdg_sw2d_curved");
        s->use();
        s->monitorSample();
    });
}

int bdg_sw2d_curved_monitor_count(const bdg_sw2d_curved* s, int* n) {
    return guard([&] {
        requireCurvedMonitorOn(s, "bdg_sw2d_curved_monitor_count");
        if (!n) throw arg_error("bdg_sw2d_curved_monitor_count: NULL argument");
        *n = s->mon.count;
    });
}

int bdg_sw2d_curved_monitor_width(const bdg_sw2d_curved* s, int* width) {
    return guard([&] {
        requireCurvedMonitorOn(s, "bdg_sw2d_curved_monitor_width");
        if (!width) throw arg_error("bdg_sw2d_curved_monitor_width: NULL argument");
        *width = s->mon.width;
    });
}

int bdg_sw2d_curved_monitor_read(bdg_sw2d_curved* s, int first, int count, double* records) {
    return guard([&] {
        requireCurvedMonitorOn(s, "bdg_sw2d_curved_monitor_read");
        s->use();
        s->mon.read("bdg_sw2d_curved_monitor_read", first, count, records, s->stream);
    });
}

int bdg_sw2d_curved_monitor_reset(bdg_sw2d_curved* s) {
    return guard([&] {
        requireCurvedMonitorOn(s, "bdg_sw2d_curved_monitor_reset");
        s->mon.reset();
    });
}

int bdg_sw2d_curved_monitor_time(bdg_sw2d_curved* s, int count, float* ms) {
    return guard([&] {
        requireCurvedMonitorOn(s, "bdg_sw2d_curved_monitor_time");
        if (count < 1 || !ms) throw arg_error("bdg_sw2d_curved_monitor_time: bad argument");
        s->use();
        s->monitorLaunch(s->mon.scratch.p, 1, 0); // once before the clock starts
        *ms = bdg_dev::timePerRun(s->stream, count, [&] { s->monitorLaunch(s->mon.scratch.p, 1, 0); });
    });
}

// ---- field statistics (run_records.hpp)
int bdg_sw2d_curved_enable_field_stats(bdg_sw2d_curved* s, const bdg_field_stats_desc* d) {
    return guard([&] {
        const std::string fn = "bdg_sw2d_curved_enable_field_stats";
        requireCurved(s, fn.c_str());
        s->fst.checkEnable(fn, d, s->partitioned());
        s->use();
        s->fst.enable(*d, s->plane(), s->bytes, s->stream, [&] {
            if (d->H) s->uploadPlanes(s->fst.H, d->H, s->Np);
        });
    });
}

int bdg_sw2d_curved_field_stats_sample(bdg_sw2d_curved* s) {
    return guard([&] {
        requireCurvedStatsOn(s, "bdg_sw2d_curved_field_stats_sample");
        s->use();
        s->fst.sample(s->statsView(), s->stream);
    });
}

int bdg_sw2d_curved_field_stats_count(const bdg_sw2d_curved* s, int* samples, int* num_periods) {
    return guard([&] {
        requireCurvedStatsOn(s, "bdg_sw2d_curved_field_stats_count");
        if (!samples || !num_periods) throw arg_error("bdg_sw2d_curved_field_stats_count: NULL argument");
        *samples = s->fst.count();
        *num_periods = s->fst.m;
    });
}

int bdg_sw2d_curved_field_stats_read(bdg_sw2d_curved* s, int which, int index, double* plane) {
    return guard([&] {
        requireCurvedStatsOn(s, "bdg_sw2d_curved_field_stats_read");
        if (!plane) throw arg_error("bdg_sw2d_curved_field_stats_read: NULL argument");
        const double* dev = s->fst.planeOf("bdg_sw2d_curved_field_stats_read", which, index);
        s->use();
        s->downloadRows(dev, plane, s->Np);
    });
}

int bdg_sw2d_curved_field_stats_samples(const bdg_sw2d_curved* s, int first, int count, double* rows) {
    return guard([&] {
        requireCurvedStatsOn(s, "bdg_sw2d_curved_field_stats_samples");
        s->fst.samples("bdg_sw2d_curved_field_stats_samples", first, count, rows);
    });
}

int bdg_sw2d_curved_field_stats_reset(bdg_sw2d_curved* s) {
    return guard([&] {
        requireCurvedStatsOn(s, "bdg_sw2d_curved_field_stats_reset");
        s->use();
        s->fst.reset(s->stream);
    });
}

int bdg_sw2d_curved_field_stats_time(bdg_sw2d_curved* s, int count, float* ms) {
    return guard([&] {
        requireCurvedStatsOn(s, "bdg_sw2d_curved_field_stats_time");
        if (count < 1 || !ms) throw arg_error("bdg_sw2d_curved_field_stats_time: bad argument");
        s->use();
        *ms = s->fst.time(s->statsView(), count, s->bytes, s->stream);
    });
}

// ---- drifters (run_records.hpp, sw2d_curved_drifter_kernel.hpp)
int bdg_sw2d_curved_enable_drifters(bdg_sw2d_curved* s, const bdg_sw2d_curved_drifter_desc* d) {
    return guard([&] {
        using namespace bdg_dev;
        const std::string fn = "bdg_sw2d_curved_enable_drifters";
        requireCurved(s, fn.c_str());
        if (!d || d->count < 1 || !d->element || !d->r || !d->s || !d->vertices || !d->neighbours || !d->vinv || !d->jacobi ||
            !d->curved_slot || d->num_curved < 0 || (d->num_curved > 0 && !d->modal))
            throw arg_error(fn + ": the descriptor, at least one drifter and the tables of bdg_trinodes_curved_drifter_tables are required");
        bdg_sw2d_curved::Drifters& m = s->drf;
        m.checkEnable(fn, d->count, d->stride, d->capacity, s->partitioned());
        const int n = d->count, K = s->K, Np = s->Np, Nq = s->N + 1;
        for (int i = 0; i < n; ++i) {
            const int e = d->element[i];
            if (e < 0 || e >= K) throw arg_error(fn + ": drifter " + std::to_string(i) + " names an element outside [0, K)");
            const double r = d->r[i], t = d->s[i];
            if (!(-1.0 - t <= 1e-10) || !(r + t <= 1e-10) || !(-1.0 - r <= 1e-10))
                throw arg_error(fn + ": drifter " + std::to_string(i) + " lies outside its element (r, s >= -1, r + s <= 0)");
        }
        // the kernel follows the neighbour entries and the rows of the side tables without a further check
        std::vector<int> nb(static_cast<size_t>(4) * K, kDriftWall);
        for (int k = 0; k < K; ++k) {
            for (int f = 0; f < 3; ++f) {
                const int v = d->neighbours[static_cast<size_t>(f) * K + k];
                if (v < kDriftOpen || v >= K) throw arg_error(fn + ": neighbour entry out of range");
                nb[static_cast<size_t>(4) * k + f] = v;
            }
            if (d->curved_slot[k] < -1 || d->curved_slot[k] >= d->num_curved) throw arg_error(fn + ": curved_slot entry out of range");
        }
        std::vector<double> vinvT(static_cast<size_t>(Np) * Np);
        for (int r = 0; r < Np; ++r)
            for (int c = 0; c < Np; ++c) vinvT[static_cast<size_t>(c) * Np + r] = d->vinv[static_cast<size_t>(r) * Np + c];
        s->use();
        try {
            m.enable(n, d->stride, d->capacity, s->timeNow, nb, d->element, d->r, d->s, {&m.vert, &m.vinvT, &m.jac, &m.modal}, s->bytes,
                     s->stream,
                     [&] {
                         m.put(m.vert, d->vertices, static_cast<size_t>(8) * K, s->bytes, s->stream);
                         m.put(m.vinvT, vinvT.data(), vinvT.size(), s->bytes, s->stream);
                         m.put(m.jac, d->jacobi, static_cast<size_t>(Nq + 1) * Nq * 3, s->bytes, s->stream);
                         m.put(m.slot, d->curved_slot, static_cast<size_t>(K), s->bytes, s->stream);
                         m.modal.alloc(static_cast<size_t>(std::max(1, d->num_curved)) * 6 * Np, s->bytes, s->stream);
                         if (d->num_curved > 0)
                             hipCheck(hipMemcpyAsync(m.modal.p, d->modal, static_cast<size_t>(d->num_curved) * 6 * Np * sizeof(double),
                                                     hipMemcpyHostToDevice, s->stream), "hipMemcpy (drifters)");
                     },
                     [&] { s->drifterLaunch(kDriftInit, 0.0, -1); });
        } catch (...) {
            m.slot.release(); // (its bytes were put back with the others')
            throw;
        }
    });
}

int bdg_sw2d_curved_drifters_advance(bdg_sw2d_curved* s, double dt, int num_steps) {
    return guard([&] {
        requireCurvedDriftersOn(s, "bdg_sw2d_curved_drifters_advance");
        if (num_steps < 0) throw arg_error("bdg_sw2d_curved_drifters_advance: num_steps < 0");
        s->drf.reserve(num_steps, "bdg_sw2d_curved_drifters_advance", "bdg_sw2d_curved");
        s->use();
        for (int i = 0; i < num_steps; ++i) {
            s->drf.t += dt;
            s->drifterAdvance(dt);
        }
    });
}

int bdg_sw2d_curved_drifters_time(bdg_sw2d_curved* s, double dt, int count, float* ms) {
    return guard([&] {
        requireCurvedDriftersOn(s, "bdg_sw2d_curved_drifters_time");
        if (!ms || count < 1) throw arg_error("bdg_sw2d_curved_drifters_time: bad argument");
        s->use();
        *ms = bdg_dev::timePerRun(s->stream, count, [&] { s->drifterAdvance(dt, false); });
    });
}

int bdg_sw2d_curved_drifters_state(bdg_sw2d_curved* s, double* x, double* y, int* element, double* r, double* sref, int* status) {
    return guard([&] {
        requireCurvedDriftersOn(s, "bdg_sw2d_curved_drifters_state");
        s->use();
        s->drf.downloadState(x, y, element, r, sref, status, {}, s->stream);
    });
}

int bdg_sw2d_curved_drifters_count(const bdg_sw2d_curved* s, int* num_records, int* num_drifters) {
    return guard([&] {
        requireCurvedDriftersOn(s, "bdg_sw2d_curved_drifters_count");
        if (num_records) *num_records = s->drf.count;
        if (num_drifters) *num_drifters = s->drf.n;
    });
}

int bdg_sw2d_curved_drifters_read(bdg_sw2d_curved* s, int first, int count, double* t, double* x, double* y, int* status) {
    return guard([&] {
        requireCurvedDriftersOn(s, "bdg_sw2d_curved_drifters_read");
        s->use();
        s->drf.readTracks("bdg_sw2d_curved_drifters_read", first, count, t, x, y, status, s->stream);
    });
}

int bdg_sw2d_curved_drifters_reset(bdg_sw2d_curved* s) {
    return guard([&] {
        requireCurvedDriftersOn(s, "bdg_sw2d_curved_drifters_reset");
        s->drf.count = 0;
    });
}

} // extern "C"
