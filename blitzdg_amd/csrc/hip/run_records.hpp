// run_records.hpp -- what the triangle solver (sw2d_device.hip) and the quadrilateral one (sw2d_quad_device.hip) share of
// the run monitor (sw2d_monitor_kernel.hpp), the field statistics (sw2d_stats_kernel.hpp) and the drifters
// (sw2d_drifter_driver.hpp) on the host: the bookkeeping of the
// records, their buffers, the launches, the reads and the all-reduce of a partitioned run. What differs stays with each
// solver: the gauge and drifter tables and their checks, the choice of H, stepDone and the partition test. The per-order
// objects never include this header.
//
// `prefix` is the solver's prefix of the C ABI ("bdg_sw2d", "bdg_sw2dq") and `fn` the entry point: messages name both.
#pragma once
#include "halo_transport.hpp"
#include "sw2d_drifter_driver.hpp"
#include "sw2d_monitor_kernel.hpp"
#include "sw2d_stats_kernel.hpp"
#include <algorithm>
#include <cmath>
#include <initializer_list>
#include <string>
#include <utility>
#include <vector>

namespace bdg_records {

using bdg_detail::arg_error;
using bdg_dev::DevBuf;
using bdg_dev::hipCheck;

// completed LSERK4 steps (of `perStep` stages) among the next `stages` stages after `stageCount`
inline long long lserkSteps(long long stageCount, long long stages, int perStep) {
    return (stageCount + stages) / perStep - stageCount / perStep;
}

// records that `steps` further steps take at one record per `stride` steps; refused before anything is launched
inline void reserve(long long done, long long steps, int stride, int free, const char* fn, const std::string& what,
                    const std::string& calls) {
    const long long take = (done + steps) / stride - done / stride;
    if (take > free)
        throw arg_error(std::string(fn) + ": the call would take " + std::to_string(take) + " " + what + " records and " +
                        std::to_string(free) + " are free (" + calls + "_read, then " + calls + "_reset)");
}

// what a sample reads: the resident state, the depth (or NULL), the owned range [0, count) and the model time
struct MonitorView {
    const double* q;
    const double* H;
    long long ld;
    int Np, fields, count;
    double g, t;
};

// the run monitor (`prefix`_enable_monitor); the solver adds the buffers of its gauge rule
struct MonitorState {
    bool on = false;
    int stride = 1, capacity = 0, numGauges = 0, width = 0;
    int count = 0;        // records taken
    int reduced = 0;      // records [0, reduced) have been all-reduced
    long long steps = 0;  // completed steps since set_state / monitor_reset
    DevBuf<double> w, H, partials, rec, stage;
    DevBuf<int> element;  // device slot of each gauge's element

    void requireOn(const char* fn, const std::string& prefix) const {
        if (!on) throw arg_error(std::string(fn) + ": the monitor is not enabled (" + prefix + "_enable_monitor)");
    }
    // the checks every `prefix`_enable_monitor makes first; Desc: weights, stride, capacity, num_gauges, gauge_element
    template <class Desc>
    void checkEnable(const std::string& fn, const Desc* d, int K) const {
        if (!d || !d->weights) throw arg_error(fn + ": the descriptor and its weights are required");
        if (on) throw arg_error(fn + ": the monitor is already enabled");
        if (d->stride < 1 || d->capacity < 1) throw arg_error(fn + ": stride and capacity must be >= 1");
        if (d->num_gauges < 0 || (d->num_gauges > 0 && !d->gauge_element)) throw arg_error(fn + ": bad gauge list");
        for (int i = 0; i < d->num_gauges; ++i)
            if (d->gauge_element[i] < 0 || d->gauge_element[i] >= K)
                throw arg_error(fn + ": gauge " + std::to_string(i) + " names an element outside [0, K)");
    }
    // the buffers: `tables()` allocates and fills w, H and the solver's `own`; the gauges' device slots, the partials, the
    // records and `spare` (one more record outside the array, or NULL; one of `own`) follow. A failure leaves the solver
    // without a monitor and `bytes` where it was.
    template <class Tables>
    void enable(int stride_, int capacity_, int ng, int fields, const int* slots, std::initializer_list<DevBuf<double>*> own,
                DevBuf<double>* spare, size_t& bytes, hipStream_t stream, Tables&& tables) {
        const int width_ = 7 + fields + ng * fields;
        const size_t bytesBefore = bytes;
        try {
            tables();
            element.alloc(static_cast<size_t>(std::max(1, ng)), bytes, stream);
            if (ng > 0)
                hipCheck(hipMemcpyAsync(element.p, slots, static_cast<size_t>(ng) * sizeof(int), hipMemcpyHostToDevice, stream),
                         "hipMemcpy (gauges)");
            partials.alloc(static_cast<size_t>(bdg_dev::kMonBlocks) * bdg_dev::kMonPartial, bytes, stream);
            rec.alloc(static_cast<size_t>(width_) * capacity_, bytes, stream);
            if (spare) spare->alloc(static_cast<size_t>(width_), bytes, stream);
            hipCheck(hipStreamSynchronize(stream), "hipStreamSynchronize"); // the host staging vectors die here
        } catch (...) {
            (void)hipStreamSynchronize(stream);
            for (DevBuf<double>* b : {&w, &H, &partials, &rec}) b->release();
            for (DevBuf<double>* b : own) b->release();
            element.release();
            bytes = bytesBefore;
            throw;
        }
        on = true;
        stride = stride_; capacity = capacity_; numGauges = ng; width = width_;
    }
    void reserve(long long more, const char* fn, const std::string& prefix) const {
        if (on) bdg_records::reserve(steps, more, stride, capacity - count, fn, "monitor", prefix + "_monitor");
    }
    // one record of `v` into to[column * cap + slot]: the reduction, then `finish` with the solver's gauge rule
    template <class Gauges>
    void launch(const MonitorView& v, double* to, int cap, int slot, void (*finish)(bdg_dev::MonFinish, Gauges), const char* finishName,
                const Gauges& gauges, hipStream_t stream) const {
        using namespace bdg_dev;
        const MonParams rp{v.q, w.p, v.H, v.ld, v.Np, v.fields, v.count, monChunk(v.count), v.g};
        hipLaunchKernelGGL(sw2d_monitor_reduce_kernel, dim3(kMonBlocks), dim3(kMonThreads), 0, stream, rp, partials.p);
        hipCheck(hipGetLastError(), "sw2d_monitor_reduce_kernel launch");
        const MonFinish fp{partials.p, v.q, v.H, element.p, to, v.ld, v.Np, v.fields, v.count, numGauges, cap, slot, v.t};
        hipLaunchKernelGGL(finish, dim3(1), dim3(kMonThreads), 0, stream, fp, gauges);
        hipCheck(hipGetLastError(), finishName);
    }
    // ... as the next record (room was reserved by the caller)
    template <class Gauges>
    void sample(const MonitorView& v, void (*finish)(bdg_dev::MonFinish, Gauges), const char* finishName, const Gauges& gauges,
                hipStream_t stream) {
        launch(v, rec.p, capacity, count, finish, finishName, gauges, stream);
        ++count;
    }
    void requireFree(const char* fn, const std::string& prefix) const {
        if (count >= capacity) throw arg_error(std::string(fn) + ": no free record (" + prefix + "_monitor_reset)");
    }
    // records [first, first + n) by row into `records`
    void read(const char* fn, int first, int n, double* records, hipStream_t stream) const {
        if (first < 0 || n < 0 || first > count - n || (n > 0 && !records)) throw arg_error(std::string(fn) + ": bad record range");
        if (n == 0) return;
        std::vector<double> cols(static_cast<size_t>(width) * n); // by column, as on the device
        hipCheck(hipMemcpy2DAsync(cols.data(), n * sizeof(double), rec.p + first, capacity * sizeof(double), n * sizeof(double),
                                  width, hipMemcpyDeviceToHost, stream), "hipMemcpy2D (records)");
        hipCheck(hipStreamSynchronize(stream), "hipStreamSynchronize");
        for (int i = 0; i < n; ++i)
            for (int c = 0; c < width; ++c) records[static_cast<size_t>(i) * width + c] = cols[static_cast<size_t>(c) * n + i];
    }
    void reset() { count = 0; reduced = 0; steps = 0; }
    // the records not yet reduced, summed / minimised / maximised over the ranks of `comm`, in the order of `stream`
    void allReduce(ncclComm_t comm, hipStream_t stream, int fields, size_t& bytes) {
        const int n = count - reduced;
        if (n <= 0) return;
        // the new records of every column but t, packed by column; the columns that share an operator are contiguous
        const int cols = width - 1;
        if (!stage.p) stage.alloc(static_cast<size_t>(cols) * capacity, bytes);
        hipCheck(hipMemcpy2DAsync(stage.p, n * sizeof(double), rec.p + capacity + reduced, capacity * sizeof(double),
                                  n * sizeof(double), cols, hipMemcpyDeviceToDevice, stream), "hipMemcpy2D (records)");
        auto reduce = [&](int firstCol, int numCols, ncclRedOp_t op) {
            if (numCols <= 0) return;
            double* at = stage.p + static_cast<size_t>(firstCol) * n;
            bdg_rccl::ncclCheck(bdg_rccl::rccl().AllReduce(at, at, static_cast<size_t>(numCols) * n, ncclDouble, op, comm, stream),
                                "ncclAllReduce");
        };
        reduce(0, fields + 1, ncclSum);                     // integrals and E
        reduce(fields + 1, 1, ncclMin);                     // min h
        reduce(fields + 2, 3, ncclMax);                     // max h, max|hu|, max|hv|
        reduce(fields + 5, cols - (fields + 5), ncclSum);   // NaN count and gauges
        hipCheck(hipMemcpy2DAsync(rec.p + capacity + reduced, capacity * sizeof(double), stage.p, n * sizeof(double),
                                  n * sizeof(double), cols, hipMemcpyDeviceToDevice, stream), "hipMemcpy2D (records)");
        reduced = count;
    }
};

// what a sample of the field statistics reads: the resident state, the depth (or NULL), the owned range [0, count) and the
// model time
struct StatsView {
    const double* q;
    const double* H;
    long long ld;
    int Np, count;
    double t;
};

// the field statistics (`prefix`_enable_field_stats, sw2d_stats_kernel.hpp): the accumulator planes on the device and, on the
// host, the log of the samples: one row t, c_1, s_1, .. c_m, s_m per sample, exactly the values passed to the kernel
struct FieldStatsState {
    bool on = false, mean = false, envelope = false;
    int stride = 1, m = 0;
    long long steps = 0;  // completed steps since set_state / field_stats_reset
    size_t plane = 0;     // entries of one plane, Np * ld
    double omega[bdg_dev::kStatsMaxPeriods] = {};
    DevBuf<double> acc, H;
    std::vector<double> log;

    int planes() const { return bdg_dev::statsPlanes(mean, envelope, m); }
    int rowWidth() const { return 1 + 2 * m; }
    int count() const { return static_cast<int>(log.size() / rowWidth()); }
    void requireOn(const char* fn, const std::string& prefix) const {
        if (!on) throw arg_error(std::string(fn) + ": field statistics are not enabled (" + prefix + "_enable_field_stats)");
    }
    // the checks of `prefix`_enable_field_stats; Desc: H, stride, num_periods, periods, mean, envelope
    template <class Desc>
    void checkEnable(const std::string& fn, const Desc* d, bool partitioned) const {
        if (!d) throw arg_error(fn + ": the descriptor is required");
        if (on) throw arg_error(fn + ": field statistics are already enabled on this solver; the call is made once");
        if (d->stride < 1) throw arg_error(fn + ": stride must be >= 1");
        if (d->num_periods < 0 || d->num_periods > bdg_dev::kStatsMaxPeriods)
            throw arg_error(fn + ": num_periods must lie in [0, " + std::to_string(bdg_dev::kStatsMaxPeriods) + "]");
        for (int j = 0; j < d->num_periods; ++j)
            if (!(d->periods[j] > 0.0) || !std::isfinite(d->periods[j]))
                throw arg_error(fn + ": period " + std::to_string(j) + " must be > 0 and finite");
        if (!d->mean && !d->envelope && d->num_periods == 0)
            throw arg_error(fn + ": nothing to accumulate (mean, envelope and periods are all off)");
        if (partitioned)
            throw arg_error(fn + ": the solver has a partition set; the field statistics of a partitioned run are not accumulated "
                                 "(single domain only)");
    }
    // -inf, +inf, 0.0 in the envelopes and 0.0 everywhere else, on `stream`
    void clear(double* to, hipStream_t stream) const {
        using namespace bdg_dev;
        hipCheck(hipMemsetAsync(to, 0, static_cast<size_t>(planes()) * plane * sizeof(double), stream), "hipMemset");
        if (!envelope) return;
        const unsigned grid = static_cast<unsigned>((plane + kStatsThreads - 1) / kStatsThreads);
        double* env = to + static_cast<size_t>(statsEnvelopeBase(mean)) * plane;
        hipLaunchKernelGGL(sw2d_stats_fill_kernel, dim3(grid), dim3(kStatsThreads), 0, stream, env, static_cast<long long>(plane),
                           -__builtin_inf());
        hipLaunchKernelGGL(sw2d_stats_fill_kernel, dim3(grid), dim3(kStatsThreads), 0, stream, env + plane,
                           static_cast<long long>(plane), __builtin_inf());
        hipCheck(hipGetLastError(), "sw2d_stats_fill_kernel launch");
    }
    // the buffers: `depth()` allocates and fills H where the caller gave one; the accumulators follow. A failure leaves the
    // solver without field statistics and `bytes` where it was.
    template <class Desc, class Depth>
    void enable(const Desc& d, size_t plane_, size_t& bytes, hipStream_t stream, Depth&& depth) {
        const size_t bytesBefore = bytes;
        // the groups are members because planes() and clear() read them; a failure puts the unset state back
        mean = d.mean != 0; envelope = d.envelope != 0; m = d.num_periods; plane = plane_;
        try {
            depth();
            acc.alloc(static_cast<size_t>(planes()) * plane, bytes);
            clear(acc.p, stream);
            hipCheck(hipStreamSynchronize(stream), "hipStreamSynchronize");
        } catch (...) {
            (void)hipStreamSynchronize(stream);
            acc.release();
            H.release();
            bytes = bytesBefore;
            mean = envelope = false; m = 0; plane = 0;
            throw;
        }
        for (int j = 0; j < m; ++j) omega[j] = 2.0 * M_PI / d.periods[j];
        on = true;
        stride = d.stride; steps = 0;
        log.clear();
    }
    // one launch of the kernel on `stream`: the sample of `v` with the row `trig` (c_1, s_1, ..) into the planes at `to`
    void launch(const StatsView& v, const double* trig, double* to, hipStream_t stream) const {
        bdg_dev::StatsParams p{v.q, v.H, to, v.ld, v.Np, v.count, {}, {}};
        for (int j = 0; j < m; ++j) {
            p.c[j] = trig[2 * j];
            p.s[j] = trig[2 * j + 1];
        }
        hipCheck(bdg_dev::statsLaunch(mean, envelope, m, p, stream), "sw2d_stats_kernel launch");
    }
    // the row of a sample at the model time t: t, cos(omega_1 t), sin(omega_1 t), ..
    void trigRow(double t, double* row) const {
        row[0] = t;
        for (int j = 0; j < m; ++j) {
            row[1 + 2 * j] = std::cos(omega[j] * t);
            row[2 + 2 * j] = std::sin(omega[j] * t);
        }
    }
    // ... accumulated and logged
    void sample(const StatsView& v, hipStream_t stream) {
        double row[1 + 2 * bdg_dev::kStatsMaxPeriods];
        trigRow(v.t, row);
        launch(v, row + 1, acc.p, stream);
        log.insert(log.end(), row, row + rowWidth());
    }
    // the device slot of a plane: `which` as BDG_FIELD_STATS_* of include/blitzdg_hip.h (sum, etaMax, hMin, speedMax, cos, sin),
    // index the field (sum) or 3 j + field (cos, sin)
    const double* planeOf(const char* fn, int which, int index) const {
        using namespace bdg_dev;
        const std::string f(fn);
        int at = -1;
        if (which == 0) {
            if (!mean) throw arg_error(f + ": the mean group is not enabled");
            if (index < 0 || index >= 3) throw arg_error(f + ": index outside [0, 3)");
            at = index;
        } else if (which >= 1 && which <= 3) {
            if (!envelope) throw arg_error(f + ": the envelope group is not enabled");
            if (index != 0) throw arg_error(f + ": index must be 0");
            at = statsEnvelopeBase(mean) + which - 1;
        } else if (which == 4 || which == 5) {
            if (m == 0) throw arg_error(f + ": the harmonic group is not enabled (no periods)");
            if (index < 0 || index >= 3 * m) throw arg_error(f + ": index outside [0, 3 * num_periods)");
            at = statsHarmonicBase(mean, envelope) + 6 * (index / 3) + (which == 5 ? 3 : 0) + index % 3;
        } else {
            throw arg_error(f + ": unknown plane");
        }
        return acc.p + static_cast<size_t>(at) * plane;
    }
    // rows [first, first + n) of the sample log into `rows`
    void samples(const char* fn, int first, int n, double* rows) const {
        if (first < 0 || n < 0 || first > count() - n || (n > 0 && !rows)) throw arg_error(std::string(fn) + ": bad sample range");
        std::copy(log.begin() + static_cast<size_t>(first) * rowWidth(), log.begin() + static_cast<size_t>(first + n) * rowWidth(), rows);
    }
    // accumulators, log and step counter as after enable
    void reset(hipStream_t stream) {
        clear(acc.p, stream);
        log.clear();
        steps = 0;
    }
    // average device milliseconds of one sample, `count` of them into scratch accumulators that live for the call
    float time(const StatsView& v, int count_, size_t& bytes, hipStream_t stream) const {
        const size_t bytesBefore = bytes;
        DevBuf<double> scratch;
        float ms = 0.0f;
        try {
            scratch.alloc(static_cast<size_t>(planes()) * plane, bytes);
            clear(scratch.p, stream);
            double row[1 + 2 * bdg_dev::kStatsMaxPeriods];
            trigRow(v.t, row);
            launch(v, row + 1, scratch.p, stream); // once before the clock starts
            ms = bdg_dev::timePerRun(stream, count_, [&] { launch(v, row + 1, scratch.p, stream); });
        } catch (...) {
            (void)hipStreamSynchronize(stream);
            bytes = bytesBefore;
            throw;
        }
        hipCheck(hipStreamSynchronize(stream), "hipStreamSynchronize");
        bytes = bytesBefore;
        return ms;
    }
};

// the drifters (`prefix`_enable_drifters); the solver adds its element tables. Elements and neighbours are device slots.
struct DrifterState {
    bool on = false;
    int n = 0, stride = 1, capacity = 0;
    int count = 0;        // records taken
    long long steps = 0;  // advances made
    double t = 0.0;       // time of the next record: the model time in the stepping calls, + dt per `prefix`_drifters_advance
    DevBuf<double> x, y, r, s, u0, v0, recT, recX, recY;
    DevBuf<int> neigh, k, status, recStatus;

    void requireOn(const char* fn, const std::string& prefix) const {
        if (!on) throw arg_error(std::string(fn) + ": drifters are not enabled (" + prefix + "_enable_drifters)");
    }
    // the checks every `prefix`_enable_drifters makes after those of its descriptor's pointers
    void checkEnable(const std::string& fn, int count_, int stride_, int capacity_, bool partitioned) const {
        if (stride_ < 1 || capacity_ < 1) throw arg_error(fn + ": stride and capacity must be >= 1");
        if (on) throw arg_error(fn + ": drifters are already enabled on this solver; the call is made once");
        if (partitioned)
            throw arg_error(fn + ": the solver has a partition set; drifters do not migrate between ranks (single domain only)");
        if (static_cast<long long>(count_) * capacity_ >= (1LL << 31)) throw arg_error(fn + ": count * capacity must stay below 2^31");
    }
    template <class T>
    static void put(DevBuf<T>& buf, const T* src, size_t count, size_t& bytes, hipStream_t stream) {
        buf.alloc(count, bytes);
        hipCheck(hipMemcpyAsync(buf.p, src, count * sizeof(T), hipMemcpyHostToDevice, stream), "hipMemcpy (drifters)");
    }
    // the buffers: `tables()` fills the solver's `own`; the neighbours, the drifters at (slots, r0, s0) and the records follow;
    // `init()` launches the kernel in mode kDriftInit (x, y from the map, (u0, v0) from the resident state). A failure leaves
    // the solver without drifters and `bytes` where it was.
    template <class Tables, class Init>
    void enable(int count_, int stride_, int capacity_, double t0, const std::vector<int>& nb, const int* slots, const double* r0,
                const double* s0, std::initializer_list<DevBuf<double>*> own, size_t& bytes, hipStream_t stream, Tables&& tables,
                Init&& init) {
        const size_t bytesBefore = bytes, num = static_cast<size_t>(count_), cells = num * capacity_;
        try {
            tables();
            put(neigh, nb.data(), nb.size(), bytes, stream);
            put(k, slots, num, bytes, stream);
            put(r, r0, num, bytes, stream);
            put(s, s0, num, bytes, stream);
            for (DevBuf<double>* b : {&x, &y, &u0, &v0}) b->alloc(num, bytes, stream);
            status.alloc(num, bytes, stream);
            recT.alloc(static_cast<size_t>(capacity_), bytes, stream);
            recX.alloc(cells, bytes, stream);
            recY.alloc(cells, bytes, stream);
            recStatus.alloc(cells, bytes, stream);
            n = count_;
            init();
            hipCheck(hipStreamSynchronize(stream), "hipStreamSynchronize"); // the host staging vectors die here
        } catch (...) {
            (void)hipStreamSynchronize(stream);
            for (DevBuf<double>* b : {&x, &y, &r, &s, &u0, &v0, &recT, &recX, &recY}) b->release();
            for (DevBuf<double>* b : own) b->release();
            for (DevBuf<int>* b : {&neigh, &k, &status, &recStatus}) b->release();
            n = 0;
            bytes = bytesBefore;
            throw;
        }
        on = true;
        stride = stride_; capacity = capacity_; count = 0; steps = 0; t = t0;
    }
    // as MonitorState::reserve: records `more` further advances would take
    void reserve(long long more, const char* fn, const std::string& prefix) const {
        if (on) bdg_records::reserve(steps, more, stride, capacity - count, fn, "drifter", prefix + "_drifters");
    }
    // one launch of the solver's drifter kernel on `stream`, reading the state q; slot < 0: no record
    template <class Tables>
    void launch(void (*kernel)(bdg_dev::DriftParams, Tables), const char* kernelName, const Tables& tab, const double* q, long long ld,
                int N, int mode, double dt, int slot, hipStream_t stream) const {
        using namespace bdg_dev;
        const DriftParams p{q, x.p, y.p, r.p, s.p, u0.p, v0.p, k.p, status.p, recT.p, recX.p, recY.p, recStatus.p, ld, N, n, mode,
                            slot, dt, t};
        hipLaunchKernelGGL(kernel, dim3((n + kDriftThreads - 1) / kDriftThreads), dim3(kDriftThreads), 0, stream, p, tab);
        hipCheck(hipGetLastError(), kernelName);
    }
    // the record slot of the next advance if one is due (room was reserved by the caller), else -1
    int takeSlot(bool record) { return record && ++steps % stride == 0 ? count++ : -1; }
    // the drifters as they are now; NULL arguments are skipped; callerOf: device slot -> caller element (empty = identity)
    void downloadState(double* x_, double* y_, int* element, double* r_, double* s_, int* status_, const std::vector<int>& callerOf,
                       hipStream_t stream) const {
        const size_t num = static_cast<size_t>(n);
        const std::pair<double*, const double*> dbl[] = {{x_, x.p}, {y_, y.p}, {r_, r.p}, {s_, s.p}};
        for (const auto& c : dbl)
            if (c.first) hipCheck(hipMemcpyAsync(c.first, c.second, num * sizeof(double), hipMemcpyDeviceToHost, stream), "hipMemcpy (drifters)");
        if (element) hipCheck(hipMemcpyAsync(element, k.p, num * sizeof(int), hipMemcpyDeviceToHost, stream), "hipMemcpy (drifters)");
        if (status_) hipCheck(hipMemcpyAsync(status_, status.p, num * sizeof(int), hipMemcpyDeviceToHost, stream), "hipMemcpy (drifters)");
        hipCheck(hipStreamSynchronize(stream), "hipStreamSynchronize");
        if (element && !callerOf.empty())
            for (size_t i = 0; i < num; ++i) element[i] = callerOf[element[i]];
    }
    // records [first, first + num) of the tracks; NULL arguments are skipped
    void readTracks(const char* fn, int first, int num, double* t_, double* x_, double* y_, int* status_, hipStream_t stream) const {
        if (first < 0 || num < 0 || first > count - num) throw arg_error(std::string(fn) + ": bad record range");
        if (num == 0) return;
        const size_t at = static_cast<size_t>(first) * n, cells = static_cast<size_t>(num) * n;
        if (t_) hipCheck(hipMemcpyAsync(t_, recT.p + first, num * sizeof(double), hipMemcpyDeviceToHost, stream), "hipMemcpy (tracks)");
        if (x_) hipCheck(hipMemcpyAsync(x_, recX.p + at, cells * sizeof(double), hipMemcpyDeviceToHost, stream), "hipMemcpy (tracks)");
        if (y_) hipCheck(hipMemcpyAsync(y_, recY.p + at, cells * sizeof(double), hipMemcpyDeviceToHost, stream), "hipMemcpy (tracks)");
        if (status_)
            hipCheck(hipMemcpyAsync(status_, recStatus.p + at, cells * sizeof(int), hipMemcpyDeviceToHost, stream), "hipMemcpy (tracks)");
        hipCheck(hipStreamSynchronize(stream), "hipStreamSynchronize");
    }
};

} // namespace bdg_records
