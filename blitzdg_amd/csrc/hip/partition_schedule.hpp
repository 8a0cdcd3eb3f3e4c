// partition_schedule.hpp -- what the partitioned runs of the curved solver (sw2d_curved_device.hip) and the quadrilateral
// one (sw2d_quad_device.hip) share on top of halo_transport.hpp: the element partition and its checks, the communicator
// set-up, exchange and barrier, and the two-chain schedule that evaluates the interior elements beside the exchange.
// Host code only. What differs stays with each solver: the record size, its launches, its stream-order fallback and
// its overlap switch.
//
// `prefix` is the solver's prefix of the C ABI ("bdg_sw2d_curved", "bdg_sw2dq"): messages name the entry point.
#pragma once
#include "halo_transport.hpp"
#include <string>

namespace bdg_halo {

using bdg_detail::arg_error;

// The mesh of a rank is ordered [interior: numInterior | partition boundary: up to numOwned | ghosts: up to K]; ghost
// columns are refreshed from their owners before every evaluation, never evaluated. sendEls: the owned elements that
// neighbour ranks need, in the order of the send records.
struct Partition {
    int numOwned = 0, numInterior = 0, numSend = 0;
    DevBuf<int> sendEls;

    // `prefix`_set_partition of a mesh of K elements; maxNeighbour[k]: the largest element that element k gathers from
    void set(const std::string& prefix, int K, const std::vector<int>& maxNeighbour, int interior, int owned,
             const int* sendElements, int send, bool commOpen, size_t& bytes, hipStream_t stream) {
        const std::string fn = prefix + "_set_partition";
        if (owned < 1 || owned > K || interior < 0 || interior > owned || send < 0 || (send > 0 && !sendElements))
            throw arg_error(fn + ": bad argument");
        for (int i = 0; i < send; ++i)
            if (sendElements[i] < 0 || sendElements[i] >= owned)
                throw arg_error(fn + ": a send element is not an owned element");
        // The two-chain schedule evaluates [0, interior) beside the exchange: it is race-free only if no such element
        // reads a ghost column and none of them is packed for a neighbour. A plan that breaks either is refused here
        // (it would otherwise give stale ghost reads, not an error).
        for (int k = 0; k < interior; ++k)
            if (maxNeighbour[static_cast<size_t>(k)] >= owned)
                throw arg_error(fn + ": element " + std::to_string(k) +
                                " is listed as interior but has a ghost neighbour (elements >= num_owned)");
        for (int i = 0; i < send; ++i)
            if (sendElements[i] < interior)
                throw arg_error(fn + ": send element " + std::to_string(sendElements[i]) +
                                " lies in the interior range [0, num_interior)");
        if (commOpen) throw arg_error(fn + ": the communicator is already initialised");
        numOwned = owned;
        numInterior = interior;
        numSend = send;
        sendEls.alloc(static_cast<size_t>(std::max(1, send)), bytes, stream);
        if (send > 0)
            hipCheck(hipMemcpyAsync(sendEls.p, sendElements, static_cast<size_t>(send) * sizeof(int), hipMemcpyHostToDevice,
                                    stream), "send list upload");
        hipCheck(hipStreamSynchronize(stream), "send list sync");
    }
};

// Two chains over the evaluations e = 0, 1, ... of one call, ordered by events only:
//   solver stream A:   wait B(e-1) -> [interior elements of evaluation e] -> signal A(e)
//   exchange stream B: wait A(e-1) -> pack, grouped send / receive, unpack of the state e reads -> [partition-boundary
//                      elements of e] -> signal B(e)
// interior(e) reads the columns boundary(e-1) wrote and overwrites columns boundary(e-1) read: it waits for B(e-1);
// boundary(e) and its pack read / overwrite columns interior(e-1) wrote / read: B waits for A(e-1). Ghost columns are
// written by the unpack and read by the boundary launch only, both on B. Ghost elements are not evaluated.
struct TwoChains {
    hipEvent_t evA[2] = {nullptr, nullptr}, evB[2] = {nullptr, nullptr}, evEntry = nullptr;
    int e = 0; // evaluations issued since begin()

    // (events that only order kernels of this device's two streams: no system-scope fence, as in bdg_sw2d_comm_init)
    void create() {
        for (hipEvent_t* ev : {&evA[0], &evA[1], &evB[0], &evB[1], &evEntry})
            hipCheck(hipEventCreateWithFlags(ev, hipEventDisableTiming | hipEventDisableSystemFence), "hipEventCreate");
    }
    ~TwoChains() { // (the owner has drained both streams)
        for (hipEvent_t ev : {evA[0], evA[1], evB[0], evB[1], evEntry})
            if (ev) (void)hipEventDestroy(ev);
    }
    void begin(hipStream_t a, hipStream_t b) {
        e = 0;
        hipCheck(hipEventRecord(evEntry, a), "hipEventRecord"); // whatever set the state, on A
        hipCheck(hipStreamWaitEvent(b, evEntry, 0), "hipStreamWaitEvent");
    }
    // one evaluation: interior(a) launches the interior elements, boundary(b) the exchange and the partition-boundary ones
    template <class Interior, class Boundary>
    void eval(hipStream_t a, hipStream_t b, Interior&& interior, Boundary&& boundary) {
        const int cur = e & 1, prev = cur ^ 1;
        if (e > 0) hipCheck(hipStreamWaitEvent(a, evB[prev], 0), "hipStreamWaitEvent");
        interior(a);
        hipCheck(hipEventRecord(evA[cur], a), "hipEventRecord");
        if (e > 0) hipCheck(hipStreamWaitEvent(b, evA[prev], 0), "hipStreamWaitEvent");
        boundary(b);
        hipCheck(hipEventRecord(evB[cur], b), "hipEventRecord");
        ++e;
    }
    void end(hipStream_t a, hipStream_t b) { // join both ways: later work on A sees the last boundary update, later work on B the last interior launch
        if (e == 0) return;
        hipCheck(hipStreamWaitEvent(a, evB[(e - 1) & 1], 0), "hipStreamWaitEvent");
        hipCheck(hipStreamWaitEvent(b, evA[(e - 1) & 1], 0), "hipStreamWaitEvent");
    }
};

// `prefix`_comm_init: the communicator, the exchange stream and buffers for records of `rows` doubles, the events
inline void commInit(const std::string& prefix, Transport& halo, const Partition& part, TwoChains& chains, int K, size_t rows,
                     int rank, int world, const void* uniqueId, const int* peerRanks, const int* sendStart,
                     const int* sendCount, const int* recvStart, const int* recvCount, int numPeers, size_t& bytes,
                     hipStream_t stream) {
    if (!uniqueId || world < 1 || rank < 0 || rank >= world || numPeers < 0 ||
        (numPeers > 0 && (!peerRanks || !sendStart || !sendCount || !recvStart || !recvCount)))
        throw arg_error(prefix + "_comm_init: bad argument");
    if (halo.comm) throw arg_error(prefix + "_comm_init: communicator already initialised");
    if (part.numOwned < 1) throw arg_error(prefix + "_comm_init: call " + prefix + "_set_partition first");
    const int ghosts = K - part.numOwned;
    std::vector<Peer> peers = parsePeers(prefix, "comm_init", peerRanks, sendStart, sendCount, recvStart, recvCount, numPeers,
                                         part.numSend, ghosts, world);
    halo.connect(uniqueId, rank, world, rows, part.numSend, ghosts, bytes);
    halo.peers = std::move(peers);
    chains.create();
    for (DevBuf<double>* b : {&halo.sendBuf, &halo.recvBuf, &halo.scalarBuf}) b->zero(stream);
    hipCheck(hipStreamSynchronize(stream), "exchange buffers");
}

namespace { // (calls the pack / unpack of this translation unit)
// ghost columns of `state` (K columns of leading dimension ld) from their owners: pack -> grouped send / receive with
// every neighbour -> unpack, in the order of stream `on`
void exchange(const Transport& halo, const Partition& part, double* state, long long ld, int rows, int K, hipStream_t on) {
    pack(state, ld, rows, part.sendEls.p, part.numSend, halo.sendBuf.p, on);
    halo.sendRecv(on, static_cast<size_t>(rows));
    unpack(state, ld, rows, part.numOwned, K - part.numOwned, halo.recvBuf.p, on);
}
} // namespace

// both streams drained on every rank: an all-reduce of one double on `stream` after the local work
inline void barrier(const Transport& halo, hipStream_t stream) {
    hipCheck(hipStreamSynchronize(halo.stream), "hipStreamSynchronize");
    hipCheck(hipStreamSynchronize(stream), "hipStreamSynchronize");
    bdg_rccl::ncclCheck(bdg_rccl::rccl().AllReduce(halo.scalarBuf.p, halo.scalarBuf.p, 1, ncclDouble, ncclMax, halo.comm, stream),
                        "ncclAllReduce");
    hipCheck(hipStreamSynchronize(stream), "hipStreamSynchronize");
}

} // namespace bdg_halo
