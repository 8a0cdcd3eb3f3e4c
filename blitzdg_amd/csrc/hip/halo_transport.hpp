// halo_transport.hpp -- the ghost exchange of a partitioned run, shared by the straight-element solver (sw2d_device.hip),
// the curved one (sw2d_curved_device.hip) and the quadrilateral one (sw2d_quad_device.hip): the neighbour table and its
// parse, the pack / unpack kernels, the grouped RCCL send / receive, and the communicator, exchange stream and staging
// buffers. The straight-element solver keeps its own events and stage schedule; the other two share the two-chain
// schedule of partition_schedule.hpp.
//
// A record is the `rows` doubles of one element, [field][node]. Records go out in the order of the send list and come
// in as the ghost elements, stored after the owned ones; each neighbour rank has one contiguous range of either.
#pragma once
#include "device_buffer.hpp"
#include "rccl_api.hpp"
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace bdg_halo {

using bdg_dev::DevBuf;
using bdg_dev::hipCheck;

struct Peer { int rank, sendStart, sendCount, recvStart, recvCount; };

// both ranges of `p` lie inside a partition of numSend send records and `ghosts` ghost elements
inline bool rangesFit(const Peer& p, int numSend, int ghosts) {
    return p.sendStart >= 0 && p.sendCount >= 0 && p.sendStart + p.sendCount <= numSend && p.recvStart >= 0 &&
           p.recvCount >= 0 && p.recvStart + p.recvCount <= ghosts;
}

// the peer table of `fn` from its five arrays. Refused: a rank outside [0, rankEnd) or equal to notRank, ranges that do
// not fit a partition of numSend send records and `ghosts` ghost elements (set with `prefix`_set_partition)
inline std::vector<Peer> parsePeers(const std::string& prefix, const char* fn, const int* ranks, const int* sendStart,
                                    const int* sendCount, const int* recvStart, const int* recvCount, int numPeers,
                                    int numSend, int ghosts, int rankEnd, int notRank = -1) {
    std::vector<Peer> peers;
    for (int i = 0; i < numPeers; ++i) {
        const Peer p{ranks[i], sendStart[i], sendCount[i], recvStart[i], recvCount[i]};
        if (p.rank < 0 || p.rank >= rankEnd || p.rank == notRank || !rangesFit(p, numSend, ghosts))
            throw bdg_detail::arg_error(prefix + "_" + fn + ": peer ranges do not fit the partition set with " + prefix + "_set_partition");
        peers.push_back(p);
    }
    return peers;
}

// internal linkage: each solver's translation unit has its own copy, and the library exports no symbol for them
namespace {

//   pack:   buf[i*rows + r] = q[r*ld + slots[i]]        (owned elements a neighbour rank needs)
//   unpack: q[r*ld + first + i] = buf[i*rows + r]       (ghost elements, stored after the owned ones)
__global__ void halo_pack_kernel(const double* __restrict__ q, double* __restrict__ buf, const int* __restrict__ slots,
                                 int count, int rows, long long ld) {
    const long long t = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (t >= static_cast<long long>(count) * rows) return;
    const long long r = t / count, i = t % count; // consecutive lanes read consecutive elements of one row
    buf[i * rows + r] = q[r * ld + slots[i]];
}

__global__ void halo_unpack_kernel(double* __restrict__ q, const double* __restrict__ buf, int first, int count,
                                   int rows, long long ld) {
    const long long t = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (t >= static_cast<long long>(count) * rows) return;
    const long long r = t / count, i = t % count;
    q[r * ld + first + i] = buf[i * rows + r];
}

// the `count` records of the elements slots[0, count) of the planes q (leading dimension ld) into buf
void pack(const double* q, long long ld, int rows, const int* slots, int count, double* buf, hipStream_t on) {
    if (count == 0) return;
    const long long n = static_cast<long long>(count) * rows;
    hipLaunchKernelGGL(halo_pack_kernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, on, q, buf, slots,
                       count, rows, ld);
    hipCheck(hipGetLastError(), "halo_pack_kernel");
}

// the `count` records of buf into the elements [first, first + count) of the planes q
void unpack(double* q, long long ld, int rows, int first, int count, const double* buf, hipStream_t on) {
    if (count == 0) return;
    const long long n = static_cast<long long>(count) * rows;
    hipLaunchKernelGGL(halo_unpack_kernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, on, q, buf, first,
                       count, rows, ld);
    hipCheck(hipGetLastError(), "halo_unpack_kernel");
}

} // namespace

struct Transport {
    std::vector<Peer> peers;
    ncclComm_t comm = nullptr; // null: no RCCL (the in-process group moves the records itself)
    int rank = 0, world = 1;
    hipStream_t stream = nullptr; // the exchange stream
    DevBuf<double> sendBuf, recvBuf, scalarBuf;

    ~Transport() {
        if (comm) (void)bdg_rccl::rccl().CommDestroy(comm);
        if (stream) (void)hipStreamDestroy(stream);
    }

    // the exchange stream and the staging buffers of numSend outgoing and `ghosts` incoming records of `rows` doubles
    void open(size_t rows, int numSend, int ghosts, size_t& bytes) {
        // (default priority: at the highest priority every stage of every order took about twice as long -- 8-way N=4 0.0958 against 0.0483 ms,
        // N=8 0.113 against 0.052, 2-way 0.293 against 0.205: profiles/r04_rehearsal_experiments.txt, call 28)
        hipCheck(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking), "hipStreamCreate");
        sendBuf.alloc(std::max<size_t>(1, static_cast<size_t>(numSend) * rows), bytes);
        recvBuf.alloc(std::max<size_t>(1, static_cast<size_t>(ghosts) * rows), bytes);
    }

    // an RCCL communicator (`uniqueId`: the 128 bytes of bdg_comm_unique_id), then open() and two doubles for all-reduces
    void connect(const void* uniqueId, int rank_, int world_, size_t rows, int numSend, int ghosts, size_t& bytes) {
        ncclUniqueId id;
        std::memcpy(&id, uniqueId, sizeof(id));
        bdg_rccl::ncclCheck(bdg_rccl::rccl().CommInitRank(&comm, world_, id, rank_), "ncclCommInitRank");
        rank = rank_;
        world = world_;
        open(rows, numSend, ghosts, bytes);
        scalarBuf.alloc(2, bytes);
    }

    // one grouped receive + send with every peer, in table order, on `on`: the peer's records of `rows` doubles each, or
    // at most maxDoubles of them
    void sendRecv(hipStream_t on, size_t rows, size_t maxDoubles = SIZE_MAX) const {
        if (peers.empty()) return;
        bdg_rccl::RcclApi& nc = bdg_rccl::rccl();
        bdg_rccl::ncclCheck(nc.GroupStart(), "ncclGroupStart");
        for (const Peer& pr : peers) {
            if (pr.recvCount > 0)
                bdg_rccl::ncclCheck(nc.Recv(recvBuf.p + static_cast<size_t>(pr.recvStart) * rows,
                                            std::min(static_cast<size_t>(pr.recvCount) * rows, maxDoubles), ncclDouble, pr.rank,
                                            comm, on), "ncclRecv");
            if (pr.sendCount > 0)
                bdg_rccl::ncclCheck(nc.Send(sendBuf.p + static_cast<size_t>(pr.sendStart) * rows,
                                            std::min(static_cast<size_t>(pr.sendCount) * rows, maxDoubles), ncclDouble, pr.rank,
                                            comm, on), "ncclSend");
        }
        bdg_rccl::ncclCheck(nc.GroupEnd(), "ncclGroupEnd");
    }
};

inline void requireComm(const Transport& halo, const std::string& prefix, const char* fn) {
    if (!halo.comm) throw bdg_detail::arg_error(std::string(fn) + ": no communicator (call " + prefix + "_comm_init first)");
}

} // namespace bdg_halo
