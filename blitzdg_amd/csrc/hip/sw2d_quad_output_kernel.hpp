// sw2d_quad_output_kernel.hpp -- output step of the quadrilateral sw2d solver (gfx950 / CDNA4, wave64): the drivers'
// primitive fields eta = h - H, u = hu / h, v = hv / h (four fields: N = hN / h) of the resident state, optionally
// interpolated to each element's equispaced (N+1)^2 lattice -- what QuadNodesProvisioner::splitElements does on the host
// before a *.vtu is written (reference src/QuadNodesProvisioner.cpp:721-749) -- before they leave the device.
//
// One launch serves every requested field: h is read once and shared by all of them, so the compulsory traffic is
// (fields + 1 (+ 1 with H)) planes in and `fields` planes out.
//
// The lattice is a tensor lattice and the nodes are the tensor Gauss-Lobatto nodes (node (N+1) j + i at r = r1d[j],
// s = r1d[i]; lattice point (N+1) n + m at r = equi[m], s = equi[n]), so the (Np, Np) matrix of splitElements factors as
// IM(n (N+1) + m, (N+1) j + i) = I1(m, j) I1(n, i) and is applied as two 1-D passes, 2 (N+1)^3 multiply-adds per field and
// element instead of (N+1)^4:
//   pass 1 (along r)  T(m, i) = sum_j I1(m, j) val(j, i)
//   pass 2 (along s)  out(n, m) = sum_i I1(n, i) T(m, i)
//
// Mapping to the hardware: a workgroup of N+1 waves owns 64 consecutive elements, lane = element, the same
// q[node * ld + k] layout as the stage kernels, so every load and store is one contiguous 512-byte wave transaction. In
// pass 1 wave w owns the node column i = w: it keeps the N+1 values of h of that column in registers for every field, forms
// the field's N+1 values and writes its N+1 sums T(., i) to LDS ([m][i][lane]: conflict-free). After a workgroup barrier
// wave w owns the lattice column m = w: it reads T(m, .) back and stores the N+1 lattice rows n (N+1) + m. A thread never
// holds more than 3 (N+1) doubles, whatever the order; LDS is 512 (N+1)^2 bytes (41 KiB at N = 8, three workgroups per CU).
// I1 is read through a uniform address with compile-time offsets (scalar loads).
//
// Contraction is off, division is the correctly rounded one and both sums run in ascending order from 0.0: without a
// lattice the values are h - H, hu / h, ... of the downloaded state bit for bit, and with one they equal the same two
// passes written in NumPy bit for bit.
#pragma once
#include <hip/hip_runtime.h>

namespace bdg_dev {

struct QuadOutParams {
    const double* q;   // the state: `fields` planes of Np*ld
    const double* H;   // Np*ld, or NULL: eta = h
    const double* I1;  // (N+1) x (N+1) row-major, or NULL: nodal values, no interpolation
    double* out;       // plane c receives field c of (eta, u, v, N)
    long long ld;      // plane stride (multiple of 64)
    int kEnd;          // the elements [0, kEnd) are written (a partitioned run: the owned ones)
    int mask;          // bit c: field c is wanted
};

template <int N, int NF, bool LAT>
__global__ __launch_bounds__(64 * (N + 1)) void sw2d_quad_output_kernel(const double* __restrict__ q, const double* __restrict__ H,
                                                                         const double* __restrict__ I1, double* __restrict__ out,
                                                                         long long ld, int kEnd, int mask) {
#pragma clang fp contract(off)
    constexpr int Nq = N + 1, Np = Nq * Nq;
    __shared__ double T[LAT ? Np * 64 : 1];
    const int e = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int k = static_cast<int>(blockIdx.x) * 64 + e;
    const bool live = k < kEnd;
    const long long plane = static_cast<long long>(Np) * ld;

    // node column i = w: h, and H where there is one
    double h[Nq], val[Nq];
#pragma unroll
    for (int j = 0; j < Nq; ++j) h[j] = live ? q[(j * Nq + w) * ld + k] : 1.0;

#pragma unroll
    for (int c = 0; c < NF; ++c) {
        if (!((mask >> c) & 1)) continue; // (uniform over the grid)
#pragma unroll
        for (int j = 0; j < Nq; ++j) {
            const long long o = (j * Nq + w) * ld + k;
            if (c == 0) val[j] = (H != nullptr && live) ? h[j] - H[o] : h[j];
            else val[j] = live ? q[c * plane + o] / h[j] : 0.0;
        }
        if (!LAT) {
            if (live) {
#pragma unroll
                for (int j = 0; j < Nq; ++j) out[c * plane + (j * Nq + w) * ld + k] = val[j];
            }
            continue;
        }
        // pass 1, along r
#pragma unroll
        for (int m = 0; m < Nq; ++m) {
            double acc = 0.0;
#pragma unroll
            for (int j = 0; j < Nq; ++j) acc = acc + I1[m * Nq + j] * val[j];
            T[(m * Nq + w) * 64 + e] = acc;
        }
        __syncthreads();
        // pass 2, along s: lattice column m = w
        double t[Nq];
#pragma unroll
        for (int i = 0; i < Nq; ++i) t[i] = T[(w * Nq + i) * 64 + e];
#pragma unroll
        for (int n = 0; n < Nq; ++n) {
            double acc = 0.0;
#pragma unroll
            for (int i = 0; i < Nq; ++i) acc = acc + I1[n * Nq + i] * t[i];
            if (live) out[c * plane + (n * Nq + w) * ld + k] = acc;
        }
        __syncthreads(); // T is rewritten by the next field
    }
}

// one order's launcher (sw2d_quad_order.hip, -DBDG_ORDER=N); fields: 3 or 4 planes in q
template <int N>
hipError_t sw2d_quad_output_launch(int fields, const QuadOutParams& p, hipStream_t stream);

hipError_t sw2d_quad_output(int order, int fields, const QuadOutParams& p, hipStream_t stream);

} // namespace bdg_dev
