// sw2d_monitor_kernel.hpp -- the run monitor of the triangle sw2d solver (gfx950 / CDNA4, wave64): conservation integrals,
// energy, extrema and a NaN count of the resident state, and the primitive fields at fixed stations (gauges), all formed on
// the device and stored as one record per sample in device memory. Two launches per sample, on the solver's stream, following
// the contract of sw2d_quad_monitor_kernel.hpp:
//
//   sw2d_monitor_reduce_kernel   a fixed grid of kTriMonBlocks workgroups of 256 threads; one partial record per workgroup
//   sw2d_monitor_finish_kernel   one workgroup: the partials combined, the gauges evaluated, the record stored
//
// The summation order is fixed, so a sample of a given state is the same bits whenever and however often it is taken:
//   * workgroup b owns the device slots [b chunk, (b + 1) chunk) of the owned range [0, count), chunk a multiple of 64
//     (triMonChunk); workgroups past the end own nothing and store the neutral partial; slots >= count (ghost elements and
//     the padding up to ld) are never read;
//   * thread t of it visits the slots k = b chunk + t, + 256, ... in ascending order, and of each the nodes 0 .. Np - 1 in
//     ascending order, acc = acc + w f for every integral (one multiply, one add, no contraction);
//   * the 256 accumulators of a workgroup are added through LDS in the tree a[t] += a[t + s], s = 128, 64, .. 1;
//   * the finish kernel adds the partials in ascending workgroup order from 0.0.
// Minima and maxima skip NaNs (fmin / fmax) and do not depend on the order; the NaN count covers every field, is a sum of
// small integers and is exact. No floating-point atomics anywhere.
//
// The slots are the solver's own: a solver that renumbered its elements sums them in its device order (the weight plane is
// uploaded through the same renumbering), so its integrals agree with those of a solver in the caller's order to the
// summation bound, not bit for bit.
//
// Lane = element: a wave reads 64 consecutive slots of one node row, q[node * ld + slot], one contiguous 512-byte transaction
// per load, the layout of the stage kernels. Every state plane, the weights and H are read once. Np and the field count are
// run-time arguments (as in sw2d_quad_monitor_kernel.hpp): one instance serves orders 1 to 8 and three or four fields.
//
// Per node: the integrands h, hu, hv (four fields: hN) and the energy density
//   e = (hu hu + hv hv) / (2 h) + (0.5 g) ((h - H) (h - H)),   H = 0 where the monitor has none,
// each operation rounded once, the division the correctly rounded one.
//
// Gauges: eta = h - H, u = hu / h, v = hv / h (N = hN / h) are formed at the nodes of the gauge's element by the rule of
// sw2d_output_kernel (sw2d_kernels.hpp) and interpolated with the gauge's row of nodal basis values,
//   value = sum_n row[n] f[n],  ascending n from 0.0, no contraction.
// A gauge on a node has a unit vector for its row and returns the nodal value bit for bit. A gauge whose slot is not in
// [0, count) (a ghost element of a partitioned run) is left at 0: its owner supplies it.
//
// Records are stored by column, rec[column * capacity + slot], so that the columns that share a reduction operator are
// contiguous for the all-reduce of a partitioned run. Column order (the record layout of include/blitzdg_hip.h):
//   t, int h, int hu, int hv, (int hN,) E, min h, max h, max|hu|, max|hv|, NaN count, then per gauge eta, u, v (, N).
#pragma once
#include <hip/hip_runtime.h>

namespace bdg_dev {

constexpr int kTriMonBlocks = 512;  // fixed grid of the reduction
constexpr int kTriMonThreads = 256;
constexpr int kTriMonPartial = 10;  // int h, int hu, int hv, int hN, E, min h, max h, max|hu|, max|hv|, NaN count

// slots per workgroup: a multiple of 64, so that every wave reads whole 512-byte rows
inline int triMonChunk(int count) {
    const int per = (count + kTriMonBlocks - 1) / kTriMonBlocks;
    return (per + 63) / 64 * 64;
}

struct TriMonParams {
    const double* q;        // the state: `fields` planes of Np*ld
    const double* w;        // quadrature weights m[n] J, Np*ld, zero in the padding
    const double* H;        // Np*ld, or NULL: H = 0
    long long ld;
    int Np, fields, count, chunk;
    double g;
};

__global__ __launch_bounds__(kTriMonThreads) void sw2d_monitor_reduce_kernel(TriMonParams p, double* __restrict__ partials) {
#pragma clang fp contract(off)
    __shared__ double red[kTriMonPartial][kTriMonThreads];
    const int Np = p.Np, t = threadIdx.x;
    const long long plane = static_cast<long long>(Np) * p.ld;
    const long long kb = static_cast<long long>(blockIdx.x) * p.chunk;
    const long long ke = kb + p.chunk < p.count ? kb + p.chunk : p.count;
    const double* __restrict__ q = p.q;
    const double* __restrict__ w = p.w;
    const double* __restrict__ H = p.H;
    const double halfG = 0.5 * p.g;
    double sh = 0.0, shu = 0.0, shv = 0.0, shn = 0.0, se = 0.0, nn = 0.0;
    double hmin = __builtin_inf(), hmax = -__builtin_inf(), humax = 0.0, hvmax = 0.0;
    for (long long k = kb + t; k < ke; k += kTriMonThreads) {
#pragma unroll 4
        for (int n = 0; n < Np; ++n) {
            const long long o = n * p.ld + k;
            const double wn = w[o], h = q[o], hu = q[plane + o], hv = q[2 * plane + o];
            const double d = H ? h - H[o] : h;
            sh = sh + wn * h;
            shu = shu + wn * hu;
            shv = shv + wn * hv;
            const double e = (hu * hu + hv * hv) / (2.0 * h) + halfG * (d * d);
            se = se + wn * e;
            hmin = fmin(hmin, h);
            hmax = fmax(hmax, h);
            humax = fmax(humax, fabs(hu));
            hvmax = fmax(hvmax, fabs(hv));
            nn += (h != h ? 1.0 : 0.0) + (hu != hu ? 1.0 : 0.0) + (hv != hv ? 1.0 : 0.0);
            if (p.fields == 4) {
                const double hn = q[3 * plane + o];
                shn = shn + wn * hn;
                nn += hn != hn ? 1.0 : 0.0;
            }
        }
    }
    red[0][t] = sh; red[1][t] = shu; red[2][t] = shv; red[3][t] = shn; red[4][t] = se;
    red[5][t] = hmin; red[6][t] = hmax; red[7][t] = humax; red[8][t] = hvmax; red[9][t] = nn;
    __syncthreads();
    for (int s = kTriMonThreads / 2; s > 0; s >>= 1) {
        if (t < s) {
#pragma unroll
            for (int c = 0; c < 5; ++c) red[c][t] = red[c][t] + red[c][t + s];
            red[5][t] = fmin(red[5][t], red[5][t + s]);
#pragma unroll
            for (int c = 6; c < 9; ++c) red[c][t] = fmax(red[c][t], red[c][t + s]);
            red[9][t] = red[9][t] + red[9][t + s];
        }
        __syncthreads();
    }
    if (t < kTriMonPartial) partials[blockIdx.x * kTriMonPartial + t] = red[t][0];
}

struct TriMonFinish {
    const double* partials; // kTriMonBlocks x kTriMonPartial
    const double* q;
    const double* H;        // or NULL
    const int* gaugeSlot;   // device slot of each gauge's element
    const double* row;      // (numGauges, Np): the nodal basis at each gauge
    double* rec;            // records by column: rec[column * capacity + slot]
    long long ld;
    int Np, fields, count, numGauges, capacity, slot;
    double t;               // model time of the sample
};

__global__ __launch_bounds__(kTriMonThreads) void sw2d_monitor_finish_kernel(TriMonFinish p) {
#pragma clang fp contract(off)
    __shared__ double sp[kTriMonBlocks * kTriMonPartial];
    const int t = threadIdx.x, nf = p.fields;
    for (int i = t; i < kTriMonBlocks * kTriMonPartial; i += kTriMonThreads) sp[i] = p.partials[i];
    __syncthreads();
    double* out = p.rec + p.slot;
    const long long cap = p.capacity;
    if (t == 0) out[0] = p.t;
    if (t < kTriMonPartial && (t != 3 || nf == 4)) {
        double acc = t == 5 ? __builtin_inf() : (t == 6 ? -__builtin_inf() : 0.0);
        for (int b = 0; b < kTriMonBlocks; ++b) {
            const double v = sp[b * kTriMonPartial + t];
            acc = t == 5 ? fmin(acc, v) : (t >= 6 && t <= 8 ? fmax(acc, v) : acc + v);
        }
        const int col = 1 + (t < 3 ? t : (nf == 4 ? t : t - 1)); // without a tracer the columns after int hv move up by one
        out[col * cap] = acc;
    }
    // one thread per (gauge, field)
    const int Np = p.Np, first = nf + 7;
    const long long plane = static_cast<long long>(Np) * p.ld;
    for (int gf = t; gf < p.numGauges * nf; gf += kTriMonThreads) {
        const int gi = gf / nf, c = gf % nf, k = p.gaugeSlot[gi];
        double val = 0.0;
        if (k >= 0 && k < p.count) {
            const double* row = p.row + static_cast<long long>(gi) * Np;
            for (int n = 0; n < Np; ++n) {
                const long long o = n * p.ld + k;
                const double h = p.q[o];
                const double f = c == 0 ? (p.H ? h - p.H[o] : h) : p.q[c * plane + o] / h;
                val = val + row[n] * f;
            }
        }
        out[(first + gf) * cap] = val;
    }
}

} // namespace bdg_dev
