// sw2d_monitor_kernel.hpp -- the run monitor of the triangle and the quadrilateral sw2d solvers (gfx950 / CDNA4, wave64):
// conservation integrals, energy, extrema and a NaN count of the resident state, and the primitive fields at fixed stations
// (gauges), all formed on the device and stored as one record per sample in device memory. Two launches per sample, on the
// solver's stream:
//
//   sw2d_monitor_reduce_kernel        a fixed grid of kMonBlocks workgroups of 256 threads; one partial record per workgroup
//   sw2d_monitor_finish_kernel        one workgroup: the partials combined, the gauges evaluated by the row rule (triangles)
//   sw2d_quad_monitor_finish_kernel   ... by the tensor rule (quadrilaterals)
//
// Both device objects include this header, so the kernels are static: each translation unit keeps its own.
//
// The summation contract. The order is fixed, so a sample of a given state is the same bits whenever and however often it is
// taken:
//   * workgroup b owns the device slots [b chunk, (b + 1) chunk) of the owned range [0, count), chunk a multiple of 64
//     (monChunk); workgroups past the end own nothing and store the neutral partial; slots >= count (ghost elements and
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
// run-time arguments: one instance serves every order of both element shapes and three or four fields.
//
// Per node: the integrands h, hu, hv (four fields: hN) and the energy density
//   e = (hu hu + hv hv) / (2 h) + (0.5 g) ((h - H) (h - H)),   H = 0 where the monitor has none,
// each operation rounded once, the division the correctly rounded one.
//
// Gauges: eta = h - H, u = hu / h, v = hv / h (N = hN / h) are formed at the nodes of the gauge's element by the rule of the
// output kernels (sw2d_output_kernel in sw2d_kernels.hpp, sw2d_quad_output_kernel.hpp) and interpolated
//   * row rule (MonRowGauges): with the gauge's row of nodal basis values,
//       value = sum_n row[n] f[n],  ascending n from 0.0, no contraction;
//   * tensor rule (MonTensorGauges): with the 1-D Lagrange basis values lr (at the gauge's r) and ls (at its s), along r first
//     and then along s (node (N+1) j + i sits at r = r1d[j], s = r1d[i]):
//       value = sum_i ls[i] (sum_j lr[j] f[(N+1) j + i]),  both sums ascending from 0.0, no contraction.
// A gauge on a node has a unit vector for its row (for lr and ls) and returns the nodal value bit for bit. A gauge whose slot
// is not in [0, count) (a ghost element of a partitioned run) is left at 0: its owner supplies it.
//
// Records are stored by column, rec[column * capacity + slot], so that the columns that share a reduction operator are
// contiguous for the all-reduce of a partitioned run. Column order (the record layout of include/blitzdg_hip.h):
//   t, int h, int hu, int hv, (int hN,) E, min h, max h, max|hu|, max|hv|, NaN count, then per gauge eta, u, v (, N).
#pragma once
#include <hip/hip_runtime.h>

namespace bdg_dev {

constexpr int kMonBlocks = 512;  // fixed grid of the reduction
constexpr int kMonThreads = 256;
constexpr int kMonPartial = 10;  // int h, int hu, int hv, int hN, E, min h, max h, max|hu|, max|hv|, NaN count

// slots per workgroup: a multiple of 64, so that every wave reads whole 512-byte rows
inline int monChunk(int count) {
    const int per = (count + kMonBlocks - 1) / kMonBlocks;
    return (per + 63) / 64 * 64;
}

struct MonParams {
    const double* q;        // the state: `fields` planes of Np*ld
    const double* w;        // quadrature weights (mass weight times J), Np*ld, zero in the padding
    const double* H;        // Np*ld, or NULL: H = 0
    long long ld;
    int Np, fields, count, chunk;
    double g;
};

static __global__ __launch_bounds__(kMonThreads) void sw2d_monitor_reduce_kernel(MonParams p, double* __restrict__ partials) {
#pragma clang fp contract(off)
    __shared__ double red[kMonPartial][kMonThreads];
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
    for (long long k = kb + t; k < ke; k += kMonThreads) {
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
    for (int s = kMonThreads / 2; s > 0; s >>= 1) {
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
    if (t < kMonPartial) partials[blockIdx.x * kMonPartial + t] = red[t][0];
}

struct MonFinish {
    const double* partials; // kMonBlocks x kMonPartial
    const double* q;
    const double* H;        // or NULL
    const int* gaugeSlot;   // device slot of each gauge's element
    double* rec;            // records by column: rec[column * capacity + slot]
    long long ld;
    int Np, fields, count, numGauges, capacity, slot;
    double t;               // model time of the sample
};

// field c of a gauge at the node of offset o: eta, or the state plane c over h
__device__ inline double monPrimitive(const MonFinish& p, int c, long long o) {
#pragma clang fp contract(off)
    const double h = p.q[o];
    return c == 0 ? (p.H ? h - p.H[o] : h) : p.q[c * (static_cast<long long>(p.Np) * p.ld) + o] / h;
}

// the row rule: one row of Np nodal basis values per gauge
struct MonRowGauges {
    const double* row;      // (numGauges, Np)
    __device__ double value(const MonFinish& p, int gi, int c, int k) const {
#pragma clang fp contract(off)
        const double* r = row + static_cast<long long>(gi) * p.Np;
        double val = 0.0;
        for (int n = 0; n < p.Np; ++n) val = val + r[n] * monPrimitive(p, c, n * p.ld + k);
        return val;
    }
};

// the tensor rule: along r, then along s
struct MonTensorGauges {
    const double* lr;       // (numGauges, Nq): the 1-D basis at each gauge's r
    const double* ls;       // ... and at its s
    int Nq;                 // N + 1
    __device__ double value(const MonFinish& p, int gi, int c, int k) const {
#pragma clang fp contract(off)
        const double* r = lr + gi * Nq;
        const double* s = ls + gi * Nq;
        double val = 0.0;
        for (int i = 0; i < Nq; ++i) {
            double acc = 0.0;
            for (int j = 0; j < Nq; ++j) acc = acc + r[j] * monPrimitive(p, c, (j * Nq + i) * p.ld + k);
            val = val + s[i] * acc;
        }
        return val;
    }
};

// one workgroup of kMonThreads: the partials to the record's columns, then one thread per (gauge, field)
template <class Gauges>
__device__ inline void monFinish(const MonFinish& p, const Gauges& gauges) {
#pragma clang fp contract(off)
    __shared__ double sp[kMonBlocks * kMonPartial];
    const int t = threadIdx.x, nf = p.fields;
    for (int i = t; i < kMonBlocks * kMonPartial; i += kMonThreads) sp[i] = p.partials[i];
    __syncthreads();
    double* out = p.rec + p.slot;
    const long long cap = p.capacity;
    if (t == 0) out[0] = p.t;
    if (t < kMonPartial && (t != 3 || nf == 4)) {
        double acc = t == 5 ? __builtin_inf() : (t == 6 ? -__builtin_inf() : 0.0);
        for (int b = 0; b < kMonBlocks; ++b) {
            const double v = sp[b * kMonPartial + t];
            acc = t == 5 ? fmin(acc, v) : (t >= 6 && t <= 8 ? fmax(acc, v) : acc + v);
        }
        const int col = 1 + (t < 3 ? t : (nf == 4 ? t : t - 1)); // without a tracer the columns after int hv move up by one
        out[col * cap] = acc;
    }
    const int first = nf + 7;
    for (int gf = t; gf < p.numGauges * nf; gf += kMonThreads) {
        const int gi = gf / nf, c = gf % nf, k = p.gaugeSlot[gi];
        out[(first + gf) * cap] = k >= 0 && k < p.count ? gauges.value(p, gi, c, k) : 0.0;
    }
}

[[maybe_unused]] static __global__ __launch_bounds__(kMonThreads) void sw2d_monitor_finish_kernel(MonFinish p, MonRowGauges gauges) {
    monFinish(p, gauges);
}

[[maybe_unused]] static __global__ __launch_bounds__(kMonThreads) void sw2d_quad_monitor_finish_kernel(MonFinish p,
                                                                                                      MonTensorGauges gauges) {
    monFinish(p, gauges);
}

} // namespace bdg_dev
