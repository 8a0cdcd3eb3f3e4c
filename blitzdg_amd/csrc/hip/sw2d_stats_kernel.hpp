// sw2d_stats_kernel.hpp -- field statistics of the triangle and the quadrilateral sw2d solvers (gfx950 / CDNA4, wave64): sums,
// extrema and harmonic sums of eta, u, v at every node, accumulated over the samples of a run in device memory. One launch per
// sample on the solver's stream; what is left for the host is a small least-squares solve at the end of the run
// (blitzdg_amd/_records.py, harmonicFit).
//
// Both device objects include this header (through run_records.hpp), so the kernels are static: each translation unit keeps
// its own. The per-order objects never include it.
//
// Per entry of the owned slots [0, count) and the nodes [0, Np) the kernel reads h, hu, hv (and H where there is one) from the
// layout q[field][node * ld + slot] that both solvers share, forms by the rule of the output and the monitor kernels
//   eta = h - H  (h without H),   u = hu / h,   v = hv / h     (the correctly rounded division)
// and updates the accumulator planes, each (Np, ld) like a state plane, in this order inside `acc`:
//   mean group      sum[f] = sum[f] + f                                    f = eta, u, v                    3 planes
//   envelope group  etaMax = fmax(etaMax, eta), hMin = fmin(hMin, h),
//                   speedMax = fmax(speedMax, sqrt(u u + v v))                                              3 planes
//   harmonic group  C[j][f] = C[j][f] + f c_j,  S[j][f] = S[j][f] + f s_j     j < m <= 4, per j: C then S   6 m planes
// c_j = cos(omega_j t) and s_j = sin(omega_j t) are formed on the host in double and passed as arguments: no transcendental
// runs on the device.
//
// The arithmetic contract. Every update is one multiply and one add, each rounded once (no contraction); u u + v v is two
// multiplies and one add; the square root is the correctly rounded one; fmax / fmin skip NaNs, as in the monitor; the
// envelopes start from -inf, +inf and 0.0 and everything else from 0.0. There are no atomics and no reductions: an entry
// depends on its own history alone, so the result does not depend on the grid or on the order of the elements, and NumPy
// restates it bit for bit (tests/fieldstats_ref.py).
//
// A group that is switched off costs no traffic: its planes are not allocated, read or written (the kernel is instantiated
// per set of groups). Per sample the pass moves 3 (+ 1 for H) + 2 (3 [mean] + 3 [envelope] + 6 m) planes.
//
// Lane = two adjacent slots of one node row: a wave reads 128 consecutive slots, two whole 512-byte rows of the stage kernels'
// layout, with one 16-byte access per lane and plane (ld is a multiple of 64 and every plane starts on a multiple of it, so
// the accesses are aligned). The last lane of an odd `count` takes its one slot with 8-byte accesses; slots >= count (ghost
// elements and the padding up to ld) are neither read nor written. Np is a run-time argument: one set of instances serves
// every order of both element shapes and three or four fields (hN is not analysed).
#pragma once
#include <hip/hip_runtime.h>

namespace bdg_dev {

constexpr int kStatsThreads = 256;
constexpr int kStatsMaxPeriods = 4;

struct StatsParams {
    const double* q;        // the state: planes of Np*ld, h, hu, hv first
    const double* H;        // Np*ld, or NULL: eta = h
    double* acc;            // the accumulator planes of the enabled groups, Np*ld each
    long long ld;
    int Np, count;
    double c[kStatsMaxPeriods], s[kStatsMaxPeriods]; // cos(omega_j t), sin(omega_j t) of this sample
};

// planes of the enabled groups, and where each group starts
constexpr int statsPlanes(bool mean, bool envelope, int m) { return (mean ? 3 : 0) + (envelope ? 3 : 0) + 6 * m; }
constexpr int statsEnvelopeBase(bool mean) { return mean ? 3 : 0; }
constexpr int statsHarmonicBase(bool mean, bool envelope) { return (mean ? 3 : 0) + (envelope ? 3 : 0); }

// W adjacent slots of one row: one 16-byte access for W = 2, one 8-byte access for W = 1
template <int W>
struct StatsVec {
    double v[W];
};
template <int W>
__device__ inline StatsVec<W> statsLoad(const double* p) {
    StatsVec<W> r;
    if constexpr (W == 2) {
        const double2 t = *reinterpret_cast<const double2*>(p);
        r.v[0] = t.x; r.v[1] = t.y;
    } else {
        r.v[0] = p[0];
    }
    return r;
}
template <int W>
__device__ inline void statsStore(double* p, const StatsVec<W>& a) {
    if constexpr (W == 2) *reinterpret_cast<double2*>(p) = make_double2(a.v[0], a.v[1]);
    else p[0] = a.v[0];
}

// the update of W slots at the offset o of every plane
template <bool MEAN, bool ENV, int M, int W>
__device__ inline void statsUpdate(const StatsParams& p, long long plane, long long o) {
#pragma clang fp contract(off)
    const double* __restrict__ q = p.q;
    double* __restrict__ acc = p.acc;
    const StatsVec<W> h = statsLoad<W>(q + o), hu = statsLoad<W>(q + plane + o), hv = statsLoad<W>(q + 2 * plane + o);
    StatsVec<W> f[3]; // eta, u, v
    if (p.H) {
        const StatsVec<W> H = statsLoad<W>(p.H + o);
#pragma unroll
        for (int i = 0; i < W; ++i) f[0].v[i] = h.v[i] - H.v[i];
    } else {
        f[0] = h;
    }
#pragma unroll
    for (int i = 0; i < W; ++i) {
        f[1].v[i] = hu.v[i] / h.v[i];
        f[2].v[i] = hv.v[i] / h.v[i];
    }
    if constexpr (MEAN) {
        StatsVec<W> a[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) a[c] = statsLoad<W>(acc + c * plane + o);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma unroll
            for (int i = 0; i < W; ++i) a[c].v[i] = a[c].v[i] + f[c].v[i];
            statsStore<W>(acc + c * plane + o, a[c]);
        }
    }
    if constexpr (ENV) {
        double* __restrict__ env = acc + statsEnvelopeBase(MEAN) * plane + o;
        StatsVec<W> etaMax = statsLoad<W>(env), hMin = statsLoad<W>(env + plane), speedMax = statsLoad<W>(env + 2 * plane);
#pragma unroll
        for (int i = 0; i < W; ++i) {
            const double uu = f[1].v[i] * f[1].v[i], vv = f[2].v[i] * f[2].v[i];
            etaMax.v[i] = fmax(etaMax.v[i], f[0].v[i]);
            hMin.v[i] = fmin(hMin.v[i], h.v[i]);
            speedMax.v[i] = fmax(speedMax.v[i], sqrt(uu + vv));
        }
        statsStore<W>(env, etaMax);
        statsStore<W>(env + plane, hMin);
        statsStore<W>(env + 2 * plane, speedMax);
    }
#pragma unroll
    for (int j = 0; j < M; ++j) {
        double* __restrict__ har = acc + (statsHarmonicBase(MEAN, ENV) + 6 * j) * plane + o;
        const double cj = p.c[j], sj = p.s[j];
        StatsVec<W> a[6]; // C eta, u, v, then S eta, u, v
#pragma unroll
        for (int c = 0; c < 6; ++c) a[c] = statsLoad<W>(har + c * plane);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma unroll
            for (int i = 0; i < W; ++i) {
                a[c].v[i] = a[c].v[i] + f[c].v[i] * cj;
                a[3 + c].v[i] = a[3 + c].v[i] + f[c].v[i] * sj;
            }
        }
#pragma unroll
        for (int c = 0; c < 6; ++c) statsStore<W>(har + c * plane, a[c]);
    }
}

// grid: x over the pairs of slots, y over the nodes
template <bool MEAN, bool ENV, int M>
static __global__ __launch_bounds__(kStatsThreads) void sw2d_stats_kernel(StatsParams p) {
    const long long k = 2 * (static_cast<long long>(blockIdx.x) * kStatsThreads + threadIdx.x);
    if (k >= p.count) return;
    const long long plane = static_cast<long long>(p.Np) * p.ld;
    const long long o = static_cast<long long>(blockIdx.y) * p.ld + k;
    if (k + 1 < p.count) statsUpdate<MEAN, ENV, M, 2>(p, plane, o);
    else statsUpdate<MEAN, ENV, M, 1>(p, plane, o); // the tail of an odd count
}

// p[0 .. n) = value (the envelopes' initial values)
static __global__ __launch_bounds__(kStatsThreads) void sw2d_stats_fill_kernel(double* __restrict__ p, long long n, double value) {
    const long long i = static_cast<long long>(blockIdx.x) * kStatsThreads + threadIdx.x;
    if (i < n) p[i] = value;
}

template <bool MEAN, bool ENV, int M>
inline hipError_t statsLaunchInstance(const StatsParams& p, hipStream_t stream) {
    const long long pairs = (static_cast<long long>(p.count) + 1) / 2;
    if (pairs == 0) return hipSuccess;
    const dim3 grid(static_cast<unsigned>((pairs + kStatsThreads - 1) / kStatsThreads), static_cast<unsigned>(p.Np));
    hipLaunchKernelGGL((sw2d_stats_kernel<MEAN, ENV, M>), grid, dim3(kStatsThreads), 0, stream, p);
    return hipGetLastError();
}

template <bool MEAN, bool ENV>
inline hipError_t statsLaunchPeriods(int m, const StatsParams& p, hipStream_t stream) {
    switch (m) {
    case 0:
        if constexpr (MEAN || ENV) return statsLaunchInstance<MEAN, ENV, 0>(p, stream);
        else return hipErrorInvalidValue; // nothing to accumulate
    case 1: return statsLaunchInstance<MEAN, ENV, 1>(p, stream);
    case 2: return statsLaunchInstance<MEAN, ENV, 2>(p, stream);
    case 3: return statsLaunchInstance<MEAN, ENV, 3>(p, stream);
    case 4: return statsLaunchInstance<MEAN, ENV, 4>(p, stream);
    default: return hipErrorInvalidValue;
    }
}

// one sample of the groups (mean, envelope, m periods) on `stream`
inline hipError_t statsLaunch(bool mean, bool envelope, int m, const StatsParams& p, hipStream_t stream) {
    if (mean) return envelope ? statsLaunchPeriods<true, true>(m, p, stream) : statsLaunchPeriods<true, false>(m, p, stream);
    return envelope ? statsLaunchPeriods<false, true>(m, p, stream) : statsLaunchPeriods<false, false>(m, p, stream);
}

} // namespace bdg_dev
