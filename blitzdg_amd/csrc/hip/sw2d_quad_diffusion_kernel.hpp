// sw2d_quad_diffusion_kernel.hpp -- diffusion, source and decay of the passive tracer hN (plane 3 of a four-field state) on
// quadrilaterals (gfx950 / CDNA4, wave64):
//   T = div(kappa h grad N) + S - k hN,   N = hN / h,
// local DG with central fluxes and no penalty, as tests/tridiff_ref.py defines it (the quadrilateral glue is
// tests/quaddiff_ref.py). A face node whose neighbour is itself (vmapP == vmapM) is a BOUNDARY node with zero diffusive flux,
// walls and the open boundary alike: the test is on the decoded entry of the solver's first gather index (QuadParams::gidx,
// wall nodes with the sign flag), never on variant B's open-boundary image.
//
// Two launches behind the unchanged stage launch of every evaluation, because the second reads the neighbours' output of the
// first. Both have the shape of sw2d_quad_stage_kernel (sw2d_quad_kernel.hpp): one 256-thread workgroup per tile of
// QuadElem<N>::E consecutive elements, rows of a tile contiguous, node items (n, e) and face-node items (fn, e), the tensor
// operators D1 | l0 | lN of the ops image in LDS (Dr = D1 (x) I, Ds = I (x) D1, a face lift one column of the inverse 1-D mass
// matrix), phases separated by workgroup barriers.
//   sw2d_quad_tracer_gradient_kernel
//     A  node items: N = hN / h of the tile to LDS;
//     B  face-node items: own trace from LDS, the neighbour's hN / h gathered; Fscale nx dN / 2 and Fscale ny dN / 2 to LDS,
//        0 at boundary nodes;
//     C  node items: the two tensor derivatives of N, the metric, the four face lifts; fx, fy = kappa h (qx, qy) into the two
//        scratch planes dp.flux (kappa a scalar or a plane).
//   sw2d_quad_tracer_divergence_kernel
//     A  node items: fx, fy of the tile to LDS;
//     B  face-node items: Fscale dF / 2, dF = nx (fx- - fx+) + ny (fy- - fy+) from the own and the gathered fluxes, at
//        boundary nodes 2 (nx fx- + ny fy-) by select;
//     C  node items: derivatives, metric and lifts, + S - k hN; a filtered evaluation puts the whole T back into LDS (the flux
//        rows are dead by then) and applies the dense Filter rows, read from global memory as the stage kernels read them;
//        then the update of plane 3 only:
//          QMODE_RHS      rhs4  += T
//          QMODE_COMBINE  qout4 += cc T
//          QMODE_LSERK    res4  += cc T,  qout4 += cb cc T
//          QMODE_HEUN     qout4 += cc T              (the sponge divides hu and hv only: the term is linear in every mode)
// Both read p.qin, which the stage launch in front of them read and did not write (sw2d_quad_device.hip: in rk2Step, heunStep
// and lserkStage qin differs from every buffer the stage writes).
// Geometry: GEN = false reads 16 numbers per element, GEN = true per-node metric and per-face-node normals, as the stage kernel.
// LDS in doubles: ops | 2 Np E | 2 NFN E (gradient), ops | 2 Np E | NFN E (divergence): 30 / 26 KB at N = 8, 29 / 26 KB at
// N = 12 (tiles of 8).
// No existing kernel header includes this one; its instances live in sw2d_quad_diffusion_order.hip.
#pragma once
#include "sw2d_quad_kernel.hpp"

namespace bdg_dev {

template <int N>
struct QuadDiffElem : QuadElem<N> {
    using Q = QuadElem<N>;
    // LDS in doubles: ops | 2 node arrays [a][n][e] (N, or fx and fy; the first reused for the unfiltered T) | 2 surface arrays
    static constexpr int OFF_SURF = Q::OFF_FL + 2 * Q::Np * Q::E;
    static constexpr int LDS_GRADIENT = OFF_SURF + 2 * Q::NFN * Q::E; // Fscale nx dN / 2, Fscale ny dN / 2
    static constexpr int LDS_DIVERGENCE = OFF_SURF + Q::NFN * Q::E;   // Fscale dF / 2
};

struct QuadDiffusionParams {
    const double* kappaField; // Np*ld plane, or nullptr: the scalar kappa
    const double* source;     // Np*ld plane S, or nullptr
    double* flux;             // 2 planes of Np*ld: fx, fy (written by the gradient pass, read by the divergence pass)
    double kappa, decay;
};

// decoded entry of the gather index: the neighbour's offset n' * ld + k', with or without the wall flag
__device__ __forceinline__ long long quad_diff_neighbour(int gi) { return gi < 0 ? -(static_cast<long long>(gi) + 1) : gi; }

template <int N, bool GEN>
__global__ __launch_bounds__(256) void sw2d_quad_tracer_gradient_kernel(const QuadParams p, const QuadDiffusionParams dp) {
    using Q = QuadDiffElem<N>;
    constexpr int Nq = Q::Nq, Np = Q::Np, NFN = Q::NFN, E = Q::E, T = Q::THREADS;
    __shared__ double lds[Q::LDS_GRADIENT];
    double* const D1 = lds;
    double* const l0 = lds + Nq * Nq;
    double* const lN = l0 + Nq;
    double* const nv = lds + Q::OFF_FL;
    double* const surf = lds + Q::OFF_SURF;

    const int tid = threadIdx.x;
    const int k0 = p.kBegin + static_cast<int>(blockIdx.x) * E;
    const long long ld = p.ld;
    const long long plane = static_cast<long long>(Np) * ld;

    for (int i = tid; i < Q::OPS_DOUBLES; i += T) lds[i] = p.ops[i];

    // ---- A: concentration of the own state
#pragma unroll
    for (int m = 0; m < Q::NI; ++m) {
        const int idx = tid + T * m;
        if (idx < Np * E) {
            const int n = idx / E, e = idx % E, k = k0 + e;
            double c = 0.0;
            if (k < p.kEnd) {
                const long long o = n * ld + k;
                c = p.qin[3 * plane + o] / p.qin[o];
            }
            nv[n * E + e] = c;
        }
    }
    __syncthreads();

    // ---- B: jump of the concentration, times Fscale / 2 and the normal
#pragma unroll
    for (int m = 0; m < Q::FI; ++m) {
        const int idx = tid + T * m;
        if (idx < NFN * E) {
            const int fn = idx / E, e = idx % E, k = k0 + e;
            double sx = 0.0, sy = 0.0;
            if (k < p.kEnd) {
                const int f = fn / Nq, nn = fn % Nq;
                const int nM = Q::fmask(f, nn);
                const long long oM = nM * ld + k;
                const long long oP = quad_diff_neighbour(p.gidx[fn * ld + k]);
                if (oP != oM) {
                    double nx, ny, fs;
                    if (GEN) {
                        nx = p.fgeo[fn * ld + k];
                        ny = p.fgeo[(NFN + fn) * ld + k];
                        fs = p.fgeo[(2 * NFN + fn) * ld + k];
                    } else {
                        nx = p.ageo[(4 + f) * ld + k];
                        ny = p.ageo[(8 + f) * ld + k];
                        fs = p.ageo[(12 + f) * ld + k];
                    }
                    const double dN = nv[nM * E + e] - p.qin[3 * plane + oP] / p.qin[oP];
                    const double w = 0.5 * fs * dN;
                    sx = w * nx;
                    sy = w * ny;
                }
            }
            surf[fn * E + e] = sx;
            surf[(NFN + fn) * E + e] = sy;
        }
    }
    __syncthreads();

    // ---- C: q = grad N - Lift(...), flux = kappa h q
    constexpr int kUnrollC = N <= 6 ? Q::NI : 1;
#pragma unroll kUnrollC
    for (int m = 0; m < Q::NI; ++m) {
        const int idx = tid + T * m;
        if (idx < Np * E) {
            const int n = idx / E, e = idx % E, k = k0 + e;
            if (k >= p.kEnd) continue;
            const int j = n / Nq, i = n % Nq;
            double sr = 0.0, ss = 0.0;
#pragma unroll
            for (int q = 0; q < Nq; ++q) {
                sr += D1[j * Nq + q] * nv[(q * Nq + i) * E + e];
                ss += D1[i * Nq + q] * nv[(j * Nq + q) * E + e];
            }
            const long long o = n * ld + k;
            double rx, sx, ry, sy;
            if (GEN) {
                rx = p.geo[o];
                sx = p.geo[plane + o];
                ry = p.geo[2 * plane + o];
                sy = p.geo[3 * plane + o];
            } else {
                rx = p.ageo[k];
                sx = p.ageo[ld + k];
                ry = p.ageo[2 * ld + k];
                sy = p.ageo[3 * ld + k];
            }
            const double a0 = l0[i], a1 = lN[j], a2 = lN[i], a3 = l0[j];
            const int s0 = j * E + e, s1 = (Nq + i) * E + e, s2 = (2 * Nq + j) * E + e, s3 = (3 * Nq + i) * E + e;
            const double qx = rx * sr + sx * ss - (a0 * surf[s0] + a1 * surf[s1] + a2 * surf[s2] + a3 * surf[s3]);
            const double qy = ry * sr + sy * ss -
                              (a0 * surf[NFN * E + s0] + a1 * surf[NFN * E + s1] + a2 * surf[NFN * E + s2] + a3 * surf[NFN * E + s3]);
            const double kh = (dp.kappaField ? dp.kappaField[o] : dp.kappa) * p.qin[o]; // own depth again: an L2 hit
            dp.flux[o] = kh * qx;
            dp.flux[plane + o] = kh * qy;
        }
    }
}

// plane 3 of the stage update of one node (offset o in plane 0) gains its share of T
template <int MODE>
__device__ __forceinline__ void quad_diff_update(const QuadParams& p, long long o, long long plane, double t) {
    const long long o3 = 3 * plane + o;
    if (MODE == QMODE_RHS) {
        p.rhs[o3] += t;
    } else if (MODE == QMODE_LSERK) {
        const double a = p.cc * t;
        p.res[o3] += a;
        p.qout[o3] += p.cb * a;
    } else { // QMODE_COMBINE, QMODE_HEUN
        p.qout[o3] += p.cc * t;
    }
}

template <int N, int MODE, bool FILT, bool GEN>
__global__ __launch_bounds__(256) void sw2d_quad_tracer_divergence_kernel(const QuadParams p, const QuadDiffusionParams dp) {
    using Q = QuadDiffElem<N>;
    constexpr int Nq = Q::Nq, Np = Q::Np, NFN = Q::NFN, E = Q::E, T = Q::THREADS;
    __shared__ double lds[Q::LDS_DIVERGENCE];
    double* const D1 = lds;
    double* const l0 = lds + Nq * Nq;
    double* const lN = l0 + Nq;
    double* const fl = lds + Q::OFF_FL;
    double* const surf = lds + Q::OFF_SURF;

    const int tid = threadIdx.x;
    const int k0 = p.kBegin + static_cast<int>(blockIdx.x) * E;
    const long long ld = p.ld;
    const long long plane = static_cast<long long>(Np) * ld;

    for (int i = tid; i < Q::OPS_DOUBLES; i += T) lds[i] = p.ops[i];

    // ---- A: fluxes of the own elements
#pragma unroll
    for (int m = 0; m < Q::NI; ++m) {
        const int idx = tid + T * m;
        if (idx < Np * E) {
            const int n = idx / E, e = idx % E, k = k0 + e;
            double fx = 0.0, fy = 0.0;
            if (k < p.kEnd) {
                const long long o = n * ld + k;
                fx = dp.flux[o];
                fy = dp.flux[plane + o];
            }
            fl[n * E + e] = fx;
            fl[(Np + n) * E + e] = fy;
        }
    }
    __syncthreads();

    // ---- B: jump of the normal flux, times Fscale / 2
#pragma unroll
    for (int m = 0; m < Q::FI; ++m) {
        const int idx = tid + T * m;
        if (idx < NFN * E) {
            const int fn = idx / E, e = idx % E, k = k0 + e;
            double s = 0.0;
            if (k < p.kEnd) {
                const int f = fn / Nq, nn = fn % Nq;
                const int nM = Q::fmask(f, nn);
                const long long oM = nM * ld + k;
                const long long oP = quad_diff_neighbour(p.gidx[fn * ld + k]);
                double nx, ny, fs;
                if (GEN) {
                    nx = p.fgeo[fn * ld + k];
                    ny = p.fgeo[(NFN + fn) * ld + k];
                    fs = p.fgeo[(2 * NFN + fn) * ld + k];
                } else {
                    nx = p.ageo[(4 + f) * ld + k];
                    ny = p.ageo[(8 + f) * ld + k];
                    fs = p.ageo[(12 + f) * ld + k];
                }
                const double fxM = fl[nM * E + e], fyM = fl[(Np + nM) * E + e];
                const double fxP = dp.flux[oP], fyP = dp.flux[plane + oP]; // (a boundary node gathers itself)
                const double dF = oP != oM ? nx * (fxM - fxP) + ny * (fyM - fyP) : 2.0 * (nx * fxM + ny * fyM);
                s = 0.5 * fs * dF;
            }
            surf[fn * E + e] = s;
        }
    }
    __syncthreads();

    // ---- C: T; unfiltered modes update right away, filtered ones keep T for the filter
    constexpr int kUnrollC = N <= 6 || FILT ? Q::NI : 1;
    double r[FILT ? Q::NI : 1];
#pragma unroll kUnrollC
    for (int m = 0; m < Q::NI; ++m) {
        const int idx = tid + T * m;
        if (FILT) r[m] = 0.0;
        if (idx < Np * E) {
            const int n = idx / E, e = idx % E, k = k0 + e;
            if (k >= p.kEnd) continue;
            const int j = n / Nq, i = n % Nq;
            double xr = 0.0, xs = 0.0, yr = 0.0, ys = 0.0;
#pragma unroll
            for (int q = 0; q < Nq; ++q) {
                const double dj = D1[j * Nq + q], di = D1[i * Nq + q];
                xr += dj * fl[(q * Nq + i) * E + e];
                xs += di * fl[(j * Nq + q) * E + e];
                yr += dj * fl[(Np + q * Nq + i) * E + e];
                ys += di * fl[(Np + j * Nq + q) * E + e];
            }
            const long long o = n * ld + k;
            double rx, sx, ry, sy;
            if (GEN) {
                rx = p.geo[o];
                sx = p.geo[plane + o];
                ry = p.geo[2 * plane + o];
                sy = p.geo[3 * plane + o];
            } else {
                rx = p.ageo[k];
                sx = p.ageo[ld + k];
                ry = p.ageo[2 * ld + k];
                sy = p.ageo[3 * ld + k];
            }
            const double a0 = l0[i], a1 = lN[j], a2 = lN[i], a3 = l0[j];
            const int s0 = j * E + e, s1 = (Nq + i) * E + e, s2 = (2 * Nq + j) * E + e, s3 = (3 * Nq + i) * E + e;
            double t = rx * xr + sx * xs + ry * yr + sy * ys - (a0 * surf[s0] + a1 * surf[s1] + a2 * surf[s2] + a3 * surf[s3]);
            if (dp.source) t += dp.source[o];
            if (dp.decay != 0.0) t -= dp.decay * p.qin[3 * plane + o];
            if (FILT) r[m] = t;
            else quad_diff_update<MODE>(p, o, plane, t);
        }
    }

    if (FILT) {
        __syncthreads(); // every derivative read of fl is done
#pragma unroll
        for (int m = 0; m < Q::NI; ++m) {
            const int idx = tid + T * m;
            if (idx < Np * E) fl[idx] = r[m]; // [n][e]: idx = n * E + e
        }
        __syncthreads();
#pragma unroll 1
        for (int m = 0; m < Q::NI; ++m) {
            const int idx = tid + T * m;
            if (idx >= Np * E) break;
            const int n = idx / E, e = idx % E, k = k0 + e;
            if (k >= p.kEnd) continue;
            double a = 0.0;
#pragma unroll 4
            for (int q = 0; q < Np; ++q) a += p.filt[n * Np + q] * fl[q * E + e];
            quad_diff_update<MODE>(p, n * ld + k, plane, a);
        }
    }
}

} // namespace bdg_dev
