// poisson2d_quad_kernel.hpp -- the elliptic operator A u = sigma u - div(kappa grad u) of poisson2d_kernel.hpp on quadrilaterals
// in parallelogram form (gfx950 / CDNA4, wave64; the definition is tests/poisson_ref.py, the quadrilateral glue
// tests/quadpoisson_ref.py). The same two passes with a launch boundary between them and the same mass product, in the shape of
// the quadrilateral tracer's diffusion passes (sw2d_quad_diffusion_kernel.hpp) instead of one lane per element: one 256-thread
// workgroup per tile of QuadElem<N>::E consecutive elements, node items (n, e) and face-node items (fn, e), the tensor operators
// D1 | l0 | lN of the ops image in LDS (Dr = D1 (x) I, Ds = I (x) D1, a face lift one column of the inverse 1-D mass matrix),
// phases separated by workgroup barriers, selects and no branches at boundary nodes.
//   poisson2d_quad_gradient_kernel
//     A  node items: u of the tile to LDS (FUSED: p = r + beta p_old, stored to the second direction plane);
//     B  face-node items: own trace from LDS, the neighbour's gathered (FUSED: updated on the fly the same way);
//        du = u- - u+ (interior), 2 (u- - g) (Dirichlet), 0 (Neumann); Fscale nx du / 2 and Fscale ny du / 2 to LDS;
//     C  node items: the two tensor derivatives, the metric, the four face lifts; qx, qy = kappa_k (...) into the two flux planes.
//   poisson2d_quad_divergence_kernel
//     A  node items: qx, qy of the tile to LDS;
//     B  face-node items: dq = nx (qx- - qx+) + ny (qy- - qy+) (interior), 0 (Dirichlet), 2 (nx qx- + ny qy- - qn) (Neumann), du
//        again from u; Fscale (dq + tau du) / 2 to LDS;
//     C  node items: derivatives, metric and lifts; A u = sigma u - [div q - Lift(...)].
//   poisson2d_quad_mass_kernel
//     w = J_k (M1 (x) M1) v_k, M1 = (V1 V1^T)^-1 the 1-D mass matrix, sum-factorised through LDS (one direction, barrier, the
//     other), stored where asked, and the tile's partial of u . w by the fixed tree of poisson_block_sum: one partial per tile.
// The KIND of a face node is a byte of a (4 Nfp, ld) plane (PoissonKind), the gather index a (4 Nfp, ld) plane of offsets
// n' ld + k' (a boundary node gathers itself), kappa_k a plane of ld values, the geometry the 16 numbers per element of
// QuadParams::ageo (rx, sx, ry, sy, then nx, ny, Fscale of each face). Parameters travel in PoissonParams; sweepBack is not read.
// LDS in doubles: ops | Np E | 2 NFN E (gradient), ops | 2 Np E | NFN E (divergence), Nq^2 | 2 Np E (mass; the tree reuses the
// first node array): at most what the diffusion passes take at the same order.
// No existing kernel header includes this one; its instances live in poisson2d_quad_order.hip.
#pragma once
#include "poisson2d_kernel.hpp"
#include "sw2d_quad_kernel.hpp"

namespace bdg_dev {

template <int N>
struct QuadPoissonElem : QuadElem<N> {
    using Q = QuadElem<N>;
    static constexpr int OFF_NODE = Q::OPS_DOUBLES;
    static constexpr int OFF_SURF_GRADIENT = OFF_NODE + Q::Np * Q::E;
    static constexpr int LDS_GRADIENT = OFF_SURF_GRADIENT + 2 * Q::NFN * Q::E; // u | Fscale nx du / 2, Fscale ny du / 2
    static constexpr int OFF_SURF_DIVERGENCE = OFF_NODE + 2 * Q::Np * Q::E;
    static constexpr int LDS_DIVERGENCE = OFF_SURF_DIVERGENCE + Q::NFN * Q::E; // qx, qy | Fscale (dq + tau du) / 2
    static constexpr int OFF_MASS = Q::Nq * Q::Nq;
    static constexpr int LDS_MASS = OFF_MASS + 2 * Q::Np * Q::E;               // M1 | v (then the tree) | the half-way sums
    static_assert(Q::Np * Q::E >= Q::THREADS, "the tree of the mass product reuses the first node array");
};

// ---- first pass
template <int N, bool DATA, bool FUSED>
__global__ __launch_bounds__(256) void poisson2d_quad_gradient_kernel(const PoissonParams p, const double* __restrict__ ops) {
    using Q = QuadPoissonElem<N>;
    constexpr int Nq = Q::Nq, Np = Q::Np, NFN = Q::NFN, E = Q::E, T = Q::THREADS;
    __shared__ double lds[Q::LDS_GRADIENT];
    double* const D1 = lds;
    double* const l0 = lds + Nq * Nq;
    double* const lN = l0 + Nq;
    double* const nv = lds + Q::OFF_NODE;
    double* const surf = lds + Q::OFF_SURF_GRADIENT;

    const int tid = threadIdx.x;
    const int k0 = p.kbegin + static_cast<int>(blockIdx.x) * E;
    const long long ld = p.ld;
    const long long plane = static_cast<long long>(Np) * ld;
    const double beta = FUSED ? p.scal[PS_BETA] : 0.0;

    for (int i = tid; i < Q::OPS_DOUBLES; i += T) lds[i] = ops[i];

    // ---- A: the input at the tile's nodes
#pragma unroll
    for (int m = 0; m < Q::NI; ++m) {
        const int idx = tid + T * m;
        if (idx < Np * E) {
            const int n = idx / E, e = idx % E, k = k0 + e;
            double u = 0.0;
            if (k < p.kend) {
                const long long o = n * ld + k;
                u = p.u[o];
                if (FUSED) {
                    u = fma(beta, p.pold[o], u);
                    p.pnew[o] = u;
                }
            }
            nv[n * E + e] = u;
        }
    }
    __syncthreads();

    // ---- B: the jump by node kind, times Fscale / 2 and the normal
#pragma unroll
    for (int m = 0; m < Q::FI; ++m) {
        const int idx = tid + T * m;
        if (idx < NFN * E) {
            const int fn = idx / E, e = idx % E, k = k0 + e;
            double sx = 0.0, sy = 0.0;
            if (k < p.kend) {
                const int f = fn / Nq, nn = fn % Nq;
                const long long fo = fn * ld + k;
                const long long oP = p.vmapP[fo];
                const unsigned kd = p.kind[fo];
                const double nx = p.ageo[(4 + f) * ld + k], ny = p.ageo[(8 + f) * ld + k], fs = p.ageo[(12 + f) * ld + k];
                const double uM = nv[Q::fmask(f, nn) * E + e];
                double uP = p.u[oP]; // (a boundary node gathers itself)
                if (FUSED) uP = fma(beta, p.pold[oP], uP);
                double gv = 0.0;
                if (DATA) gv = p.g[fo];
                const double inner = uM - uP, dir = 2.0 * (uM - gv);
                const double du = kd == PK_INTERIOR ? inner : (kd == PK_DIRICHLET ? dir : 0.0);
                const double w = 0.5 * fs * du;
                sx = w * nx;
                sy = w * ny;
            }
            surf[fn * E + e] = sx;
            surf[(NFN + fn) * E + e] = sy;
        }
    }
    __syncthreads();

    // ---- C: q = kappa_k (grad u - Lift(...))
    constexpr int kUnrollC = N <= 6 ? Q::NI : 1;
#pragma unroll kUnrollC
    for (int m = 0; m < Q::NI; ++m) {
        const int idx = tid + T * m;
        if (idx < Np * E) {
            const int n = idx / E, e = idx % E, k = k0 + e;
            if (k >= p.kend) continue;
            const int j = n / Nq, i = n % Nq;
            double sr = 0.0, ss = 0.0;
#pragma unroll
            for (int q = 0; q < Nq; ++q) {
                sr += D1[j * Nq + q] * nv[(q * Nq + i) * E + e];
                ss += D1[i * Nq + q] * nv[(j * Nq + q) * E + e];
            }
            const double rx = p.ageo[k], sx = p.ageo[ld + k], ry = p.ageo[2 * ld + k], sy = p.ageo[3 * ld + k];
            const double a0 = l0[i], a1 = lN[j], a2 = lN[i], a3 = l0[j];
            const int s0 = j * E + e, s1 = (Nq + i) * E + e, s2 = (2 * Nq + j) * E + e, s3 = (3 * Nq + i) * E + e;
            const double qx = rx * sr + sx * ss - (a0 * surf[s0] + a1 * surf[s1] + a2 * surf[s2] + a3 * surf[s3]);
            const double qy = ry * sr + sy * ss -
                              (a0 * surf[NFN * E + s0] + a1 * surf[NFN * E + s1] + a2 * surf[NFN * E + s2] + a3 * surf[NFN * E + s3]);
            const double kap = p.kap[k];
            const long long o = n * ld + k;
            p.q[o] = kap * qx;
            p.q[plane + o] = kap * qy;
        }
    }
}

// ---- second pass. u: what the first pass differentiated (FUSED launches: p.pnew).
template <int N, bool DATA>
__global__ __launch_bounds__(256) void poisson2d_quad_divergence_kernel(const PoissonParams p, const double* __restrict__ u,
                                                                        const double* __restrict__ ops) {
    using Q = QuadPoissonElem<N>;
    constexpr int Nq = Q::Nq, Np = Q::Np, NFN = Q::NFN, E = Q::E, T = Q::THREADS;
    __shared__ double lds[Q::LDS_DIVERGENCE];
    double* const D1 = lds;
    double* const l0 = lds + Nq * Nq;
    double* const lN = l0 + Nq;
    double* const fl = lds + Q::OFF_NODE;
    double* const surf = lds + Q::OFF_SURF_DIVERGENCE;

    const int tid = threadIdx.x;
    const int k0 = p.kbegin + static_cast<int>(blockIdx.x) * E;
    const long long ld = p.ld;
    const long long plane = static_cast<long long>(Np) * ld;
    const double* __restrict__ qxp = p.q;
    const double* __restrict__ qyp = p.q + plane;

    for (int i = tid; i < Q::OPS_DOUBLES; i += T) lds[i] = ops[i];

    // ---- A: the fluxes at the tile's nodes
#pragma unroll
    for (int m = 0; m < Q::NI; ++m) {
        const int idx = tid + T * m;
        if (idx < Np * E) {
            const int n = idx / E, e = idx % E, k = k0 + e;
            double fx = 0.0, fy = 0.0;
            if (k < p.kend) {
                const long long o = n * ld + k;
                fx = qxp[o];
                fy = qyp[o];
            }
            fl[n * E + e] = fx;
            fl[(Np + n) * E + e] = fy;
        }
    }
    __syncthreads();

    // ---- B: Fscale (dq + tau du) / 2 by node kind
#pragma unroll
    for (int m = 0; m < Q::FI; ++m) {
        const int idx = tid + T * m;
        if (idx < NFN * E) {
            const int fn = idx / E, e = idx % E, k = k0 + e;
            double s = 0.0;
            if (k < p.kend) {
                const int f = fn / Nq, nn = fn % Nq;
                const int nM = Q::fmask(f, nn);
                const long long fo = fn * ld + k;
                const long long oP = p.vmapP[fo];
                const unsigned kd = p.kind[fo];
                const double nx = p.ageo[(4 + f) * ld + k], ny = p.ageo[(8 + f) * ld + k], fs = p.ageo[(12 + f) * ld + k];
                const double uM = u[nM * ld + k], uP = u[oP];
                const double fxM = fl[nM * E + e], fyM = fl[(Np + nM) * E + e];
                const double fxP = qxp[oP], fyP = qyp[oP]; // (a boundary node gathers itself)
                double gv = 0.0, qnv = 0.0;
                if (DATA) {
                    gv = p.g[fo];
                    qnv = p.qn[fo];
                }
                const double duI = uM - uP, duD = 2.0 * (uM - gv);
                const double du = kd == PK_INTERIOR ? duI : (kd == PK_DIRICHLET ? duD : 0.0);
                const double dqI = nx * (fxM - fxP) + ny * (fyM - fyP);
                const double dqN = 2.0 * ((nx * fxM + ny * fyM) - qnv);
                const double dq = kd == PK_INTERIOR ? dqI : (kd == PK_DIRICHLET ? 0.0 : dqN);
                s = 0.5 * fs * fma(p.tau, du, dq);
            }
            surf[fn * E + e] = s;
        }
    }
    __syncthreads();

    // ---- C: A u = sigma u - (div q - Lift(...))
    constexpr int kUnrollC = N <= 6 ? Q::NI : 1;
#pragma unroll kUnrollC
    for (int m = 0; m < Q::NI; ++m) {
        const int idx = tid + T * m;
        if (idx < Np * E) {
            const int n = idx / E, e = idx % E, k = k0 + e;
            if (k >= p.kend) continue;
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
            const double rx = p.ageo[k], sx = p.ageo[ld + k], ry = p.ageo[2 * ld + k], sy = p.ageo[3 * ld + k];
            const double a0 = l0[i], a1 = lN[j], a2 = lN[i], a3 = l0[j];
            const int s0 = j * E + e, s1 = (Nq + i) * E + e, s2 = (2 * Nq + j) * E + e, s3 = (3 * Nq + i) * E + e;
            const double div = rx * xr + sx * xs + ry * yr + sy * ys - (a0 * surf[s0] + a1 * surf[s1] + a2 * surf[s2] + a3 * surf[s3]);
            const long long o = n * ld + k;
            p.out[o] = fma(p.sigma, u[o], -div); // own u again: an L2 hit
        }
    }
}

// ---- mass product and mass inner product. mass1: (Nq, Nq) row-major 1-D mass matrix; jac: (ld) J_k. w (may be nullptr): J M v.
// partial[tile] = sum over the tile's elements of u_k . (J_k M v_k); items past kend add zero.
template <int N>
__global__ __launch_bounds__(256) void poisson2d_quad_mass_kernel(const double* __restrict__ u, const double* __restrict__ v,
                                                                  double* __restrict__ w, const double* __restrict__ mass1,
                                                                  const double* __restrict__ jac, double* __restrict__ partial,
                                                                  long long ld, int kbegin, int kend) {
    using Q = QuadPoissonElem<N>;
    constexpr int Nq = Q::Nq, Np = Q::Np, E = Q::E, T = Q::THREADS;
    __shared__ double lds[Q::LDS_MASS];
    double* const M1 = lds;
    double* const vv = lds + Q::OFF_MASS;
    double* const hw = vv + Np * E;

    const int tid = threadIdx.x;
    const int k0 = kbegin + static_cast<int>(blockIdx.x) * E;

    for (int i = tid; i < Nq * Nq; i += T) M1[i] = mass1[i];

    // ---- A: v at the tile's nodes
#pragma unroll
    for (int m = 0; m < Q::NI; ++m) {
        const int idx = tid + T * m;
        if (idx < Np * E) {
            const int n = idx / E, e = idx % E, k = k0 + e;
            vv[n * E + e] = k < kend ? v[n * ld + k] : 0.0;
        }
    }
    __syncthreads();

    // ---- B: along the second index
    constexpr int kUnroll = N <= 6 ? Q::NI : 1;
#pragma unroll kUnroll
    for (int m = 0; m < Q::NI; ++m) {
        const int idx = tid + T * m;
        if (idx < Np * E) {
            const int n = idx / E, e = idx % E;
            const int j = n / Nq, i = n % Nq;
            double a = 0.0;
#pragma unroll
            for (int q = 0; q < Nq; ++q) a = fma(M1[i * Nq + q], vv[(j * Nq + q) * E + e], a);
            hw[n * E + e] = a;
        }
    }
    __syncthreads();

    // ---- C: along the first index, J_k, the product with u
    double dot = 0.0;
#pragma unroll kUnroll
    for (int m = 0; m < Q::NI; ++m) {
        const int idx = tid + T * m;
        if (idx < Np * E) {
            const int n = idx / E, e = idx % E, k = k0 + e;
            if (k >= kend) continue;
            const int j = n / Nq, i = n % Nq;
            double a = 0.0;
#pragma unroll
            for (int q = 0; q < Nq; ++q) a = fma(M1[j * Nq + q], hw[(q * Nq + i) * E + e], a);
            a *= jac[k];
            const long long o = n * ld + k;
            if (w) w[o] = a;
            dot = fma(u[o], a, dot);
        }
    }
    // (vv is dead since the barrier behind B: the tree takes its first 256 doubles)
    const double total = poisson_block_sum<T>(dot, vv);
    if (tid == 0) partial[blockIdx.x] = total;
}

} // namespace bdg_dev
