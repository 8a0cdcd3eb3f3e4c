// poisson2d_kernel.hpp -- the elliptic operator A u = sigma u - div(kappa grad u) on straight-sided triangles and the pieces of a
// device-resident conjugate-gradient loop in the mass inner product (the definition is restated in
// tests/poisson_ref.py). Hesthaven and Warburton's stabilised central flux form: the tracer's two diffusion passes
// (sw2d_diffusion_kernel.hpp) plus boundary kinds and a penalty, in two passes over the mesh with a launch boundary between them
// (the second reads the neighbours' output of the first):
//   poisson2d_gradient_kernel    du = u- - u+ (interior), 2 (u- - g) (Dirichlet), 0 (Neumann) at the face nodes;
//                                qx = kappa_k (rx Dr u + sx Ds u - Lift(Fscale nx du / 2)), qy likewise, into two scratch planes
//   poisson2d_divergence_kernel  dq = nx (qx- - qx+) + ny (qy- - qy+) (interior), 0 (Dirichlet), 2 (nx qx- + ny qy- - qn) (Neumann);
//                                A u = sigma u - [rx Dr qx + sx Ds qx + ry Dr qy + sy Ds qy - Lift(Fscale (dq + tau du) / 2)]
// The KIND of a face node is a byte of a (3 Nfp, ld) plane built at set-up (0 interior, 1 Dirichlet, 2 Neumann): no list is
// searched here. Both passes have the form of the tracer's: one wave of 64 elements, one lane per element, the Np nodal values
// and the 3 Nfp scaled jumps in registers, output rows one at a time from the wave-uniform VnOps image, face values through the
// gather index, selects and no branches at boundary nodes, the 13 numbers per element of p.ageo for geometry. DATA: the planes
// g and qn, each (3 Nfp, ld), are read (both must be set: the host passes planes of zeros for the one that is not given).
// FUSED (the conjugate-gradient loop): the input of the first pass is the new search direction p = r + beta p_old, formed on the
// fly at the element's own nodes and at the gathered neighbour nodes (beta from device memory) and stored to a SECOND direction
// plane -- the neighbours still read p_old --, so the direction update costs no launch of its own.
//   poisson2d_mass_kernel        w = J_k (V V^T)^-1 v_k (stored where asked) and the partial sums of u . w per workgroup: the mass
//                                product and the mass inner product
// and the flat vector kernels of the loop (poisson2d_cg_update_kernel, poisson2d_axpy_kernel, poisson2d_weighted_sum_kernel,
// poisson2d_shift_kernel) with poisson2d_finish_kernel, the one block that adds the partial sums in a fixed order and writes alpha,
// beta and the residual norm to device memory. Nothing here uses a floating-point atomic: a sum is bit for bit the same from
// run to run.
#pragma once
#include "sw2d_vn_kernel.hpp"

namespace bdg_dev {

// device scalars of the loop (doubles)
enum PoissonScalar {
    PS_RR = 0,     // <r, r> of the current residual
    PS_RR_PREV,    // ... of the one before
    PS_PAP,        // <p, A p>
    PS_ALPHA,
    PS_BETA,
    PS_SUM,        // the last plain sum (mass_dot, weighted sums)
    PS_MEAN,       // the last mean (weighted sum / area)
    PS_COUNT
};

enum PoissonKind : unsigned char { PK_INTERIOR = 0, PK_DIRICHLET = 1, PK_NEUMANN = 2 };

struct PoissonParams {
    const double* u;            // (Np, ld) input; FUSED: the residual r
    const double* pold;         // FUSED: previous direction
    double* pnew;               // FUSED: new direction (the second pass reads it as u)
    const double* scal;         // PoissonScalar
    double* q;                  // 2 planes of Np*ld: qx, qy
    double* out;                // (Np, ld) A u
    const double* ageo;         // 13 planes of ld: rx, sx, ry, sy, nx[3], ny[3], Fscale[3]
    const int* vmapP;           // (3 Nfp, ld) gather offsets n' ld + k'
    const unsigned char* kind;  // (3 Nfp, ld) PoissonKind
    const double* kap;          // (ld) kappa_k
    const double* g;            // DATA: (3 Nfp, ld)
    const double* qn;           // DATA: (3 Nfp, ld)
    double sigma, tau;
    long long ld;
    int kbegin, kend;
    int sweepBack;
};

// ---- first pass. ops: plain VnOps image.
template <int N, bool DATA, bool FUSED>
__global__ __launch_bounds__(64) void poisson2d_gradient_kernel(const PoissonParams p, const double* __restrict__ ops) {
    using E = Elem<N>;
    constexpr int Np = E::Np, Nfp = E::Nfp, NFN = E::NFN;
    const unsigned tile = stage_tile(blockIdx.x, gridDim.x, static_cast<unsigned>(p.sweepBack));
    const unsigned k = static_cast<unsigned>(p.kbegin) + tile * 64u + threadIdx.x;
    if (k >= static_cast<unsigned>(p.kend)) return;
    const unsigned k8 = k * 8u, k4 = k * 4u;
    const long long ld = p.ld, plane = static_cast<long long>(Np) * ld;
    const double* __restrict__ uin = p.u;
    const double* __restrict__ pold = FUSED ? p.pold : p.u;
    const double beta = FUSED ? p.scal[PS_BETA] : 0.0;

    // ---- the input at the nodes
    double U[Np];
#pragma unroll
    for (int m = 0; m < Np; ++m) {
        U[m] = ld_row(uin + m * ld, k8);
        if constexpr (FUSED) {
            U[m] = fma(beta, ld_row(pold + m * ld, k8), U[m]);
            st_row(p.pnew + m * ld, k8, U[m]);
        }
        if (m % 6 == 5) __builtin_amdgcn_sched_barrier(0); // a few nodes' loads in flight at a time, as in the tracer's passes
    }
    __builtin_amdgcn_sched_barrier(0);

    // ---- scaled jumps at the face nodes: Fscale du / 2
    double s[NFN];
    double fnx[3], fny[3];
#pragma unroll
    for (int f = 0; f < 3; ++f) {
        fnx[f] = ld_row(p.ageo + (4 + f) * ld, k8);
        fny[f] = ld_row(p.ageo + (7 + f) * ld, k8);
        const double fs = ld_row(p.ageo + (10 + f) * ld, k8);
#pragma unroll
        for (int n = 0; n < Nfp; ++n) {
            const int j = f * Nfp + n, m = E::fmask(f, n);
            const unsigned o8 = static_cast<unsigned>(ld_row(p.vmapP + j * ld, k4)) * 8u;
            const unsigned kd = ld_row(p.kind + j * ld, k);
            double uP = ld_row(uin, o8);
            if constexpr (FUSED) uP = fma(beta, ld_row(pold, o8), uP);
            double gv = 0.0;
            if constexpr (DATA) gv = ld_row(p.g + j * ld, k8);
            const double inner = U[m] - uP, dir = 2.0 * (U[m] - gv);
            const double du = kd == PK_INTERIOR ? inner : (kd == PK_DIRICHLET ? dir : 0.0);
            s[j] = 0.5 * fs * du;
            __builtin_amdgcn_sched_barrier(0); // one face node at a time
        }
    }

    // ---- output rows, one node at a time
    const double rx = ld_row(p.ageo, k8), sx = ld_row(p.ageo + ld, k8), ry = ld_row(p.ageo + 2 * ld, k8),
                 sy = ld_row(p.ageo + 3 * ld, k8);
    const double kap = ld_row(p.kap, k8);
#pragma unroll 1
    for (int i = 0; i < Np; ++i) {
        const double* __restrict__ row = ops + static_cast<size_t>(i) * VnOps<N>::ROW;
        const long long io = static_cast<long long>(i) * ld;
        double a = 0.0, b = 0.0;
#pragma unroll
        for (int m = 0; m < Np; ++m) {
            a = fma(row[2 * m], U[m], a);
            b = fma(row[2 * m + 1], U[m], b);
        }
        double lx = 0.0, ly = 0.0;
#pragma unroll
        for (int f = 0; f < 3; ++f) {
            double l = 0.0;
#pragma unroll
            for (int n = 0; n < Nfp; ++n) l = fma(row[2 * Np + f * Nfp + n], s[f * Nfp + n], l);
            lx = fma(fnx[f], l, lx);
            ly = fma(fny[f], l, ly);
        }
        st_row(p.q + io, k8, kap * ((rx * a + sx * b) - lx));
        st_row(p.q + plane + io, k8, kap * ((ry * a + sy * b) - ly));
    }
}

// ---- second pass. ops: plain VnOps image. u: what the first pass differentiated (FUSED launches: p.pnew).
template <int N, bool DATA>
__global__ __launch_bounds__(64) void poisson2d_divergence_kernel(const PoissonParams p, const double* __restrict__ u,
                                                                  const double* __restrict__ ops) {
    using E = Elem<N>;
    constexpr int Np = E::Np, Nfp = E::Nfp, NFN = E::NFN;
    const unsigned tile = stage_tile(blockIdx.x, gridDim.x, static_cast<unsigned>(p.sweepBack));
    const unsigned k = static_cast<unsigned>(p.kbegin) + tile * 64u + threadIdx.x;
    if (k >= static_cast<unsigned>(p.kend)) return;
    const unsigned k8 = k * 8u, k4 = k * 4u;
    const long long ld = p.ld, plane = static_cast<long long>(Np) * ld;
    const double* __restrict__ qxp = p.q;
    const double* __restrict__ qyp = p.q + plane;

    // ---- the fluxes at the nodes
    double F[Np], G[Np];
#pragma unroll
    for (int m = 0; m < Np; ++m) {
        F[m] = ld_row(qxp + m * ld, k8);
        G[m] = ld_row(qyp + m * ld, k8);
        if (m % 6 == 5) __builtin_amdgcn_sched_barrier(0);
    }
    __builtin_amdgcn_sched_barrier(0);

    // ---- scaled jumps at the face nodes: Fscale (dq + tau du) / 2
    double s[NFN];
#pragma unroll
    for (int f = 0; f < 3; ++f) {
        const double nxf = ld_row(p.ageo + (4 + f) * ld, k8), nyf = ld_row(p.ageo + (7 + f) * ld, k8),
                     fs = ld_row(p.ageo + (10 + f) * ld, k8);
#pragma unroll
        for (int n = 0; n < Nfp; ++n) {
            const int j = f * Nfp + n, m = E::fmask(f, n);
            const unsigned o8 = static_cast<unsigned>(ld_row(p.vmapP + j * ld, k4)) * 8u;
            const unsigned kd = ld_row(p.kind + j * ld, k);
            const double uM = ld_row(u + m * ld, k8), uP = ld_row(u, o8);
            const double qxP = ld_row(qxp, o8), qyP = ld_row(qyp, o8);
            double gv = 0.0, qnv = 0.0;
            if constexpr (DATA) {
                gv = ld_row(p.g + j * ld, k8);
                qnv = ld_row(p.qn + j * ld, k8);
            }
            const double duI = uM - uP, duD = 2.0 * (uM - gv);
            const double du = kd == PK_INTERIOR ? duI : (kd == PK_DIRICHLET ? duD : 0.0);
            const double dqI = nxf * (F[m] - qxP) + nyf * (G[m] - qyP);
            const double dqN = 2.0 * ((nxf * F[m] + nyf * G[m]) - qnv);
            const double dq = kd == PK_INTERIOR ? dqI : (kd == PK_DIRICHLET ? 0.0 : dqN);
            s[j] = 0.5 * fs * fma(p.tau, du, dq);
            __builtin_amdgcn_sched_barrier(0); // one face node at a time
        }
    }

    // ---- output rows, one node at a time
    const double rx = ld_row(p.ageo, k8), sx = ld_row(p.ageo + ld, k8), ry = ld_row(p.ageo + 2 * ld, k8),
                 sy = ld_row(p.ageo + 3 * ld, k8);
#pragma unroll 1
    for (int i = 0; i < Np; ++i) {
        const double* __restrict__ row = ops + static_cast<size_t>(i) * VnOps<N>::ROW;
        const long long io = static_cast<long long>(i) * ld;
        double a = 0.0, b = 0.0, cG = 0.0, d = 0.0;
#pragma unroll
        for (int m = 0; m < Np; ++m) {
            a = fma(row[2 * m], F[m], a);
            b = fma(row[2 * m + 1], F[m], b);
            cG = fma(row[2 * m], G[m], cG);
            d = fma(row[2 * m + 1], G[m], d);
        }
        double lift = 0.0;
#pragma unroll
        for (int j = 0; j < NFN; ++j) lift = fma(row[2 * Np + j], s[j], lift);
        const double div = ((rx * a + sx * b) + (ry * cG + sy * d)) - lift;
        st_row(p.out + io, k8, fma(p.sigma, ld_row(u + io, k8), -div));
    }
}

// The sum of one value per lane over a wave, by a fixed tree of cross-lane moves: the same bits whatever else runs.
__device__ __forceinline__ double poisson_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// ---- mass product and mass inner product. mass: (Np, Np) row-major (V V^T)^-1; jac: (ld) J_k. w (may be nullptr): J M v.
// partial[tile] = sum over the tile's elements of u_k . (J_k M v_k); lanes past kend add zero.
template <int N>
__global__ __launch_bounds__(64) void poisson2d_mass_kernel(const double* __restrict__ u, const double* __restrict__ v,
                                                            double* __restrict__ w, const double* __restrict__ mass,
                                                            const double* __restrict__ jac, double* __restrict__ partial,
                                                            long long ld, int kbegin, int kend) {
    constexpr int Np = Elem<N>::Np;
    const unsigned k = static_cast<unsigned>(kbegin) + blockIdx.x * 64u + threadIdx.x;
    double dot = 0.0;
    if (k < static_cast<unsigned>(kend)) {
        const unsigned k8 = k * 8u;
        double V[Np];
#pragma unroll
        for (int m = 0; m < Np; ++m) V[m] = ld_row(v + m * ld, k8);
        const double J = ld_row(jac, k8);
#pragma unroll 1
        for (int i = 0; i < Np; ++i) {
            const double* __restrict__ row = mass + static_cast<size_t>(i) * Np;
            double r = 0.0;
#pragma unroll
            for (int m = 0; m < Np; ++m) r = fma(row[m], V[m], r);
            r *= J;
            if (w) st_row(w + static_cast<long long>(i) * ld, k8, r);
            dot = fma(ld_row(u + static_cast<long long>(i) * ld, k8), r, dot);
        }
    }
    dot = poisson_wave_sum(dot);
    if (threadIdx.x == 0) partial[blockIdx.x] = dot;
}

// The sum of one value per thread over a block of BLOCK threads (a power of two), in a fixed order; the result in thread 0.
template <int BLOCK>
__device__ __forceinline__ double poisson_block_sum(double v, double* sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int st = BLOCK / 2; st > 0; st >>= 1) {
        if (static_cast<int>(threadIdx.x) < st) sh[threadIdx.x] += sh[threadIdx.x + st];
        __syncthreads();
    }
    return sh[0];
}

// ---- x += alpha p, r -= alpha Ap, s -= alpha w over n = Np ld entries (padding lanes hold zeros and keep them), and the partial
// sums of r . s (s = J M r, so that their sum is <r, r>). alpha from device memory.
template <int BLOCK, int ITEMS>
__global__ __launch_bounds__(BLOCK) void poisson2d_cg_update_kernel(double* __restrict__ x, double* __restrict__ r,
                                                                    double* __restrict__ s, const double* __restrict__ pdir,
                                                                    const double* __restrict__ Ap, const double* __restrict__ w,
                                                                    const double* __restrict__ scal, double* __restrict__ partial,
                                                                    long long n) {
    __shared__ double sh[BLOCK];
    const double alpha = scal[PS_ALPHA];
    double acc = 0.0;
    const long long base = static_cast<long long>(blockIdx.x) * BLOCK * ITEMS + threadIdx.x;
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        const long long i = base + static_cast<long long>(it) * BLOCK;
        if (i < n) {
            x[i] = fma(alpha, pdir[i], x[i]);
            const double rn = fma(-alpha, Ap[i], r[i]), sn = fma(-alpha, w[i], s[i]);
            r[i] = rn;
            s[i] = sn;
            acc = fma(rn, sn, acc);
        }
    }
    const double total = poisson_block_sum<BLOCK>(acc, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

// ---- y += a x over n entries (a from the host).
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void poisson2d_axpy_kernel(double* __restrict__ y, double a, const double* __restrict__ x, long long n) {
    const long long i = static_cast<long long>(blockIdx.x) * BLOCK + threadIdx.x;
    if (i < n) y[i] = fma(a, x[i], y[i]);
}

// ---- partial sums of wts . u over n entries (wts = J M 1, zero in the padding: their sum with u is the integral of u).
template <int BLOCK, int ITEMS>
__global__ __launch_bounds__(BLOCK) void poisson2d_weighted_sum_kernel(const double* __restrict__ wts, const double* __restrict__ u,
                                                                       double* __restrict__ partial, long long n) {
    __shared__ double sh[BLOCK];
    double acc = 0.0;
    const long long base = static_cast<long long>(blockIdx.x) * BLOCK * ITEMS + threadIdx.x;
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        const long long i = base + static_cast<long long>(it) * BLOCK;
        if (i < n) acc = fma(wts[i], u[i], acc);
    }
    const double total = poisson_block_sum<BLOCK>(acc, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

// ---- u -= mean at the nodes of real elements (columns k < K of the (Np, ld) plane: the padding keeps its zeros), and, where s is
// given, s -= mean wts (wts = J M 1, so that s = J M u stays what it is). mean = scal[PS_MEAN].
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void poisson2d_shift_kernel(double* __restrict__ u, double* __restrict__ s,
                                                                const double* __restrict__ wts, const double* __restrict__ scal,
                                                                long long n, long long ld, int K) {
    const long long i = static_cast<long long>(blockIdx.x) * BLOCK + threadIdx.x;
    if (i >= n) return;
    const double mean = scal[PS_MEAN];
    if (i % ld < K) u[i] -= mean;
    if (s) s[i] = fma(-mean, wts[i], s[i]);
}

// What the one finishing block does with the sum of the partials.
enum PoissonFinish {
    PF_SUM = 0,    // scal[PS_SUM] = sum
    PF_MEAN,       // scal[PS_SUM] = sum, scal[PS_MEAN] = sum / area
    PF_ALPHA,      // scal[PS_PAP] = sum, scal[PS_ALPHA] = rr / sum (0 when the sum is 0)
    PF_BETA,       // rr_prev = rr, rr = sum, beta = rr / rr_prev (0 when rr_prev is 0)
    PF_REBETA,     // rr = sum, beta = rr / rr_prev: after the residual's mean was removed at a convergence check
    PF_START       // rr = rr_prev = sum, beta = 0: the first residual
};

// ---- one block: the partials in a fixed order (thread t takes t, t + BLOCK, ...; then the tree), then the scalars, written by
// thread 0 with ordinary stores.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void poisson2d_finish_kernel(const double* __restrict__ partial, int count, int what,
                                                                 double area, double* __restrict__ scal) {
    __shared__ double sh[BLOCK];
    double acc = 0.0;
    for (int i = threadIdx.x; i < count; i += BLOCK) acc += partial[i];
    const double sum = poisson_block_sum<BLOCK>(acc, sh);
    if (threadIdx.x != 0) return;
    if (what == PF_SUM) {
        scal[PS_SUM] = sum;
    } else if (what == PF_MEAN) {
        scal[PS_SUM] = sum;
        scal[PS_MEAN] = sum / area;
    } else if (what == PF_ALPHA) {
        scal[PS_PAP] = sum;
        scal[PS_ALPHA] = sum != 0.0 ? scal[PS_RR] / sum : 0.0;
    } else if (what == PF_BETA) {
        const double prev = scal[PS_RR];
        scal[PS_RR_PREV] = prev;
        scal[PS_RR] = sum;
        scal[PS_BETA] = prev != 0.0 ? sum / prev : 0.0;
    } else if (what == PF_REBETA) {
        const double prev = scal[PS_RR_PREV];
        scal[PS_RR] = sum;
        scal[PS_BETA] = prev != 0.0 ? sum / prev : 0.0;
    } else {
        scal[PS_RR] = sum;
        scal[PS_RR_PREV] = sum;
        scal[PS_BETA] = 0.0;
    }
}

} // namespace bdg_dev
