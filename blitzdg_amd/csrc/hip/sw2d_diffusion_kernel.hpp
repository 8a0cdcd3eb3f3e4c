// sw2d_diffusion_kernel.hpp -- diffusion, sources and decay of the passive tracer hN (field 3 of a four-field triangle state):
//   d(hN)/dt = (advection) + div(kappa h grad N) + S - k hN,   N = hN / h,
// the first second-order operator of the code base (the definition is restated in tests/tridiff_ref.py). Local
// DG with central fluxes and no penalty, in two passes over the mesh with a launch boundary between them (the second reads the
// neighbours' output of the first):
//   sw2d_tracer_gradient_kernel    dN = N- - N+ at face nodes, 0 at boundary nodes;
//                                  qx = rx Dr N + sx Ds N - Lift(Fscale nx dN / 2), qy likewise with ry, sy, ny;
//                                  fx = kappa h qx, fy = kappa h qy into two scratch planes (kappa a scalar or a plane)
//   sw2d_tracer_diffusion_kernel   dF = nx (fx- - fx+) + ny (fy- - fy+), 2 (nx fx- + ny fy-) at boundary nodes (zero normal flux);
//                                  T = rx Dr fx + sx Ds fx + ry Dr fy + sy Ds fy - Lift(Fscale dF / 2) + S - k hN
// A BOUNDARY node is a face node whose gather index points at itself (no neighbour: walls and the open boundary alike; the tracer
// crosses the open boundary by advection only), so the passes need neither the wall flag nor variant B's open-boundary tables.
// T enters the stage whose launches were just issued on the same stream, ADDED to what they wrote to plane 3 -- they read qin
// and write rhs / res / qout, which are other buffers, so qin is still the state of this evaluation:
//   MODE_RHS      rhs4 += T
//   MODE_LSERK    res4 += cc T,  qout4 += cb cc T     (res = ca res + cc R, qout = qin + cb res are linear in R)
//   MODE_COMBINE  qout4 += cc T                       (the tracer is never sponged)
// Planes 0-2 are never touched. Both kernels have the rolled form of sw2d_stage_vb_tracer_kernel: one wave of 64 elements, one
// lane per element, the Np nodal values and the 3 Nfp scaled jumps in registers, output rows one at a time from wave-uniform
// operator rows (VnOps image), face values through the gather index, selects and no branches at boundary nodes. NODAL: metric
// per output node and normals / scales per face node (p.geo, p.fgeo), else the 13 numbers per element of p.ageo. A filtered
// evaluation: on straight-sided elements with T linear in the fluxes (no S, k = 0) the rows of the second pass are pre-filtered;
// otherwise (per-node geometry, where the metric multiplies after the differentiation, or a pointwise part, which no operator
// row carries) the second pass leaves the whole unfiltered T in a scratch plane and sw2d_tracer_diffusion_filter_kernel applies
// Filter rows to all of it, then the update.
#pragma once
#include "sw2d_vn_kernel.hpp"

namespace bdg_dev {

struct DiffusionParams {
    const double* kappaField; // (Np, ld) or nullptr: kappa at every node
    double kappa;
    const double* source;     // (Np, ld) S or nullptr
    double decay;             // k
    double* flux;             // 2 planes of Np*ld: fx, fy
    double* raw;              // 1 plane of Np*ld (filtered evaluations in two steps) or nullptr
};

// ---- first pass. ops: plain VnOps image.
template <int N, bool NODAL>
__global__ __launch_bounds__(64) void sw2d_tracer_gradient_kernel(const StageParams p, const DiffusionParams dp,
                                                                  const double* __restrict__ ops) {
    using E = Elem<N>;
    constexpr int Np = E::Np, Nfp = E::Nfp, NFN = E::NFN;
    const unsigned tile = stage_tile(blockIdx.x, gridDim.x, static_cast<unsigned>(p.sweepBack));
    const unsigned k = static_cast<unsigned>(p.kbegin) + tile * 64u + threadIdx.x;
    if (k >= static_cast<unsigned>(p.kend)) return;
    const unsigned k8 = k * 8u, k4 = k * 4u;
    const long long ld = p.ld, plane = static_cast<long long>(Np) * ld, fplane = static_cast<long long>(NFN) * ld;
    const double* __restrict__ qin = p.qin;
    const double* __restrict__ qN = qin + 3 * plane;

    // ---- concentrations at the nodes
    double C[Np];
#pragma unroll
    for (int m = 0; m < Np; ++m) {
        C[m] = ld_row(qN + m * ld, k8) * fast_rcp(ld_row(qin + m * ld, k8));
        if (m % 6 == 5) __builtin_amdgcn_sched_barrier(0); // a few nodes' loads in flight at a time, as in sw2d_stage_vb_tracer_kernel
    }
    __builtin_amdgcn_sched_barrier(0);

    // ---- scaled jumps at the face nodes: Fscale dN / 2, times the normal per face node where it differs from node to node
    double sx[NFN], sy[NODAL ? NFN : 1];
    double fnx[3], fny[3];
#pragma unroll
    for (int f = 0; f < 3; ++f) {
        double fsa = 0.0;
        fnx[f] = fny[f] = 0.0;
        if constexpr (!NODAL) {
            fnx[f] = ld_row(p.ageo + (4 + f) * ld, k8);
            fny[f] = ld_row(p.ageo + (7 + f) * ld, k8);
            fsa = ld_row(p.ageo + (10 + f) * ld, k8);
        }
#pragma unroll
        for (int n = 0; n < Nfp; ++n) {
            const int j = f * Nfp + n, m = E::fmask(f, n);
            const int id = ld_row(p.vmapP + j * ld, k4);
            const unsigned o8 = static_cast<unsigned>(id < 0 ? -(id + 1) : id) * 8u;
            const bool bnd = o8 == static_cast<unsigned>(m * ld) * 8u + k8;
            const double CP = ld_row(qN, o8) * fast_rcp(ld_row(qin, o8));
            const double fs = NODAL ? ld_row(p.fgeo + 2 * fplane + j * ld, k8) : fsa;
            const double half = 0.5 * fs * (bnd ? 0.0 : C[m] - CP);
            if constexpr (NODAL) {
                sx[j] = half * ld_row(p.fgeo + j * ld, k8);
                sy[j] = half * ld_row(p.fgeo + fplane + j * ld, k8);
            } else {
                sx[j] = half;
            }
            __builtin_amdgcn_sched_barrier(0); // one face node at a time
        }
    }

    // ---- output rows, one node at a time
    double rxa = 0.0, sxa = 0.0, rya = 0.0, sya = 0.0;
    if constexpr (!NODAL) {
        rxa = ld_row(p.ageo, k8);
        sxa = ld_row(p.ageo + ld, k8);
        rya = ld_row(p.ageo + 2 * ld, k8);
        sya = ld_row(p.ageo + 3 * ld, k8);
    }
    const bool field = dp.kappaField != nullptr;
    const double* __restrict__ kap = field ? dp.kappaField : qin; // (a valid row either way: the select is on the value)
#pragma unroll 1
    for (int i = 0; i < Np; ++i) {
        const double* __restrict__ row = ops + static_cast<size_t>(i) * VnOps<N>::ROW;
        const long long io = static_cast<long long>(i) * ld;
        const double rx = NODAL ? ld_row(p.geo + io, k8) : rxa, sxm = NODAL ? ld_row(p.geo + plane + io, k8) : sxa,
                     ry = NODAL ? ld_row(p.geo + 2 * plane + io, k8) : rya, sym = NODAL ? ld_row(p.geo + 3 * plane + io, k8) : sya;
        double a = 0.0, b = 0.0;
#pragma unroll
        for (int m = 0; m < Np; ++m) {
            a = fma(row[2 * m], C[m], a);
            b = fma(row[2 * m + 1], C[m], b);
        }
        double lx = 0.0, ly = 0.0;
        if constexpr (NODAL) {
#pragma unroll
            for (int j = 0; j < NFN; ++j) {
                lx = fma(row[2 * Np + j], sx[j], lx);
                ly = fma(row[2 * Np + j], sy[j], ly);
            }
        } else {
#pragma unroll
            for (int f = 0; f < 3; ++f) {
                double l = 0.0;
#pragma unroll
                for (int n = 0; n < Nfp; ++n) l = fma(row[2 * Np + f * Nfp + n], sx[f * Nfp + n], l);
                lx = fma(fnx[f], l, lx);
                ly = fma(fny[f], l, ly);
            }
        }
        const double kv = ld_row(kap + io, k8);
        const double kh = (field ? kv : dp.kappa) * ld_row(qin + io, k8);
        st_row(dp.flux + io, k8, kh * ((rx * a + sxm * b) - lx));
        st_row(dp.flux + plane + io, k8, kh * ((ry * a + sym * b) - ly));
    }
}

// The update of plane 3 by one row r of T (or of Filter T) at node offset io: added to what the stage's own launches wrote.
template <int MODE>
__device__ __forceinline__ void diffusion_add_row(const StageParams& p, long long fo, long long io, unsigned k8, double r) {
    if constexpr (MODE == MODE_RHS) {
        st_row(p.rhs + fo + io, k8, ld_row(p.rhs + fo + io, k8) + r);
    } else if constexpr (MODE == MODE_LSERK) {
        const double d = p.cc * r;
        st_row(p.res + fo + io, k8, ld_row(p.res + fo + io, k8) + d);
        st_row(p.qout + fo + io, k8, fma(p.cb, d, ld_row(p.qout + fo + io, k8)));
    } else {
        st_row(p.qout + fo + io, k8, fma(p.cc, r, ld_row(p.qout + fo + io, k8)));
    }
}

// ---- second pass. ops: VnOps image, plain -- or, NODAL = false and no pointwise part, pre-multiplied by the Filter. RAW: the
// unfiltered T goes to dp.raw whatever MODE says (sw2d_tracer_diffusion_filter_kernel does the update).
template <int N, int MODE, bool NODAL, bool RAW = false>
__global__ __launch_bounds__(64) void sw2d_tracer_diffusion_kernel(const StageParams p, const DiffusionParams dp,
                                                                   const double* __restrict__ ops) {
    using E = Elem<N>;
    constexpr int Np = E::Np, Nfp = E::Nfp, NFN = E::NFN;
    const unsigned tile = stage_tile(blockIdx.x, gridDim.x, static_cast<unsigned>(p.sweepBack));
    const unsigned k = static_cast<unsigned>(p.kbegin) + tile * 64u + threadIdx.x;
    if (k >= static_cast<unsigned>(p.kend)) return;
    const unsigned k8 = k * 8u, k4 = k * 4u;
    const long long ld = p.ld, plane = static_cast<long long>(Np) * ld, fplane = static_cast<long long>(NFN) * ld;
    const double* __restrict__ fxp = dp.flux;
    const double* __restrict__ fyp = dp.flux + plane;

    // ---- the fluxes at the nodes
    double F[Np], G[Np];
#pragma unroll
    for (int m = 0; m < Np; ++m) {
        F[m] = ld_row(fxp + m * ld, k8);
        G[m] = ld_row(fyp + m * ld, k8);
        if (m % 6 == 5) __builtin_amdgcn_sched_barrier(0);
    }
    __builtin_amdgcn_sched_barrier(0);

    // ---- scaled normal-flux jumps at the face nodes
    double s[NFN];
#pragma unroll
    for (int f = 0; f < 3; ++f) {
        double nxa = 0.0, nya = 0.0, fsa = 0.0;
        if constexpr (!NODAL) {
            nxa = ld_row(p.ageo + (4 + f) * ld, k8);
            nya = ld_row(p.ageo + (7 + f) * ld, k8);
            fsa = ld_row(p.ageo + (10 + f) * ld, k8);
        }
#pragma unroll
        for (int n = 0; n < Nfp; ++n) {
            const int j = f * Nfp + n, m = E::fmask(f, n);
            const int id = ld_row(p.vmapP + j * ld, k4);
            const unsigned o8 = static_cast<unsigned>(id < 0 ? -(id + 1) : id) * 8u;
            const bool bnd = o8 == static_cast<unsigned>(m * ld) * 8u + k8;
            const double nxf = NODAL ? ld_row(p.fgeo + j * ld, k8) : nxa;
            const double nyf = NODAL ? ld_row(p.fgeo + fplane + j * ld, k8) : nya;
            const double fs = NODAL ? ld_row(p.fgeo + 2 * fplane + j * ld, k8) : fsa;
            const double fxP = ld_row(fxp, o8), fyP = ld_row(fyp, o8);
            // (a boundary node reads itself: the mirrored flux makes the jump twice the own normal flux)
            const double dx = F[m] - (bnd ? -F[m] : fxP), dy = G[m] - (bnd ? -G[m] : fyP);
            s[j] = 0.5 * fs * (nxf * dx + nyf * dy);
            __builtin_amdgcn_sched_barrier(0); // one face node at a time
        }
    }

    // ---- output rows, one node at a time
    const long long fo = 3 * plane;
    double rxa = 0.0, sxa = 0.0, rya = 0.0, sya = 0.0;
    if constexpr (!NODAL) {
        rxa = ld_row(p.ageo, k8);
        sxa = ld_row(p.ageo + ld, k8);
        rya = ld_row(p.ageo + 2 * ld, k8);
        sya = ld_row(p.ageo + 3 * ld, k8);
    }
    const bool hasS = dp.source != nullptr;
    const double* __restrict__ srcp = hasS ? dp.source : p.qin;
#pragma unroll 1
    for (int i = 0; i < Np; ++i) {
        const double* __restrict__ row = ops + static_cast<size_t>(i) * VnOps<N>::ROW;
        const long long io = static_cast<long long>(i) * ld;
        const double rx = NODAL ? ld_row(p.geo + io, k8) : rxa, sx = NODAL ? ld_row(p.geo + plane + io, k8) : sxa,
                     ry = NODAL ? ld_row(p.geo + 2 * plane + io, k8) : rya, sy = NODAL ? ld_row(p.geo + 3 * plane + io, k8) : sya;
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
        double T = ((rx * a + sx * b) + (ry * cG + sy * d)) - lift;
        // the pointwise part (zero where the rows are pre-filtered: the host sends those launches without one)
        const double sv = ld_row(srcp + io, k8);
        T += (hasS ? sv : 0.0) - dp.decay * ld_row(p.qin + fo + io, k8);
        if constexpr (RAW) st_row(dp.raw + io, k8, T);
        else diffusion_add_row<MODE>(p, fo, io, k8, T);
    }
}

// ---- last step of a filtered evaluation in two steps: rows of dp.raw -> Filter rows, then the update. filt: (Np, Np) row-major.
template <int N, int MODE>
__global__ __launch_bounds__(64) void sw2d_tracer_diffusion_filter_kernel(const StageParams p, const DiffusionParams dp,
                                                                          const double* __restrict__ filt) {
    using E = Elem<N>;
    constexpr int Np = E::Np;
    const unsigned tile = stage_tile(blockIdx.x, gridDim.x, static_cast<unsigned>(p.sweepBack));
    const unsigned k = static_cast<unsigned>(p.kbegin) + tile * 64u + threadIdx.x;
    if (k >= static_cast<unsigned>(p.kend)) return;
    const unsigned k8 = k * 8u;
    const long long ld = p.ld, plane = static_cast<long long>(Np) * ld, fo = 3 * plane;
    double R[Np];
#pragma unroll
    for (int m = 0; m < Np; ++m) R[m] = ld_row(dp.raw + m * ld, k8);
#pragma unroll 1
    for (int i = 0; i < Np; ++i) {
        const double* __restrict__ row = filt + static_cast<size_t>(i) * Np;
        double r = 0.0;
#pragma unroll
        for (int m = 0; m < Np; ++m) r = fma(row[m], R[m], r);
        diffusion_add_row<MODE>(p, fo, static_cast<long long>(i) * ld, k8, r);
    }
}

} // namespace bdg_dev
