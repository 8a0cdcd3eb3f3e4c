// sw2d_viscosity_kernel.hpp -- horizontal eddy viscosity of the triangle solver, constant or Smagorinsky (the
// definition is restated in tests/triviscosity_ref.py):
//   d(hu)/dt += T_u = div(nu h grad u),  d(hv)/dt += T_v = div(nu h grad v),   u = hu / h, v = hv / h,
//   nu = nu0 + Cs^2 D^2 |S|,  |S| = sqrt(2 u_x^2 + 2 v_y^2 + (u_y + v_x)^2),  D^2 = 2 J / (N+1)^2.
// The discretisation is the tracer's (sw2d_diffusion_kernel.hpp): local DG, central fluxes, no penalty, zero viscous stress at
// a BOUNDARY node (a face node whose gather index points at itself: walls and the open boundary alike -- free slip). Two passes
// over the mesh for BOTH momentum components, each pass taking the components in turn inside one launch -- the registers of a
// lane hold one field's Np nodal values and 3 Nfp jumps at a time, as in the tracer's passes, so that no order needs scratch:
//   sw2d_viscosity_gradient_kernel    per component: q = (rx Dr + sx Ds) u - Lift(Fscale nx du / 2), likewise qy, into flux
//                                     planes 0-3 (qx_u, qy_u, qx_v, qy_v). Then, node by node, the lane's own four values back
//                                     (stored a few hundred instructions earlier, still in cache), |S| from them, nu, and
//                                     f = nu h q in their place. The u_x ... v_y of |S| are the gradients that diffuse, lifts
//                                     included. J = 1 / (rx sy - sx ry) at the node. nuOut != nullptr: nu as well.
//   sw2d_viscosity_divergence_kernel  per component: dF = nx (fx- - fx+) + ny (fy- - fy+), 2 (nx fx- + ny fy-) at boundary
//                                     nodes; T = rx Dr fx + sx Ds fx + ry Dr fy + sy Ds fy - Lift(Fscale dF / 2)
// T enters the stage whose launches were just issued on the same stream, ADDED to planes 1 and 2 of what they wrote (they read
// qin and write rhs / res / qout, which are other buffers):
//   MODE_RHS      rhs += T
//   MODE_LSERK    res += cc T,  qout += cb cc T
//   MODE_COMBINE  qout = sponge(qout + cc T): the stage launch of a viscous solver runs with the sponge off (a division by
//                 exactly 1), and the division of the Heun step is made here, after T: q1 = sponge(q + dt (R + T))
// Planes 0 and 3 are never touched. A filtered evaluation: pre-filtered rows in the second pass on straight-sided elements;
// per-node geometry (the metric multiplies after the differentiation): the unfiltered T of both components into two scratch
// planes and sw2d_viscosity_filter_kernel applies Filter rows, then the update.
#pragma once
#include "sw2d_vn_kernel.hpp"

namespace bdg_dev {

struct ViscosityParams {
    const double* nuField; // (Np, ld) nu0 at every node, or nullptr
    double nu;             // nu0 when nuField is nullptr
    double cs2d2;          // Cs^2 * 2 / (N+1)^2: nu = nu0 + cs2d2 J |S|
    double* flux;          // 4 planes of Np*ld: nu h (qx_u, qy_u, qx_v, qy_v)
    double* raw;           // 2 planes of Np*ld (filtered evaluations in two steps) or nullptr
    double* nuOut;         // 1 plane of Np*ld: nu of the state the gradient pass read, or nullptr
    // MODE_COMBINE: the momentum relaxation x /= (1 + sigma x^2) after the update; sigma per node, or the scalar
    const double* spongeField;
    double sponge;
};

// ---- first pass. ops: plain VnOps image.
template <int N, bool NODAL>
__global__ __launch_bounds__(64) void sw2d_viscosity_gradient_kernel(const StageParams p, const ViscosityParams vp,
                                                                     const double* __restrict__ ops) {
    using E = Elem<N>;
    constexpr int Np = E::Np, Nfp = E::Nfp, NFN = E::NFN;
    const unsigned tile = stage_tile(blockIdx.x, gridDim.x, static_cast<unsigned>(p.sweepBack));
    const unsigned k = static_cast<unsigned>(p.kbegin) + tile * 64u + threadIdx.x;
    if (k >= static_cast<unsigned>(p.kend)) return;
    unsigned k8 = k * 8u, k4 = k * 4u;
    long long ld = p.ld;
    const double* __restrict__ qin = p.qin;
    double* flux = vp.flux; // (read back below: no __restrict__)
    const bool field = vp.nuField != nullptr;
    const double* __restrict__ nup = field ? vp.nuField : qin; // (a valid row either way: the select is on the value)

#pragma unroll 1
    for (int c = 0; c < 2; ++c) {
        // (the second component starts from scratch: without this the row addresses, the gather index and the geometry of the
        // first are kept in registers across the loop, and the large orders spill)
        asm volatile("" : "+s"(ld), "+v"(k8), "+v"(k4) : : "memory");
        const long long plane = static_cast<long long>(Np) * ld, fplane = static_cast<long long>(NFN) * ld;
        const double* __restrict__ qc = qin + (1 + c) * plane;

        // ---- the velocity component at the nodes
        double C[Np];
#pragma unroll
        for (int m = 0; m < Np; ++m) {
            C[m] = ld_row(qc + m * ld, k8) * fast_rcp(ld_row(qin + m * ld, k8));
            if (m % 6 == 5) __builtin_amdgcn_sched_barrier(0); // a few nodes' loads in flight at a time
        }
        __builtin_amdgcn_sched_barrier(0);

        // ---- scaled jumps at the face nodes: Fscale du / 2, times the normal per face node where it differs from node to node
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
                const double CP = ld_row(qc, o8) * fast_rcp(ld_row(qin, o8));
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
            const double gx = (rx * a + sxm * b) - lx, gy = (ry * a + sym * b) - ly;
            st_row(flux + 2 * c * plane + io, k8, gx);
            st_row(flux + (2 * c + 1) * plane + io, k8, gy);
        }
    }

    // ---- nu at the nodes from the four gradient components this lane has just stored, and f = nu h q in their place
    const long long plane = static_cast<long long>(Np) * ld;
#pragma unroll 1
    for (int i = 0; i < Np; ++i) {
        const long long io = static_cast<long long>(i) * ld;
        const double ux = ld_row(flux + io, k8), uy = ld_row(flux + plane + io, k8), vx = ld_row(flux + 2 * plane + io, k8),
                     vy = ld_row(flux + 3 * plane + io, k8);
        double rx, sxm, ry, sym;
        if constexpr (NODAL) {
            rx = ld_row(p.geo + io, k8); sxm = ld_row(p.geo + plane + io, k8);
            ry = ld_row(p.geo + 2 * plane + io, k8); sym = ld_row(p.geo + 3 * plane + io, k8);
        } else {
            rx = ld_row(p.ageo, k8); sxm = ld_row(p.ageo + ld, k8);
            ry = ld_row(p.ageo + 2 * ld, k8); sym = ld_row(p.ageo + 3 * ld, k8);
        }
        const double shear = uy + vx;
        const double S = sqrt(2.0 * (ux * ux) + 2.0 * (vy * vy) + shear * shear);
        const double J = 1.0 / (rx * sym - sxm * ry);
        const double nv = ld_row(nup + io, k8);
        const double nu = (field ? nv : vp.nu) + vp.cs2d2 * J * S;
        const double nh = nu * ld_row(qin + io, k8);
        st_row(flux + io, k8, nh * ux);
        st_row(flux + plane + io, k8, nh * uy);
        st_row(flux + 2 * plane + io, k8, nh * vx);
        st_row(flux + 3 * plane + io, k8, nh * vy);
        if (vp.nuOut) st_row(vp.nuOut + io, k8, nu);
    }
}

// The update of momentum plane fo by one row r of T (or of Filter T) at node offset io: added to what the stage's own launches
// wrote; the Heun step's division follows the sum.
template <int MODE>
__device__ __forceinline__ void viscosity_add_row(const StageParams& p, const ViscosityParams& vp, long long fo, long long io,
                                                  unsigned k8, double r) {
    if constexpr (MODE == MODE_RHS) {
        st_row(p.rhs + fo + io, k8, ld_row(p.rhs + fo + io, k8) + r);
    } else if constexpr (MODE == MODE_LSERK) {
        const double d = p.cc * r;
        st_row(p.res + fo + io, k8, ld_row(p.res + fo + io, k8) + d);
        st_row(p.qout + fo + io, k8, fma(p.cb, d, ld_row(p.qout + fo + io, k8)));
    } else {
        const bool sf = vp.spongeField != nullptr;
        const double* __restrict__ spp = sf ? vp.spongeField : p.qin; // (no field: any valid plane, the value is not used)
        const double sv = ld_row(spp + io, k8);
        st_row(p.qout + fo + io, k8, sponge_relax(fma(p.cc, r, ld_row(p.qout + fo + io, k8)), sf ? sv : vp.sponge));
    }
}

// ---- second pass. ops: VnOps image, plain -- or, NODAL = false, pre-multiplied by the Filter. RAW: the unfiltered T of the
// two components goes to vp.raw whatever MODE says (sw2d_viscosity_filter_kernel does the update).
template <int N, int MODE, bool NODAL, bool RAW = false>
__global__ __launch_bounds__(64) void sw2d_viscosity_divergence_kernel(const StageParams p, const ViscosityParams vp,
                                                                       const double* __restrict__ ops) {
    using E = Elem<N>;
    constexpr int Np = E::Np, Nfp = E::Nfp, NFN = E::NFN;
    const unsigned tile = stage_tile(blockIdx.x, gridDim.x, static_cast<unsigned>(p.sweepBack));
    const unsigned k = static_cast<unsigned>(p.kbegin) + tile * 64u + threadIdx.x;
    if (k >= static_cast<unsigned>(p.kend)) return;
    unsigned k8 = k * 8u, k4 = k * 4u;
    long long ld = p.ld;

#pragma unroll 1
    for (int c = 0; c < 2; ++c) {
        asm volatile("" : "+s"(ld), "+v"(k8), "+v"(k4) : : "memory"); // (as in the first pass: nothing of the first component is kept)
        const long long plane = static_cast<long long>(Np) * ld, fplane = static_cast<long long>(NFN) * ld;
        const double* __restrict__ fxp = vp.flux + 2 * c * plane;
        const double* __restrict__ fyp = fxp + plane;

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
        const long long fo = (1 + c) * plane;
        double rxa = 0.0, sxa = 0.0, rya = 0.0, sya = 0.0;
        if constexpr (!NODAL) {
            rxa = ld_row(p.ageo, k8);
            sxa = ld_row(p.ageo + ld, k8);
            rya = ld_row(p.ageo + 2 * ld, k8);
            sya = ld_row(p.ageo + 3 * ld, k8);
        }
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
            const double T = ((rx * a + sx * b) + (ry * cG + sy * d)) - lift;
            if constexpr (RAW) st_row(vp.raw + c * plane + io, k8, T);
            else viscosity_add_row<MODE>(p, vp, fo, io, k8, T);
        }
    }
}

// ---- last step of a filtered evaluation in two steps: rows of vp.raw -> Filter rows, then the update. filt: (Np, Np) row-major.
template <int N, int MODE>
__global__ __launch_bounds__(64) void sw2d_viscosity_filter_kernel(const StageParams p, const ViscosityParams vp,
                                                                   const double* __restrict__ filt) {
    using E = Elem<N>;
    constexpr int Np = E::Np;
    const unsigned tile = stage_tile(blockIdx.x, gridDim.x, static_cast<unsigned>(p.sweepBack));
    const unsigned k = static_cast<unsigned>(p.kbegin) + tile * 64u + threadIdx.x;
    if (k >= static_cast<unsigned>(p.kend)) return;
    const unsigned k8 = k * 8u;
    const long long ld = p.ld, plane = static_cast<long long>(Np) * ld;
#pragma unroll 1
    for (int c = 0; c < 2; ++c) {
        double R[Np];
#pragma unroll
        for (int m = 0; m < Np; ++m) R[m] = ld_row(vp.raw + c * plane + m * ld, k8);
#pragma unroll 1
        for (int i = 0; i < Np; ++i) {
            const double* __restrict__ row = filt + static_cast<size_t>(i) * Np;
            double r = 0.0;
#pragma unroll
            for (int m = 0; m < Np; ++m) r = fma(row[m], R[m], r);
            viscosity_add_row<MODE>(p, vp, (1 + c) * plane, static_cast<long long>(i) * ld, k8, r);
        }
    }
}

// ---- the largest nu of a plane, in a fixed order and without atomics: `nblocks` workgroups of 256 lanes each reduce a
// contiguous share of the n entries into part[block] (lane l takes entries l, l + 256, ... of the share, then a tree over the
// 256); a second launch with one workgroup reduces the partials the same way into out[0]. nu >= 0 and the padding columns of
// the plane are zero, so 0 is the neutral element. (A template only so that every per-order object carries its own copy.)
template <int N>
__global__ __launch_bounds__(256) void sw2d_viscosity_max_kernel(const double* __restrict__ in, long long n, double* __restrict__ out) {
    __shared__ double sm[256];
    const long long share = (n + gridDim.x - 1) / gridDim.x;
    const long long lo = static_cast<long long>(blockIdx.x) * share, hi = lo + share < n ? lo + share : n;
    double a = 0.0;
    for (long long i = lo + threadIdx.x; i < hi; i += 256) a = fmax(a, in[i]);
    sm[threadIdx.x] = a;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (static_cast<int>(threadIdx.x) < s) sm[threadIdx.x] = fmax(sm[threadIdx.x], sm[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = sm[0];
}

} // namespace bdg_dev
