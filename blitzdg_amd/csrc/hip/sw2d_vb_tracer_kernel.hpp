// sw2d_vb_tracer_kernel.hpp -- a passive tracer hN (field 3 of a four-field state) carried through variant B, the tidal
// right-hand side of sw2d_vb_kernel.hpp. The reference's tidal driver (src/sw2d/main.cpp:279-484) has no tracer; the
// definition is the one of the quadrilateral solver (sw2d_quadb4_kernel.hpp) on triangles:
//   concentrations from the depths BEFORE the star states, NM = hN- / h-, NP = hN+ / h+; a wall node takes NP = NM, an
//   open-boundary node then NP = Nopen (it wins where a node is both, as hP does);
//   star tracer hNM* = hM* NM, hNP* = hP* NP (a true rescale: hN = c h with Nopen = c gives r4 = c r1 over a bed that jumps);
//   F4 = (hN* hu*) / h*, G4 = (hN* hv*) / h* on both sides,
//   d4 = 1/2 ((F4M - F4P) nx + (G4M - G4P) ny - lam (hNM* - hNP*)) with variant B's ONE global speed (the tracer does not enter it);
//   r4 = -div((hN hu) / h, (hN hv) / h) + Lift(Fscale d4), no source.
// The equation is a pass of its own -- fused RHS + stage update of plane 3 only -- launched behind the three-field variant-B
// launch on the same stream and the same input state: that launch writes qout and leaves the speed of the NEXT evaluation
// in the other accumulator, so planes 0-2 of qin and *vp.lam are still those of this evaluation. Two forms:
//   sw2d_stage_vb_tracer_unrolled_kernel  straight-sided elements, N <= 4: the structure of sw2d_stage_tracer_kernel (one lane
//                                         per element in one-wave workgroups, everything unrolled, operators through scalar
//                                         loads, the filter folded into the operator image) with vb_trace's boundary rules
//   sw2d_stage_vb_tracer_kernel           every order, straight-sided (13 numbers per element) or per-node geometry: the rolled
//                                         output-row form of sw2d_stage_vn_kernel for one field, i.e. the fourth wave that
//                                         kernel would have; on per-node geometry a filtered evaluation is its unfiltered rows
//                                         followed by sw2d_vb_tracer_filter_kernel (the metric multiplies after the
//                                         differentiation), on straight-sided elements the rows of the image are pre-filtered
#pragma once
#include "sw2d_vn_kernel.hpp"

namespace bdg_dev {

// The concentration the open boundary feeds: one scalar, or one value per open-boundary face node. The values of an element's
// open nodes are consecutive in `openN`, in the order of its face nodes, from openBase[slot] on (slot: the element's device
// slot, as the bit masks of VbParams::obc are stored).
struct VbTracerParams {
    const int* openBase;   // (1, ld) or nullptr: nOpenC at every open-boundary node
    const double* openN;
    double nOpenC;
};

// '-' and '+' tracer fluxes of one face node: s4 without the face scale. h, hu, hv, hN: the element's own values at the node;
// hq, huq, hvq, hNq: the neighbour's; HM, HP: the still-water depth on both sides; nOpen: the open-boundary concentration here.
__device__ __forceinline__ double vb_tracer_jump(double h, double hu, double hv, double hN, double hq, double huq, double hvq,
                                                 double hNq, double HM, double HP, bool open, bool wall, double nOpen,
                                                 double nxf, double nyf, double tide, double lam) {
    const double NM = hN * fast_rcp(h);
    const double NPi = hNq * fast_rcp(hq);
    // open boundary: the surface follows the tide, the momentum is the element's own (:348-353); reflective wall (:340-345)
    const bool own = open | wall;
    const double un2 = (open ? 0.0 : 2.0) * (hu * nxf + hv * nyf);
    const double hP = open ? HM + tide : (wall ? h : hq);
    const double huP = own ? hu - nxf * un2 : huq;
    const double hvP = own ? hv - nyf * un2 : hvq;
    const double NP = open ? nOpen : (wall ? NM : NPi);
    const double bM = -HM, bP = -HP, mx = fmax(bP, bM);
    const double hMs = fmax(0.0, h + bM - mx), hPs = fmax(0.0, hP + bP - mx);
    const double rM = fast_rcp(hMs), rP = fast_rcp(hPs);
    const double huMs = hMs * (hu * rM), hvMs = hMs * (hv * rM);     // hMstar*(huM/hM) with hM already = hMstar
    const double huPs = hPs * (huP * rP), hvPs = hPs * (hvP * rP);
    const double hNMs = hMs * NM, hNPs = hPs * NP;
    const double dF = (hNMs * huMs) * rM - (hNPs * huPs) * rP;
    const double dG = (hNMs * hvMs) * rM - (hNPs * hvPs) * rP;
    return dF * nxf + dG * nyf - lam * (hNMs - hNPs);
}

// ---- unrolled form (N <= 4, straight-sided elements). p.opsAffine: AffineOps image, plain or pre-filtered.
template <int N, int MODE>
__global__ __launch_bounds__(64) void sw2d_stage_vb_tracer_unrolled_kernel(const StageParams p, const VbParams vp,
                                                                           const VbTracerParams tp) {
    using E = Elem<N>;
    constexpr int Np = E::Np, Nfp = E::Nfp, NFN = E::NFN;

    const unsigned tile = stage_tile(blockIdx.x, gridDim.x, static_cast<unsigned>(p.sweepBack));
    const unsigned k = static_cast<unsigned>(p.kbegin) + tile * blockDim.x + threadIdx.x;
    if (k >= static_cast<unsigned>(p.kend)) return;
    const unsigned k8 = k * 8u, k4 = k * 4u;

    const long long ld = p.ld, plane = static_cast<long long>(Np) * ld;
    const double* __restrict__ ops = p.opsAffine;
    const double* __restrict__ qin = p.qin;
    const double lam = *vp.lam;
    // Per-node concentrations: the table is read at every face node, entry 0 where the node is not an open one (one line, no
    // traffic) -- by a select on the address and not by a branch, which would split this body's one scheduling region. Without
    // a table the same loads go to valid words whose values are not used.
    const bool table = tp.openBase != nullptr;
    const int* __restrict__ basep = table ? tp.openBase : vp.obc;
    const double* __restrict__ tabp = table ? tp.openN : vp.lam;

    // ---- first batch: gather indices, own state, geometry, depth at the face nodes
    int idx[NFN];
#pragma unroll
    for (int j = 0; j < NFN; ++j) idx[j] = ld_row(p.vmapP + j * ld, k4);
    const int tags = ld_row(vp.obc, k4);
    const int base = ld_row(basep, k4);
    double h[Np], hu[Np], hv[Np], hN[Np];
#pragma unroll
    for (int n = 0; n < Np; ++n) {
        h[n] = ld_row(qin + n * ld, k8);
        hu[n] = ld_row(qin + plane + n * ld, k8);
        hv[n] = ld_row(qin + 2 * plane + n * ld, k8);
        hN[n] = ld_row(qin + 3 * plane + n * ld, k8);
    }
    const double* __restrict__ ag = p.ageo;
    const double rx = ld_row(ag, k8), sx = ld_row(ag + ld, k8), ry = ld_row(ag + 2 * ld, k8), sy = ld_row(ag + 3 * ld, k8);
    double fnx[3], fny[3], fsc[3];
#pragma unroll
    for (int f = 0; f < 3; ++f) {
        fnx[f] = ld_row(ag + (4 + f) * ld, k8);
        fny[f] = ld_row(ag + (7 + f) * ld, k8);
        fsc[f] = ld_row(ag + (10 + f) * ld, k8);
    }
    double HM[NFN];
#pragma unroll
    for (int f = 0; f < 3; ++f)
#pragma unroll
        for (int n = 0; n < Nfp; ++n) HM[f * Nfp + n] = ld_row(vp.H + E::fmask(f, n) * ld, k8);
    __builtin_amdgcn_sched_barrier(0);
    // ---- second batch: neighbour traces, neighbour depth, open-boundary concentrations
    double hP[NFN], huP[NFN], hvP[NFN], hNP[NFN], HP[NFN], nOp[NFN];
#pragma unroll
    for (int j = 0; j < NFN; ++j) {
        const unsigned o8 = static_cast<unsigned>(idx[j] < 0 ? -(idx[j] + 1) : idx[j]) * 8u;
        hP[j] = ld_row(qin, o8);
        huP[j] = ld_row(qin + plane, o8);
        hvP[j] = ld_row(qin + 2 * plane, o8);
        hNP[j] = ld_row(qin + 3 * plane, o8);
        HP[j] = ld_row(vp.H, o8);
        const bool here = table & (((tags >> j) & 1) != 0);
        const unsigned at = here ? static_cast<unsigned>(base + __popc(static_cast<unsigned>(tags) & ((1u << j) - 1u))) : 0u;
        nOp[j] = ld_row(tabp, at * 8u);
    }
    __builtin_amdgcn_sched_barrier(0);

    double R[Np];
#pragma unroll
    for (int i = 0; i < Np; ++i) R[i] = 0.0;

    // ---- surface term with star states, face by face
#pragma unroll
    for (int f = 0; f < 3; ++f) {
        const double nxf = fnx[f], nyf = fny[f], half_fs = 0.5 * fsc[f];
#pragma unroll
        for (int n = 0; n < Nfp; ++n) {
            const int j = f * Nfp + n, m = E::fmask(f, n);
            const bool open = ((tags >> j) & 1) != 0, wall = (idx[j] < 0) & !open;
            const double s4 = half_fs * vb_tracer_jump(h[m], hu[m], hv[m], hN[m], hP[j], huP[j], hvP[j], hNP[j], HM[j], HP[j], open, wall,
                                                       table ? nOp[j] : tp.nOpenC, nxf, nyf, vp.tide, lam);
#pragma unroll
            for (int i = 0; i < Np; ++i) R[i] = fma(ops[AffineOps<N>::OFF_LIFT + j * Np + i], s4, R[i]);
        }
    }

    // ---- stage input needed at the very end: issue now, lands during the volume loop
    const long long fo = 3 * plane;
    double oldv[Np];
    if constexpr (MODE != MODE_RHS) {
        const double* __restrict__ base2 = ((MODE == MODE_LSERK) ? p.res : p.qbase) + fo;
#pragma unroll
        for (int i = 0; i < Np; ++i) oldv[i] = ld_row(base2 + i * ld, k8);
    }
    __builtin_amdgcn_sched_barrier(0);

    // ---- volume term
#pragma unroll
    for (int m = 0; m < Np; ++m) {
        const double r = fast_rcp(h[m] * p.one);
        const double F4 = (hN[m] * hu[m]) * r, G4 = (hN[m] * hv[m]) * r;
        const double a = -(rx * F4 + ry * G4), b = -(sx * F4 + sy * G4);
#pragma unroll
        for (int i = 0; i < Np; ++i) R[i] = fma(ops[AffineOps<N>::OFF_D + 2 * (m * Np + i)], a, R[i]);
#pragma unroll
        for (int i = 0; i < Np; ++i) R[i] = fma(ops[AffineOps<N>::OFF_D + 2 * (m * Np + i) + 1], b, R[i]);
    }

    // ---- stage update / output of the tracer field (never sponged: the relaxation is the momentum's)
    if constexpr (MODE == MODE_RHS) {
#pragma unroll
        for (int i = 0; i < Np; ++i) st_row(p.rhs + fo + i * ld, k8, R[i]);
    } else if constexpr (MODE == MODE_LSERK) {
#pragma unroll
        for (int i = 0; i < Np; ++i) {
            const double n1 = p.ca * oldv[i] + p.cc * R[i];
            st_row(p.res + fo + i * ld, k8, n1);
            st_row(p.qout + fo + i * ld, k8, hN[i] + p.cb * n1);
        }
    } else {
#pragma unroll
        for (int i = 0; i < Np; ++i) st_row(p.qout + fo + i * ld, k8, p.ca * oldv[i] + p.cb * hN[i] + p.cc * R[i]);
    }
}

// ---- general form: one wave of 64 elements, rolled. ops: VnOps image (row i = {Dr[i][m], Ds[i][m]} interleaved, then
// Lift[i][j]), plain -- or, NODAL = false only, pre-multiplied by the Filter. NODAL: metric per output node and normals / scales
// per face node (p.geo, p.fgeo); else the 13 numbers per element of p.ageo.
template <int N, int MODE, bool NODAL>
__global__ __launch_bounds__(64) void sw2d_stage_vb_tracer_kernel(const StageParams p, const VbParams vp, const VbTracerParams tp,
                                                                  const double* __restrict__ ops) {
    using E = Elem<N>;
    constexpr int Np = E::Np, Nfp = E::Nfp, NFN = E::NFN;
    const unsigned tile = stage_tile(blockIdx.x, gridDim.x, static_cast<unsigned>(p.sweepBack));
    const unsigned k = static_cast<unsigned>(p.kbegin) + tile * 64u + threadIdx.x;
    if (k >= static_cast<unsigned>(p.kend)) return;
    const unsigned k8 = k * 8u, k4 = k * 4u;
    const long long ld = p.ld, plane = static_cast<long long>(Np) * ld, fplane = static_cast<long long>(NFN) * ld;
    const double* __restrict__ qin = p.qin;
    const double lam = *vp.lam;

    // ---- fluxes of the tracer at the nodes
    double F[Np], G[Np];
#pragma unroll
    for (int m = 0; m < Np; ++m) {
        const double h = ld_row(qin + m * ld, k8), hu = ld_row(qin + plane + m * ld, k8), hv = ld_row(qin + 2 * plane + m * ld, k8);
        const double hN = ld_row(qin + 3 * plane + m * ld, k8);
        const double r = fast_rcp(h);
        F[m] = (hN * hu) * r;
        G[m] = (hN * hv) * r;
        // (a few nodes' loads in flight at a time: hoisted all at once they would not fit the register file at N >= 6)
        if (m % 6 == 5) __builtin_amdgcn_sched_barrier(0);
    }
    __builtin_amdgcn_sched_barrier(0);

    // ---- scaled flux jumps at the face nodes
    double s[NFN];
    const int tags = ld_row(vp.obc, k4);
    // (the table read at every face node through a select on the address, as in the unrolled form: a branch per node would end the
    // basic block the barriers below order)
    const bool table = tp.openBase != nullptr;
    const double* __restrict__ tabp = table ? tp.openN : vp.lam;
    const int base = ld_row(table ? tp.openBase : vp.obc, k4);
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
            const double nxf = NODAL ? ld_row(p.fgeo + j * ld, k8) : nxa;
            const double nyf = NODAL ? ld_row(p.fgeo + fplane + j * ld, k8) : nya;
            const double fs = NODAL ? ld_row(p.fgeo + 2 * fplane + j * ld, k8) : fsa;
            const unsigned o8 = static_cast<unsigned>(id < 0 ? -(id + 1) : id) * 8u;
            const bool open = ((tags >> j) & 1) != 0, wall = (id < 0) & !open;
            const unsigned at = (table & open) ? static_cast<unsigned>(base + __popc(static_cast<unsigned>(tags) & ((1u << j) - 1u))) : 0u;
            const double nTab = ld_row(tabp, at * 8u);
            const double nOpen = table ? nTab : tp.nOpenC;
            s[j] = 0.5 * fs * vb_tracer_jump(ld_row(qin + m * ld, k8), ld_row(qin + plane + m * ld, k8), ld_row(qin + 2 * plane + m * ld, k8),
                                             ld_row(qin + 3 * plane + m * ld, k8), ld_row(qin, o8), ld_row(qin + plane, o8),
                                             ld_row(qin + 2 * plane, o8), ld_row(qin + 3 * plane, o8), ld_row(vp.H + m * ld, k8),
                                             ld_row(vp.H, o8), open, wall, nOpen, nxf, nyf, vp.tide, lam);
            __builtin_amdgcn_sched_barrier(0); // one face node at a time, for the same reason
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
        double R = -(rx * a + sx * b) - (ry * cG + sy * d);
        double lift = 0.0;
#pragma unroll
        for (int j = 0; j < NFN; ++j) lift = fma(row[2 * Np + j], s[j], lift);
        R += lift;
        if constexpr (MODE == MODE_RHS) {
            st_row(p.rhs + fo + io, k8, R);
        } else if constexpr (MODE == MODE_LSERK) {
            const double n1 = p.ca * ld_row(p.res + fo + io, k8) + p.cc * R;
            st_row(p.res + fo + io, k8, n1);
            st_row(p.qout + fo + io, k8, ld_row(qin + fo + io, k8) + p.cb * n1);
        } else {
            st_row(p.qout + fo + io, k8, p.ca * ld_row(p.qbase + fo + io, k8) + p.cb * ld_row(qin + fo + io, k8) + p.cc * R);
        }
    }
}

// ---- second pass of a FILTERED evaluation on per-node geometry: rows R of plane 3 of `raw` -> Filter R, then the update of
// MODE. filt: (Np, Np) row-major. One lane per element.
template <int N, int MODE>
__global__ __launch_bounds__(64) void sw2d_vb_tracer_filter_kernel(const StageParams p, const double* __restrict__ raw,
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
    for (int m = 0; m < Np; ++m) R[m] = ld_row(raw + fo + m * ld, k8);
#pragma unroll 1
    for (int i = 0; i < Np; ++i) {
        const double* __restrict__ row = filt + static_cast<size_t>(i) * Np;
        const long long io = static_cast<long long>(i) * ld;
        double r = 0.0;
#pragma unroll
        for (int m = 0; m < Np; ++m) r = fma(row[m], R[m], r);
        if constexpr (MODE == MODE_RHS) {
            st_row(p.rhs + fo + io, k8, r);
        } else if constexpr (MODE == MODE_LSERK) {
            const double n1 = p.ca * ld_row(p.res + fo + io, k8) + p.cc * r;
            st_row(p.res + fo + io, k8, n1);
            st_row(p.qout + fo + io, k8, ld_row(p.qin + fo + io, k8) + p.cb * n1);
        } else {
            st_row(p.qout + fo + io, k8, p.ca * ld_row(p.qbase + fo + io, k8) + p.cb * ld_row(p.qin + fo + io, k8) + p.cc * r);
        }
    }
}

} // namespace bdg_dev
