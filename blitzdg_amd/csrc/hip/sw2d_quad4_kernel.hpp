// sw2d_quad4_kernel.hpp -- the four-field, source-carrying form of the quadrilateral sw2d stage kernel (gfx950 / CDNA4,
// wave64): passive tracer hN, Coriolis f, quadratic drag CD, bed slope zx, zy. Device restatement of the reference's
// Python right-hand side (swhelpers/rhs.py:178-311 with the fluxes of swhelpers/flux.py), which reads nothing
// triangle-specific, on the Gauss-Lobatto tensor element of sw2d_quad_kernel.hpp. Same tiles, phases, geometry forms, modes
// and element-range launch as the three-field kernel there; what differs is the arithmetic (that function's, not the
// script's):
//   traces are re-formed through the velocities, uM = huM / hM, huM = hM uM (rhs.py:212-233), before the wall mirror;
//   fluxes go through velocities: F2 = hu u + g h^2 / 2, G2 = hu v, F3 = hv u, G3 = hv v + g h^2 / 2, F4 = hN u, G4 = hN v
//   (F3 and G2 are two arrays), so phase A writes eight planes hu, hv, F2, G2, F3, G3, F4, G4 and phase C differentiates
//   eight; one Lax-Friedrichs speed per face for all four equations; four surface planes;
//   SRC = true adds, pointwise and before the filter, (f hv - CD |u| u) - g h zx to RHS2 and -(f hu - CD |u| v) - g h zy to
//   RHS3 (the sign of the drag in RHS3 is the reference's, rhs.py:307; each sum is formed first and added once, so it
//   differs from the reference's three additions in the last bit). SRC = false compiles none of it.
// The tracer rides in the same pass: with eight flux planes a tile needs 39 KB of LDS at N = 4 and 107 KB at N = 8. A second
// phase that re-uses two flux planes for F4, G4 (six planes) would change the number of resident workgroups per CU only at
// N = 7 (86 -> 70 KB: 1 -> 2), and costs two more workgroup barriers at every order; DESIGN section 3.8 has the table.
// It lives beside sw2d_quad_kernel.hpp rather than in it as further template parameters so that the three-field
// instances (and their kernel arguments) are compiled from unchanged text.
#pragma once
#include "sw2d_quad_kernel.hpp"

namespace bdg_dev {

template <int N>
struct Quad4Elem : QuadElem<N> {
    using Q = QuadElem<N>;
    // LDS in doubles: ops | 8 flux arrays [a][n][e] (reused for the filtered RHS) | speeds [fn][e] | surface [c][fn][e]
    static constexpr int OFF_SPD = Q::OFF_FL + 8 * Q::Np * Q::E;
    static constexpr int OFF_SURF = OFF_SPD + Q::NFN * Q::E;
    static constexpr int LDS_DOUBLES = OFF_SURF + 4 * Q::NFN * Q::E;
};

struct Quad4Params {
    QuadParams q;       // as the three-field kernel, every state / residual / rhs buffer with 4 planes: h, hu, hv, hN
    const double* zx;   // SRC: Np*ld
    const double* zy;
    const double* fcor; // SRC: Np*ld, or nullptr: fconst
    double fconst, CD;
};

// the stage update of one node (offset o in plane 0) from its right-hand side v[0..3]
template <int MODE>
__device__ __forceinline__ void store4(const QuadParams& p, long long o, long long plane, const double (&v)[4]) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const long long oc = c * plane + o;
        if (MODE == QMODE_RHS) {
            p.rhs[oc] = v[c];
        } else if (MODE == QMODE_COMBINE) {
            p.qout[oc] = p.qbase[oc] + p.cc * v[c];
        } else {
            const double a = p.ca * p.res[oc] + p.cc * v[c];
            p.res[oc] = a;
            p.qout[oc] = p.qin[oc] + p.cb * a; // own state again: an L2 hit
        }
    }
}

// the source terms of one node (offset o), rhs.py:300-309: s2 is added to RHS2 and s3 to RHS3; u = hu / h, v = hv / h
__device__ __forceinline__ void sources4(const Quad4Params& pp, long long o, double h, double hu, double hv, double u, double v,
                                         double& s2, double& s3) {
    const double cdn = pp.CD * sqrt(u * u + v * v);
    const double f = pp.fcor ? pp.fcor[o] : pp.fconst;
    const double gh = pp.q.g * h;
    s2 = (f * hv - cdn * u) - gh * pp.zx[o];
    s3 = -(f * hu - cdn * v) - gh * pp.zy[o];
}

template <int N, int MODE, bool FILT, bool GEN, bool SRC>
__global__ __launch_bounds__(256) void sw2d_quad4_stage_kernel(const Quad4Params pp) {
    using Q = Quad4Elem<N>;
    constexpr int Nq = Q::Nq, Np = Q::Np, NFN = Q::NFN, E = Q::E, T = Q::THREADS;
    __shared__ double lds[Q::LDS_DOUBLES];
    double* const D1 = lds;
    double* const l0 = lds + Nq * Nq;
    double* const lN = l0 + Nq;
    double* const fl = lds + Q::OFF_FL;
    double* const spd = lds + Q::OFF_SPD;
    double* const surf = lds + Q::OFF_SURF;

    const QuadParams& p = pp.q;
    const int tid = threadIdx.x;
    const int k0 = p.kBegin + static_cast<int>(blockIdx.x) * E;
    const long long ld = p.ld;
    const long long plane = static_cast<long long>(Np) * ld;
    const double g = p.g;

    for (int i = tid; i < Q::OPS_DOUBLES; i += T) lds[i] = p.ops[i];

    // Phase C visits the node items of phase A again. Where its item loop is unrolled, the sources are formed in phase A, from
    // the state and the velocities that are in registers there, and carried across (2 doubles per item); where it stays rolled
    // (N = 7, 8 unfiltered) they are formed in phase C from a second read of the node. Above N = 8 the tile has 8 elements and
    // a thread at most 6 items: with sources the loop is unrolled again and the sources come from phase A (rolled, with the
    // sources formed in it, these instances took 256 VGPRs and 188-256 AGPRs, and scratch at N = 11, 12; unrolled 132-240, none).
    constexpr int kUnrollC = N <= 6 || FILT || (SRC && N > 8) ? Q::NI : 1;
    constexpr bool kSrcEarly = SRC && kUnrollC == Q::NI;
    double src2[kSrcEarly ? Q::NI : 1], src3[kSrcEarly ? Q::NI : 1];

    // ---- A: volume fluxes of the own state (flux.py)
#pragma unroll
    for (int m = 0; m < Q::NI; ++m) {
        const int idx = tid + T * m;
        if (kSrcEarly) src2[m] = src3[m] = 0.0;
        if (idx < Np * E) {
            const int n = idx / E, e = idx % E, k = k0 + e;
            double h = 1.0, hu = 0.0, hv = 0.0, hN = 0.0;
            if (k < p.kEnd) {
                const long long o = n * ld + k;
                h = p.qin[o];
                hu = p.qin[plane + o];
                hv = p.qin[2 * plane + o];
                hN = p.qin[3 * plane + o];
            }
            const double u = hu / h, v = hv / h, ph = 0.5 * g * h * h;
            if (kSrcEarly && k < p.kEnd) sources4(pp, n * ld + k, h, hu, hv, u, v, src2[m], src3[m]);
            fl[(0 * Np + n) * E + e] = hu;
            fl[(1 * Np + n) * E + e] = hv;
            fl[(2 * Np + n) * E + e] = hu * u + ph;
            fl[(3 * Np + n) * E + e] = hu * v;
            fl[(4 * Np + n) * E + e] = hv * u;
            fl[(5 * Np + n) * E + e] = hv * v + ph;
            fl[(6 * Np + n) * E + e] = hN * u;
            fl[(7 * Np + n) * E + e] = hN * v;
        }
    }

    // ---- B: traces (rhs.py:204-256), node speeds
    double jt[Q::FI][4], jq[Q::FI][4], fs[Q::FI];
#pragma unroll
    for (int m = 0; m < Q::FI; ++m) {
        const int idx = tid + T * m;
#pragma unroll
        for (int c = 0; c < 4; ++c) jt[m][c] = jq[m][c] = 0.0;
        fs[m] = 0.0;
        if (idx < NFN * E) {
            const int fn = idx / E, e = idx % E, k = k0 + e;
            double lam = 0.0;
            if (k < p.kEnd) {
                const int f = fn / Nq, nn = fn % Nq;
                const long long oM = Q::fmask(f, nn) * ld + k;
                const double hM = p.qin[oM], hNM = p.qin[3 * plane + oM];
                double uM = p.qin[plane + oM] / hM, vM = p.qin[2 * plane + oM] / hM;
                const int gi = p.gidx[fn * ld + k];
                const bool wall = gi < 0;
                const long long oP = wall ? -(static_cast<long long>(gi) + 1) : gi;
                const double hP = p.qin[oP], hNP = p.qin[3 * plane + oP];
                double uP = p.qin[plane + oP] / hP, vP = p.qin[2 * plane + oP] / hP;
                double nx, ny;
                if (GEN) {
                    nx = p.fgeo[fn * ld + k];
                    ny = p.fgeo[(NFN + fn) * ld + k];
                    fs[m] = p.fgeo[(2 * NFN + fn) * ld + k];
                } else {
                    nx = p.ageo[(4 + f) * ld + k];
                    ny = p.ageo[(8 + f) * ld + k];
                    fs[m] = p.ageo[(12 + f) * ld + k];
                }
                const double huM = hM * uM, hvM = hM * vM;
                double huP = hP * uP, hvP = hP * vP;
                if (wall) {
                    const double un = huM * nx + hvM * ny;
                    huP = huM - 2 * nx * un;
                    hvP = hvM - 2 * ny * un;
                }
                uM = huM / hM; vM = hvM / hM;
                uP = huP / hP; vP = hvP / hP;
                const double phM = 0.5 * g * hM * hM, phP = 0.5 * g * hP * hP;
                const double F2M = huM * uM + phM, G2M = huM * vM, F3M = hvM * uM, G3M = hvM * vM + phM;
                const double F2P = huP * uP + phP, G2P = huP * vP, F3P = hvP * uP, G3P = hvP * vP + phP;
                jt[m][0] = (huM - huP) * nx + (hvM - hvP) * ny;
                jt[m][1] = (F2M - F2P) * nx + (G2M - G2P) * ny;
                jt[m][2] = (F3M - F3P) * nx + (G3M - G3P) * ny;
                jt[m][3] = (hNM * uM - hNP * uP) * nx + (hNM * vM - hNP * vP) * ny;
                jq[m][0] = hM - hP;
                jq[m][1] = huM - huP;
                jq[m][2] = hvM - hvP;
                jq[m][3] = hNM - hNP;
                const double sM = sqrt(uM * uM + vM * vM) + sqrt(g * hM);
                const double sP = sqrt(uP * uP + vP * vP) + sqrt(g * hP);
                lam = sM > sP ? sM : sP;
            }
            spd[fn * E + e] = lam;
        }
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < Q::FI; ++m) {
        const int idx = tid + T * m;
        if (idx < NFN * E) {
            const int fn = idx / E, e = idx % E, f = fn / Nq;
            double lam = spd[(f * Nq) * E + e];
#pragma unroll
            for (int n2 = 1; n2 < Nq; ++n2) {
                const double s2 = spd[(f * Nq + n2) * E + e];
                lam = s2 > lam ? s2 : lam;
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) surf[(c * NFN + fn) * E + e] = fs[m] * (0.5 * (jt[m][c] - lam * jq[m][c]));
        }
    }
    __syncthreads();

    // ---- C: volume + surface terms and sources; unfiltered modes update right away, filtered ones keep the rows for the
    // filter. Above N = 6 the item loop stays rolled, as in the three-field kernel.
    double r[FILT ? Q::NI : 1][4];
#pragma unroll kUnrollC
    for (int m = 0; m < Q::NI; ++m) {
        const int idx = tid + T * m;
        if (FILT) r[m][0] = r[m][1] = r[m][2] = r[m][3] = 0.0;
        if (idx < Np * E) {
            const int n = idx / E, e = idx % E, k = k0 + e;
            const int j = n / Nq, i = n % Nq;
            double rx, sx, ry, sy;
            const int kk = k < p.kEnd ? k : p.kBegin;
            if (GEN) {
                rx = p.geo[n * ld + kk];
                sx = p.geo[plane + n * ld + kk];
                ry = p.geo[2 * plane + n * ld + kk];
                sy = p.geo[3 * plane + n * ld + kk];
            } else {
                rx = p.ageo[kk];
                sx = p.ageo[ld + kk];
                ry = p.ageo[2 * ld + kk];
                sy = p.ageo[3 * ld + kk];
            }
            const double a0 = l0[i], a1 = lN[j], a2 = lN[i], a3 = l0[j];
            const int s0 = j * E + e, s1 = (Nq + i) * E + e, s2 = (2 * Nq + j) * E + e, s3 = (3 * Nq + i) * E + e;
            double v[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) { // equation c: F = plane 2c, G = plane 2c + 1
                double fr = 0.0, fs2 = 0.0, gr = 0.0, gs = 0.0;
#pragma unroll
                for (int q = 0; q < Nq; ++q) {
                    const double dj = D1[j * Nq + q], di = D1[i * Nq + q];
                    fr += dj * fl[(2 * c * Np + q * Nq + i) * E + e];
                    fs2 += di * fl[(2 * c * Np + j * Nq + q) * E + e];
                    gr += dj * fl[((2 * c + 1) * Np + q * Nq + i) * E + e];
                    gs += di * fl[((2 * c + 1) * Np + j * Nq + q) * E + e];
                }
                v[c] = -(rx * fr + sx * fs2) - (ry * gr + sy * gs);
                const int sc = c * NFN * E;
                v[c] += a0 * surf[sc + s0] + a1 * surf[sc + s1] + a2 * surf[sc + s2] + a3 * surf[sc + s3];
            }
            if (kSrcEarly) {
                v[1] += src2[m];
                v[2] += src3[m];
            } else if (SRC) {
                const long long o = n * ld + kk;
                const double h = p.qin[o], hu = fl[(0 * Np + n) * E + e], hv = fl[(1 * Np + n) * E + e];
                double s2, s3;
                sources4(pp, o, h, hu, hv, hu / h, hv / h, s2, s3);
                v[1] += s2;
                v[2] += s3;
            }
            if (FILT) {
#pragma unroll
                for (int c = 0; c < 4; ++c) r[m][c] = v[c];
            } else if (k < p.kEnd) {
                store4<MODE>(p, n * ld + k, plane, v);
            }
        }
    }

    if (FILT) {
        __syncthreads(); // every derivative read of fl is done
#pragma unroll
        for (int m = 0; m < Q::NI; ++m) {
            const int idx = tid + T * m;
            if (idx < Np * E) {
                const int n = idx / E, e = idx % E;
#pragma unroll
                for (int c = 0; c < 4; ++c) fl[(c * Np + n) * E + e] = r[m][c];
            }
        }
        __syncthreads();
    }
    // Above N = 8 a filtered row goes from the LDS planes straight into the stage update, as in the three-field kernel.
    constexpr bool kFiltStream = FILT && N > 8;
    if (kFiltStream) {
#pragma unroll 1
        for (int m = 0; m < Q::NI; ++m) {
            const int idx = tid + T * m;
            if (idx >= Np * E) break;
            const int n = idx / E, e = idx % E, k = k0 + e;
            double a[4] = {0.0, 0.0, 0.0, 0.0};
            for (int q = 0; q < Np; ++q) {
                const double w = p.filt[n * Np + q];
#pragma unroll
                for (int c = 0; c < 4; ++c) a[c] += w * fl[(c * Np + q) * E + e];
            }
            if (k < p.kEnd) store4<MODE>(p, n * ld + k, plane, a);
        }
    } else if (FILT) {
#pragma unroll
        for (int m = 0; m < Q::NI; ++m) {
            const int idx = tid + T * m;
            if (idx < Np * E) {
                const int n = idx / E, e = idx % E;
                double a[4] = {0.0, 0.0, 0.0, 0.0};
                for (int q = 0; q < Np; ++q) {
                    const double w = p.filt[n * Np + q];
#pragma unroll
                    for (int c = 0; c < 4; ++c) a[c] += w * fl[(c * Np + q) * E + e];
                }
#pragma unroll
                for (int c = 0; c < 4; ++c) r[m][c] = a[c];
            }
        }
#pragma unroll
        for (int m = 0; m < Q::NI; ++m) {
            const int idx = tid + T * m;
            if (idx >= Np * E) continue;
            const int n = idx / E, e = idx % E, k = k0 + e;
            if (k < p.kEnd) store4<MODE>(p, n * ld + k, plane, r[m]);
        }
    }
}

// one order's launcher (sw2d_quad_order.hip, -DBDG_ORDER=N)
template <int N>
hipError_t sw2d_quad4_launch(int mode, bool filter, bool general, bool sources, const Quad4Params& p, hipStream_t stream);

hipError_t sw2d_quad4_stage(int order, int mode, bool filter, bool general, bool sources, const Quad4Params& p,
                            hipStream_t stream);

} // namespace bdg_dev
