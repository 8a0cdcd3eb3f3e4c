// sw2d_quad_kernel.hpp -- HIP kernel (gfx950 / CDNA4, wave64) for the shallow-water nodal DG right-hand side on
// quadrilaterals, fused with the Runge-Kutta stage update. Device restatement of the reference script's
// sw2dComputeRHS (sw2dquads.py:24-133: local Lax-Friedrichs flux with one speed per face, reflective walls on
// BCmap[3], strong form) and of its midpoint-RK2 + filter loop body (:183-207); LSERK4 stages as the triangle path.
//
// The tensor structure of the Gauss-Lobatto element is used instead of dense operators:
//   Dr = D1 (x) I, Ds = I (x) D1      -> 2 (N+1) multiply-adds per node and differentiated array, not 2 Np;
//   Lift: face f is the identity along the face times one column (l0 or lN) of the inverse 1-D mass matrix
//                                     -> 4 multiply-adds per node and field, not 4 Nfp.
// Node (N+1) j + i sits at r = r1d[j], s = s1d[i]; faces are s=-1 (i = 0), r=+1 (j = N), s=+1 (i = N), r=-1 (j = 0).
//
// Mapping to the hardware: one 256-thread workgroup owns a tile of E consecutive elements (E = 64 / 32 / 16 for
// N = 1 / 2 / 3..8, so every access to one nodal row of a tile is a contiguous run of E doubles, >= 128 bytes; E = 8 for
// N = 9..12, 64-byte runs, which keeps two or three workgroups on a CU where a tile of 16 leaves one: DESIGN section 3.8) of the
// element range [kBegin, kEnd): tile kBegin + blockIdx.x * E, one workgroup per tile (a single domain evaluates [0, K); a
// partitioned run its interior and partition-boundary ranges, never its ghosts). Three phases, separated by workgroup barriers:
//   A  node items (n, e): load h, hu, hv, write hu, hv, F2, G2, G3 to LDS;
//   B  face-node items (f, n, e): own trace and neighbour trace (gathered through vmapP; the wall flag rides in the sign
//      bit of the gather index), node speeds to LDS, barrier, per-face maximum speed, lifted flux jump * Fscale to LDS;
//   C  node items: tensor derivatives of the five flux arrays from LDS, metric terms, the four face lifts, then
//      (optionally) the dense Np x Np filter through LDS, and the stage update.
// Geometry: GEN = true reads per-node rx..sy and per-face-node nx, ny, Fscale (any bilinear quadrilateral);
// GEN = false reads 16 constants per element (parallelograms: rx, sx, ry, sy, then nx, ny, Fscale of each face).
#pragma once
#include <hip/hip_runtime.h>

namespace bdg_dev {

template <int N>
struct QuadElem {
    static constexpr int Nq = N + 1;
    static constexpr int Np = Nq * Nq;
    static constexpr int NFN = 4 * Nq;
    static constexpr int E = N == 1 ? 64 : (N == 2 ? 32 : (N <= 8 ? 16 : 8)); // elements per workgroup tile
    static constexpr int THREADS = 256;
    static constexpr int NI = (Np * E + THREADS - 1) / THREADS;  // node items per thread
    static constexpr int FI = (NFN * E + THREADS - 1) / THREADS; // face-node items per thread
    // ops image (global and LDS): D1 (Nq x Nq) | l0 (Nq) | lN (Nq)
    static constexpr int OPS_DOUBLES = Nq * Nq + 2 * Nq;
    // LDS in doubles: ops | 5 flux arrays [a][n][e] (reused for the filtered RHS) | speeds [fn][e] | surface [c][fn][e]
    static constexpr int OFF_FL = OPS_DOUBLES;
    static constexpr int OFF_SPD = OFF_FL + 5 * Np * E;
    static constexpr int OFF_SURF = OFF_SPD + NFN * E;
    static constexpr int LDS_DOUBLES = OFF_SURF + 3 * NFN * E;
    __host__ __device__ static constexpr int fmask(int f, int n) {
        return f == 0 ? Nq * n : (f == 1 ? Nq * N + n : (f == 2 ? Nq * n + N : n));
    }
};

enum QuadMode {
    QMODE_RHS = 0,     // rhs = [Filter] R(qin)
    QMODE_COMBINE = 1, // qout = qbase + cc [Filter] R(qin)            (midpoint RK2 predictor / corrector)
    QMODE_LSERK = 2,   // res = ca res + cc R(qin); qout = qin + cb res
    QMODE_HEUN = 3     // variant B only (sw2d_quadb_kernel.hpp): qout = sp(ca qbase + cb qin + cc [Filter] R(qin))
};

struct QuadParams {
    const double* qin;   // 3 planes of Np*ld: h, hu, hv
    const double* qbase; // QMODE_COMBINE
    double* qout;        // QMODE_COMBINE / QMODE_LSERK (never qin in QMODE_LSERK: neighbours still read it)
    double* res;         // QMODE_LSERK: 3 planes, in place
    double* rhs;         // QMODE_RHS: 3 planes
    const double* geo;   // GEN: rx, sx, ry, sy, 4 planes of Np*ld
    const double* fgeo;  // GEN: nx, ny, Fscale, 3 planes of NFN*ld
    const double* ageo;  // !GEN: 16 planes of ld
    const int* gidx;     // NFN*ld: neighbour trace offset n'*ld + k', wall nodes as -(offset + 1)
    const double* ops;   // QuadElem<N>::OPS_DOUBLES
    const double* filt;  // Np x Np, row-major (filtered modes)
    long long ld;        // plane stride (multiple of 64)
    int kBegin, kEnd;    // the elements evaluated; every other column is only read, as a neighbour
    double g, ca, cb, cc;
};

// the stage update of one node (offset o in plane 0) from its right-hand side (v1, v2, v3)
template <int MODE>
__device__ __forceinline__ void store(const QuadParams& p, long long o, long long plane, double v1, double v2, double v3) {
    if (MODE == QMODE_RHS) {
        p.rhs[o] = v1;
        p.rhs[plane + o] = v2;
        p.rhs[2 * plane + o] = v3;
    } else if (MODE == QMODE_COMBINE) {
        p.qout[o] = p.qbase[o] + p.cc * v1;
        p.qout[plane + o] = p.qbase[plane + o] + p.cc * v2;
        p.qout[2 * plane + o] = p.qbase[2 * plane + o] + p.cc * v3;
    } else {
        const double a = p.ca * p.res[o] + p.cc * v1;
        const double b = p.ca * p.res[plane + o] + p.cc * v2;
        const double c = p.ca * p.res[2 * plane + o] + p.cc * v3;
        p.res[o] = a;
        p.res[plane + o] = b;
        p.res[2 * plane + o] = c;
        // own state again (read in phase A a few microseconds earlier: an L2 hit, not HBM traffic)
        p.qout[o] = p.qin[o] + p.cb * a;
        p.qout[plane + o] = p.qin[plane + o] + p.cb * b;
        p.qout[2 * plane + o] = p.qin[2 * plane + o] + p.cb * c;
    }
}

template <int N, int MODE, bool FILT, bool GEN>
__global__ __launch_bounds__(256) void sw2d_quad_stage_kernel(const QuadParams p) {
    using Q = QuadElem<N>;
    constexpr int Nq = Q::Nq, Np = Q::Np, NFN = Q::NFN, E = Q::E, T = Q::THREADS;
    __shared__ double lds[Q::LDS_DOUBLES];
    double* const D1 = lds;
    double* const l0 = lds + Nq * Nq;
    double* const lN = l0 + Nq;
    double* const fl = lds + Q::OFF_FL;
    double* const spd = lds + Q::OFF_SPD;
    double* const surf = lds + Q::OFF_SURF;

    const int tid = threadIdx.x;
    const int k0 = p.kBegin + static_cast<int>(blockIdx.x) * E;
    const long long ld = p.ld;
    const long long plane = static_cast<long long>(Np) * ld;
    const double g = p.g;

    for (int i = tid; i < Q::OPS_DOUBLES; i += T) lds[i] = p.ops[i];

    // ---- A: volume fluxes of the own state
#pragma unroll
    for (int m = 0; m < Q::NI; ++m) {
        const int idx = tid + T * m;
        if (idx < Np * E) {
            const int n = idx / E, e = idx % E, k = k0 + e;
            double h = 1.0, hu = 0.0, hv = 0.0;
            if (k < p.kEnd) {
                const long long o = n * ld + k;
                h = p.qin[o];
                hu = p.qin[plane + o];
                hv = p.qin[2 * plane + o];
            }
            const double ph = 0.5 * g * h * h;
            fl[(0 * Np + n) * E + e] = hu;
            fl[(1 * Np + n) * E + e] = hv;
            fl[(2 * Np + n) * E + e] = (hu * hu) / h + ph;
            fl[(3 * Np + n) * E + e] = (hu * hv) / h;
            fl[(4 * Np + n) * E + e] = (hv * hv) / h + ph;
        }
    }

    // ---- B: traces, node speeds
    double jt[Q::FI][3], jq[Q::FI][3], fs[Q::FI];
#pragma unroll
    for (int m = 0; m < Q::FI; ++m) {
        const int idx = tid + T * m;
        jt[m][0] = jt[m][1] = jt[m][2] = 0.0;
        jq[m][0] = jq[m][1] = jq[m][2] = 0.0;
        fs[m] = 0.0;
        if (idx < NFN * E) {
            const int fn = idx / E, e = idx % E, k = k0 + e;
            double lam = 0.0;
            if (k < p.kEnd) {
                const int f = fn / Nq, nn = fn % Nq;
                const long long oM = Q::fmask(f, nn) * ld + k;
                const double hM = p.qin[oM], huM = p.qin[plane + oM], hvM = p.qin[2 * plane + oM];
                const int gi = p.gidx[fn * ld + k];
                const bool wall = gi < 0;
                const long long oP = wall ? -(static_cast<long long>(gi) + 1) : gi;
                const double hP = p.qin[oP];
                double huP = p.qin[plane + oP], hvP = p.qin[2 * plane + oP];
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
                if (wall) {
                    const double un = huM * nx + hvM * ny;
                    huP = huM - 2 * nx * un;
                    hvP = hvM - 2 * ny * un;
                }
                const double phM = 0.5 * g * hM * hM, phP = 0.5 * g * hP * hP;
                const double F2M = (huM * huM) / hM + phM, G2M = (huM * hvM) / hM, G3M = (hvM * hvM) / hM + phM;
                const double F2P = (huP * huP) / hP + phP, G2P = (huP * hvP) / hP, G3P = (hvP * hvP) / hP + phP;
                jt[m][0] = (huM - huP) * nx + (hvM - hvP) * ny;
                jt[m][1] = (F2M - F2P) * nx + (G2M - G2P) * ny;
                jt[m][2] = (G2M - G2P) * nx + (G3M - G3P) * ny;
                jq[m][0] = hM - hP;
                jq[m][1] = huM - huP;
                jq[m][2] = hvM - hvP;
                const double uM = huM / hM, vM = hvM / hM, uP = huP / hP, vP = hvP / hP;
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
            for (int c = 0; c < 3; ++c) surf[(c * NFN + fn) * E + e] = fs[m] * (0.5 * (jt[m][c] - lam * jq[m][c]));
        }
    }
    __syncthreads();

    // ---- C: volume + surface terms; unfiltered modes update right away, filtered ones keep the rows for the filter.
    // Above N = 6 the item loop stays rolled: unrolled, its derivative sums need more than 256 VGPRs.
    constexpr int kUnrollC = N <= 6 || FILT ? Q::NI : 1;
    double r1[FILT ? Q::NI : 1], r2[FILT ? Q::NI : 1], r3[FILT ? Q::NI : 1];
#pragma unroll kUnrollC
    for (int m = 0; m < Q::NI; ++m) {
        const int idx = tid + T * m;
        if (FILT) r1[m] = r2[m] = r3[m] = 0.0;
        if (idx < Np * E) {
            const int n = idx / E, e = idx % E, k = k0 + e;
            const int j = n / Nq, i = n % Nq;
            double dr[5], ds[5];
#pragma unroll
            for (int a = 0; a < 5; ++a) {
                double sr = 0.0, ss = 0.0;
#pragma unroll
                for (int q = 0; q < Nq; ++q) {
                    sr += D1[j * Nq + q] * fl[(a * Np + q * Nq + i) * E + e];
                    ss += D1[i * Nq + q] * fl[(a * Np + j * Nq + q) * E + e];
                }
                dr[a] = sr;
                ds[a] = ss;
            }
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
            double v1 = -(rx * dr[0] + sx * ds[0]) - (ry * dr[1] + sy * ds[1]);
            double v2 = -(rx * dr[2] + sx * ds[2]) - (ry * dr[3] + sy * ds[3]);
            double v3 = -(rx * dr[3] + sx * ds[3]) - (ry * dr[4] + sy * ds[4]);
            const double a0 = l0[i], a1 = lN[j], a2 = lN[i], a3 = l0[j];
            const int s0 = j * E + e, s1 = (Nq + i) * E + e, s2 = (2 * Nq + j) * E + e, s3 = (3 * Nq + i) * E + e;
            v1 += a0 * surf[s0] + a1 * surf[s1] + a2 * surf[s2] + a3 * surf[s3];
            v2 += a0 * surf[NFN * E + s0] + a1 * surf[NFN * E + s1] + a2 * surf[NFN * E + s2] + a3 * surf[NFN * E + s3];
            v3 += a0 * surf[2 * NFN * E + s0] + a1 * surf[2 * NFN * E + s1] + a2 * surf[2 * NFN * E + s2] +
                  a3 * surf[2 * NFN * E + s3];
            if (FILT) {
                r1[m] = v1; r2[m] = v2; r3[m] = v3;
            } else if (k < p.kEnd) {
                store<MODE>(p, n * ld + k, plane, v1, v2, v3);
            }
        }
    }

    // Above N = 8 a filtered row goes from the LDS planes straight into the stage update, one item at a time, instead of
    // waiting in registers until every row of the thread is filtered.
    constexpr bool kFiltStream = FILT && N > 8;
    if (FILT) {
        __syncthreads(); // every derivative read of fl is done
#pragma unroll
        for (int m = 0; m < Q::NI; ++m) {
            const int idx = tid + T * m;
            if (idx < Np * E) {
                const int n = idx / E, e = idx % E;
                fl[(0 * Np + n) * E + e] = r1[m];
                fl[(1 * Np + n) * E + e] = r2[m];
                fl[(2 * Np + n) * E + e] = r3[m];
            }
        }
        __syncthreads();
    }
    if (kFiltStream) {
#pragma unroll 1
        for (int m = 0; m < Q::NI; ++m) {
            const int idx = tid + T * m;
            if (idx >= Np * E) break;
            const int n = idx / E, e = idx % E, k = k0 + e;
            double a = 0.0, b = 0.0, c = 0.0;
            for (int q = 0; q < Np; ++q) {
                const double w = p.filt[n * Np + q];
                a += w * fl[(0 * Np + q) * E + e];
                b += w * fl[(1 * Np + q) * E + e];
                c += w * fl[(2 * Np + q) * E + e];
            }
            if (k < p.kEnd) store<MODE>(p, n * ld + k, plane, a, b, c);
        }
    } else if (FILT) {
#pragma unroll
        for (int m = 0; m < Q::NI; ++m) {
            const int idx = tid + T * m;
            if (idx < Np * E) {
                const int n = idx / E, e = idx % E;
                double a = 0.0, b = 0.0, c = 0.0;
                for (int q = 0; q < Np; ++q) {
                    const double w = p.filt[n * Np + q];
                    a += w * fl[(0 * Np + q) * E + e];
                    b += w * fl[(1 * Np + q) * E + e];
                    c += w * fl[(2 * Np + q) * E + e];
                }
                r1[m] = a; r2[m] = b; r3[m] = c;
            }
        }
    }

    if (FILT && !kFiltStream) {
#pragma unroll
        for (int m = 0; m < Q::NI; ++m) {
            const int idx = tid + T * m;
            if (idx >= Np * E) continue;
            const int n = idx / E, e = idx % E, k = k0 + e;
            if (k < p.kEnd) store<MODE>(p, n * ld + k, plane, r1[m], r2[m], r3[m]);
        }
    }
}

// one order's launcher (sw2d_quad_order.hip, -DBDG_ORDER=N)
template <int N>
hipError_t sw2d_quad_launch(int mode, bool filter, bool general, const QuadParams& p, hipStream_t stream);

hipError_t sw2d_quad_stage(int order, int mode, bool filter, bool general, const QuadParams& p, hipStream_t stream);
int sw2d_quad_tile(int order); // E of QuadElem<order>

} // namespace bdg_dev
