// sw2d_quadb4_kernel.hpp -- variant B of the quadrilateral sw2d right-hand side with a passive tracer hN as a fourth field
// (gfx950 / CDNA4, wave64): sw2d_quadb_stage_kernel (sw2d_quadb_kernel.hpp: tidal physics, star states, one global speed read
// from device memory, Heun store with the sponge) with one more equation. The reference's tidal driver has no tracer; the
// definition is tests/quadrefB4.py. Components 1 to 3 are computed by the statements of sw2d_quadb_stage_kernel. The fourth:
//   B  the concentrations come from the depths BEFORE the star states: NM = hNM / hM, NP = hNP / hP; a wall node takes
//      NP = NM, an open-boundary node NP = Nopen (it wins where a node is both, as hP does). The star tracer is
//      hNM* = hM* NM, hNP* = hP* NP: a true rescale, unlike the momentum lines whose rescale is an identity, so that a uniform
//      concentration stays uniform over a discontinuous bed. F4 = (hN* hu) / h*, G4 = (hN* hv) / h* in the form of G2, the
//      same global speed (the tracer does not enter it: sw2d_quadb_speed_kernel runs unchanged on the first three planes);
//   C  div((hN hu) / h, (hN hv) / h) as a fourth flux pair through the same D1 contractions, no source term.
// Nopen is a scalar, or one value per open-boundary node: the host sorts the open nodes' gather-index positions fn * ld + k
// into openKey with their values beside them in openN, and an open node finds its slot by binary search (only open nodes
// search; there is no per-face-node plane). The gather index is variant B's image with INT_MIN on open nodes.
// LDS: ops | 7 flux arrays | 4 surface arrays: 33 KB at N = 4, 92 KB at N = 8, 91 KB at N = 12 (tiles of 8), below the
// 107 / 103 KB of sw2d_quad4_stage_kernel there, one workgroup per CU from N = 7 on in both; DESIGN section 3.8 has the table.
// It lives beside sw2d_quadb_kernel.hpp so that the three-field instances are compiled from unchanged text.
#pragma once
#include "sw2d_quadb_kernel.hpp"

namespace bdg_dev {

template <int N>
struct QuadB4Elem : QuadElem<N> {
    using Q = QuadElem<N>;
    static constexpr int NFLUX = 7; // hu, hv, F2, G2, G3, F4, G4
    // LDS in doubles: ops | 7 flux arrays [a][n][e] (reused for the filtered RHS) | surface [c][fn][e]
    static constexpr int OFF_SURF = Q::OFF_FL + NFLUX * Q::Np * Q::E;
    static constexpr int LDS_DOUBLES = OFF_SURF + 4 * Q::NFN * Q::E;
    // Filtered instances above N = 6 put the unfiltered rows into four LDS planes of their own [c][n][e] instead of carrying them
    // in registers across an unrolled item loop (which spilled at N = 7, 8, 11, 12): 107 KB at N = 7, 133 KB at N = 8, 134 KB at N = 12
    static constexpr bool FILT_LDS = N > 6;
    static constexpr int OFF_ROWS = LDS_DOUBLES;
    static constexpr int LDS_DOUBLES_FILT = LDS_DOUBLES + (FILT_LDS ? 4 * Q::Np * Q::E : 0);
};

struct QuadB4Params {
    QuadBParams b;            // every state / residual / rhs buffer with 4 planes: h, hu, hv, hN
    const long long* openKey; // numOpen sorted positions fn * ld + k of the open-boundary nodes, or nullptr: nOpenC everywhere
    const double* openN;      // numOpen concentrations, in the order of openKey
    int numOpen;
    double nOpenC;
};

// the concentration an open-boundary node at gather-index position `key` takes on its '+' side
__device__ __forceinline__ double quadb4_open(const QuadB4Params& pp, long long key) {
    if (!pp.openKey) return pp.nOpenC;
    int lo = 0, hi = pp.numOpen;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (pp.openKey[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return pp.openN[lo < pp.numOpen ? lo : pp.numOpen - 1]; // (every open node is in the table: the clamp is never taken)
}

// the stage update of one node (offset o in plane 0) from its right-hand side v[0..3]; hN is updated like h
template <int MODE>
__device__ __forceinline__ void storeB4(const QuadBParams& pb, long long o, long long plane, const double (&v)[4]) {
    const QuadParams& p = pb.q;
    if (MODE == QMODE_HEUN) {
        const double sc = pb.sponge ? pb.sponge[o] : pb.spongeC;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const long long oc = c * plane + o;
            const double a = p.ca * p.qbase[oc] + p.cb * p.qin[oc] + p.cc * v[c];
            p.qout[oc] = (c == 1 || c == 2) ? a / (1.0 + sc * a * a) : a;
        }
        return;
    }
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

template <int N, int MODE, bool FILT, bool GEN>
__global__ __launch_bounds__(256) void sw2d_quadb4_stage_kernel(const QuadB4Params pp) {
    using Q = QuadB4Elem<N>;
    constexpr int Nq = Q::Nq, Np = Q::Np, NFN = Q::NFN, E = Q::E, T = Q::THREADS, NFLUX = Q::NFLUX;
    constexpr bool kFiltLds = FILT && Q::FILT_LDS;
    __shared__ double lds[FILT ? Q::LDS_DOUBLES_FILT : Q::LDS_DOUBLES];
    double* const D1 = lds;
    double* const l0 = lds + Nq * Nq;
    double* const lN = l0 + Nq;
    double* const fl = lds + Q::OFF_FL;
    double* const surf = lds + Q::OFF_SURF;
    const QuadBParams& pb = pp.b;
    const QuadParams& p = pb.q;

    const int tid = threadIdx.x;
    const int k0 = p.kBegin + static_cast<int>(blockIdx.x) * E;
    const long long ld = p.ld;
    const long long plane = static_cast<long long>(Np) * ld;
    const double g = p.g;
    const double lam = *pb.lam;

    for (int i = tid; i < Q::OPS_DOUBLES; i += T) lds[i] = p.ops[i];

    // ---- A: volume fluxes of the own state
#pragma unroll
    for (int m = 0; m < Q::NI; ++m) {
        const int idx = tid + T * m;
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
            const double ph = 0.5 * g * h * h;
            fl[(0 * Np + n) * E + e] = hu;
            fl[(1 * Np + n) * E + e] = hv;
            fl[(2 * Np + n) * E + e] = (hu * hu) / h + ph;
            fl[(3 * Np + n) * E + e] = (hu * hv) / h;
            fl[(4 * Np + n) * E + e] = (hv * hv) / h + ph;
            fl[(5 * Np + n) * E + e] = (hN * hu) / h;
            fl[(6 * Np + n) * E + e] = (hN * hv) / h;
        }
    }

    // ---- B: traces with boundary conditions and star states, lifted flux jump * Fscale to LDS
#pragma unroll
    for (int m = 0; m < Q::FI; ++m) {
        const int idx = tid + T * m;
        if (idx < NFN * E) {
            const int fn = idx / E, e = idx % E, k = k0 + e;
            double s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;
            if (k < p.kEnd) {
                const int f = fn / Nq, nn = fn % Nq;
                const long long oM = Q::fmask(f, nn) * ld + k;
                const int gi = p.gidx[fn * ld + k];
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
                const QuadBTrace t = quadb_trace(p.qin, pb.H, plane, oM, gi, nx, ny, pb.tide, false);
                // concentrations from the depths before the star states (the loads repeat quadb_trace's: same addresses)
                const double NM = p.qin[3 * plane + oM] / p.qin[oM];
                double NP;
                if (gi == kQuadBOpen) {
                    NP = quadb4_open(pp, fn * ld + k);
                } else if (gi < 0) {
                    NP = NM;
                } else {
                    NP = p.qin[3 * plane + gi] / p.qin[gi];
                }
                const double hNM = t.hM * NM, hNP = t.hP * NP;
                const double phM = 0.5 * g * t.hM * t.hM, phP = 0.5 * g * t.hP * t.hP;
                const double F2M = (t.huM * t.huM) / t.hM + phM, G2M = (t.huM * t.hvM) / t.hM, G3M = (t.hvM * t.hvM) / t.hM + phM;
                const double F2P = (t.huP * t.huP) / t.hP + phP, G2P = (t.huP * t.hvP) / t.hP, G3P = (t.hvP * t.hvP) / t.hP + phP;
                const double F4M = (hNM * t.huM) / t.hM, G4M = (hNM * t.hvM) / t.hM;
                const double F4P = (hNP * t.huP) / t.hP, G4P = (hNP * t.hvP) / t.hP;
                const double hfs = 0.5 * fs;
                s1 = hfs * ((t.huM - t.huP) * nx + (t.hvM - t.hvP) * ny - lam * (t.hM - t.hP));
                s2 = hfs * ((F2M - F2P) * nx + (G2M - G2P) * ny - lam * (t.huM - t.huP));
                s3 = hfs * ((G2M - G2P) * nx + (G3M - G3P) * ny - lam * (t.hvM - t.hvP));
                s4 = hfs * ((F4M - F4P) * nx + (G4M - G4P) * ny - lam * (hNM - hNP));
            }
            surf[(0 * NFN + fn) * E + e] = s1;
            surf[(1 * NFN + fn) * E + e] = s2;
            surf[(2 * NFN + fn) * E + e] = s3;
            surf[(3 * NFN + fn) * E + e] = s4;
        }
    }
    __syncthreads();

    // ---- C: volume + surface + source terms; unfiltered modes update right away, filtered ones keep the rows for the
    // filter. Above N = 6 the item loop stays rolled, as in sw2d_quadb_stage_kernel.
    constexpr int kUnrollC = N <= 6 ? Q::NI : 1;
    constexpr int kUnrollA = N <= 8 ? NFLUX : 1; // (the flux-array loop rolled above N = 8: unrolled, N = 12 spilled)
    double* const rows = kFiltLds ? lds + Q::OFF_ROWS : fl;
    double r[FILT && !kFiltLds ? Q::NI : 1][4];
#pragma unroll kUnrollC
    for (int m = 0; m < Q::NI; ++m) {
        const int idx = tid + T * m;
        if (FILT && !kFiltLds) r[m][0] = r[m][1] = r[m][2] = r[m][3] = 0.0;
        if (idx < Np * E) {
            const int n = idx / E, e = idx % E, k = k0 + e;
            const int j = n / Nq, i = n % Nq;
            double rx, sx, ry, sy;
            const int kk = k < p.kEnd ? k : p.kBegin;
            const long long o = n * ld + kk;
            if (GEN) {
                rx = p.geo[o];
                sx = p.geo[plane + o];
                ry = p.geo[2 * plane + o];
                sy = p.geo[3 * plane + o];
            } else {
                rx = p.ageo[kk];
                sx = p.ageo[ld + kk];
                ry = p.ageo[2 * ld + kk];
                sy = p.ageo[3 * ld + kk];
            }
            // one flux array at a time, each derivative folded into its equations at once (G2 enters two), which keeps the
            // live values at two accumulators and four sums: with all fourteen derivatives formed first, the filtered
            // instances of N = 7, 8, 11, 12 spilled to scratch
            double v[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll kUnrollA
            for (int a = 0; a < NFLUX; ++a) {
                double sr = 0.0, ss = 0.0;
#pragma unroll
                for (int q = 0; q < Nq; ++q) {
                    sr += D1[j * Nq + q] * fl[(a * Np + q * Nq + i) * E + e];
                    ss += D1[i * Nq + q] * fl[(a * Np + j * Nq + q) * E + e];
                }
                const double dx = rx * sr + sx * ss, dy = ry * sr + sy * ss;
                // hu -> x of eq 1; hv -> y of eq 1; F2 -> x of eq 2; G2 -> y of eq 2 and x of eq 3; G3 -> y of eq 3; F4, G4 -> eq 4
                if (a == 0) v[0] -= dx;
                if (a == 1) v[0] -= dy;
                if (a == 2) v[1] -= dx;
                if (a == 3) { v[1] -= dy; v[2] -= dx; }
                if (a == 4) v[2] -= dy;
                if (a == 5) v[3] -= dx;
                if (a == 6) v[3] -= dy;
            }
            const double a0 = l0[i], a1 = lN[j], a2 = lN[i], a3 = l0[j];
            const int s0 = j * E + e, s1 = (Nq + i) * E + e, s2 = (2 * Nq + j) * E + e, s3 = (3 * Nq + i) * E + e;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int sc = c * NFN * E;
                v[c] += a0 * surf[sc + s0] + a1 * surf[sc + s1] + a2 * surf[sc + s2] + a3 * surf[sc + s3];
            }
            // sources of the momentum equations, as sw2d_quadb_stage_kernel forms them; the tracer has none. A padding
            // column reads element kBegin's h and Hx, its rows are never stored
            {
                const double h = p.qin[o], hu = fl[(0 * Np + n) * E + e], hv = fl[(1 * Np + n) * E + e];
                const double u = hu / h, w = hv / h;
                const double nrm = sqrt(u * u + w * w);
                v[1] += g * h * pb.Hx[o] - pb.cd * u * nrm + pb.fcor * hv;
                v[2] += g * h * pb.Hy[o] - pb.cd * w * nrm - pb.fcor * hu;
            }
            if (kFiltLds) {
#pragma unroll
                for (int c = 0; c < 4; ++c) rows[(c * Np + n) * E + e] = v[c];
            } else if (FILT) {
#pragma unroll
                for (int c = 0; c < 4; ++c) r[m][c] = v[c];
            } else if (k < p.kEnd) {
                storeB4<MODE>(pb, n * ld + k, plane, v);
            }
        }
    }

    // Up to N = 6 the rows go from registers into the flux planes once every derivative read of those is done; above, they are in
    // their own planes already and go from there straight into the stage update (one barrier, not two).
    constexpr bool kFiltStream = kFiltLds;
    if (kFiltLds) {
        __syncthreads();
    } else if (FILT) {
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
    if (kFiltStream) {
#pragma unroll 1
        for (int m = 0; m < Q::NI; ++m) {
            const int idx = tid + T * m;
            if (idx >= Np * E) break;
            const int n = idx / E, e = idx % E, k = k0 + e;
            double a[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4 // (left to the compiler, the 64 rows of N = 7 were unrolled whole and the Heun instance spilled)
            for (int q = 0; q < Np; ++q) {
                const double w = p.filt[n * Np + q];
#pragma unroll
                for (int c = 0; c < 4; ++c) a[c] += w * rows[(c * Np + q) * E + e];
            }
            if (k < p.kEnd) storeB4<MODE>(pb, n * ld + k, plane, a);
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
            if (k < p.kEnd) storeB4<MODE>(pb, n * ld + k, plane, r[m]);
        }
    }
}

// one order's launcher (sw2d_quadb4_order.hip, -DBDG_ORDER=N)
template <int N>
hipError_t sw2d_quadb4_launch(int mode, bool filter, bool general, const QuadB4Params& p, hipStream_t stream);

hipError_t sw2d_quadb4_stage(int order, int mode, bool filter, bool general, const QuadB4Params& p, hipStream_t stream); // sw2d_quad_device.hip

} // namespace bdg_dev
