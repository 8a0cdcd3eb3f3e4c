// sw2d_quadb_kernel.hpp -- "variant B" of the quadrilateral sw2d right-hand side (gfx950 / CDNA4, wave64): the physics of
// the reference's tidal driver, src/sw2d/main.cpp:279-484 computeRHS, on the tile / three-phase structure and the tensor
// operators D1, l0, lN of sw2d_quad_stage_kernel (sw2d_quad_kernel.hpp), three fields. Against that kernel:
//   B  gathers the still-water depth H on both sides of every face node; wall nodes take hP = hM and the reflected momentum
//      (:340-345), open-boundary nodes huP = huM, hvP = hvM, hP = HM + tide (:348-353, the tide value formed by the host once
//      per evaluation); star states (:359-368); ONE Lax-Friedrichs speed for the whole mesh, read from device memory (:414),
//      so the per-face speed plane in LDS and its barrier are gone;
//   C  adds g h Hx - CD u|u| + f hv to RHS2 and g h Hy - CD v|u| - f hu to RHS3 (:461-483), before the filter;
//   a Heun store qout = sp(ca qbase + cb qin + cc R), sp(x) = x / (1 + c x^2) on hu and hv (:218-236), c an (Np, K) array or
//      a scalar: both halves of the driver's SSP-RK2 step, the sponge fused into the stage store.
// The gather index is a second image of gidx in which an open-boundary node is INT_MIN: no other entry has that value (wall
// nodes are -(offset + 1) >= -(2^31 - 1)), its '+' trace is formed from the own trace alone, and the gather stays one load.
// Quirks kept, as sw2d_vb_kernel.hpp keeps them: hM is overwritten by hMstar before the momentum rescale (:366-368), so the
// rescale is hMstar * (huM / hMstar) (NaN for a dry star state) and the hydrostatic correction of :420-421,
// 1/2 g hM^2 - 1/2 g hMstar^2 with hM = hMstar already, is identically zero: it is not formed here.
// sw2d_quadb_speed_kernel is the speed pass: max over the face nodes of the elements [kBegin, kEnd) of the '-' side's speed,
// and of the '+' side's where it is formed locally (wall and open-boundary nodes). An interior node's '+' speed is the
// neighbour's '-' speed at the same node (the star formulas are symmetric in bM, bP), so the maximum over all elements is
// max(spdM, spdP) of :400-414, on a partition without current ghosts as well.
#pragma once
#include "sw2d_quad_kernel.hpp"
#include <climits>

namespace bdg_dev {

constexpr int kQuadBOpen = INT_MIN; // gather-index value of an open-boundary node

template <int N>
struct QuadBElem : QuadElem<N> {
    // LDS in doubles: ops | 5 flux arrays [a][n][e] (reused for the filtered RHS) | surface [c][fn][e]
    static constexpr int OFF_SURF = QuadElem<N>::OFF_FL + 5 * QuadElem<N>::Np * QuadElem<N>::E;
    static constexpr int LDS_DOUBLES = OFF_SURF + 3 * QuadElem<N>::NFN * QuadElem<N>::E;
};

struct QuadBParams {
    QuadParams q;         // gidx: the image with open-boundary nodes; ca, cb, cc also of QMODE_HEUN
    const double* H;      // (Np, ld) still-water depth
    const double* Hx;     // (Np, ld) bed slopes as the driver builds them (main.cpp:128-133)
    const double* Hy;
    const double* lam;    // device scalar: the global speed of this evaluation
    const double* sponge; // QMODE_HEUN: (Np, ld) sponge coefficient, or nullptr for the scalar
    double spongeC;
    double tide;          // open-boundary elevation of this evaluation
    double fcor, cd;
};

// '-' and '+' traces of one face node after boundary conditions and star states (:336-368)
struct QuadBTrace {
    double hM, huM, hvM, hP, huP, hvP;
};

__device__ __forceinline__ QuadBTrace quadb_trace(const double* __restrict__ qin, const double* __restrict__ H, long long plane,
                                                  long long oM, int gi, double nx, double ny, double tide, bool local) {
    // local: form only what this element's own columns and H give (speed pass): an interior node's '+' side repeats its '-' side
    const bool open = gi == kQuadBOpen, wall = gi < 0 && !open;
    const long long oP = gi >= 0 ? gi : (open ? oM : -(static_cast<long long>(gi) + 1));
    const double hM = qin[oM], huM = qin[plane + oM], hvM = qin[2 * plane + oM];
    const double HM = H[oM], HP = H[oP];
    double hP, huP, hvP;
    if (open) {
        hP = HM + tide;
        huP = huM;
        hvP = hvM;
    } else if (wall) {
        const double un = huM * nx + hvM * ny;
        hP = hM;
        huP = huM - 2 * nx * un;
        hvP = hvM - 2 * ny * un;
    } else if (local) {
        hP = hM;
        huP = huM;
        hvP = hvM;
    } else {
        hP = qin[oP];
        huP = qin[plane + oP];
        hvP = qin[2 * plane + oP];
    }
    const double bM = -HM, bP = -HP, mx = bP > bM ? bP : bM;
    const double hMs = fmax(0.0, hM + bM - mx);
    const double hPs = (local && gi >= 0) ? hMs : fmax(0.0, hP + bP - mx); // (local, interior: the '-' star state again)
    QuadBTrace t;
    t.hM = hMs;
    t.hP = hPs;
    t.huM = hMs * (huM / hMs); // hMstar*(huM/hM) with hM already = hMstar
    t.hvM = hMs * (hvM / hMs);
    t.huP = hPs * (huP / hPs);
    t.hvP = hPs * (hvP / hPs);
    return t;
}

// the stage update of one node (offset o in plane 0) from its right-hand side (v1, v2, v3)
template <int MODE>
__device__ __forceinline__ void storeB(const QuadBParams& pb, long long o, long long plane, double v1, double v2, double v3) {
    if (MODE == QMODE_HEUN) {
        const QuadParams& p = pb.q;
        const double a = p.ca * p.qbase[o] + p.cb * p.qin[o] + p.cc * v1;
        const double b = p.ca * p.qbase[plane + o] + p.cb * p.qin[plane + o] + p.cc * v2;
        const double c = p.ca * p.qbase[2 * plane + o] + p.cb * p.qin[2 * plane + o] + p.cc * v3;
        const double sc = pb.sponge ? pb.sponge[o] : pb.spongeC;
        p.qout[o] = a;
        p.qout[plane + o] = b / (1.0 + sc * b * b);
        p.qout[2 * plane + o] = c / (1.0 + sc * c * c);
    } else {
        store<MODE>(pb.q, o, plane, v1, v2, v3);
    }
}

template <int N, int MODE, bool FILT, bool GEN>
__global__ __launch_bounds__(256) void sw2d_quadb_stage_kernel(const QuadBParams pb) {
    using Q = QuadBElem<N>;
    constexpr int Nq = Q::Nq, Np = Q::Np, NFN = Q::NFN, E = Q::E, T = Q::THREADS;
    __shared__ double lds[Q::LDS_DOUBLES];
    double* const D1 = lds;
    double* const l0 = lds + Nq * Nq;
    double* const lN = l0 + Nq;
    double* const fl = lds + Q::OFF_FL;
    double* const surf = lds + Q::OFF_SURF;
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

    // ---- B: traces with boundary conditions and star states, lifted flux jump * Fscale to LDS
#pragma unroll
    for (int m = 0; m < Q::FI; ++m) {
        const int idx = tid + T * m;
        if (idx < NFN * E) {
            const int fn = idx / E, e = idx % E, k = k0 + e;
            double s1 = 0.0, s2 = 0.0, s3 = 0.0;
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
                const double phM = 0.5 * g * t.hM * t.hM, phP = 0.5 * g * t.hP * t.hP;
                const double F2M = (t.huM * t.huM) / t.hM + phM, G2M = (t.huM * t.hvM) / t.hM, G3M = (t.hvM * t.hvM) / t.hM + phM;
                const double F2P = (t.huP * t.huP) / t.hP + phP, G2P = (t.huP * t.hvP) / t.hP, G3P = (t.hvP * t.hvP) / t.hP + phP;
                const double hfs = 0.5 * fs;
                s1 = hfs * ((t.huM - t.huP) * nx + (t.hvM - t.hvP) * ny - lam * (t.hM - t.hP));
                s2 = hfs * ((F2M - F2P) * nx + (G2M - G2P) * ny - lam * (t.huM - t.huP));
                s3 = hfs * ((G2M - G2P) * nx + (G3M - G3P) * ny - lam * (t.hvM - t.hvP));
            }
            surf[(0 * NFN + fn) * E + e] = s1;
            surf[(1 * NFN + fn) * E + e] = s2;
            surf[(2 * NFN + fn) * E + e] = s3;
        }
    }
    __syncthreads();

    // ---- C: volume + surface + source terms; unfiltered modes update right away, filtered ones keep the rows for the
    // filter. Above N = 6 the item loop stays rolled, as in sw2d_quad_stage_kernel.
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
            double v1 = -(rx * dr[0] + sx * ds[0]) - (ry * dr[1] + sy * ds[1]);
            double v2 = -(rx * dr[2] + sx * ds[2]) - (ry * dr[3] + sy * ds[3]);
            double v3 = -(rx * dr[3] + sx * ds[3]) - (ry * dr[4] + sy * ds[4]);
            const double a0 = l0[i], a1 = lN[j], a2 = lN[i], a3 = l0[j];
            const int s0 = j * E + e, s1 = (Nq + i) * E + e, s2 = (2 * Nq + j) * E + e, s3 = (3 * Nq + i) * E + e;
            v1 += a0 * surf[s0] + a1 * surf[s1] + a2 * surf[s2] + a3 * surf[s3];
            v2 += a0 * surf[NFN * E + s0] + a1 * surf[NFN * E + s1] + a2 * surf[NFN * E + s2] + a3 * surf[NFN * E + s3];
            v3 += a0 * surf[2 * NFN * E + s0] + a1 * surf[2 * NFN * E + s1] + a2 * surf[2 * NFN * E + s2] +
                  a3 * surf[2 * NFN * E + s3];
            // sources: hu, hv are still in the flux planes, h comes from a second read of the node (an L2 hit); a padding
            // column reads element kBegin's h and Hx, its rows are never stored
            {
                const double h = p.qin[o], hu = fl[(0 * Np + n) * E + e], hv = fl[(1 * Np + n) * E + e];
                const double u = hu / h, v = hv / h;
                const double nrm = sqrt(u * u + v * v);
                v2 += g * h * pb.Hx[o] - pb.cd * u * nrm + pb.fcor * hv;
                v3 += g * h * pb.Hy[o] - pb.cd * v * nrm - pb.fcor * hu;
            }
            if (FILT) {
                r1[m] = v1; r2[m] = v2; r3[m] = v3;
            } else if (k < p.kEnd) {
                storeB<MODE>(pb, n * ld + k, plane, v1, v2, v3);
            }
        }
    }

    // Above N = 8 a filtered row goes from the LDS planes straight into the stage update (sw2d_quad_stage_kernel).
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
            if (k < p.kEnd) storeB<MODE>(pb, n * ld + k, plane, a, b, c);
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
            if (k < p.kEnd) storeB<MODE>(pb, n * ld + k, plane, r1[m], r2[m], r3[m]);
        }
    }
}

// ---- the speed pass: one grid-stride loop over the face nodes of [kBegin, kEnd); out: bit pattern of the maximum, merged
// by an atomic maximum per workgroup (speeds are non-negative doubles, whose bit patterns order as they do; a NaN goes in
// as the positive quiet NaN, above every number, so it stays). The caller zeroes *out first.
template <bool GEN>
__global__ __launch_bounds__(256) void sw2d_quadb_speed_kernel(const QuadBParams pb, int N, unsigned long long* out) {
    const QuadParams& p = pb.q;
    const int Nq = N + 1, Np = Nq * Nq, NFN = 4 * Nq, cols = p.kEnd - p.kBegin;
    const long long ld = p.ld, plane = static_cast<long long>(Np) * ld, total = static_cast<long long>(NFN) * cols;
    const double g = p.g;
    double best = 0.0;
    bool bad = false;
    for (long long it = blockIdx.x * 256LL + threadIdx.x; it < total; it += 256LL * gridDim.x) {
        const int fn = static_cast<int>(it / cols), k = p.kBegin + static_cast<int>(it % cols), f = fn / Nq, nn = fn % Nq;
        const int node = f == 0 ? Nq * nn : (f == 1 ? Nq * N + nn : (f == 2 ? Nq * nn + N : nn));
        const long long oM = node * ld + k;
        const int gi = p.gidx[fn * ld + k];
        double nx, ny;
        if (GEN) {
            nx = p.fgeo[fn * ld + k];
            ny = p.fgeo[(NFN + fn) * ld + k];
        } else {
            nx = p.ageo[(4 + f) * ld + k];
            ny = p.ageo[(8 + f) * ld + k];
        }
        const QuadBTrace t = quadb_trace(p.qin, pb.H, plane, oM, gi, nx, ny, pb.tide, true);
        const double uM = t.huM / t.hM, vM = t.hvM / t.hM, uP = t.huP / t.hP, vP = t.hvP / t.hP;
        const double spdM = sqrt(uM * uM + vM * vM) + sqrt(g * t.hM);
        const double spdP = sqrt(uP * uP + vP * vP) + sqrt(g * t.hP);
        if (spdM != spdM || spdP != spdP) bad = true;
        best = fmax(best, fmax(spdM, spdP));
    }
    __shared__ double smax[256];
    __shared__ int sBad;
    if (threadIdx.x == 0) sBad = 0;
    __syncthreads();
    if (bad) sBad = 1;
    smax[threadIdx.x] = best;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (static_cast<int>(threadIdx.x) < s) smax[threadIdx.x] = fmax(smax[threadIdx.x], smax[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const unsigned long long bits = sBad ? 0x7ff8000000000000ULL : static_cast<unsigned long long>(__double_as_longlong(smax[0]));
        atomicMax(out, bits);
    }
}

// one order's launcher (sw2d_quadb_order.hip, -DBDG_ORDER=N)
template <int N>
hipError_t sw2d_quadb_launch(int mode, bool filter, bool general, const QuadBParams& p, hipStream_t stream);

hipError_t sw2d_quadb_stage(int order, int mode, bool filter, bool general, const QuadBParams& p, hipStream_t stream);
// the speed pass of [p.q.kBegin, p.q.kEnd) into *out (zeroed first, on the stream); both in sw2d_quad_device.hip
hipError_t sw2d_quadb_speed(int order, bool general, const QuadBParams& p, double* out, hipStream_t stream);

} // namespace bdg_dev
