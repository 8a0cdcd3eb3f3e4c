// sw2d_curved_driver_kernel.hpp -- what the curved solver's driver does after its RK2 + filter step (gfx950 / CDNA4, wave64;
// reference sw2d_curved.py:231-302): the adaptive time step with its blow-up check, and the six output fields
// eta = h - H, u = hu / h, v = hv / h, B = hN / h, h and the vorticity
//   vort = (rx (Dr v) + sx (Ds v)) - (ry (Dr u) + sy (Ds u))
// on per-node geometry, optionally interpolated to each element's equispaced lattice (the (Np, Np) matrix IM of
// TriangleNodesProvisioner::splitOperators) before they leave the device.
//
// Np is a run-time argument, as in sw2d_monitor_kernel.hpp: the dt kernels serve the orders 1 to 8 with one instance each, the
// output kernel with one per LDS size class (MAXNP = 15, 28, 45: orders up to 4, 6, 8), and only sw2d_curved_device.hip includes
// this header. The state is q[(field Np + node) ld + element], ld a multiple of 64 and lane = element, so every load and store
// is a whole 512-byte row. The tile-order list of the nodal-trace form is a visiting order, not a renumbering: these kernels
// ignore it. Elements >= count (ghost elements of a partitioned run, the padding up to ld) are neither read nor written.
//
// ---- the dt pass: sw2d_curved_dt_kernel (a grid of 256-thread workgroups, one element per thread), then
// sw2d_curved_dt_finish_kernel (one workgroup). Per element and face entry j of the 3 Nfp, with n_j the face-node list:
//   u = hu[n_j] / h[n_j], v = hv[n_j] / h[n_j],  val = (fac |Fscale[j]|) (c[n_j] + sqrt(u u + v v)),  fac = (N+1)^2 0.5
// in exactly that association, contraction off, division and square root the correctly rounded ones: val equals the NumPy
// expression of sw2d_curved.py:281 on the downloaded state bit for bit, and a maximum does not depend on its order. Over all
// Np nodes: max|h| and a count of the NaNs of h; a NaN val is counted too (fmax drops NaNs). The workgroup's three partials
// (speed maximum, max|h|, NaN count) are combined through LDS in the tree a[t] op= a[t + s], s = 128 .. 1; the finish kernel
// combines the workgroups' partials the same way and stores three doubles. No floating-point atomics.
//
// ---- the output step: sw2d_curved_output_kernel, one launch for all requested fields. A workgroup of four waves owns 64
// consecutive elements; the state is read from HBM once (the lattice instance asks for h, hN and H a second time when it stages
// eta, B and h: rows the same workgroup read microseconds earlier).
//   1. The waves split the nodes (node n to wave n mod 4): h, hu, hv (hN, H as wanted) are read, u and v formed once and
//      staged in LDS as [node][lane] (2 MAXNP 512 bytes: 46 KB at N = 8, 15 KB up to N = 4, so that the low orders keep eight
//      waves per SIMD; consecutive lanes, consecutive doubles: conflict-free).
//      Without a lattice the five pointwise fields are stored here: h - H, hu / h, hv / h, hN / h, h of the downloaded state
//      bit for bit.
//   2. The waves split the output rows (row i to wave i mod 4). For row i a lane keeps four accumulators
//        Dr v = sum_m Dr[i, m] v[m],  Ds v,  Dr u,  Ds u   (and, with a lattice, sum_m IM[i, m] u[m] and ... v[m])
//      over m = 0 .. Np - 1 in ascending order from 0.0, acc = acc + a f (one multiply, one add, no contraction), u and v read
//      back from LDS, the matrix entries through wave-uniform addresses (scalar loads). Then
//        vort = (rx drv + sx dsv) - (ry dru + sy dsu)
//      with the four metric values of (node i, element) -- every product and sum rounded once, in that association.
//   3. With a lattice the nodal values go through LDS a second time (as in sw2d_quad_output_kernel.hpp): the nodal vorticity
//      rows a wave formed (at most ceil(MAXNP / 4) = 12: registers, indexed at compile time) replace u once every wave is done
//      with it, eta replaces v, and the rows out[i] = sum_m IM[i, m] f[m] are formed as above; then B and h likewise.
// A lane holds O(1) accumulators per row whatever the order, the row loops are run-time loops, and nothing is indexed
// dynamically: no scratch at any order. Static LDS: 2 MAXNP 512 bytes. The four metric values of a row are requested before its
// sums are formed, and the node loop of step 1 is unrolled, so that the loads of several rows are in flight together.
#pragma once
#include <hip/hip_runtime.h>

namespace bdg_dev {

constexpr int kCurvedDrvThreads = 256;
constexpr int kCurvedDrvMaxNp = 45;                         // order 8
constexpr int kCurvedOutWaves = 4;
// the LDS size class of the output kernel that serves Np nodes
constexpr int curvedOutClass(int Np) { return Np <= 15 ? 15 : (Np <= 28 ? 28 : kCurvedDrvMaxNp); }

struct CurvedDtParams {
    const double* q;        // the state: h, hu, hv planes of Np*ld (the tracer plane is not read)
    const double* fscale;   // (3 Nfp, ld)
    const double* c;        // (Np, ld), or NULL: cConst
    const int* faceNodes;   // 3 Nfp local node indices
    long long ld;
    int Np, nFace, count;
    double cConst, fac;     // fac = (N+1)^2 0.5
};

// max / max / sum of the three partials of a workgroup, through LDS; the result is in red[.][0]
__device__ inline void curvedDtTree(double (*red)[kCurvedDrvThreads], int t) {
    for (int s = kCurvedDrvThreads / 2; s > 0; s >>= 1) {
        if (t < s) {
            red[0][t] = fmax(red[0][t], red[0][t + s]);
            red[1][t] = fmax(red[1][t], red[1][t + s]);
            red[2][t] = red[2][t] + red[2][t + s];
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kCurvedDrvThreads) void sw2d_curved_dt_kernel(CurvedDtParams p, double* __restrict__ partials) {
#pragma clang fp contract(off)
    __shared__ double red[3][kCurvedDrvThreads];
    const int t = threadIdx.x, Np = p.Np;
    const long long ld = p.ld, plane = static_cast<long long>(Np) * ld;
    const long long k = static_cast<long long>(blockIdx.x) * kCurvedDrvThreads + t;
    const double* __restrict__ q = p.q;
    const double* __restrict__ fs = p.fscale;
    const double* __restrict__ c = p.c;
    double smax = 0.0, hmax = 0.0, nn = 0.0;
    if (k < p.count) {
#pragma unroll 4
        for (int n = 0; n < Np; ++n) {
            const double h = q[n * ld + k];
            hmax = fmax(hmax, fabs(h));
            nn += h != h ? 1.0 : 0.0;
        }
#pragma unroll 2
        for (int j = 0; j < p.nFace; ++j) {
            const long long o = p.faceNodes[j] * ld + k;
            const double h = q[o], u = q[plane + o] / h, v = q[2 * plane + o] / h;
            const double cc = c ? c[o] : p.cConst;
            const double val = (p.fac * fabs(fs[j * ld + k])) * (cc + sqrt(u * u + v * v));
            nn += val != val ? 1.0 : 0.0;
            smax = fmax(smax, val);
        }
    }
    red[0][t] = smax; red[1][t] = hmax; red[2][t] = nn;
    __syncthreads();
    curvedDtTree(red, t);
    if (t < 3) partials[3 * blockIdx.x + t] = red[t][0];
}

// out[0] = speed maximum, out[1] = max|h|, out[2] = NaN count
__global__ __launch_bounds__(kCurvedDrvThreads) void sw2d_curved_dt_finish_kernel(const double* __restrict__ partials, int nblocks,
                                                                                  double* __restrict__ out) {
    __shared__ double red[3][kCurvedDrvThreads];
    const int t = threadIdx.x;
    double smax = 0.0, hmax = 0.0, nn = 0.0;
    for (int b = t; b < nblocks; b += kCurvedDrvThreads) {
        smax = fmax(smax, partials[3 * b]);
        hmax = fmax(hmax, partials[3 * b + 1]);
        nn = nn + partials[3 * b + 2];
    }
    red[0][t] = smax; red[1][t] = hmax; red[2][t] = nn;
    __syncthreads();
    curvedDtTree(red, t);
    if (t < 3) out[t] = red[t][0];
}

struct CurvedOutParams {
    const double* q;                    // the state: four planes of Np*ld
    const double* H;                    // Np*ld, or NULL: eta = h
    const double *Dr, *Ds;              // (Np, Np) row-major
    const double *rx, *sx, *ry, *sy;    // Np*ld each
    const double* IM;                   // (Np, Np) row-major (LAT instance only)
    double* out;                        // plane c receives field c of (eta, u, v, B, h, vort)
    long long ld;
    int Np, count;                      // the elements [0, count) are written
    int mask;                           // bit c: field c is wanted
};

enum { CURVED_OUT_ETA = 0, CURVED_OUT_U, CURVED_OUT_V, CURVED_OUT_B, CURVED_OUT_H, CURVED_OUT_VORT, CURVED_OUT_FIELDS };

// rows i = w, w + 4, ... of IM applied to the nodal planes A -> field fa and B -> field fb (either unwanted: skipped)
__device__ inline void curvedOutLattice(const CurvedOutParams& p, const double* A, const double* B, int fa, int fb, int w, int e,
                                        long long k, bool live) {
#pragma clang fp contract(off)
    const int Np = p.Np;
    const long long plane = static_cast<long long>(Np) * p.ld;
    const bool wa = (p.mask >> fa) & 1, wb = (p.mask >> fb) & 1;
    if (!wa && !wb) return;
    for (int i = w; i < Np; i += kCurvedOutWaves) {
        const double* __restrict__ row = p.IM + i * Np;
        double a = 0.0, b = 0.0;
#pragma unroll 4
        for (int m = 0; m < Np; ++m) {
            const double x = row[m];
            a = a + x * A[m * 64 + e];
            b = b + x * B[m * 64 + e];
        }
        if (live) {
            if (wa) p.out[fa * plane + i * p.ld + k] = a;
            if (wb) p.out[fb * plane + i * p.ld + k] = b;
        }
    }
}

template <bool LAT, int MAXNP>
__global__ __launch_bounds__(64 * kCurvedOutWaves) void sw2d_curved_output_kernel(CurvedOutParams p) {
#pragma clang fp contract(off)
    constexpr int kRows = (MAXNP + kCurvedOutWaves - 1) / kCurvedOutWaves; // rows of a wave
    __shared__ double U[MAXNP * 64], V[MAXNP * 64];
    const int e = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)); // wave-uniform: rows by scalar loads
    const int Np = p.Np, mask = p.mask;
    const long long ld = p.ld, plane = static_cast<long long>(Np) * ld;
    const long long k = static_cast<long long>(blockIdx.x) * 64 + e;
    const bool live = k < p.count;
    const double* __restrict__ q = p.q;
    const double* __restrict__ H = p.H;
    double* __restrict__ out = p.out;
    const bool wEta = (mask >> CURVED_OUT_ETA) & 1, wU = (mask >> CURVED_OUT_U) & 1, wV = (mask >> CURVED_OUT_V) & 1;
    const bool wB = (mask >> CURVED_OUT_B) & 1, wH = (mask >> CURVED_OUT_H) & 1, wVort = (mask >> CURVED_OUT_VORT) & 1;

    // 1. u and v, once, to LDS; without a lattice the pointwise fields leave here
#pragma unroll 4
    for (int n = w; n < Np; n += kCurvedOutWaves) {
        const long long o = n * ld + k;
        const double h = live ? q[o] : 1.0;
        const double u = live ? q[plane + o] / h : 0.0, v = live ? q[2 * plane + o] / h : 0.0;
        U[n * 64 + e] = u;
        V[n * 64 + e] = v;
        if (!LAT && live) {
            if (wEta) out[CURVED_OUT_ETA * plane + o] = H ? h - H[o] : h;
            if (wU) out[CURVED_OUT_U * plane + o] = u;
            if (wV) out[CURVED_OUT_V * plane + o] = v;
            if (wB) out[CURVED_OUT_B * plane + o] = q[3 * plane + o] / h;
            if (wH) out[CURVED_OUT_H * plane + o] = h;
        }
    }
    __syncthreads();

    // 2. the derivative rows (with a lattice: the rows of u and v too)
    double vn[kRows];
    if (wVort || (LAT && (wU || wV))) {
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            const int i = w + kCurvedOutWaves * r;
            vn[r] = 0.0;
            if (i >= Np) continue; // (uniform over the wave)
            const double* __restrict__ dr = p.Dr + i * Np;
            const double* __restrict__ ds = p.Ds + i * Np;
            const long long o = i * ld + k;
            const bool geo = wVort && live;
            const double rx = geo ? p.rx[o] : 0.0, sx = geo ? p.sx[o] : 0.0, ry = geo ? p.ry[o] : 0.0, sy = geo ? p.sy[o] : 0.0;
            double drv = 0.0, dsv = 0.0, dru = 0.0, dsu = 0.0, lu = 0.0, lv = 0.0;
#pragma unroll 4
            for (int m = 0; m < Np; ++m) {
                const double u = U[m * 64 + e], v = V[m * 64 + e], a = dr[m], b = ds[m];
                drv = drv + a * v;
                dsv = dsv + b * v;
                dru = dru + a * u;
                dsu = dsu + b * u;
                if (LAT) {
                    const double x = p.IM[i * Np + m];
                    lu = lu + x * u;
                    lv = lv + x * v;
                }
            }
            if (wVort) {
                vn[r] = (rx * drv + sx * dsv) - (ry * dru + sy * dsu);
                if (!LAT && live) out[CURVED_OUT_VORT * plane + o] = vn[r];
            }
            if (LAT && live) {
                if (wU) out[CURVED_OUT_U * plane + o] = lu;
                if (wV) out[CURVED_OUT_V * plane + o] = lv;
            }
        }
    }
    if (!LAT) return;

    // 3. the other fields through LDS a second time: vort and eta, then B and h
    if (wVort || wEta) {
        __syncthreads(); // every wave is done with u and v
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            const int i = w + kCurvedOutWaves * r;
            if (i >= Np) continue;
            const long long o = i * ld + k;
            const double h = live ? q[o] : 1.0;
            U[i * 64 + e] = vn[r];
            V[i * 64 + e] = (H && live) ? h - H[o] : h;
        }
        __syncthreads();
        curvedOutLattice(p, U, V, CURVED_OUT_VORT, CURVED_OUT_ETA, w, e, k, live);
    }
    if (wB || wH) {
        __syncthreads();
        for (int n = w; n < Np; n += kCurvedOutWaves) {
            const long long o = n * ld + k;
            const double h = live ? q[o] : 1.0;
            U[n * 64 + e] = live ? q[3 * plane + o] / h : 0.0;
            V[n * 64 + e] = h;
        }
        __syncthreads();
        curvedOutLattice(p, U, V, CURVED_OUT_B, CURVED_OUT_H, w, e, k, live);
    }
}

} // namespace bdg_dev
