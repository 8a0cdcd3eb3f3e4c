// sw2d_curved_drifter_kernel.hpp -- Lagrangian drifters on triangle meshes with curved elements (gfx950 / CDNA4, wave64): points
// that move with the velocity (hu / h, hv / h) of the resident state, are followed from element to element -- through curved
// elements and along curved walls -- and recorded, all on the device. The launch, its modes, the Heun advance, the status bits
// and the records are those of sw2d_drifter_driver.hpp; the straight-sided elements, the basis and the velocity are those of
// sw2d_drifter_kernel.hpp; this file adds the elements whose nodal map is not affine: their tables, the init map and locate.
//
//   sw2d_curved_drifter_kernel   the driver's body with the policy CurvedTriDrift
//
// The order is a run-time argument: one instance serves N = 1..8. The kernel reads the state planes 0..2 in the layout
// q[node * ld + element] and the tables below, and writes only the drifter arrays and the record buffer. Nothing here names a
// solver: the tables are plain arrays (bdg_trinodes_curved_drifter_tables).
//
// Tables. tri: vert, neigh, vinvT, jac of sw2d_drifter_kernel.hpp; vert of a listed element holds its corner NODES (the ends of
// its curved faces). curvedSlot[k]: -1 for a straight-sided element, else the element's row c in `modal`.
// modal[(6 c + p) Np + m], p = 0..5: the modal coefficients (nodal values multiplied by Vinv) of the six planes x, y, Dr x,
// Ds x, Dr y, Ds y of the element. With P_m the basis values at (r, s) (triDriftBasis), each of
//   X, Y, Xr, Xs, Yr, Ys = sum_m P_m modal[(6 c + p) Np + m],  ascending m from 0.0, no contraction
// is the nodal map and its Jacobian at (r, s); the derivative planes lie in P^N, so this is exact.
//
// init(k, r, s): on a listed element (X, Y) of (r, s); else the affine map of sw2d_drifter_kernel.hpp.
//
// locate(x, y, k): at most kTriDriftHops hops; (wk, wf), the first wall face the search crossed, is shared by both kinds of
// element. An element with curvedSlot < 0 takes the hop of sw2d_drifter_kernel.hpp (closed-form inverse, straight-wall
// projection, corner rule) unchanged. In a listed element, per hop:
//   1. (r, s) = the closed-form inverse of the affine map of the corner triangle (as on straight elements); not finite: lost.
//      Both are clipped to [-1.5, 1.5].
//   2. Newton on the modal map, at most kCurvedDriftNewton iterations: det = Xr Ys - Xs Yr at the iterate; a determinant that is
//      not positive and finite ends the iteration with step = inf; with (fx, fy) = (x - X, y - Y),
//        dr = (Ys fx - Xs fy) / det,  ds = (Xr fy - Yr fx) / det;
//      a dr or ds that is not finite ends the iteration with step = inf; the new iterate is r + dr, s + ds, each clipped to
//      [-1.5, 1.5]; step = max(|r_new - r|, |s_new - s|) (the clipped step); the iteration stops at step <= 1e-14.
//      "Converged" means the last step <= 1e-10.
//   3. The violations of the faces 0..2 are (-1 - s, r + s, -1 - r). The largest <= 1e-12: found in k if converged, else lost.
//   4. Otherwise the face f of the largest (lowest index on a tie) is crossed; an unconverged iterate serves for this choice:
//      to the neighbour; at an open face the drifter has exited.
//   5. At a wall an unconverged search loses the drifter. A converged one: if an earlier wall crossing of this search was at
//      another face (another element or another face index than the FIRST wall face of the search), the point goes to the end
//      vertex of face f that is nearer to it (|p - a|^2 <= |p - b|^2: a; a -> b the face's vertices in vert), the corner rule of
//      sw2d_drifter_kernel.hpp. Else face 0 sets s = -1, face 2 sets r = -1, face 1 subtracts 0.5 (r + s) from both, and
//      (x, y) = (X, Y) of the new (r, s): the point lies on the curved wall. The wall bit is set and the same element is searched
//      again (the drifter slides along the wall).
// Hops used up: lost.
//
// The basis values of a lane live in LDS, sb[m][lane], as in sw2d_drifter_kernel.hpp; locate and init use the same column the
// velocity uses afterwards. The modal coefficients are per-lane 8-byte gathers, 6 Np per Newton iteration (2 Np in init and at a
// wall); no atomics, vector stores only.
#pragma once
#include "sw2d_drifter_kernel.hpp"

namespace bdg_dev {

constexpr int kCurvedDriftNewton = 12;
constexpr double kCurvedDriftClip = 1.5;

struct CurvedTriDriftTables {
    TriDriftTables tri;
    const int* curvedSlot;  // per element: -1 or the row in modal
    const double* modal;    // (rows, 6, Np)
    int N;                  // the order (DriftParams::N, which init and locate do not see)
};

// sum_m P_m c[m], ascending from 0.0
__device__ inline double curvedDriftSum(const double* __restrict__ c, int Np, const double* P) {
#pragma clang fp contract(off)
    double a = 0.0;
    for (int m = 0; m < Np; ++m) a = a + P[m * kDriftThreads] * c[m];
    return a;
}

// (X, Y) of the listed element with the coefficient block c at (r, s)
__device__ inline void curvedDriftMap(const double* __restrict__ jac, const double* __restrict__ c, int N, double r, double s,
                                      double* P, double& X, double& Y) {
    const int Np = (N + 1) * (N + 2) / 2;
    triDriftBasis(jac, N, r, s, P);
    X = curvedDriftSum(c, Np, P);
    Y = curvedDriftSum(c + Np, Np, P);
}

__device__ inline double curvedDriftClipped(double v) { return v > kCurvedDriftClip ? kCurvedDriftClip : (v < -kCurvedDriftClip ? -kCurvedDriftClip : v); }

// one hop of locate in the listed element k with the coefficient block c; the results of triDriftHop
__device__ inline int curvedDriftHop(const TriDriftTables& tab, const double* __restrict__ c, int N, double& x, double& y, int& k,
                                     double& r, double& s, double* P, int& wall, int& wk, int& wf) {
#pragma clang fp contract(off)
    const int Np = (N + 1) * (N + 2) / 2;
    const double* v = tab.vert + 8LL * k;
    const double x0 = v[0], y0 = v[1], x1 = v[2], y1 = v[3], x2 = v[4], y2 = v[5];
    {
        const double e1x = x1 - x0, e1y = y1 - y0, e2x = x2 - x0, e2y = y2 - y0;
        const double det = e1x * e2y - e2x * e1y;
        const double dx = x - x0, dy = y - y0;
        r = 2.0 * ((dx * e2y - e2x * dy) / det) - 1.0;
        s = 2.0 * ((e1x * dy - dx * e1y) / det) - 1.0;
    }
    if (!(fabs(r) < __builtin_inf()) || !(fabs(s) < __builtin_inf())) return kDriftLost;
    r = curvedDriftClipped(r);
    s = curvedDriftClipped(s);
    double step = __builtin_inf();
    for (int it = 0; it < kCurvedDriftNewton; ++it) {
        triDriftBasis(tab.jac, N, r, s, P);
        const double X = curvedDriftSum(c, Np, P), Y = curvedDriftSum(c + Np, Np, P);
        const double Xr = curvedDriftSum(c + 2 * Np, Np, P), Xs = curvedDriftSum(c + 3 * Np, Np, P);
        const double Yr = curvedDriftSum(c + 4 * Np, Np, P), Ys = curvedDriftSum(c + 5 * Np, Np, P);
        const double det = Xr * Ys - Xs * Yr;
        step = __builtin_inf();
        if (!(det > 0.0) || det == __builtin_inf()) break;
        const double fx = x - X, fy = y - Y;
        const double dr = (Ys * fx - Xs * fy) / det, ds = (Xr * fy - Yr * fx) / det;
        if (!(fabs(dr) < __builtin_inf()) || !(fabs(ds) < __builtin_inf())) break;
        const double rn = curvedDriftClipped(r + dr), sn = curvedDriftClipped(s + ds);
        step = fmax(fabs(rn - r), fabs(sn - s));
        r = rn; s = sn;
        if (step <= 1e-14) break;
    }
    const bool converged = step <= 1e-10;
    int f = 0;
    double worst = -1.0 - s;
    if (r + s > worst) { worst = r + s; f = 1; }
    if (-1.0 - r > worst) { worst = -1.0 - r; f = 2; }
    if (worst <= 1e-12) return converged ? 0 : kDriftLost;
    const int nb = tab.neigh[4LL * k + f];
    if (nb >= 0) { k = nb; return -1; }
    if (nb != kDriftWall) return kDriftExited;
    if (!converged) return kDriftLost;
    if (wk >= 0 && (wk != k || wf != f)) { // a corner: to the nearer end of this face
        const double ax = f == 0 ? x0 : (f == 1 ? x1 : x2), ay = f == 0 ? y0 : (f == 1 ? y1 : y2);
        const double bx = f == 0 ? x1 : (f == 1 ? x2 : x0), by = f == 0 ? y1 : (f == 1 ? y2 : y0);
        const double da = (x - ax) * (x - ax) + (y - ay) * (y - ay), db = (x - bx) * (x - bx) + (y - by) * (y - by);
        if (da <= db) { x = ax; y = ay; } else { x = bx; y = by; }
    } else {
        if (f == 0) s = -1.0;
        else if (f == 2) r = -1.0;
        else { const double h = 0.5 * (r + s); r = r - h; s = s - h; }
        curvedDriftMap(tab.jac, c, N, r, s, P, x, y);
    }
    if (wk < 0) { wk = k; wf = f; }
    wall = kDriftTouched;
    return -1;
}

// triangles with curved elements as the element policy of sw2d_drifter_driver.hpp
struct CurvedTriDrift {
    using Tables = CurvedTriDriftTables;
    static constexpr int kRows = kTriDriftMaxNp;
    __device__ static void init(const Tables& tab, int k, double r, double s, double* P, double& x, double& y) {
        const int c = tab.curvedSlot[k];
        if (c < 0) return TriDrift::init(tab.tri, k, r, s, P, x, y);
        const int N = tab.N, Np = (N + 1) * (N + 2) / 2;
        curvedDriftMap(tab.tri.jac, tab.modal + 6LL * c * Np, N, r, s, P, x, y);
    }
    __device__ static int locate(const Tables& tab, double& x, double& y, int& k, double& r, double& s, double* P, int& wall) {
        const int N = tab.N, Np = (N + 1) * (N + 2) / 2;
        int wk = -1, wf = -1;
        for (int hop = 0; hop < kTriDriftHops; ++hop) {
            const int c = tab.curvedSlot[k];
            const int res = c < 0 ? triDriftHop(tab.tri.vert, tab.tri.neigh, x, y, k, r, s, wall, wk, wf)
                                  : curvedDriftHop(tab.tri, tab.modal + 6LL * c * Np, N, x, y, k, r, s, P, wall, wk, wf);
            if (res >= 0) return res;
        }
        return kDriftLost;
    }
    __device__ static bool velocity(const DriftParams& p, const Tables& tab, int k, double r, double s, double* P, double& u,
                                    double& v) {
        return triDriftVelocity(p, tab.tri, k, r, s, P, u, v);
    }
};

__global__ __launch_bounds__(kDriftThreads) void sw2d_curved_drifter_kernel(DriftParams p, CurvedTriDriftTables tab) {
    driftBody<CurvedTriDrift>(p, tab);
}

} // namespace bdg_dev
