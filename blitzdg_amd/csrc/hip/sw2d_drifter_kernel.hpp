// sw2d_drifter_kernel.hpp -- Lagrangian drifters of the triangle sw2d solver (gfx950 / CDNA4, wave64): points that move with the
// velocity (hu / h, hv / h) of the resident state, are followed from element to element and recorded, all on the device. The
// launch, its modes, the Heun advance, the status bits and the records are those of sw2d_drifter_driver.hpp, shared with
// sw2d_quad_drifter_kernel.hpp; this file is the triangle: the tables, the init map, locate and the velocity.
//
//   sw2d_drifter_kernel   the driver's body with the policy TriDrift
//   triDriftHop           one hop of locate; sw2d_curved_drifter_kernel.hpp takes it for its straight-sided elements
//
// The order is a run-time argument (as in sw2d_monitor_kernel.hpp): one instance serves N = 1..8. The kernel reads the state planes
// 0..2 in the solver's device layout q[node * ld + slot] (plane stride Np * ld) and the tables below, and writes only the drifter
// arrays and the record buffer. Elements are device slots throughout (the host maps the caller's numbering both ways).
//
// Tables (bdg_trinodes_drifter_tables). vert[8 k + (x0, y0, x1, y1, x2, y2, -, -)]: the corner nodes of element k, one 64-byte
// line per element; vertex 0, 1, 2 sit at (r, s) = (-1, -1), (1, -1), (-1, 1), so face 0 (s = -1) runs from vertex 0 to 1, face 1
// (r + s = 0) from 1 to 2 and face 2 (r = -1) from 2 to 0. With e1 = v1 - v0, e2 = v2 - v0 the affine map is
//   x(r, s) = x0 + ((0.5 (1 + r)) e1x + (0.5 (1 + s)) e2x),  y likewise.
// neigh[4 k + f], f = 0..2: the element across face f, kDriftWall or kDriftOpen (entry 3 pads to 16 bytes).
// vinvT[n Np + m] = Vinv[m][n], the inverse Vandermonde matrix transposed. jac[(g (N + 1) + n) 3 + (A, B, C)], g = 0 .. N + 1: the
// three-term recurrences p_0 = A_0, p_n = (A_n x + B_n) p_{n-1} + C_n p_{n-2} (C_1 = 0) of sqrt(2) P_n^(0,0) (g = 0) and of the
// orthonormal Jacobi polynomials P_n^(2i+1,0) (g = i + 1): the kernel takes no square roots.
//
// locate(x, y, k): at most kTriDriftHops hops. In each, with d = (x, y) - v0 and det = e1x e2y - e2x e1y of element k,
//   r = 2 ((dx e2y - e2x dy) / det) - 1,  s = 2 ((e1x dy - dx e1y) / det) - 1
// (the closed-form inverse of the affine map, no iteration); r or s not finite loses the drifter. The violations of the faces 0..2
// are (-1 - s, r + s, -1 - r): the largest <= 1e-12 is "found in k"; otherwise the face of the largest (lowest index on a tie) is
// crossed: to the neighbour; at an open face the drifter has exited; at a wall, with a -> b the face's vertices, the point is
// projected orthogonally onto the face's line, t = ((p - a).(b - a)) / ((b - a).(b - a)) (not clamped), p = a + t (b - a), the
// wall bit is set and the same element is searched again (the drifter slides along the wall). Corners: when a wall face is
// crossed and an earlier wall crossing of the same search was at another face (another element or another face index than the
// FIRST wall face of the search), the point goes instead to the end vertex of the face now crossed that is nearer to it
// (|p - a|^2 <= |p - b|^2: a), so alternating projections cannot use up the hops in an acute corner. Hops used up: lost.
//
// Basis at (r, s): a = 2 (1 + r) / (1 - s) - 1 (a = -1 at s = 1), b = s; column (i, j), i = 0..N outer, j = 0..N - i, holds
//   P_ij = (L_i(a) (1 - b)^i) J^i_j(b),
// L_i by the recurrence g = 0, (1 - b)^i by repeated multiplication from 1.0, J^i_j by the recurrence g = i + 1: the basis of
// TriangleNodesProvisioner::computeVandermondeMatrix.
//
// Velocity at (k, r, s): u = hu / h, v = hv / h at the element's nodes, value = sum_n row[n] f[n] with row[n] = sum_m P_m vinvT[n][m],
// every sum ascending from 0.0, no contraction: the gauge rule of sw2d_monitor_kernel.hpp with the row formed on the device. A
// velocity that is not finite loses the drifter.
//
// The basis values of a lane live in LDS, sb[m][lane] (run-time indexed, so not in registers; one column per lane: consecutive
// lanes read consecutive 8-byte words, no bank conflicts, and no barrier). vinvT and jac are read with wave-uniform addresses
// (scalar loads); four rows are formed per pass over the column, each in its own ascending order. The state reads are scattered
// 8-byte gathers, 3 Np per evaluation.
#pragma once
#include "sw2d_drifter_driver.hpp"

namespace bdg_dev {

constexpr int kTriDriftMaxNp = 45;      // N = 8
constexpr int kTriDriftHops = 32;

struct TriDriftTables {
    const double* vert;     // 8 per element
    const int* neigh;       // 4 per element
    const double* vinvT;    // Np x Np
    const double* jac;      // (N+2) x (N+1) x 3
};

// one hop of locate in the straight-sided element k: -1 to go on (k or x, y changed), else 0 found, kDriftExited or kDriftLost;
// (wk, wf): the first wall face this search crossed (-1: none yet)
__device__ inline int triDriftHop(const double* __restrict__ vert, const int* __restrict__ neigh, double& x, double& y, int& k,
                                  double& r, double& s, int& wall, int& wk, int& wf) {
#pragma clang fp contract(off)
    const double* c = vert + 8LL * k;
    const double x0 = c[0], y0 = c[1], x1 = c[2], y1 = c[3], x2 = c[4], y2 = c[5];
    const double e1x = x1 - x0, e1y = y1 - y0, e2x = x2 - x0, e2y = y2 - y0;
    const double det = e1x * e2y - e2x * e1y;
    const double dx = x - x0, dy = y - y0;
    r = 2.0 * ((dx * e2y - e2x * dy) / det) - 1.0;
    s = 2.0 * ((e1x * dy - dx * e1y) / det) - 1.0;
    if (!(fabs(r) < __builtin_inf()) || !(fabs(s) < __builtin_inf())) return kDriftLost;
    int f = 0;
    double worst = -1.0 - s;
    if (r + s > worst) { worst = r + s; f = 1; }
    if (-1.0 - r > worst) { worst = -1.0 - r; f = 2; }
    if (worst <= 1e-12) return 0;
    const int nb = neigh[4LL * k + f];
    if (nb >= 0) { k = nb; return -1; }
    if (nb != kDriftWall) return kDriftExited;
    const double ax = f == 0 ? x0 : (f == 1 ? x1 : x2), ay = f == 0 ? y0 : (f == 1 ? y1 : y2);
    const double bx = f == 0 ? x1 : (f == 1 ? x2 : x0), by = f == 0 ? y1 : (f == 1 ? y2 : y0);
    if (wk >= 0 && (wk != k || wf != f)) { // a corner: to the nearer end of this face
        const double da = (x - ax) * (x - ax) + (y - ay) * (y - ay), db = (x - bx) * (x - bx) + (y - by) * (y - by);
        if (da <= db) { x = ax; y = ay; } else { x = bx; y = by; }
    } else {
        const double ex = bx - ax, ey = by - ay;
        const double t = ((x - ax) * ex + (y - ay) * ey) / (ex * ex + ey * ey);
        x = ax + t * ex;
        y = ay + t * ey;
    }
    if (wk < 0) { wk = k; wf = f; }
    wall = kDriftTouched;
    return -1;
}

// 0 found, kDriftExited or kDriftLost; k, r, s and (at a wall) x, y updated; wall: kDriftTouched or unchanged
__device__ inline int triDriftLocate(const double* __restrict__ vert, const int* __restrict__ neigh, double& x, double& y, int& k,
                                     double& r, double& s, int& wall) {
    int wk = -1, wf = -1;
    for (int hop = 0; hop < kTriDriftHops; ++hop) {
        const int res = triDriftHop(vert, neigh, x, y, k, r, s, wall, wk, wf);
        if (res >= 0) return res;
    }
    return kDriftLost;
}

// the orthonormal simplex basis at (r, s) into the lane's LDS column P[m * kDriftThreads]
__device__ inline void triDriftBasis(const double* __restrict__ jac, int N, double r, double s, double* P) {
#pragma clang fp contract(off)
    const int Nq = N + 1;
    const double a = s != 1.0 ? 2.0 * (1.0 + r) / (1.0 - s) - 1.0 : -1.0;
    const double om = 1.0 - s;
    double pw = 1.0, lp = 0.0, lc = 0.0;
    int col = 0;
    for (int i = 0; i <= N; ++i) {
        const double* cl = jac + 3 * i;
        const double ln = i == 0 ? cl[0] : (cl[0] * a + cl[1]) * lc + cl[2] * lp;
        lp = lc; lc = ln;
        if (i > 0) pw = pw * om;
        const double fa = lc * pw;
        const double* cj = jac + 3 * Nq * (i + 1);
        double jp = 0.0, jc = 0.0;
        for (int j = 0; j <= N - i; ++j) {
            const double jn = j == 0 ? cj[0] : (cj[3 * j] * s + cj[3 * j + 1]) * jc + cj[3 * j + 2] * jp;
            jp = jc; jc = jn;
            P[col * kDriftThreads] = fa * jc;
            ++col;
        }
    }
}

// (u, v) at (k, r, s); false if either is not finite
__device__ inline bool triDriftVelocity(const DriftParams& p, const TriDriftTables& tab, int k, double r, double s, double* P,
                                        double& u, double& v) {
#pragma clang fp contract(off)
    const int Np = (p.N + 1) * (p.N + 2) / 2;
    const long long plane = static_cast<long long>(Np) * p.ld;
    const double* __restrict__ q = p.q;
    const double* __restrict__ vt = tab.vinvT;
    triDriftBasis(tab.jac, p.N, r, s, P);
    double su = 0.0, sv = 0.0;
    for (int n0 = 0; n0 < Np; n0 += 4) {
        // rows n0 .. n0 + 3 (past the end: the last row again, not used), one pass over the lane's column
        const double* v0 = vt + static_cast<long long>(n0) * Np;
        const double* v1 = vt + static_cast<long long>(min(n0 + 1, Np - 1)) * Np;
        const double* v2 = vt + static_cast<long long>(min(n0 + 2, Np - 1)) * Np;
        const double* v3 = vt + static_cast<long long>(min(n0 + 3, Np - 1)) * Np;
        double row[4] = {0.0, 0.0, 0.0, 0.0};
        for (int m = 0; m < Np; ++m) {
            const double pm = P[m * kDriftThreads];
            row[0] = row[0] + pm * v0[m];
            row[1] = row[1] + pm * v1[m];
            row[2] = row[2] + pm * v2[m];
            row[3] = row[3] + pm * v3[m];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (n0 + j < Np) {
                const long long o = (n0 + j) * p.ld + k;
                const double h = q[o];
                su = su + row[j] * (q[plane + o] / h);
                sv = sv + row[j] * (q[2 * plane + o] / h);
            }
        }
    }
    u = su; v = sv;
    return fabs(su) < __builtin_inf() && fabs(sv) < __builtin_inf();
}

// the triangle as the element policy of sw2d_drifter_driver.hpp
struct TriDrift {
    using Tables = TriDriftTables;
    static constexpr int kRows = kTriDriftMaxNp;
    __device__ static void init(const Tables& tab, int k, double r, double s, double*, double& x, double& y) {
#pragma clang fp contract(off)
        const double* c = tab.vert + 8LL * k;
        const double wr = 0.5 * (1.0 + r), ws = 0.5 * (1.0 + s);
        x = c[0] + (wr * (c[2] - c[0]) + ws * (c[4] - c[0]));
        y = c[1] + (wr * (c[3] - c[1]) + ws * (c[5] - c[1]));
    }
    __device__ static int locate(const Tables& tab, double& x, double& y, int& k, double& r, double& s, double*, int& wall) {
        return triDriftLocate(tab.vert, tab.neigh, x, y, k, r, s, wall);
    }
    __device__ static bool velocity(const DriftParams& p, const Tables& tab, int k, double r, double s, double* P, double& u,
                                    double& v) {
        return triDriftVelocity(p, tab, k, r, s, P, u, v);
    }
};

// (static: sw2d_curved_drifter_kernel.hpp brings this header into a second device object, which does not launch this kernel)
[[maybe_unused]] static __global__ __launch_bounds__(kDriftThreads) void sw2d_drifter_kernel(DriftParams p, TriDriftTables tab) {
    driftBody<TriDrift>(p, tab);
}

} // namespace bdg_dev
