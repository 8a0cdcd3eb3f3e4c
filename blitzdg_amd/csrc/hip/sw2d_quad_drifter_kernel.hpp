// sw2d_quad_drifter_kernel.hpp -- Lagrangian drifters of the quadrilateral sw2d solver (gfx950 / CDNA4, wave64): points that move
// with the velocity (hu / h, hv / h) of the resident state, are followed from element to element and recorded, all on the device.
// The launch, its modes, the Heun advance, the status bits and the records are those of sw2d_drifter_driver.hpp, shared with
// sw2d_drifter_kernel.hpp; this file is the quadrilateral: the tables, the init map, locate and the velocity.
//
//   sw2d_quad_drifter_kernel   the driver's body with the policy QuadDrift
//
// The order is a run-time argument (as in sw2d_monitor_kernel.hpp): one instance serves every order. The kernel reads the
// state planes 0..2 and the element tables and writes only the drifter arrays and the record buffer.
//
// Element tables (bdg_quadnodes_drifter_tables): per element the bilinear map of its four corner nodes,
//   x(r, s) = xc + ax r + bx s + cx r s,  y likewise: bil[8 k + (xc, ax, bx, cx, yc, ay, by, cy)], one 64-byte line per element;
// the neighbour across each face, neigh[4 k + f], f = 0..3 = (s = -1, r = +1, s = +1, r = -1): an element, kDriftWall or
// kDriftOpen; the Gauss-Lobatto points r1d and their barycentric weights c_a = 1 / prod_{b != a} (r1d[a] - r1d[b]).
//
// locate(x, y, k): at most kQuadDriftHops hops. In each, Newton on the bilinear map of k from (r, s) = (0, 0), coordinates relative
// to (xc, yc), at most kQuadDriftNewton iterations, stopped at max(|dr|, |ds|) <= 1e-14. A determinant that is not positive and
// finite, an iterate that is not finite or a last step above 1e-10 loses the drifter. The violations (-1 - s, r - 1, s - 1, -1 - r)
// of the faces 0..3: the largest <= 1e-12 is "found in k"; otherwise the face of the largest (lowest index on a tie) is crossed:
// to the neighbour; at a wall that face's coordinate is clamped to +-1, (x, y) recomputed from the map, the wall bit set and the
// same element searched again (the drifter slides along the wall); at an open face the drifter has exited. Hops used up: lost.
//
// Velocity at (k, r, s): u = hu / h, v = hv / h at the element's nodes, interpolated by the tensor gauge rule of
// sw2d_monitor_kernel.hpp, value = sum_i ls[i] (sum_j lr[j] f[(N+1) j + i]), both sums ascending from 0.0, no contraction;
// lr, ls by the second barycentric form, t_a = c_a / (r - r1d[a]), l_a = t_a / sum_b t_b (ascending), on a node the exact unit
// vector. A velocity that is not finite loses the drifter.
//
// The basis values of a lane live in LDS, sb[a][lane], lr in the rows [0, kQuadDriftMaxNq) and ls in the next kQuadDriftMaxNq
// (run-time indexed, so not in registers; one column per lane: no bank conflicts and no barrier). The state reads are scattered
// 8-byte gathers, 3 Np per evaluation.
#pragma once
#include "sw2d_drifter_driver.hpp"

namespace bdg_dev {

constexpr int kQuadDriftMaxNq = 13;      // BDG_SW2DQ_MAX_ORDER + 1
constexpr int kQuadDriftHops = 32;
constexpr int kQuadDriftNewton = 12;

struct QuadDriftTables {
    const double* bil;      // 8 per element
    const int* neigh;       // 4 per element
    const double* r1d;      // N+1 Gauss-Lobatto points
    const double* bary;     // N+1 barycentric weights
};

// 0 found, kDriftExited or kDriftLost; k, r, s and (at a wall) x, y updated; wall: kDriftTouched or unchanged
__device__ inline int quadDriftLocate(const double* __restrict__ bil, const int* __restrict__ neigh, double& x, double& y, int& k,
                                      double& r, double& s, int& wall) {
#pragma clang fp contract(off)
    for (int hop = 0; hop < kQuadDriftHops; ++hop) {
        const double* c = bil + 8LL * k;
        const double xc = c[0], ax = c[1], bx = c[2], cx = c[3], yc = c[4], ay = c[5], by = c[6], cy = c[7];
        const double dx = x - xc, dy = y - yc;
        double step = __builtin_inf();
        r = 0.0; s = 0.0;
        for (int it = 0; it < kQuadDriftNewton; ++it) {
            const double fx = ax * r + bx * s + cx * (r * s) - dx, fy = ay * r + by * s + cy * (r * s) - dy;
            const double j11 = ax + cx * s, j12 = bx + cx * r, j21 = ay + cy * s, j22 = by + cy * r;
            const double det = j11 * j22 - j12 * j21;
            if (!(det > 0.0) || det == __builtin_inf()) return kDriftLost;
            const double dr = (j12 * fy - j22 * fx) / det, ds = (j21 * fx - j11 * fy) / det;
            r = r + dr; s = s + ds;
            if (!(fabs(r) < __builtin_inf()) || !(fabs(s) < __builtin_inf())) return kDriftLost;
            step = fmax(fabs(dr), fabs(ds));
            if (step <= 1e-14) break;
        }
        if (!(step <= 1e-10)) return kDriftLost;
        int f = 0;
        double worst = -1.0 - s;
        if (r - 1.0 > worst) { worst = r - 1.0; f = 1; }
        if (s - 1.0 > worst) { worst = s - 1.0; f = 2; }
        if (-1.0 - r > worst) { worst = -1.0 - r; f = 3; }
        if (worst <= 1e-12) return 0;
        const int nb = neigh[4LL * k + f];
        if (nb >= 0) { k = nb; continue; }
        if (nb != kDriftWall) return kDriftExited;
        if (f == 0) s = -1.0; else if (f == 1) r = 1.0; else if (f == 2) s = 1.0; else r = -1.0;
        x = xc + (ax * r + bx * s + cx * (r * s));
        y = yc + (ay * r + by * s + cy * (r * s));
        wall = kDriftTouched;
    }
    return kDriftLost;
}

// the 1-D basis at r into the lane's LDS column b[a * kDriftThreads]
__device__ inline void quadDriftBasis(const double* __restrict__ r1d, const double* __restrict__ bary, int Nq, double r, double* b) {
#pragma clang fp contract(off)
    int on = -1;
    double sum = 0.0;
    for (int a = 0; a < Nq; ++a) {
        const double d = r - r1d[a];
        if (d == 0.0) on = a;
        const double t = bary[a] / d;
        b[a * kDriftThreads] = t;
        sum = sum + t;
    }
    for (int a = 0; a < Nq; ++a) b[a * kDriftThreads] = on >= 0 ? (a == on ? 1.0 : 0.0) : b[a * kDriftThreads] / sum;
}

// (u, v) at (k, r, s); false if either is not finite
__device__ inline bool quadDriftVelocity(const DriftParams& p, const QuadDriftTables& tab, int k, double r, double s, double* lr,
                                         double* ls, double& u, double& v) {
#pragma clang fp contract(off)
    const int Nq = p.N + 1;
    const long long plane = static_cast<long long>(Nq) * Nq * p.ld;
    const double* __restrict__ q = p.q;
    quadDriftBasis(tab.r1d, tab.bary, Nq, r, lr);
    quadDriftBasis(tab.r1d, tab.bary, Nq, s, ls);
    double su = 0.0, sv = 0.0;
    for (int i = 0; i < Nq; ++i) {
        double au = 0.0, av = 0.0;
        for (int j = 0; j < Nq; ++j) {
            const long long o = (j * Nq + i) * p.ld + k;
            const double h = q[o], l = lr[j * kDriftThreads];
            au = au + l * (q[plane + o] / h);
            av = av + l * (q[2 * plane + o] / h);
        }
        const double l = ls[i * kDriftThreads];
        su = su + l * au;
        sv = sv + l * av;
    }
    u = su; v = sv;
    return fabs(su) < __builtin_inf() && fabs(sv) < __builtin_inf();
}

// the quadrilateral as the element policy of sw2d_drifter_driver.hpp
struct QuadDrift {
    using Tables = QuadDriftTables;
    static constexpr int kRows = 2 * kQuadDriftMaxNq;
    __device__ static void init(const Tables& tab, int k, double r, double s, double*, double& x, double& y) {
#pragma clang fp contract(off)
        const double* c = tab.bil + 8LL * k;
        x = c[0] + (c[1] * r + c[2] * s + c[3] * (r * s));
        y = c[4] + (c[5] * r + c[6] * s + c[7] * (r * s));
    }
    __device__ static int locate(const Tables& tab, double& x, double& y, int& k, double& r, double& s, double*, int& wall) {
        return quadDriftLocate(tab.bil, tab.neigh, x, y, k, r, s, wall);
    }
    __device__ static bool velocity(const DriftParams& p, const Tables& tab, int k, double r, double s, double* sb, double& u,
                                    double& v) {
        return quadDriftVelocity(p, tab, k, r, s, sb, sb + kQuadDriftMaxNq * kDriftThreads, u, v);
    }
};

__global__ __launch_bounds__(kDriftThreads) void sw2d_quad_drifter_kernel(DriftParams p, QuadDriftTables tab) {
    driftBody<QuadDrift>(p, tab);
}

} // namespace bdg_dev
