// sw2d_quad_drifter_kernel.hpp -- Lagrangian drifters of the quadrilateral sw2d solver (gfx950 / CDNA4, wave64): points that move
// with the velocity (hu / h, hv / h) of the resident state, are followed from element to element and recorded, all on the device.
// One launch per advance, on the solver's stream, no atomics, no host synchronisation:
//
//   sw2d_quad_drifter_kernel   lane = drifter, kQuadDriftThreads per workgroup. mode kQuadDriftAdvance: one Heun advance by dt
//                              and, with slot >= 0, the record of that step; kQuadDriftSample: (u0, v0) sampled again from the
//                              state (after set_state); kQuadDriftInit: x, y from (element, r, s), then the sample.
//
// The order is a run-time argument (as in sw2d_quad_monitor_kernel.hpp): one instance serves every order. The kernel reads the
// state planes 0..2 and the element tables and writes only the drifter arrays and the record buffer.
//
// Element tables (bdg_quadnodes_drifter_tables): per element the bilinear map of its four corner nodes,
//   x(r, s) = xc + ax r + bx s + cx r s,  y likewise: bil[8 k + (xc, ax, bx, cx, yc, ay, by, cy)], one 64-byte line per element;
// the neighbour across each face, neigh[4 k + f], f = 0..3 = (s = -1, r = +1, s = +1, r = -1): an element, kQuadDriftWall or
// kQuadDriftOpen; the Gauss-Lobatto points r1d and their barycentric weights c_a = 1 / prod_{b != a} (r1d[a] - r1d[b]).
//
// locate(x, y, k): at most kQuadDriftHops hops. In each, Newton on the bilinear map of k from (r, s) = (0, 0), coordinates relative
// to (xc, yc), at most kQuadDriftNewton iterations, stopped at max(|dr|, |ds|) <= 1e-14. A determinant that is not positive and
// finite, an iterate that is not finite or a last step above 1e-10 loses the drifter. The violations (-1 - s, r - 1, s - 1, -1 - r)
// of the faces 0..3: the largest <= 1e-12 is "found in k"; otherwise the face of the largest (lowest index on a tie) is crossed:
// to the neighbour; at a wall that face's coordinate is clamped to +-1, (x, y) recomputed from the map, the wall bit set and the
// same element searched again (the drifter slides along the wall); at an open face the drifter has exited. Hops used up: lost.
//
// Velocity at (k, r, s): u = hu / h, v = hv / h at the element's nodes, interpolated by the gauge rule of
// sw2d_quad_monitor_kernel.hpp, value = sum_i ls[i] (sum_j lr[j] f[(N+1) j + i]), both sums ascending from 0.0, no contraction;
// lr, ls by the second barycentric form, t_a = c_a / (r - r1d[a]), l_a = t_a / sum_b t_b (ascending), on a node the exact unit
// vector. A velocity that is not finite loses the drifter.
//
// One advance (Heun): predictor (x*, y*) = (x, y) + dt (u0, v0), located from k, (u*, v*) sampled there (an open face met by the
// predictor only ends its search: the sample is taken where it stopped); corrector (x, y) += dt / 2 ((u0, v0) + (u*, v*)),
// located from the old k; (u0, v0) sampled at the new position. Status: 0 moving, 1 exited through an open face (frozen at the
// corrector position), 2 lost (frozen where it was before the advance), + 4 once it has touched a wall. Frozen drifters are
// recorded and not moved.
//
// The basis values of a lane live in LDS, sb[a][lane] (run-time indexed, so not in registers; one column per lane: no bank
// conflicts and no barrier). The state reads are scattered 8-byte gathers, 3 Np per evaluation.
#pragma once
#include <hip/hip_runtime.h>

namespace bdg_dev {

constexpr int kQuadDriftThreads = 128;
constexpr int kQuadDriftMaxNq = 13;      // BDG_SW2DQ_MAX_ORDER + 1
constexpr int kQuadDriftHops = 32;
constexpr int kQuadDriftNewton = 12;
constexpr int kQuadDriftWall = -1;       // neighbour entries
constexpr int kQuadDriftOpen = -2;
constexpr int kQuadDriftExited = 1;      // status
constexpr int kQuadDriftLost = 2;
constexpr int kQuadDriftTouched = 4;
enum { kQuadDriftAdvance = 0, kQuadDriftSample = 1, kQuadDriftInit = 2 };

struct QuadDriftParams {
    const double* q;        // the state: planes of Np*ld, 0..2 read
    const double* bil;      // 8 per element
    const int* neigh;       // 4 per element
    const double* r1d;      // N+1 Gauss-Lobatto points
    const double* bary;     // N+1 barycentric weights
    double* x; double* y; double* r; double* s; double* u0; double* v0;   // per drifter
    int* k; int* status;
    double* recT;           // [capacity]
    double* recX;           // [capacity * n], record-major
    double* recY;
    int* recStatus;
    long long ld;
    int N, n, mode, slot;   // slot < 0: no record
    double dt, t;
};

// 0 found, kQuadDriftExited or kQuadDriftLost; k, r, s and (at a wall) x, y updated; wall: kQuadDriftTouched or 0
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
            if (!(det > 0.0) || det == __builtin_inf()) return kQuadDriftLost;
            const double dr = (j12 * fy - j22 * fx) / det, ds = (j21 * fx - j11 * fy) / det;
            r = r + dr; s = s + ds;
            if (!(fabs(r) < __builtin_inf()) || !(fabs(s) < __builtin_inf())) return kQuadDriftLost;
            step = fmax(fabs(dr), fabs(ds));
            if (step <= 1e-14) break;
        }
        if (!(step <= 1e-10)) return kQuadDriftLost;
        int f = 0;
        double worst = -1.0 - s;
        if (r - 1.0 > worst) { worst = r - 1.0; f = 1; }
        if (s - 1.0 > worst) { worst = s - 1.0; f = 2; }
        if (-1.0 - r > worst) { worst = -1.0 - r; f = 3; }
        if (worst <= 1e-12) return 0;
        const int nb = neigh[4LL * k + f];
        if (nb >= 0) { k = nb; continue; }
        if (nb != kQuadDriftWall) return kQuadDriftExited;
        if (f == 0) s = -1.0; else if (f == 1) r = 1.0; else if (f == 2) s = 1.0; else r = -1.0;
        x = xc + (ax * r + bx * s + cx * (r * s));
        y = yc + (ay * r + by * s + cy * (r * s));
        wall = kQuadDriftTouched;
    }
    return kQuadDriftLost;
}

// the 1-D basis at r into the lane's LDS column b[a * kQuadDriftThreads]
__device__ inline void quadDriftBasis(const double* __restrict__ r1d, const double* __restrict__ bary, int Nq, double r, double* b) {
#pragma clang fp contract(off)
    int on = -1;
    double sum = 0.0;
    for (int a = 0; a < Nq; ++a) {
        const double d = r - r1d[a];
        if (d == 0.0) on = a;
        const double t = bary[a] / d;
        b[a * kQuadDriftThreads] = t;
        sum = sum + t;
    }
    for (int a = 0; a < Nq; ++a) b[a * kQuadDriftThreads] = on >= 0 ? (a == on ? 1.0 : 0.0) : b[a * kQuadDriftThreads] / sum;
}

// (u, v) at (k, r, s); false if either is not finite
__device__ inline bool quadDriftVelocity(const QuadDriftParams& p, int k, double r, double s, double* lr, double* ls, double& u,
                                         double& v) {
#pragma clang fp contract(off)
    const int Nq = p.N + 1;
    const long long plane = static_cast<long long>(Nq) * Nq * p.ld;
    const double* __restrict__ q = p.q;
    quadDriftBasis(p.r1d, p.bary, Nq, r, lr);
    quadDriftBasis(p.r1d, p.bary, Nq, s, ls);
    double su = 0.0, sv = 0.0;
    for (int i = 0; i < Nq; ++i) {
        double au = 0.0, av = 0.0;
        for (int j = 0; j < Nq; ++j) {
            const long long o = (j * Nq + i) * p.ld + k;
            const double h = q[o], l = lr[j * kQuadDriftThreads];
            au = au + l * (q[plane + o] / h);
            av = av + l * (q[2 * plane + o] / h);
        }
        const double l = ls[i * kQuadDriftThreads];
        su = su + l * au;
        sv = sv + l * av;
    }
    u = su; v = sv;
    return fabs(su) < __builtin_inf() && fabs(sv) < __builtin_inf();
}

__global__ __launch_bounds__(kQuadDriftThreads) void sw2d_quad_drifter_kernel(QuadDriftParams p) {
#pragma clang fp contract(off)
    __shared__ double sb[2 * kQuadDriftMaxNq][kQuadDriftThreads];
    const int i = blockIdx.x * kQuadDriftThreads + threadIdx.x;
    if (i == 0 && p.slot >= 0) p.recT[p.slot] = p.t;
    if (i >= p.n) return;
    double* lr = &sb[0][threadIdx.x];
    double* ls = &sb[kQuadDriftMaxNq][threadIdx.x];
    int k = p.k[i], st = p.status[i];
    double x = p.x[i], y = p.y[i], r = p.r[i], s = p.s[i], u0 = p.u0[i], v0 = p.v0[i];
    const bool frozen = (st & (kQuadDriftExited | kQuadDriftLost)) != 0;
    if (p.mode != kQuadDriftAdvance) {
        if (p.mode == kQuadDriftInit) {
            const double* c = p.bil + 8LL * k;
            x = c[0] + (c[1] * r + c[2] * s + c[3] * (r * s));
            y = c[4] + (c[5] * r + c[6] * s + c[7] * (r * s));
            p.x[i] = x; p.y[i] = y;
        }
        if (!frozen) {
            if (!quadDriftVelocity(p, k, r, s, lr, ls, u0, v0)) p.status[i] = st | kQuadDriftLost;
            p.u0[i] = u0; p.v0[i] = v0;
        }
        return;
    }
    if (!frozen) {
        // every result into temporaries: a lost drifter stays where it was
        int wall = 0, kp = k, kc = k, res;
        double xp = x + p.dt * u0, yp = y + p.dt * v0, rp, sp, up, vp;
        bool ok = quadDriftLocate(p.bil, p.neigh, xp, yp, kp, rp, sp, wall) != kQuadDriftLost;
        ok = ok && quadDriftVelocity(p, kp, rp, sp, lr, ls, up, vp);
        if (ok) {
            double xn = x + (0.5 * p.dt) * (u0 + up), yn = y + (0.5 * p.dt) * (v0 + vp), rn, sn, un = u0, vn = v0;
            res = quadDriftLocate(p.bil, p.neigh, xn, yn, kc, rn, sn, wall);
            ok = res != kQuadDriftLost && (res == kQuadDriftExited || quadDriftVelocity(p, kc, rn, sn, lr, ls, un, vn));
            if (ok) {
                x = xn; y = yn; k = kc; r = rn; s = sn; u0 = un; v0 = vn;
                st |= res;
                p.x[i] = x; p.y[i] = y; p.r[i] = r; p.s[i] = s; p.u0[i] = u0; p.v0[i] = v0; p.k[i] = k;
            }
        }
        st |= wall | (ok ? 0 : kQuadDriftLost);
        p.status[i] = st;
    }
    if (p.slot >= 0) {
        const long long o = static_cast<long long>(p.slot) * p.n + i;
        p.recX[o] = x; p.recY[o] = y; p.recStatus[o] = st;
    }
}

} // namespace bdg_dev
