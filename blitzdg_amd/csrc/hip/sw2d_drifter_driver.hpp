// sw2d_drifter_driver.hpp -- what the drifter kernels of the triangle and the quadrilateral sw2d solvers share (gfx950 / CDNA4,
// wave64): the arguments, the status and neighbour codes, the modes and the body of one launch. The element headers
// (sw2d_drifter_kernel.hpp, sw2d_quad_drifter_kernel.hpp, sw2d_curved_drifter_kernel.hpp) supply a policy E each and instantiate the body in their kernel:
//
//   E::Tables                                    the element tables, passed by value as the kernel's second argument
//   E::kRows                                     LDS rows of kDriftThreads doubles a lane's basis values take
//   E::init(tab, k, r, s, sb, x, y)              x, y from the element's map
//   E::locate(tab, x, y, k, r, s, sb, wall)      0 found, kDriftExited or kDriftLost; k, r, s and (at a wall) x, y updated;
//                                                wall: kDriftTouched or unchanged
//   E::velocity(p, tab, k, r, s, sb, u, v)       (u, v) at (k, r, s); false if either is not finite; sb: the lane's LDS column
//
// Lane = drifter, kDriftThreads per workgroup, one launch per advance on the solver's stream, no atomics, no host
// synchronisation. mode kDriftAdvance: one Heun advance by dt and, with slot >= 0, the record of that step; kDriftSample:
// (u0, v0) sampled again from the state (after set_state); kDriftInit: x, y from (element, r, s), then the sample.
//
// One advance (Heun): predictor (x*, y*) = (x, y) + dt (u0, v0), located from k, (u*, v*) sampled there (an open face met by the
// predictor only ends its search: the sample is taken where it stopped); corrector (x, y) += (dt / 2) ((u0, v0) + (u*, v*)),
// located from the old k; (u0, v0) sampled at the new position. Status: 0 moving, 1 exited through an open face (frozen at the
// corrector position), 2 lost (frozen where it was before the advance), + 4 once it has touched a wall. Frozen drifters are
// recorded and not moved. Records are record-major: recT[slot], recX / recY / recStatus[slot * n + drifter].
#pragma once
#include <hip/hip_runtime.h>

namespace bdg_dev {

constexpr int kDriftThreads = 128;
constexpr int kDriftWall = -1;       // neighbour entries
constexpr int kDriftOpen = -2;
constexpr int kDriftExited = 1;      // status
constexpr int kDriftLost = 2;
constexpr int kDriftTouched = 4;
enum { kDriftAdvance = 0, kDriftSample = 1, kDriftInit = 2 };

struct DriftParams {
    const double* q;        // the state: planes of Np*ld, 0..2 read
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

template <class E>
__device__ inline void driftBody(const DriftParams& p, const typename E::Tables& tab) {
#pragma clang fp contract(off)
    __shared__ double sb[E::kRows][kDriftThreads];
    const int i = blockIdx.x * kDriftThreads + threadIdx.x;
    if (i == 0 && p.slot >= 0) p.recT[p.slot] = p.t;
    if (i >= p.n) return;
    double* P = &sb[0][threadIdx.x];
    int k = p.k[i], st = p.status[i];
    double x = p.x[i], y = p.y[i], r = p.r[i], s = p.s[i], u0 = p.u0[i], v0 = p.v0[i];
    const bool frozen = (st & (kDriftExited | kDriftLost)) != 0;
    if (p.mode != kDriftAdvance) {
        if (p.mode == kDriftInit) {
            E::init(tab, k, r, s, P, x, y);
            p.x[i] = x; p.y[i] = y;
        }
        if (!frozen) {
            if (!E::velocity(p, tab, k, r, s, P, u0, v0)) p.status[i] = st | kDriftLost;
            p.u0[i] = u0; p.v0[i] = v0;
        }
        return;
    }
    if (!frozen) {
        // every result into temporaries: a lost drifter stays where it was
        int wall = 0, kp = k, kc = k, res;
        double xp = x + p.dt * u0, yp = y + p.dt * v0, rp, sp, up, vp;
        bool ok = E::locate(tab, xp, yp, kp, rp, sp, P, wall) != kDriftLost;
        ok = ok && E::velocity(p, tab, kp, rp, sp, P, up, vp);
        if (ok) {
            double xn = x + (0.5 * p.dt) * (u0 + up), yn = y + (0.5 * p.dt) * (v0 + vp), rn, sn, un = u0, vn = v0;
            res = E::locate(tab, xn, yn, kc, rn, sn, P, wall);
            ok = res != kDriftLost && (res == kDriftExited || E::velocity(p, tab, kc, rn, sn, P, un, vn));
            if (ok) {
                x = xn; y = yn; k = kc; r = rn; s = sn; u0 = un; v0 = vn;
                st |= res;
                p.x[i] = x; p.y[i] = y; p.r[i] = r; p.s[i] = s; p.u0[i] = u0; p.v0[i] = v0; p.k[i] = k;
            }
        }
        st |= wall | (ok ? 0 : kDriftLost);
        p.status[i] = st;
    }
    if (p.slot >= 0) {
        const long long o = static_cast<long long>(p.slot) * p.n + i;
        p.recX[o] = x; p.recY[o] = y; p.recStatus[o] = st;
    }
}

} // namespace bdg_dev
