// The element-table checks the device solvers share (element_tables.hpp).
#include "element_tables.hpp"
#include "capi_internal.hpp"
#include "parallel_for.hpp"
#include <algorithm>
#include <atomic>
#include <cmath>

namespace blitzdg {
namespace element_tables {

using bdg_detail::arg_error;

// 1e-8: far above the round-off the tables carry from Dr*x on small elements, far below any real curvature (the figures are
// with the straight solver's use of it, sw2d_device.hip).
bool trianglesAreAffine(const Geometry& g, int Np, int Nfp, int K) {
    const double tol = 1e-8;
    std::atomic<bool> ok{true};
    detail::parallelFor(K, [&](int k) {
        const double scale = std::fabs(g.rx[k]) + std::fabs(g.sx[k]) + std::fabs(g.ry[k]) + std::fabs(g.sy[k]);
        for (int n = 1; n < Np; ++n) {
            const size_t o = static_cast<size_t>(n) * K + k;
            if (std::fabs(g.rx[o] - g.rx[k]) > tol * scale || std::fabs(g.sx[o] - g.sx[k]) > tol * scale ||
                std::fabs(g.ry[o] - g.ry[k]) > tol * scale || std::fabs(g.sy[o] - g.sy[k]) > tol * scale ||
                (g.J && std::fabs(g.J[o] - g.J[k]) > tol * std::fabs(g.J[k])))
                ok = false;
        }
        for (int f = 0; f < 3; ++f) {
            const size_t o0 = static_cast<size_t>(f) * Nfp * K + k;
            for (int n = 1; n < Nfp; ++n) {
                const size_t o = o0 + static_cast<size_t>(n) * K;
                if (std::fabs(g.nx[o] - g.nx[o0]) > tol || std::fabs(g.ny[o] - g.ny[o0]) > tol ||
                    std::fabs(g.Fscale[o] - g.Fscale[o0]) > tol * std::fabs(g.Fscale[o0]))
                    ok = false;
            }
        }
    });
    return ok;
}

bool parallelogramForm(const Geometry& g, int Np, int Nq, int K, size_t stride, double* ag, double* jac) {
    std::atomic<bool> para{true};
    const double* met[5] = {g.rx, g.sx, g.ry, g.sy, g.J};
    const double* fg[3] = {g.nx, g.ny, g.Fscale};
    detail::parallelFor(K, [&](int k) {
        double scale = 0.0;
        for (int a = 0; a < 4; ++a)
            for (int n = 0; n < Np; ++n) scale = std::max(scale, std::fabs(met[a][static_cast<size_t>(n) * K + k]));
        for (int a = 0; a < (jac ? 5 : 4); ++a) {
            const double* tab = met[a];
            double mean = 0.0;
            for (int n = 0; n < Np; ++n) mean += tab[static_cast<size_t>(n) * K + k];
            mean /= Np;
            const double sc = a < 4 ? scale : std::fabs(mean);
            for (int n = 0; n < Np; ++n)
                if (!(std::fabs(tab[static_cast<size_t>(n) * K + k] - mean) <= 1e-10 * sc)) para = false;
            if (a < 4) ag[a * stride + k] = mean;
            else jac[k] = mean;
        }
        for (int c = 0; c < 3; ++c)
            for (int f = 0; f < 4; ++f) {
                double mean = 0.0, sc = 0.0;
                for (int n = 0; n < Nq; ++n) {
                    const double v = fg[c][static_cast<size_t>(f * Nq + n) * K + k];
                    mean += v;
                    sc = std::max(sc, std::fabs(v));
                }
                mean /= Nq;
                if (c < 2) sc = 1.0;
                for (int n = 0; n < Nq; ++n)
                    if (!(std::fabs(fg[c][static_cast<size_t>(f * Nq + n) * K + k] - mean) <= 1e-10 * sc)) para = false;
                ag[(4 + 4 * c + f) * stride + k] = mean;
            }
    });
    return para;
}

namespace {
double maxAbs(const double* a, size_t n) {
    double m = 0.0;
    for (size_t i = 0; i < n; ++i) m = std::max(m, std::fabs(a[i]));
    return m;
}
} // namespace

std::vector<double> tensorOperators(const std::string& fn, int N, const double* Dr, const double* Ds, const double* Lift) {
    const int Nq = N + 1, Np = Nq * Nq, NFN = 4 * Nq;
    std::vector<double> ops(static_cast<size_t>(Nq) * Nq + 2 * Nq);
    double* D1 = ops.data();
    double* l0 = D1 + Nq * Nq;
    double* lN = l0 + Nq;
    for (int j = 0; j < Nq; ++j)
        for (int m = 0; m < Nq; ++m) D1[j * Nq + m] = Dr[static_cast<size_t>(Nq * j) * Np + Nq * m];
    for (int i = 0; i < Nq; ++i) l0[i] = Lift[static_cast<size_t>(i) * NFN + 0];          // face 0, q = j = 0
    for (int j = 0; j < Nq; ++j) lN[j] = Lift[static_cast<size_t>(Nq * j) * NFN + Nq];    // face 1, q = i = 0
    const double tolD = 1e-13 * std::max(maxAbs(Dr, static_cast<size_t>(Np) * Np), maxAbs(Ds, static_cast<size_t>(Np) * Np));
    const double tolL = 1e-13 * maxAbs(Lift, static_cast<size_t>(Np) * NFN);
    // (a zero table would pass a tolerance relative to its own largest entry)
    if (!(tolD > 0.0) || !(tolL > 0.0))
        throw arg_error(fn + ": Dr / Ds or Lift is identically zero or not finite: these are not the operators of an "
                             "element of order " + std::to_string(N));
    double errD = 0.0, errL = 0.0;
    for (int j = 0; j < Nq; ++j)
        for (int i = 0; i < Nq; ++i) {
            const size_t row = static_cast<size_t>(Nq * j + i);
            for (int jj = 0; jj < Nq; ++jj)
                for (int ii = 0; ii < Nq; ++ii) {
                    const int col = Nq * jj + ii;
                    const double er = (ii == i ? D1[j * Nq + jj] : 0.0), es = (jj == j ? D1[i * Nq + ii] : 0.0);
                    errD = std::max(errD, std::fabs(Dr[row * Np + col] - er));
                    errD = std::max(errD, std::fabs(Ds[row * Np + col] - es));
                }
            for (int q = 0; q < Nq; ++q) {
                const double e0 = q == j ? l0[i] : 0.0, e1 = q == i ? lN[j] : 0.0;
                const double e2 = q == j ? lN[i] : 0.0, e3 = q == i ? l0[j] : 0.0;
                errL = std::max(errL, std::fabs(Lift[row * NFN + q] - e0));
                errL = std::max(errL, std::fabs(Lift[row * NFN + Nq + q] - e1));
                errL = std::max(errL, std::fabs(Lift[row * NFN + 2 * Nq + q] - e2));
                errL = std::max(errL, std::fabs(Lift[row * NFN + 3 * Nq + q] - e3));
            }
        }
    if (!(errD <= tolD))
        throw arg_error(fn + ": Dr / Ds are not the Gauss-Lobatto tensor operators D1 (x) I, I (x) D1 (deviation " +
                        std::to_string(errD) + "); the quadrilateral kernel has no dense-operator form");
    if (!(errL <= tolL))
        throw arg_error(fn + ": Lift does not have the face-wise tensor form of the Gauss-Lobatto element (deviation " +
                        std::to_string(errL) + "); the quadrilateral kernel has no dense-operator form");
    return ops;
}

} // namespace element_tables
} // namespace blitzdg
