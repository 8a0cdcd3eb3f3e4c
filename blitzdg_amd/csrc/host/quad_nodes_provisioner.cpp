// QuadNodesProvisioner implementation (setup path; CPU only). The tables follow the reference's
// src/QuadNodesProvisioner.cpp conventions (nodes :230-243, Fmask :245-295, Vandermonde :72-89, bilinear map and
// normals :277-447, coordinate-matched maps :449-560, filter :170-202, splitElements :721-838); they are assembled from
// 1-D factors.
#include "blitzdg/QuadNodesProvisioner.hpp"
#include "parallel_for.hpp"
#include <algorithm>
#include <cmath>
#include <limits>
#include <stdexcept>
#include <string>

namespace blitzdg {

const index_type QuadNodesProvisioner::NumFaces = 4;
const real_type QuadNodesProvisioner::NodeTol = 1.e-5;

QuadNodesProvisioner::QuadNodesProvisioner(index_type NOrder_, const MeshManager& meshManager)
    : NumElements{meshManager.get_NumElements()}, NOrder{NOrder_}, NumLocalPoints{(NOrder_ + 1) * (NOrder_ + 1)},
      NumFacePoints{NOrder_ + 1}, Mesh2D{&meshManager} {
    if (NOrder < 1) throw std::invalid_argument("QuadNodesProvisioner: order must be >= 1");
    if (meshManager.get_NumFaces() != 4)
        throw std::invalid_argument("QuadNodesProvisioner: the mesh holds triangles, not quadrangles");
    buildNodes();
    buildLift();
    buildPhysicalGrid();
    buildMaps();
}

void QuadNodesProvisioner::computeVandermondeMatrix(index_type N, const real_vector_type& r, const real_vector_type& s,
                                                    real_matrix_type& Vout) const {
    const index_type n = r.size();
    Vout.resize(n, (N + 1) * (N + 1));
    real_vector_type p(n), q(n);
    for (index_type i = 0; i <= N; ++i) {
        Jacobi.computeJacobiPolynomial(s, 0.0, 0.0, i, p);
        for (index_type j = 0; j <= N; ++j) {
            Jacobi.computeJacobiPolynomial(r, 0.0, 0.0, j, q);
            for (index_type m = 0; m < n; ++m) Vout(m, (N + 1) * i + j) = p(m) * q(m);
        }
    }
}

void QuadNodesProvisioner::computeGradVandermondeMatrix(index_type N, const real_vector_type& r,
                                                        const real_vector_type& s, real_matrix_type& V2Dr,
                                                        real_matrix_type& V2Ds) const {
    const index_type n = r.size();
    V2Dr.resize(n, (N + 1) * (N + 1));
    V2Ds.resize(n, (N + 1) * (N + 1));
    real_vector_type ps(n), pr(n), dps(n), dpr(n);
    for (index_type i = 0; i <= N; ++i) {
        Jacobi.computeJacobiPolynomial(s, 0.0, 0.0, i, ps);
        Jacobi.computeGradJacobi(s, 0.0, 0.0, i, dps);
        for (index_type j = 0; j <= N; ++j) {
            Jacobi.computeJacobiPolynomial(r, 0.0, 0.0, j, pr);
            Jacobi.computeGradJacobi(r, 0.0, 0.0, j, dpr);
            for (index_type m = 0; m < n; ++m) {
                V2Dr(m, (N + 1) * i + j) = dpr(m) * ps(m);
                V2Ds(m, (N + 1) * i + j) = pr(m) * dps(m);
            }
        }
    }
}

void QuadNodesProvisioner::computeInterpMatrix(const real_vector_type& rout, const real_vector_type& sout,
                                               real_matrix_type& IM) const {
    real_matrix_type Vout;
    computeVandermondeMatrix(NOrder, rout, sout, Vout);
    const index_type n = rout.size(), Np = NumLocalPoints;
    IM.resize(n, Np);
    for (index_type a = 0; a < n; ++a)
        for (index_type b = 0; b < Np; ++b) {
            real_type acc = 0;
            for (index_type m = 0; m < Np; ++m) acc += Vout(a, m) * Vinv(m, b);
            IM(a, b) = acc;
        }
}

void QuadNodesProvisioner::splitOperators(real_matrix_type& IM, real_matrix_type& I1,
                                          std::vector<index_type>& localE2V) const {
    const index_type N = NOrder, Nq = N + 1, Np = NumLocalPoints;
    real_vector_type rout(Np), sout(Np), equi(Nq);
    for (index_type m = 0; m < Nq; ++m) equi(m) = -1.0 + 2.0 * static_cast<real_type>(m) / static_cast<real_type>(N);
    for (index_type n = 0; n < Nq; ++n)
        for (index_type m = 0; m < Nq; ++m) {
            rout(n * Nq + m) = equi(m);
            sout(n * Nq + m) = equi(n);
        }
    computeInterpMatrix(rout, sout, IM);
    // I1 = V1(equispaced) V1^-1
    VandermondeBuilders vb;
    real_matrix_type Vequi(Nq, Nq), unused;
    vb.computeVandermondeMatrix(equi, Vequi, unused, false);
    I1.resize(Nq, Nq);
    for (index_type a = 0; a < Nq; ++a)
        for (index_type b = 0; b < Nq; ++b) {
            real_type acc = 0;
            for (index_type m = 0; m < Nq; ++m) acc += Vequi(a, m) * V1inv(m, b);
            I1(a, b) = acc;
        }
    localE2V.clear();
    for (index_type n = 0; n < N; ++n)
        for (index_type m = 0; m < N; ++m)
            localE2V.insert(localE2V.end(), {n * Nq + m, n * Nq + m + 1, (n + 1) * Nq + m, (n + 1) * Nq + m + 1});
}

void QuadNodesProvisioner::splitElements(const real_matrix_type& x, const real_matrix_type& y, const real_matrix_type& field,
                                         real_matrix_type& xnew, real_matrix_type& ynew, real_matrix_type& fieldnew) const {
    const index_type Np = field.rows(), K = field.cols();
    if (Np != NumLocalPoints || x.rows() != Np || y.rows() != Np || x.cols() != K || y.cols() != K)
        throw std::runtime_error("splitElements: x, y and field must be (Np, K)");
    real_matrix_type IM, I1;
    std::vector<index_type> quads;
    splitOperators(IM, I1, quads);
    const index_type nLocal = static_cast<index_type>(quads.size() / 4);
    auto interpolate = [&](const real_matrix_type& f) { // (Np, Np) x (Np, K), K contiguous
        real_matrix_type out(Np, K);
        detail::parallelFor(Np, [&](index_type i) {
            real_type* o = out.data() + static_cast<std::size_t>(i) * K;
            for (index_type m = 0; m < Np; ++m) {
                const real_type a = IM(i, m);
                const real_type* src = f.data() + static_cast<std::size_t>(m) * K;
                for (index_type k = 0; k < K; ++k) o[k] += a * src[k];
            }
        }, 1);
        return out;
    };
    const real_matrix_type lx = interpolate(x), ly = interpolate(y), lf = interpolate(field);
    xnew.resize(4, nLocal * K);
    ynew.resize(4, nLocal * K);
    fieldnew.resize(4, nLocal * K);
    for (index_type k = 0; k < K; ++k)
        for (index_type l = 0; l < nLocal; ++l)
            for (index_type c = 0; c < 4; ++c) {
                const index_type v = quads[4 * l + c], i = k * nLocal + l;
                xnew(c, i) = lx(v, k);
                ynew(c, i) = ly(v, k);
                fieldnew(c, i) = lf(v, k);
            }
}

std::vector<real_type> QuadNodesProvisioner::gaussLobattoWeights() const {
    // w_a = 2 / (N (N+1) P_N(r_a)^2) with the orthonormal P~_N = sqrt((2N+1)/2) P_N of V1's last column
    const index_type N = NOrder, Nq = N + 1;
    std::vector<real_type> w1(Nq);
    for (index_type a = 0; a < Nq; ++a)
        w1[a] = static_cast<real_type>(2 * N + 1) / (static_cast<real_type>(N) * static_cast<real_type>(N + 1) * V1(a, N) * V1(a, N));
    return w1;
}

void QuadNodesProvisioner::quadratureWeights(real_matrix_type& w) const {
    const index_type Nq = NOrder + 1, Np = NumLocalPoints, K = NumElements;
    const std::vector<real_type> w1 = gaussLobattoWeights();
    w.resizeUninitialized(Np, K);
    for (index_type j = 0; j < Nq; ++j)
        for (index_type i = 0; i < Nq; ++i) {
            const index_type n = Nq * j + i;
            const real_type ww = w1[j] * w1[i];
            for (index_type k = 0; k < K; ++k) w(n, k) = ww * J(n, k);
        }
}

void QuadNodesProvisioner::lagrangeBasis1D(const real_type* nodes, index_type n, real_type r, real_type* basis) {
    for (index_type a = 0; a < n; ++a)
        if (r == nodes[a]) { // on a node: the unit vector, exactly
            for (index_type b = 0; b < n; ++b) basis[b] = b == a ? 1.0 : 0.0;
            return;
        }
    // second barycentric form: l_a(r) = (c_a / (r - x_a)) / sum_b c_b / (r - x_b), c_a = 1 / prod_{b != a} (x_a - x_b)
    real_type sum = 0;
    for (index_type a = 0; a < n; ++a) {
        real_type c = 1;
        for (index_type b = 0; b < n; ++b)
            if (b != a) c *= nodes[a] - nodes[b];
        basis[a] = 1 / (c * (r - nodes[a]));
        sum += basis[a];
    }
    for (index_type a = 0; a < n; ++a) basis[a] /= sum;
}

void QuadNodesProvisioner::locatePoints(const real_type* px, const real_type* py, index_type n, index_type* element,
                                        real_type* rOut, real_type* sOut) const {
    const index_type Nq = NOrder + 1, Np = NumLocalPoints, K = NumElements;
    constexpr real_type inside = 1.0 + 1e-10;
    // bounding boxes of the elements' nodes, widened by 1e-9 of their size
    std::vector<real_type> box(static_cast<std::size_t>(4) * K);
    for (index_type k = 0; k < K; ++k) {
        real_type x0 = xGrid(0, k), x1 = x0, y0 = yGrid(0, k), y1 = y0;
        for (index_type m = 1; m < Np; ++m) {
            x0 = std::min(x0, xGrid(m, k)); x1 = std::max(x1, xGrid(m, k));
            y0 = std::min(y0, yGrid(m, k)); y1 = std::max(y1, yGrid(m, k));
        }
        const real_type pad = 1e-9 * std::max(x1 - x0, y1 - y0);
        box[4 * k] = x0 - pad; box[4 * k + 1] = x1 + pad; box[4 * k + 2] = y0 - pad; box[4 * k + 3] = y1 + pad;
    }
    detail::parallelFor(n, [&](index_type p) {
        std::vector<real_type> X(Np), Y(Np), Xr(Np), Xs(Np), Yr(Np), Ys(Np), lr(Nq), ls(Nq);
        element[p] = -1;
        rOut[p] = 0;
        sOut[p] = 0;
        for (index_type k = 0; k < K; ++k) {
            if (px[p] < box[4 * k] || px[p] > box[4 * k + 1] || py[p] < box[4 * k + 2] || py[p] > box[4 * k + 3]) continue;
            // the element's nodal map and its derivatives at the nodes (the derivative of the interpolant is the
            // interpolant of D1 applied to the nodal values)
            // coordinates relative to the element's first node: the rounding of the map is then that of the element's
            // size, not of its distance from the origin (a mesh in UTM coordinates has 1e6 m offsets and 1e2 m cells)
            const real_type x0 = xGrid(0, k), y0 = yGrid(0, k);
            for (index_type m = 0; m < Np; ++m) { X[m] = xGrid(m, k) - x0; Y[m] = yGrid(m, k) - y0; }
            const real_type qx = px[p] - x0, qy = py[p] - y0;
            for (index_type j = 0; j < Nq; ++j)
                for (index_type i = 0; i < Nq; ++i) {
                    real_type a = 0, b = 0, c = 0, d = 0;
                    for (index_type m = 0; m < Nq; ++m) {
                        a += D1(j, m) * X[Nq * m + i]; b += D1(j, m) * Y[Nq * m + i];
                        c += D1(i, m) * X[Nq * j + m]; d += D1(i, m) * Y[Nq * j + m];
                    }
                    Xr[Nq * j + i] = a; Yr[Nq * j + i] = b; Xs[Nq * j + i] = c; Ys[Nq * j + i] = d;
                }
            real_type r = 0, s = 0;
            bool converged = false;
            for (int it = 0; it < 50 && !converged; ++it) {
                lagrangeBasis1D(r, lr.data());
                lagrangeBasis1D(s, ls.data());
                real_type x = 0, y = 0, xr = 0, xs = 0, yr = 0, ys = 0;
                for (index_type j = 0; j < Nq; ++j)
                    for (index_type i = 0; i < Nq; ++i) {
                        const real_type l = lr[j] * ls[i];
                        const index_type m = Nq * j + i;
                        x += l * X[m]; y += l * Y[m];
                        xr += l * Xr[m]; xs += l * Xs[m]; yr += l * Yr[m]; ys += l * Ys[m];
                    }
                const real_type det = xr * ys - xs * yr;
                if (!(std::fabs(det) > 0)) break;
                const real_type fx = qx - x, fy = qy - y;
                const real_type dr = (ys * fx - xs * fy) / det, ds = (xr * fy - yr * fx) / det;
                r += dr;
                s += ds;
                if (!(std::fabs(r) < 10 && std::fabs(s) < 10)) break; // the point is far outside this element
                // Newton converges quadratically: a step of 1e-12 leaves an error at the rounding of the map, far below
                // the 1e-10 of the inside test. (A smaller figure is below that rounding and may never be met.)
                converged = std::max(std::fabs(dr), std::fabs(ds)) <= 1e-12;
            }
            if (converged && std::fabs(r) <= inside && std::fabs(s) <= inside) {
                element[p] = k;
                rOut[p] = r;
                sOut[p] = s;
                break; // ascending k: the lowest element index wins
            }
        }
    }, 8);
}

void QuadNodesProvisioner::buildNodes() {
    const index_type N = NOrder, Nq = N + 1, Np = NumLocalPoints;
    r1d.resize(Nq);
    Jacobi.computeGaussLobottoPoints(0.0, 0.0, N, r1d);
    rGrid.resize(Np);
    sGrid.resize(Np);
    for (index_type j = 0; j < Nq; ++j)
        for (index_type i = 0; i < Nq; ++i) {
            rGrid(Nq * j + i) = r1d(j);
            sGrid(Nq * j + i) = r1d(i);
        }
    // Faces s=-1, r=+1, s=+1, r=-1, nodes in increasing index (the reference's NodeTol scans select exactly these).
    Fmask.resize(Nq, NumFaces);
    for (index_type n = 0; n < Nq; ++n) {
        Fmask(n, 0) = Nq * n;         // s = -1: i = 0
        Fmask(n, 1) = Nq * N + n;     // r = +1: j = N
        Fmask(n, 2) = Nq * n + N;     // s = +1: i = N
        Fmask(n, 3) = n;              // r = -1: j = 0
    }

    // 1-D operators: V1(a, b) = P_b(r_a), D1 = V1r V1^-1
    VandermondeBuilders vb;
    V1.resize(Nq, Nq);
    V1inv.resize(Nq, Nq);
    vb.computeVandermondeMatrix(r1d, V1, V1inv);
    real_matrix_type V1r(Nq, Nq);
    vb.computeGradVandermonde(r1d, V1r);
    D1.resize(Nq, Nq);
    for (index_type a = 0; a < Nq; ++a)
        for (index_type b = 0; b < Nq; ++b) {
            real_type acc = 0;
            for (index_type m = 0; m < Nq; ++m) acc += V1r(a, m) * V1inv(m, b);
            D1(a, b) = acc;
        }

    // V = V1 (x) V1 in the node / mode orders above; Vinv = V1inv (x) V1inv
    computeVandermondeMatrix(N, rGrid, sGrid, V);
    Vinv.resize(Np, Np);
    for (index_type i = 0; i < Nq; ++i)
        for (index_type j = 0; j < Nq; ++j)
            for (index_type jn = 0; jn < Nq; ++jn)
                for (index_type in = 0; in < Nq; ++in)
                    Vinv(Nq * i + j, Nq * jn + in) = V1inv(i, in) * V1inv(j, jn);

    // Dr acts along j (stride N+1), Ds along i (contiguous)
    Filter.resize(Np, Np); // zero until buildFilter
    Dr.resize(Np, Np);
    Ds.resize(Np, Np);
    for (index_type j = 0; j < Nq; ++j)
        for (index_type i = 0; i < Nq; ++i)
            for (index_type m = 0; m < Nq; ++m) {
                Dr(Nq * j + i, Nq * m + i) = D1(j, m);
                Ds(Nq * j + i, Nq * j + m) = D1(i, m);
            }
}

void QuadNodesProvisioner::buildLift() {
    // LIFT = (V V^T) E with V V^T = M1^-1 (x) M1^-1 and E holding the 1-D face mass matrix M1 on each face's rows:
    // face 0 (i = 0), column q: node (j, i) gets [j == q] * M1^-1(i, 0); face 1 (j = N): [i == q] * M1^-1(j, N);
    // face 2 (i = N): [j == q] * M1^-1(i, N); face 3 (j = 0): [i == q] * M1^-1(j, 0).
    const index_type N = NOrder, Nq = N + 1, Np = NumLocalPoints;
    real_matrix_type Minv(Nq, Nq);
    for (index_type a = 0; a < Nq; ++a)
        for (index_type b = 0; b < Nq; ++b) {
            real_type acc = 0;
            for (index_type m = 0; m < Nq; ++m) acc += V1(a, m) * V1(b, m);
            Minv(a, b) = acc;
        }
    Lift.resize(Np, NumFaces * Nq);
    for (index_type j = 0; j < Nq; ++j)
        for (index_type i = 0; i < Nq; ++i) {
            const index_type n = Nq * j + i;
            Lift(n, 0 * Nq + j) = Minv(i, 0);
            Lift(n, 1 * Nq + i) = Minv(j, N);
            Lift(n, 2 * Nq + j) = Minv(i, N);
            Lift(n, 3 * Nq + i) = Minv(j, 0);
        }
}

void QuadNodesProvisioner::buildPhysicalGrid() {
    const index_type N = NOrder, Nq = N + 1, Np = NumLocalPoints, K = NumElements, NFN = NumFaces * Nq;
    const index_vector_type& EToV = Mesh2D->get_Elements();
    const real_vector_type& Vert = Mesh2D->get_Vertices();
    const index_type dim = Mesh2D->get_Dim();
    xGrid.resizeUninitialized(Np, K); yGrid.resizeUninitialized(Np, K);
    J.resizeUninitialized(Np, K);
    rx.resizeUninitialized(Np, K); sx.resizeUninitialized(Np, K);
    ry.resizeUninitialized(Np, K); sy.resizeUninitialized(Np, K);
    nx.resizeUninitialized(NFN, K); ny.resizeUninitialized(NFN, K); Fscale.resizeUninitialized(NFN, K);
    detail::parallelChunks(K, [&](int kBegin, int kEnd) {
        std::vector<real_type> x(Np), y(Np), xr(Np), xs(Np), yr(Np), ys(Np);
        for (int k = kBegin; k < kEnd; ++k) {
            real_type vx[4], vy[4];
            for (int v = 0; v < 4; ++v) {
                vx[v] = Vert(EToV(4 * k + v) * dim);
                vy[v] = Vert(EToV(4 * k + v) * dim + 1);
            }
            for (int n = 0; n < Np; ++n) {
                const real_type r = rGrid(n), s = sGrid(n);
                const real_type wa = 0.25 * (1 - r) * (1 - s), wb = 0.25 * (1 + r) * (1 - s);
                const real_type wc = 0.25 * (1 + r) * (1 + s), wd = 0.25 * (1 - r) * (1 + s);
                x[n] = wa * vx[0] + wb * vx[1] + wc * vx[2] + wd * vx[3];
                y[n] = wa * vy[0] + wb * vy[1] + wc * vy[2] + wd * vy[3];
                xGrid(n, k) = x[n];
                yGrid(n, k) = y[n];
            }
            for (int j = 0; j < Nq; ++j)
                for (int i = 0; i < Nq; ++i) {
                    real_type a = 0, b = 0, c = 0, d = 0;
                    for (int m = 0; m < Nq; ++m) {
                        a += D1(j, m) * x[Nq * m + i]; b += D1(j, m) * y[Nq * m + i];
                        c += D1(i, m) * x[Nq * j + m]; d += D1(i, m) * y[Nq * j + m];
                    }
                    const int n = Nq * j + i;
                    xr[n] = a; yr[n] = b; xs[n] = c; ys[n] = d;
                    const real_type jac = a * d - c * b;
                    J(n, k) = jac;
                    rx(n, k) = d / jac;
                    ry(n, k) = -c / jac;
                    sx(n, k) = -b / jac;
                    sy(n, k) = a / jac;
                }
            for (int f = 0; f < NumFaces; ++f)
                for (int n = 0; n < Nq; ++n) {
                    const int v = Fmask(n, f), row = f * Nq + n;
                    real_type ex, ey;
                    switch (f) {
                    case 0: ex = yr[v]; ey = -xr[v]; break;
                    case 1: ex = ys[v]; ey = -xs[v]; break;
                    case 2: ex = -yr[v]; ey = xr[v]; break;
                    default: ex = -ys[v]; ey = xs[v]; break;
                    }
                    const real_type norm = std::sqrt(ex * ex + ey * ey);
                    nx(row, k) = ex / norm;
                    ny(row, k) = ey / norm;
                    Fscale(row, k) = norm / J(v, k);
                }
        }
    });
}

void QuadNodesProvisioner::buildMaps() {
    const index_type Nq = NumFacePoints, Np = NumLocalPoints, K = NumElements, NF = NumFaces;
    const index_vector_type& E2E = Mesh2D->get_EToE();
    const index_vector_type& E2F = Mesh2D->get_EToF();
    const index_vector_type& E2V = Mesh2D->get_Elements();
    const real_vector_type& Vert = Mesh2D->get_Vertices();
    const index_type dim = Mesh2D->get_Dim();
    const index_type total = K * NF * Nq;
    vmapM.resizeUninitialized(total);
    vmapP.resizeUninitialized(total);
    mapP.resizeUninitialized(total);
    detail::parallelChunks(K, [&](int kBegin, int kEnd) {
        for (int k = kBegin; k < kEnd; ++k)
            for (int f = 0; f < NF; ++f) {
                const int k2 = E2E(NF * k + f), f2 = E2F(NF * k + f);
                const int v1 = E2V(NF * k + f), v2 = E2V(NF * k + (f + 1) % NF);
                const real_type refd = std::hypot(Vert(dim * v1) - Vert(dim * v2), Vert(dim * v1 + 1) - Vert(dim * v2 + 1));
                for (int n = 0; n < Nq; ++n) {
                    const int g = (k * NF + f) * Nq + n;
                    const int vM = Fmask(n, f);
                    vmapM(g) = vM + Np * k;
                    const real_type x1 = xGrid(vM, k), y1 = yGrid(vM, k);
                    int hit = -1;
                    for (int nP = 0; nP < Nq; ++nP) {
                        const int vP = Fmask(nP, f2);
                        if (std::hypot(x1 - xGrid(vP, k2), y1 - yGrid(vP, k2)) < refd * NodeTol) hit = nP;
                    }
                    if (hit < 0)
                        throw std::runtime_error("QuadNodesProvisioner::buildMaps: face " + std::to_string(f) + " of element " +
                                                 std::to_string(k) + " does not match its neighbour's nodes (non-conforming mesh)");
                    vmapP(g) = Fmask(hit, f2) + Np * k2;
                    mapP(g) = hit + f2 * Nq + k2 * NF * Nq;
                }
            }
    });
    index_type nb = 0;
    for (index_type i = 0; i < total; ++i) nb += vmapP(i) == vmapM(i);
    mapB.resize(nb);
    vmapB.resize(nb);
    nb = 0;
    for (index_type i = 0; i < total; ++i)
        if (vmapP(i) == vmapM(i)) {
            mapB(nb) = i;
            vmapB(nb) = vmapM(i);
            ++nb;
        }
    buildBCHash();
}

void QuadNodesProvisioner::buildBCHash() { buildBCHash(Mesh2D->get_BCType()); }

void QuadNodesProvisioner::buildBCHash(const index_vector_type& bcType) {
    const index_type Nq = NumFacePoints;
    if (bcType.size() != NumFaces * NumElements)
        throw std::invalid_argument("buildBCHash: expected NumElements*4 entries");
    for (index_type face = 0; face < bcType.size(); ++face) {
        const index_type bct = bcType(face);
        if (bct == 0) continue;
        std::vector<index_type>& nodes = BCmap[bct];
        for (index_type n = 0; n < Nq; ++n) nodes.push_back(face * Nq + n);
    }
}

void QuadNodesProvisioner::buildFilter(real_type Nc, index_type s) {
    const index_type N = NOrder, Np = NumLocalPoints;
    const real_type alpha = -std::log(std::numeric_limits<real_type>::epsilon());
    std::vector<real_type> diag(Np, 0.0);
    index_type count = 0;
    for (index_type i = 0; i <= N; ++i)
        for (index_type j = 0; j <= N - i; ++j) {
            if (i + j >= Nc) {
                const real_type kk = (static_cast<real_type>(i + j) - Nc) / (static_cast<real_type>(N) - Nc);
                diag[count] = std::exp(-alpha * std::pow(kk, s));
            } else {
                diag[count] = 1.0;
            }
            ++count;
        }
    Filter.resize(Np, Np);
    for (index_type a = 0; a < Np; ++a)
        for (index_type b = 0; b < Np; ++b) {
            real_type acc = 0;
            for (index_type m = 0; m < count; ++m) acc += V(a, m) * diag[m] * Vinv(m, b);
            Filter(a, b) = acc;
        }
}

DGContext2D QuadNodesProvisioner::get_DGContext() const {
    return DGContext2D(NOrder, NumLocalPoints, NumFacePoints, NumElements, NumFaces, &Filter, &rGrid, &sGrid, &xGrid,
                       &yGrid, &Fscale, &Fmask, &noGather, &noGather, &V, &Vinv, &J, &rx, &ry, &sx, &sy, &nx, &ny, &Dr,
                       &Ds, &Lift, &vmapM, &vmapP, &BCmap);
}

} // namespace blitzdg
