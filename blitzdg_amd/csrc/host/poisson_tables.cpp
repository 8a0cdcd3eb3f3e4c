// Host tables of the elliptic solver (poisson_tables.hpp). Layouts: poisson2d_kernel.hpp, poisson2d_quad_kernel.hpp.
#include "poisson_tables.hpp"
#include "capi_internal.hpp"
#include "element_order.hpp"
#include "element_tables.hpp"
#include <algorithm>
#include <cmath>
#include <string>

namespace blitzdg {
namespace poisson_tables {
namespace {

using bdg_detail::arg_error;

// M = Vinv^T Vinv (Np, Np)
std::vector<double> massMatrix(const double* Vinv, int Np) {
    std::vector<double> M(static_cast<size_t>(Np) * Np, 0.0);
    for (int m = 0; m < Np; ++m)
        for (int i = 0; i < Np; ++i) {
            const double a = Vinv[static_cast<size_t>(m) * Np + i];
            for (int j = 0; j < Np; ++j) M[static_cast<size_t>(i) * Np + j] += a * Vinv[static_cast<size_t>(m) * Np + j];
        }
    return M;
}

// The 1-D factor M1 (Nq, Nq) of M = M1 (x) M1, held to 1e-12 max|entry|.
std::vector<double> quadMassFactor(const std::string& fn, int N, const std::vector<double>& M) {
    const int Nq = N + 1, Np = Nq * Nq;
    if (!(M[0] > 0.0)) throw arg_error(fn + ": Vinv does not give a positive definite mass matrix");
    const double m00 = std::sqrt(M[0]);
    std::vector<double> M1(static_cast<size_t>(Nq) * Nq, 0.0);
    for (int a = 0; a < Nq; ++a)
        for (int b = 0; b < Nq; ++b) M1[a * Nq + b] = M[static_cast<size_t>(Nq * a) * Np + Nq * b] / m00;
    double maxM = 0.0, err = 0.0;
    for (int j = 0; j < Nq; ++j)
        for (int i = 0; i < Nq; ++i)
            for (int jj = 0; jj < Nq; ++jj)
                for (int ii = 0; ii < Nq; ++ii) {
                    const double v = M[static_cast<size_t>(Nq * j + i) * Np + Nq * jj + ii];
                    maxM = std::max(maxM, std::fabs(v));
                    err = std::max(err, std::fabs(v - M1[j * Nq + jj] * M1[i * Nq + ii]));
                }
    if (!(err <= 1e-12 * maxM))
        throw arg_error(fn + ": (V V^T)^-1 is not the tensor product of a 1-D mass matrix with itself (Vinv = V1^-1 (x) V1^-1 "
                             "expected); the mass product is sum-factorised");
    return M1;
}

} // namespace

void requireSigma(double sigma, const char* fn) {
    if (!(sigma >= 0.0) || !std::isfinite(sigma)) throw arg_error(std::string(fn) + ": sigma must be finite and >= 0");
}

Tables build(const bdg_poisson2d_desc& d, Family family, const std::vector<int>& fmask) {
    const bool quad = family == kQuadrilaterals;
    const std::string fn = quad ? "bdg_poisson2d_create_quad" : "bdg_poisson2d_create";
    const int faces = quad ? 4 : 3;
    if (d.order < 1 || d.order > kMaxOrder[family]) throw arg_error(fn + ": order must be 1.." + std::to_string(kMaxOrder[family]));
    if (d.flags & BDG_SW2D_NODAL_GEOMETRY)
        throw arg_error(fn + ": per-node geometry is not supported (" +
                        (quad ? "quadrilaterals in parallelogram form only)" : "straight-sided triangles only)"));
    if (!d.kappa_elements && (!(d.kappa > 0.0) || !std::isfinite(d.kappa))) throw arg_error(fn + ": kappa must be finite and > 0");
    requireSigma(d.sigma, fn.c_str());
    if (!(d.tau_scale >= 0.0) || !std::isfinite(d.tau_scale)) throw arg_error(fn + ": tau_scale must be finite and >= 0");
    if (d.num_elements < 1) throw arg_error(fn + ": num_elements must be >= 1");
    if (!d.Dr || !d.Ds || !d.Lift || !d.Vinv || !d.rx || !d.sx || !d.ry || !d.sy || !d.J || !d.nx || !d.ny || !d.Fscale ||
        !d.vmapM || !d.vmapP)
        throw arg_error(fn + ": a required table pointer is NULL");
    if (d.num_dirichlet < 0 || (d.num_dirichlet > 0 && !d.mapD)) throw arg_error(fn + ": bad Dirichlet-node list");

    Tables t;
    const int N = t.N = d.order, Nfp = t.Nfp = N + 1, Np = t.Np = quad ? Nfp * Nfp : Nfp * (N + 2) / 2;
    const int NFN = t.NFN = faces * Nfp, K = t.K = d.num_elements;
    if (fmask.size() != static_cast<size_t>(NFN)) throw arg_error(fn + ": no kernels compiled for this order");
    const long long ld = t.ld = (static_cast<long long>(K) + 63) / 64 * 64;
    if (quad) {
        if (static_cast<long long>(Np) * ld >= (1LL << 31)) throw arg_error(fn + ": Np*K exceeds 2^31 nodes (32-bit gather offsets)");
    } else {
        // Lane addresses are a wave-uniform row pointer plus a 32-bit unsigned BYTE offset (8 * node offset).
        if (static_cast<long long>(Np) * ld * 8 > 4294967295LL)
            throw arg_error(fn + ": Np*K exceeds 2^29 nodes (32-bit byte offsets within a plane)");
    }
    double kappaMax = d.kappa;
    if (d.kappa_elements) {
        kappaMax = 0.0;
        for (int k = 0; k < K; ++k) {
            if (!(d.kappa_elements[k] > 0.0) || !std::isfinite(d.kappa_elements[k]))
                throw arg_error(fn + ": every kappa must be finite and > 0");
            kappaMax = std::max(kappaMax, d.kappa_elements[k]);
        }
        t.kap.assign(d.kappa_elements, d.kappa_elements + K);
    } else {
        t.kap.assign(K, d.kappa);
    }

    // ---- operator and mass images
    const std::vector<double> M = massMatrix(d.Vinv, Np);
    if (quad) {
        t.ops = element_tables::tensorOperators(fn, N, d.Dr, d.Ds, d.Lift);
        t.mass = quadMassFactor(fn, N, M);
    } else {
        const int ROW = 2 * Np + NFN;
        t.ops.resize(static_cast<size_t>(ROW) * Np);
        for (int i = 0; i < Np; ++i) {
            for (int m = 0; m < Np; ++m) {
                t.ops[static_cast<size_t>(i) * ROW + 2 * m] = d.Dr[i * Np + m];
                t.ops[static_cast<size_t>(i) * ROW + 2 * m + 1] = d.Ds[i * Np + m];
            }
            for (int j = 0; j < NFN; ++j) t.ops[static_cast<size_t>(i) * ROW + 2 * Np + j] = d.Lift[i * NFN + j];
        }
        t.mass = M;
    }

    // ---- the index tables
    const size_t nFaceNodes = static_cast<size_t>(NFN) * K;
    const long long totalNodes = static_cast<long long>(Np) * K;
    for (int k = 0; k < K; ++k)
        for (int j = 0; j < NFN; ++j)
            if (d.vmapM[static_cast<size_t>(k) * NFN + j] != fmask[j] + Np * k)
                throw arg_error(fn + (quad ? ": vmapM is not the Gauss-Lobatto face numbering (faces s=-1, r=+1, s=+1, r=-1)"
                                           : ": vmapM does not follow the warp&blend face-node ordering (Fmask) these kernels are "
                                             "specialised for"));
    for (size_t i = 0; i < nFaceNodes; ++i)
        if (d.vmapP[i] < 0 || d.vmapP[i] >= totalNodes) throw arg_error(fn + ": vmapP entry out of range");
    t.kinds.resize(nFaceNodes);
    for (int k = 0; k < K; ++k)
        for (int j = 0; j < NFN; ++j) {
            const size_t i = static_cast<size_t>(k) * NFN + j;
            t.kinds[static_cast<size_t>(j) * K + k] = d.vmapP[i] == d.vmapM[i] ? kNeumann : kInterior;
        }
    for (int i = 0; i < d.num_dirichlet; ++i) {
        const int m = d.mapD[i];
        if (m < 0 || static_cast<size_t>(m) >= nFaceNodes) throw arg_error(fn + ": Dirichlet-node index out of range");
        unsigned char& e = t.kinds[static_cast<size_t>(m % NFN) * K + m / NFN];
        if (e == kInterior) throw arg_error(fn + ": a mapD entry is not a boundary face node");
        e = kDirichlet;
    }
    t.hasDirichlet = d.num_dirichlet > 0;

    // ---- geometry: what the family's kernels read per element, and J_k
    const element_tables::Geometry g{d.rx, d.sx, d.ry, d.sy, d.J, d.nx, d.ny, d.Fscale};
    t.geoRows = quad ? 16 : 13;
    if (quad) {
        t.means.resize(static_cast<size_t>(17) * K);
        for (int r = 0; r < 16; ++r) t.geo[r] = t.means.data() + static_cast<size_t>(r) * K;
        t.jac = t.means.data() + static_cast<size_t>(16) * K;
        if (!element_tables::parallelogramForm(g, Np, Nfp, K, K, t.means.data(), t.means.data() + static_cast<size_t>(16) * K))
            throw arg_error(fn + ": the mesh is not in parallelogram form (metric terms constant per element to 1e-10). On a general "
                                 "bilinear quadrilateral the variable metric does not commute with the mass matrix, M A is not "
                                 "symmetric and conjugate gradients has no licence (DESIGN.md 3.13)");
    } else {
        if (!element_tables::trianglesAreAffine(g, Np, Nfp, K))
            throw arg_error(fn + ": the geometry tables are not those of straight-sided elements");
        // one metric value per element, one normal / scale per face: row 0 of each table, the first node of each face
        const double* met[4] = {d.rx, d.sx, d.ry, d.sy};
        const double* fg[3] = {d.nx, d.ny, d.Fscale};
        for (int a = 0; a < 4; ++a) t.geo[a] = met[a];
        for (int c = 0; c < 3; ++c)
            for (int f = 0; f < 3; ++f) t.geo[4 + 3 * c + f] = fg[c] + static_cast<size_t>(f) * Nfp * K;
        t.jac = d.J;
    }
    for (int k = 0; k < K; ++k)
        if (!(t.jac[k] > 0.0)) throw arg_error(fn + ": J must be positive");

    // ---- the column sums of M (the nodal quadrature weights), the weights J M 1, the area and the penalty
    double fscaleMax = 0.0;
    for (size_t i = 0; i < nFaceNodes; ++i) fscaleMax = std::max(fscaleMax, std::fabs(d.Fscale[i]));
    std::vector<double> colsum(Np, 0.0);
    for (int i = 0; i < Np; ++i)
        for (int j = 0; j < Np; ++j) colsum[i] += M[static_cast<size_t>(j) * Np + i];
    t.wts.resize(static_cast<size_t>(Np) * K);
    for (int i = 0; i < Np; ++i)
        for (int k = 0; k < K; ++k) t.wts[static_cast<size_t>(i) * K + k] = colsum[i] * t.jac[k];
    double refArea = 0.0;
    for (int i = 0; i < Np; ++i) refArea += colsum[i];
    for (int k = 0; k < K; ++k) t.area += refArea * t.jac[k];
    t.tau = (d.tau_scale > 0.0 ? d.tau_scale : 1.0) * Np * fscaleMax / 2.0 * kappaMax;

    // ---- element numbering: triangles by the straight sw2d solver's rule; quadrilaterals keep the caller's order, as
    // Sw2dQuadSolver does, unless BDG_SW2D_REORDER asks for the breadth-first one
    namespace eo = element_order;
    if (quad) {
        if ((d.flags & BDG_SW2D_REORDER) != 0 && !(d.flags & BDG_SW2D_KEEP_ORDER)) t.perm = eo::bfsOrder(d.vmapP, K, Np, Nfp, 4);
    } else if ((d.flags & BDG_SW2D_REORDER) != 0 ||
               (!(d.flags & BDG_SW2D_KEEP_ORDER) && eo::renumberingWanted(d.vmapP, K, Np, Nfp, d.order))) {
        t.perm = eo::renumbering(d.vmapP, K, Np, Nfp, eo::patchSetting());
    }
    t.offP.resize(nFaceNodes);
    const int* perm = t.perm.empty() ? nullptr : t.perm.data();
    for (int k = 0; k < K; ++k)
        for (int j = 0; j < NFN; ++j) {
            const int v = d.vmapP[static_cast<size_t>(k) * NFN + j];
            const int n2 = v % Np, k2 = v / Np;
            t.offP[static_cast<size_t>(j) * K + k] = static_cast<int>(n2 * ld + (perm ? perm[k2] : k2));
        }
    return t;
}

} // namespace poisson_tables
} // namespace blitzdg
