// Host tables of the elliptic solver (bdg_poisson2d_create, bdg_poisson2d_create_quad) from the caller's descriptor alone, for
// both element families: validation, face-node kinds, geometry rows, weights, penalty, element numbering, gather offsets, operator
// and mass images. Plain host arithmetic, no HIP: poisson2d_device.hip uploads what build() returns.
#pragma once
#include "blitzdg_hip.h"
#include <vector>

namespace blitzdg {
namespace poisson_tables {

enum Family { kTriangles = 0, kQuadrilaterals = 1 };
constexpr int kMaxOrder[2] = {8, 12};

// One byte per face node (PoissonKind of poisson2d_kernel.hpp).
enum Kind : unsigned char { kInterior = 0, kDirichlet = 1, kNeumann = 2 };

// Row tables are (rows, K) images in the caller's element numbering. The geometry rows and J_k of triangles are rows of the
// descriptor's own tables (they are constant per element): Tables is of use only while the descriptor it was built from is.
struct Tables {
    Tables() = default;
    Tables(Tables&&) = default;        // (moved, never copied: geo and jac may point into means)
    int N = 0, Np = 0, Nfp = 0, NFN = 0, K = 0;
    long long ld = 0;                  // K rounded up to 64
    double tau = 0.0, area = 0.0;
    bool hasDirichlet = false;
    int geoRows = 0;                   // 13 (affine triangles) or 16 (parallelograms)
    const double* geo[16] = {};        // geoRows rows of K: the numbers the family's kernels read per element
    const double* jac = nullptr;       // (K)
    std::vector<double> means;         // quadrilaterals: the (16 + 1, K) means that geo and jac point into
    std::vector<double> kap;           // (K)
    std::vector<double> wts;           // (Np, K): J M 1
    std::vector<unsigned char> kinds;  // (NFN, K)
    std::vector<int> perm;             // caller element -> device slot (empty = identity)
    std::vector<int> offP;             // (NFN, K): reference numbering (n' + Np k') -> n' ld + slot(k'); a boundary node gathers itself
    std::vector<double> ops;           // triangles: VnOps image, row i = {Dr[i][m], Ds[i][m]} for m < Np, then Lift[i][j]; else D1 | l0 | lN
    std::vector<double> mass;          // triangles: M = Vinv^T Vinv (Np, Np); quadrilaterals: its 1-D factor M1 (Nq, Nq)
};

// `fn`: sigma must be finite and >= 0 (bdg_poisson2d_set_shift asks as well).
void requireSigma(double sigma, const char* fn);

// Everything above. fmask[f Nfp + n] is the kernels' volume node of face node (f, n); empty: no kernels for this order. Throws
// bdg_detail::arg_error with the texts of bdg_poisson2d_create / bdg_poisson2d_create_quad.
Tables build(const bdg_poisson2d_desc& d, Family family, const std::vector<int>& fmask);

} // namespace poisson_tables
} // namespace blitzdg
