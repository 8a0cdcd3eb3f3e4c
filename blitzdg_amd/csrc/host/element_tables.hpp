// What the device solvers accept as "straight-sided triangles", "quadrilaterals in parallelogram form" and "the Gauss-Lobatto
// tensor operators", decided from a descriptor's tables alone. Plain host arithmetic, no HIP: sw2d_device.hip,
// sw2d_quad_device.hip and poisson_tables.cpp (the elliptic solver) all ask here, so each definition exists once.
#pragma once
#include <cstddef>
#include <string>
#include <vector>

namespace blitzdg {
namespace element_tables {

// The geometry tables of a descriptor: (Np, K) metric terms and J, (faces Nfp, K) face terms. J may be nullptr (not held).
struct Geometry {
    const double *rx, *sx, *ry, *sy, *J, *nx, *ny, *Fscale;
};

// True when the metric terms (and J, where given) are constant per element and the face terms constant per
// face (straight-sided triangles), to round-off: then one value per element/face suffices.
bool trianglesAreAffine(const Geometry& g, int Np, int Nfp, int K);

// Parallelogram form of a quadrilateral mesh: metric terms (and J, where given) constant per element, nx, ny, Fscale per face, to
// 1e-10 relative. Fills the 16 numbers of every element, ag[row * stride + k] (rx, sx, ry, sy, then nx, ny, Fscale of the four
// faces), and jac[k] where J is given: means over the nodes, summed in ascending order. Returns false when any element fails
// (what was filled is then of no use). Runs on the parallelFor workers.
bool parallelogramForm(const Geometry& g, int Np, int Nq, int K, std::size_t stride, double* ag, double* jac);

// D1 | l0 | lN from Dr = D1 (x) I, Ds = I (x) D1 and the face-wise lift of the Gauss-Lobatto quadrilateral, each held to 1e-13
// max|entry|; a zero or non-finite table is refused. Throws bdg_detail::arg_error, `fn` names the caller.
std::vector<double> tensorOperators(const std::string& fn, int N, const double* Dr, const double* Ds, const double* Lift);

} // namespace element_tables
} // namespace blitzdg
