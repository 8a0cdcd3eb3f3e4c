// Element numberings of the sw2d solvers, from the face-neighbour graph alone (a solver descriptor
// carries no coordinates), and the rule that decides whether a mesh is renumbered.
// The neighbour of face f of element k is vmapP[(3 k + f) Nfp] / Np: a plain (K, 3) neighbour table
// (EToE) is the same thing with Np = Nfp = 1. Boundary faces name their own element.
#pragma once
#include <vector>

namespace blitzdg {
namespace element_order {

// Patch size of a renumbering when BDG_SW2D_ORDER_PATCH does not pin one: 0, the breadth-first order. On the
// 10^6-triangle box at N = 4 it is the fastest of 0 / 64 / 256 / 1024 / 4096 (0.300 ms against 0.306 in the
// caller's row-by-row order; the patch orders take 0.328 / 0.324 / 0.319 / 0.314: they miss less in L2, but a
// patch breaks the lane +- 1 runs at its rim and a gather instruction touches more lines), and on a
// shuffled mesh the caller's index inside a patch means nothing (0.32 ms against 0.39 ... 0.53).
constexpr int kDefaultPatch = 0;

// Breadth-first numbering from element 0. perm[k] = device slot. `faces` is 3, or 4 for a quadrilateral mesh, whose
// neighbour of face f is vmapP[(4 k + f) Nfp] / Np; every other function here is for triangles.
std::vector<int> bfsOrder(const int* vmapP, int K, int Np, int Nfp, int faces);

// Compact patches of `patch` elements grown over the face graph, slots handed out patch by patch and
// by caller index inside a patch. perm[k] = device slot. patch >= K on a connected mesh is the identity.
std::vector<int> patchOrder(const int* vmapP, int K, int Np, int Nfp, int patch);

// BDG_SW2D_ORDER_PATCH (=n pins the patch size, 0 = bfsOrder), read when a solver is created.
int patchSetting();

// The numbering of a renumbering solver: patchOrder, or bfsOrder when patch <= 0.
std::vector<int> renumbering(const int* vmapP, int K, int Np, int Nfp, int patch);

// Bytes one element moves per LSERK4 stage, averaged over a step, on the affine face-link kernels
// (1412 at N = 4: sw2d_affine_kernel.hpp).
int stageBytesPerElement(int order);

// Slots that make up 1 MiB of stage traffic, or 0 where the far-neighbour rule is off: when the whole mesh
// moves no more than one XCD's 4 MiB L2 per stage, and at N >= 5 (the matrix-core kernels gain nothing from
// a renumbered box: 250 k triangles at N = 8, 0.285 ms as given, 0.283 breadth-first).
int farWindow(int order, int K);

// The automatic decision: mean neighbour distance above 4 sqrt(K) (a shuffled mesh), or more than a tenth of
// the faces with their neighbour beyond farWindow() slots (at N = 4: the row-by-row order of a box over 371
// cells wide). Integer sums: the same answer for any worker count.
bool renumberingWanted(const int* vmapP, int K, int Np, int Nfp, int order);

} // namespace element_order
} // namespace blitzdg
