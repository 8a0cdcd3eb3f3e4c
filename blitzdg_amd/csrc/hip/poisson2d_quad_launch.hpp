// The quadrilateral family's launch table of the elliptic operator's passes and of the mass product (poisson2d_quad_kernel.hpp),
// compiled per order in poisson2d_quad_order.hip with -DBDG_ORDER=N. It is a PoissonKernelTable (poisson2d_launch.hpp) filled
// for quadrilaterals -- Np = (N+1)^2, four faces, gradient / divergence / mass with the same arguments -- so that the loop of
// poisson2d_device.hip drives both families through one type. What differs: `ops` is the tensor image D1 | l0 | lN, the `mass`
// argument of mass() the (N+1, N+1) 1-D mass matrix, p.ageo holds 16 planes, p.vmapP / p.kind / p.g / p.qn are (4 Nfp, ld), and
// mass() writes one partial per tile of poisson_quad_tile_elements(order) elements.
#pragma once
#include "poisson2d_launch.hpp"

namespace bdg_dev {

constexpr int kPoissonQuadMaxOrder = 12;

const PoissonKernelTable* poisson_quad_kernel_table(int order); // nullptr if the order is not compiled in
int poisson_quad_tile_elements(int order);                      // QuadElem<order>::E; 0 if the order is not compiled in

} // namespace bdg_dev
