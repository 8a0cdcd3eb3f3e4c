// QuadNodesProvisioner: every table of the 2-D quadrilateral nodal DG discretisation (Gauss-Lobatto tensor nodes,
// V / Dr / Ds / Lift / Filter, bilinear physical grid and metric terms, normals / Fscale, vmapM / vmapP / BC maps),
// handed out as a DGContext2D.
//
// Public surface follows the reference's include/QuadNodesProvisioner.hpp:90-206; conventions (all matched):
//  * node (N+1)*j + i sits at r = r1d[j], s = s1d[i] (r1d = s1d = the N+1 Gauss-Lobatto points);
//  * faces are s=-1, r=+1, s=+1, r=-1, each listing its nodes in increasing node index (so faces 2 and 3 run
//    against the counter-clockwise sense); face f joins element vertices f and (f+1) mod 4;
//  * Vandermonde column (N+1)*i + j is P_i(s) P_j(r) (orthonormal Legendre).
// The operators are assembled from their 1-D factors: Dr = D1 (x) I, Ds = I (x) D1 and the lift of each face is
// the identity along the face times one column of the inverse 1-D mass matrix across it, so the structure the
// device kernel relies on holds exactly rather than to round-off.
#pragma once
#include "DGContext2D.hpp"
#include "JacobiBuilders.hpp"
#include "MeshManager.hpp"
#include "Types.hpp"
#include <vector>

namespace blitzdg {

class QuadNodesProvisioner {
public:
    static const index_type NumFaces;
    static const real_type NodeTol;

    QuadNodesProvisioner(index_type NOrder, const MeshManager& meshManager);
    QuadNodesProvisioner(const QuadNodesProvisioner&) = delete;
    QuadNodesProvisioner& operator=(const QuadNodesProvisioner&) = delete;
    QuadNodesProvisioner(QuadNodesProvisioner&&) = default;

    /// V(n, (N+1)*i + j) = P_i(s_n) P_j(r_n) at the given points.
    void computeVandermondeMatrix(index_type N, const real_vector_type& r, const real_vector_type& s,
                                  real_matrix_type& V) const;
    /// V2Dr(n, (N+1)*i + j) = P_i(s_n) P_j'(r_n), V2Ds(n, .) = P_i'(s_n) P_j(r_n).
    void computeGradVandermondeMatrix(index_type N, const real_vector_type& r, const real_vector_type& s,
                                      real_matrix_type& V2Dr, real_matrix_type& V2Ds) const;
    /// IM = V(rout, sout) Vinv: interpolation from the nodes to (rout, sout).
    void computeInterpMatrix(const real_vector_type& rout, const real_vector_type& sout, real_matrix_type& IM) const;
    /// Output step (reference src/QuadNodesProvisioner.cpp:721-838): interpolate a nodal field to the equispaced
    /// (N+1)^2 lattice of its element (point n (N+1) + m at r = -1 + 2m/N, s = -1 + 2n/N) and cut the element into N^2
    /// small quadrilaterals with corners (n,m), (n,m+1), (n+1,m), (n+1,m+1); xnew, ynew, fieldnew become (4, N^2*K),
    /// one column per small quadrilateral, element-major.
    void splitElements(const real_matrix_type& x, const real_matrix_type& y, const real_matrix_type& field,
                       real_matrix_type& xnew, real_matrix_type& ynew, real_matrix_type& fieldnew) const;
    /// The pieces of splitElements: IM (Np, Np) from computeInterpMatrix; its 1-D factor I1 (N+1, N+1), the Lagrange
    /// interpolation from the Gauss-Lobatto points to the equispaced ones (IM(n (N+1) + m, (N+1) j + i) = I1(m, j) I1(n, i));
    /// and the local connectivity of the N^2 small quadrilaterals (lattice point indices, 4 per quadrilateral).
    void splitOperators(real_matrix_type& IM, real_matrix_type& I1, std::vector<index_type>& localE2V) const;

    /// The N+1 Gauss-Lobatto quadrature weights, w1[a] = (2N+1) / (N (N+1) V1(a, N)^2): the row sums of the 1-D mass matrix
    /// (V1 V1^T)^-1.
    std::vector<real_type> gaussLobattoWeights() const;
    /// Collocated quadrature weights (Np, K): w((N+1) j + i, k) = w1[j] w1[i] J((N+1) j + i, k).
    void quadratureWeights(real_matrix_type& w) const;
    /// The N+1 Lagrange basis values of the nodes `nodes` at abscissa r (barycentric formula); an abscissa that equals a
    /// node bit for bit gives the exact unit vector.
    static void lagrangeBasis1D(const real_type* nodes, index_type n, real_type r, real_type* basis);
    /// ... of this provisioner's Gauss-Lobatto points.
    void lagrangeBasis1D(real_type r, real_type* basis) const { lagrangeBasis1D(r1d.data(), NOrder + 1, r, basis); }
    /// For each point (x[p], y[p]) the element that contains it and its reference coordinates: Newton iteration on the
    /// element's nodal map x(r, s), y(r, s), candidates by element bounding boxes. |r|, |s| <= 1 + 1e-10 is inside; a point
    /// on a shared edge or vertex goes to the lowest element index; a point in no element gets element -1 (r = s = 0).
    void locatePoints(const real_type* x, const real_type* y, index_type n, index_type* element, real_type* r,
                      real_type* s) const;

    void buildNodes();
    void buildLift();
    void buildPhysicalGrid();
    void buildMaps();
    /// Appends the face-node lists of the mesh's BC table to BCmap (as the reference, never cleared).
    void buildBCHash();
    void buildBCHash(const index_vector_type& bcType);
    /// The reference's construction (src/QuadNodesProvisioner.cpp:170-202), quirk included: the exponential
    /// weights are enumerated over the TRIANGLE index set i + j <= N into the first (N+1)(N+2)/2 diagonal entries
    /// of an Np x Np diagonal, the other entries stay 0; Filter = V diag Vinv.
    void buildFilter(real_type Nc, index_type s);

    const real_matrix_type& get_xGrid() const { return xGrid; }
    const real_matrix_type& get_yGrid() const { return yGrid; }
    const real_vector_type& get_rGrid() const { return rGrid; }
    const real_vector_type& get_sGrid() const { return sGrid; }
    const real_vector_type& get_r1d() const { return r1d; }
    const real_matrix_type& get_V() const { return V; }
    const real_matrix_type& get_Vinv() const { return Vinv; }
    const real_matrix_type& get_Dr() const { return Dr; }
    const real_matrix_type& get_Ds() const { return Ds; }
    const real_matrix_type& get_Lift() const { return Lift; }
    const real_matrix_type& get_Filter() const { return Filter; }
    const real_matrix_type& get_J() const { return J; }
    const real_matrix_type& get_rx() const { return rx; }
    const real_matrix_type& get_ry() const { return ry; }
    const real_matrix_type& get_sx() const { return sx; }
    const real_matrix_type& get_sy() const { return sy; }
    const real_matrix_type& get_nx() const { return nx; }
    const real_matrix_type& get_ny() const { return ny; }
    const real_matrix_type& get_Fscale() const { return Fscale; }
    const index_matrix_type& get_Fmask() const { return Fmask; }
    const index_vector_type& get_vmapM() const { return vmapM; }
    const index_vector_type& get_vmapP() const { return vmapP; }
    const index_vector_type& get_mapP() const { return mapP; }
    const index_vector_type& get_vmapB() const { return vmapB; }
    const index_vector_type& get_mapB() const { return mapB; }
    const index_hashmap& get_bcMap() const { return BCmap; }
    const MeshManager& get_MeshManager() const { return *Mesh2D; }
    DGContext2D get_DGContext() const;

    index_type get_NumLocalPoints() const { return NumLocalPoints; }
    index_type get_NumFacePoints() const { return NumFacePoints; }
    index_type get_NumElements() const { return NumElements; }
    index_type get_NOrder() const { return NOrder; }

private:
    index_type NumElements, NOrder, NumLocalPoints, NumFacePoints;
    real_vector_type r1d;          // Gauss-Lobatto points
    real_matrix_type V1, V1inv, D1; // 1-D Vandermonde, its inverse, differentiation matrix
    real_matrix_type xGrid, yGrid;
    real_vector_type rGrid, sGrid;
    real_matrix_type V, Vinv, Dr, Ds, Lift, Filter, J, rx, sx, ry, sy, nx, ny, Fscale;
    index_matrix_type Fmask;
    index_vector_type vmapM, vmapP, mapP, vmapB, mapB;
    index_hashmap BCmap;
    std::vector<index_type> noGather; // DGContext2D slots the quadrilateral path does not fill
    const MeshManager* Mesh2D;
    JacobiBuilders Jacobi;
};

} // namespace blitzdg
