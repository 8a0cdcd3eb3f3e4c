// C ABI, host-setup group (see include/blitzdg_hip.h). Thin handles around the
// C++ classes; tables are exported as borrowed views so the Python front end
// (blitzdg_amd/pyblitzdg.py) can mirror the reference's boost::python module
// (src/pyblitzdg/pyblitzdg.cpp:59-201) without copying on this side.
#include "capi_internal.hpp"
#include "element_order.hpp"
#include "parallel_for.hpp"
#include "blitzdg/Advec1d.hpp"
#include "blitzdg/Burgers1d.hpp"
#include "blitzdg/LSERK4.hpp"
#include "blitzdg/TriangleCubatureRules.hpp"
#include "blitzdg/VtkOutputter.hpp"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

using namespace blitzdg;

namespace bdg_detail {
thread_local std::string g_last_error;
void set_error(const std::string& msg) { g_last_error = msg; }
} // namespace bdg_detail

using bdg_detail::guard;
using bdg_detail::set_error;

namespace {
void view(bdg_table* out, const real_matrix_type& m) { *out = {m.data(), m.rows(), m.cols(), BDG_F64}; }
void view(bdg_table* out, const index_matrix_type& m) { *out = {m.data(), m.rows(), m.cols(), BDG_I32}; }
void view(bdg_table* out, const real_vector_type& v) { *out = {v.data(), v.size(), 1, BDG_F64}; }
void view(bdg_table* out, const index_vector_type& v) { *out = {v.data(), v.size(), 1, BDG_I32}; }
void view(bdg_table* out, const std::vector<index_type>& v) {
    *out = {v.data(), static_cast<int>(v.size()), 1, BDG_I32};
}
void view2(bdg_table* out, const index_vector_type& v, int cols) {
    *out = {v.data(), cols ? v.size() / cols : 0, cols, BDG_I32};
}
} // namespace

extern "C" {

const char* bdg_last_error(void) { return bdg_detail::g_last_error.c_str(); }
int bdg_version(void) { return 100; }

// ------------------------------------------------------------------ mesh

int bdg_mesh_create(bdg_mesh** out) {
    return guard([&] {
        if (!out) throw bdg_detail::arg_error("bdg_mesh_create: out is NULL");
        *out = new bdg_mesh();
    });
}

void bdg_mesh_destroy(bdg_mesh* mesh) { delete mesh; }

int bdg_mesh_read(bdg_mesh* mesh, const char* path) {
    return guard([&] {
        if (!mesh || !path) throw bdg_detail::arg_error("bdg_mesh_read: NULL argument");
        mesh->mgr.readMesh(path);
    });
}

int bdg_mesh_write(const bdg_mesh* mesh, const char* gmsh_path) {
    return guard([&] {
        if (!mesh || !gmsh_path) throw bdg_detail::arg_error("bdg_mesh_write: NULL argument");
        mesh->mgr.writeMesh(gmsh_path);
    });
}

int bdg_mesh_write_cache(const bdg_mesh* mesh, const char* cache_path) {
    return guard([&] {
        if (!mesh || !cache_path) throw bdg_detail::arg_error("bdg_mesh_write_cache: NULL argument");
        mesh->mgr.writeCache(cache_path);
    });
}

int bdg_mesh_read_cache(bdg_mesh* mesh, const char* cache_path) {
    return guard([&] {
        if (!mesh || !cache_path) throw bdg_detail::arg_error("bdg_mesh_read_cache: NULL argument");
        mesh->mgr.readCache(cache_path);
    });
}

int bdg_mesh_build(bdg_mesh* mesh, const int* etov, int K, const double* vert, int Nv, int dim) {
    return guard([&] {
        if (!mesh || !etov || !vert || K < 1 || Nv < 3) throw bdg_detail::arg_error("bdg_mesh_build: bad argument");
        mesh->mgr.buildMesh(etov, K, vert, Nv, dim);
    });
}

int bdg_mesh_build_box(bdg_mesh* mesh, int nx, int ny, double x0, double x1, double y0, double y1,
                       unsigned long long seed) {
    return guard([&] {
        if (!mesh) throw bdg_detail::arg_error("bdg_mesh_build_box: mesh is NULL");
        mesh->mgr.buildBoxMesh(nx, ny, x0, x1, y0, y1, seed);
    });
}

int bdg_mesh_set_bctype(bdg_mesh* mesh, const int* bctype, int n) {
    return guard([&] {
        if (!mesh || !bctype) throw bdg_detail::arg_error("bdg_mesh_set_bctype: NULL argument");
        mesh->mgr.set_BCType(bctype, n);
    });
}

int bdg_mesh_partition(bdg_mesh* mesh, int nparts) {
    return guard([&] {
        if (!mesh) throw bdg_detail::arg_error("bdg_mesh_partition: mesh is NULL");
        mesh->mgr.partitionMesh(nparts);
    });
}

int bdg_mesh_build_quads(bdg_mesh* mesh, const int* etov, int K, const double* vert, int Nv, int dim) {
    return guard([&] {
        if (!mesh || !etov || !vert || K < 1 || Nv < 4) throw bdg_detail::arg_error("bdg_mesh_build_quads: bad argument");
        mesh->mgr.buildMesh(etov, K, 4, vert, Nv, dim);
    });
}

int bdg_mesh_num_faces(const bdg_mesh* mesh) { return mesh ? mesh->mgr.get_NumFaces() : -1; }
int bdg_mesh_num_elements(const bdg_mesh* mesh) { return mesh ? mesh->mgr.get_NumElements() : -1; }
int bdg_mesh_num_verts(const bdg_mesh* mesh) { return mesh ? mesh->mgr.get_NumVerts() : -1; }

int bdg_mesh_table(const bdg_mesh* mesh, int which, bdg_table* out) {
    return guard([&] {
        if (!mesh || !out) throw bdg_detail::arg_error("bdg_mesh_table: NULL argument");
        const MeshManager& m = mesh->mgr;
        switch (which) {
        case BDG_MESH_VERTICES: *out = {m.get_Vertices().data(), m.get_NumVerts(), m.get_Dim(), BDG_F64}; break;
        case BDG_MESH_ELEMENTS: view2(out, m.get_Elements(), m.get_NumFaces()); break;
        case BDG_MESH_ETOE: view2(out, m.get_EToE(), m.get_NumFaces()); break;
        case BDG_MESH_ETOF: view2(out, m.get_EToF(), m.get_NumFaces()); break;
        case BDG_MESH_BCTYPE: view2(out, m.get_BCType(), m.get_NumFaces()); break;
        case BDG_MESH_EPART: view(out, m.get_ElementPartitionMap()); break;
        case BDG_MESH_NPART: view(out, m.get_VertexPartitionMap()); break;
        default: throw bdg_detail::arg_error("bdg_mesh_table: unknown table id");
        }
    });
}

// ------------------------------------------------------------------ triangle nodes

int bdg_trinodes_create(int order, const bdg_mesh* mesh, bdg_trinodes** out) {
    return guard([&] {
        if (!mesh || !out) throw bdg_detail::arg_error("bdg_trinodes_create: NULL argument");
        if (mesh->mgr.get_NumElements() < 1) throw bdg_detail::arg_error("bdg_trinodes_create: mesh is empty");
        *out = new bdg_trinodes{TriangleNodesProvisioner(order, mesh->mgr)};
    });
}

void bdg_trinodes_destroy(bdg_trinodes* nodes) { delete nodes; }

int bdg_trinodes_build_filter(bdg_trinodes* nodes, double Nc, int s) {
    return guard([&] {
        if (!nodes) throw bdg_detail::arg_error("bdg_trinodes_build_filter: nodes is NULL");
        nodes->prov.buildFilter(Nc, s);
        nodes->hasFilter = true;
    });
}

int bdg_trinodes_build_bchash(bdg_trinodes* nodes, const int* bctype, int n) {
    return guard([&] {
        if (!nodes || !bctype) throw bdg_detail::arg_error("bdg_trinodes_build_bchash: NULL argument");
        index_vector_type bc(n);
        std::copy(bctype, bctype + n, bc.begin());
        nodes->prov.buildBCHash(bc);
    });
}

// Hx, Hy of the variant-B driver (reference src/sw2d/main.cpp:128-133): physical gradient of H, then the
// dealiasing filter applied to each component. Either element family: `fn` names the caller.
} // extern "C"
namespace {
// Acc: the type the sums run in (quadrilaterals: long double, so that the slopes of a deep bed keep 1e-13 of their size at
// order 12, where double sums lose 7e-13 to the cancellation of H's mean; triangles: double, as they always were).
template <typename Acc, typename Prov>
void bedSlopesOf(const Prov& p, const char* fn, const double* H, double* Hx, double* Hy) {
    const int Np = p.get_NumLocalPoints(), K = p.get_NumElements();
    const real_matrix_type& Dr = p.get_Dr(), &Ds = p.get_Ds(), &F = p.get_Filter();
    if (F.rows() != Np) throw bdg_detail::arg_error(std::string(fn) + ": call buildFilter first");
    const real_matrix_type& rx = p.get_rx(), &sx = p.get_sx(), &ry = p.get_ry(), &sy = p.get_sy();
    blitzdg::detail::parallelChunks(K, [&](int kBegin, int kEnd) {
        std::vector<Acc> gx(Np), gy(Np);
        for (int k = kBegin; k < kEnd; ++k) {
            for (int i = 0; i < Np; ++i) {
                Acc dr = 0.0, ds = 0.0;
                for (int m = 0; m < Np; ++m) {
                    const Acc hm = H[static_cast<size_t>(m) * K + k];
                    dr += Dr(i, m) * hm;
                    ds += Ds(i, m) * hm;
                }
                gx[i] = rx(i, k) * dr + sx(i, k) * ds;
                gy[i] = ry(i, k) * dr + sy(i, k) * ds;
            }
            for (int i = 0; i < Np; ++i) {
                Acc ax = 0.0, ay = 0.0;
                for (int m = 0; m < Np; ++m) {
                    ax += F(i, m) * gx[m];
                    ay += F(i, m) * gy[m];
                }
                Hx[static_cast<size_t>(i) * K + k] = static_cast<double>(ax);
                Hy[static_cast<size_t>(i) * K + k] = static_cast<double>(ay);
            }
        }
    });
}

// buildSpongeCoeff (reference src/sw2d/main.cpp:516-556): strength*(1 - d/radius) where d < radius is
// the distance to the closest open-boundary node, 0 elsewhere.
template <typename Prov>
void spongeCoeffOf(const Prov& p, int numFaces, const char* fn, const int* mapO, int num_out, double strength, double radius,
                   double* coeff) {
    const int Np = p.get_NumLocalPoints(), K = p.get_NumElements(), NFN = numFaces * p.get_NumFacePoints();
    const real_matrix_type& x = p.get_xGrid(), &y = p.get_yGrid();
    const index_vector_type& vmapM = p.get_vmapM();
    std::vector<double> xo(num_out), yo(num_out);
    for (int i = 0; i < num_out; ++i) {
        if (mapO[i] < 0 || mapO[i] >= NFN * K) throw bdg_detail::arg_error(std::string(fn) + ": node index out of range");
        const int v = vmapM(mapO[i]);
        xo[i] = x(v % Np, v / Np);
        yo[i] = y(v % Np, v / Np);
    }
    blitzdg::detail::parallelFor(K, [&](int k) {
        for (int n = 0; n < Np; ++n) {
            double closest = 1.0e12;
            for (int i = 0; i < num_out; ++i) {
                const double dist = std::hypot(x(n, k) - xo[i], y(n, k) - yo[i]);
                if (dist < radius && dist < closest) closest = dist;
            }
            coeff[static_cast<size_t>(n) * K + k] = closest < 1.0e12 ? strength * (1.0 - closest / radius) : 0.0;
        }
    }, 16);
}
} // namespace
extern "C" {

int bdg_trinodes_bed_slopes(const bdg_trinodes* nodes, const double* H, double* Hx, double* Hy) {
    return guard([&] {
        if (!nodes || !H || !Hx || !Hy) throw bdg_detail::arg_error("bdg_trinodes_bed_slopes: NULL argument");
        bedSlopesOf<double>(nodes->prov, "bdg_trinodes_bed_slopes", H, Hx, Hy);
    });
}

int bdg_trinodes_sponge_coeff(const bdg_trinodes* nodes, const int* mapO, int num_out, double strength, double radius,
                              double* coeff) {
    return guard([&] {
        if (!nodes || !coeff || num_out < 0 || (num_out > 0 && !mapO))
            throw bdg_detail::arg_error("bdg_trinodes_sponge_coeff: bad argument");
        spongeCoeffOf(nodes->prov, 3, "bdg_trinodes_sponge_coeff", mapO, num_out, strength, radius, coeff);
    });
}

int bdg_quadnodes_bed_slopes(const bdg_quadnodes* nodes, const double* H, double* Hx, double* Hy) {
    return guard([&] {
        if (!nodes || !H || !Hx || !Hy) throw bdg_detail::arg_error("bdg_quadnodes_bed_slopes: NULL argument");
        bedSlopesOf<long double>(nodes->prov, "bdg_quadnodes_bed_slopes", H, Hx, Hy);
    });
}

int bdg_quadnodes_sponge_coeff(const bdg_quadnodes* nodes, const int* mapO, int num_out, double strength, double radius,
                               double* coeff) {
    return guard([&] {
        if (!nodes || !coeff || num_out < 0 || (num_out > 0 && !mapO))
            throw bdg_detail::arg_error("bdg_quadnodes_sponge_coeff: bad argument");
        spongeCoeffOf(nodes->prov, 4, "bdg_quadnodes_sponge_coeff", mapO, num_out, strength, radius, coeff);
    });
}

// ---- output step (reference splitElements + VtkOutputter)
int bdg_trinodes_split_count(const bdg_trinodes* nodes) {
    if (!nodes) return -1;
    const int N = nodes->prov.get_NOrder();
    return N * N;
}

int bdg_trinodes_split_operators(const bdg_trinodes* nodes, double* IM, int* local_triangles) {
    return guard([&] {
        if (!nodes || !IM || !local_triangles) throw bdg_detail::arg_error("bdg_trinodes_split_operators: NULL argument");
        real_matrix_type im;
        std::vector<index_type> tri;
        nodes->prov.splitOperators(im, tri);
        std::copy(im.data(), im.data() + static_cast<size_t>(im.rows()) * im.cols(), IM);
        std::copy(tri.begin(), tri.end(), local_triangles);
    });
}

int bdg_trinodes_split_elements(const bdg_trinodes* nodes, const double* field, double* xnew, double* ynew,
                                double* fieldnew) {
    return guard([&] {
        if (!nodes || !field || !xnew || !ynew || !fieldnew) throw bdg_detail::arg_error("bdg_trinodes_split_elements: NULL argument");
        const auto& p = nodes->prov;
        const int Np = p.get_NumLocalPoints(), K = p.get_NumElements();
        real_matrix_type f(Np, K), xn, yn, fn;
        std::copy(field, field + static_cast<size_t>(Np) * K, f.data());
        p.splitElements(p.get_xGrid(), p.get_yGrid(), f, xn, yn, fn);
        const size_t n = static_cast<size_t>(3) * xn.cols();
        std::copy(xn.data(), xn.data() + n, xnew);
        std::copy(yn.data(), yn.data() + n, ynew);
        std::copy(fn.data(), fn.data() + n, fieldnew);
    });
}

int bdg_trinodes_write_vtu(const bdg_trinodes* nodes, const char* path, const double* field, const char* field_name) {
    return guard([&] {
        if (!nodes || !path || !field || !field_name) throw bdg_detail::arg_error("bdg_trinodes_write_vtu: NULL argument");
        const auto& p = nodes->prov;
        const int Np = p.get_NumLocalPoints(), K = p.get_NumElements();
        real_matrix_type f(Np, K);
        std::copy(field, field + static_cast<size_t>(Np) * K, f.data());
        blitzdg::VtkOutputter(p).writeFieldToFile(path, f, field_name);
    });
}

int bdg_write_vtu_triangles(const char* path, const double* x, const double* y, const double* field, int num_triangles,
                            const char* field_name) {
    return guard([&] {
        if (!path || !x || !y || !field || !field_name || num_triangles < 0)
            throw bdg_detail::arg_error("bdg_write_vtu_triangles: bad argument");
        real_matrix_type xm(3, num_triangles), ym(3, num_triangles), fm(3, num_triangles);
        const size_t n = static_cast<size_t>(3) * num_triangles;
        std::copy(x, x + n, xm.data());
        std::copy(y, y + n, ym.data());
        std::copy(field, field + n, fm.data());
        blitzdg::VtkOutputter::writeTriangles(path, xm, ym, fm, field_name);
    });
}

// ---- the same output step on quadrilaterals (reference QuadNodesProvisioner::splitElements + VtkOutputter's VTK_QUAD branch)
int bdg_quadnodes_split_count(const bdg_quadnodes* nodes) {
    if (!nodes) return -1;
    const int N = nodes->prov.get_NOrder();
    return N * N;
}

int bdg_quadnodes_split_operators(const bdg_quadnodes* nodes, double* IM, double* I1, int* local_quads) {
    return guard([&] {
        if (!nodes || !IM || !I1 || !local_quads) throw bdg_detail::arg_error("bdg_quadnodes_split_operators: NULL argument");
        real_matrix_type im, i1;
        std::vector<index_type> quads;
        nodes->prov.splitOperators(im, i1, quads);
        std::copy(im.data(), im.data() + static_cast<size_t>(im.rows()) * im.cols(), IM);
        std::copy(i1.data(), i1.data() + static_cast<size_t>(i1.rows()) * i1.cols(), I1);
        std::copy(quads.begin(), quads.end(), local_quads);
    });
}

int bdg_quadnodes_split_elements(const bdg_quadnodes* nodes, const double* field, double* xnew, double* ynew,
                                 double* fieldnew) {
    return guard([&] {
        if (!nodes || !field || !xnew || !ynew || !fieldnew) throw bdg_detail::arg_error("bdg_quadnodes_split_elements: NULL argument");
        const auto& p = nodes->prov;
        const int Np = p.get_NumLocalPoints(), K = p.get_NumElements();
        real_matrix_type f(Np, K), xn, yn, fn;
        std::copy(field, field + static_cast<size_t>(Np) * K, f.data());
        p.splitElements(p.get_xGrid(), p.get_yGrid(), f, xn, yn, fn);
        const size_t n = static_cast<size_t>(4) * xn.cols();
        std::copy(xn.data(), xn.data() + n, xnew);
        std::copy(yn.data(), yn.data() + n, ynew);
        std::copy(fn.data(), fn.data() + n, fieldnew);
    });
}

// ---- set-up of the run monitor (bdg_sw2dq_enable_monitor): weights, point location, 1-D basis values
int bdg_quadnodes_quadrature_weights(const bdg_quadnodes* nodes, double* w) {
    return guard([&] {
        if (!nodes || !w) throw bdg_detail::arg_error("bdg_quadnodes_quadrature_weights: NULL argument");
        real_matrix_type m;
        nodes->prov.quadratureWeights(m);
        std::copy(m.data(), m.data() + static_cast<size_t>(m.rows()) * m.cols(), w);
    });
}

int bdg_quadnodes_locate_points(const bdg_quadnodes* nodes, const double* x, const double* y, int n, int* element, double* r,
                                double* s) {
    return guard([&] {
        if (!nodes || n < 0 || (n > 0 && (!x || !y || !element || !r || !s)))
            throw bdg_detail::arg_error("bdg_quadnodes_locate_points: bad argument");
        nodes->prov.locatePoints(x, y, n, element, r, s);
    });
}

int bdg_quadnodes_lagrange_basis(const bdg_quadnodes* nodes, const double* r, int n, double* basis) {
    return guard([&] {
        if (!nodes || n < 0 || (n > 0 && (!r || !basis))) throw bdg_detail::arg_error("bdg_quadnodes_lagrange_basis: bad argument");
        const int Nq = nodes->prov.get_NOrder() + 1;
        for (int p = 0; p < n; ++p) nodes->prov.lagrangeBasis1D(r[p], basis + static_cast<size_t>(p) * Nq);
    });
}

// ---- the same set-up for the triangle solver's monitor (bdg_sw2d_enable_monitor): weights, point location, interpolation rows
int bdg_trinodes_quadrature_weights(const bdg_trinodes* nodes, double* w) {
    return guard([&] {
        if (!nodes || !w) throw bdg_detail::arg_error("bdg_trinodes_quadrature_weights: NULL argument");
        real_matrix_type m;
        nodes->prov.quadratureWeights(m);
        std::copy(m.data(), m.data() + static_cast<size_t>(m.rows()) * m.cols(), w);
    });
}

int bdg_trinodes_locate_points(const bdg_trinodes* nodes, const double* x, const double* y, int n, int* element, double* r,
                               double* s) {
    return guard([&] {
        if (!nodes || n < 0 || (n > 0 && (!x || !y || !element || !r || !s)))
            throw bdg_detail::arg_error("bdg_trinodes_locate_points: bad argument");
        nodes->prov.locatePoints(x, y, n, element, r, s);
    });
}

int bdg_trinodes_interpolation_rows(const bdg_trinodes* nodes, const double* r, const double* s, int n, double* rows) {
    return guard([&] {
        if (!nodes || n < 0 || (n > 0 && (!r || !s || !rows)))
            throw bdg_detail::arg_error("bdg_trinodes_interpolation_rows: bad argument");
        nodes->prov.interpolationRows(r, s, n, rows);
    });
}

// ---- set-up of the triangle solver's drifters (bdg_sw2d_enable_drifters): corner vertices, neighbour table, basis tables
int bdg_trinodes_drifter_tables(const bdg_trinodes* nodes, const int* mapO, int num_out, double* vertices, int* neighbours,
                                double* vinv, double* jacobi) {
    return guard([&] {
        if (!nodes || !vertices || !neighbours || !vinv || !jacobi || num_out < 0 || (num_out > 0 && !mapO))
            throw bdg_detail::arg_error("bdg_trinodes_drifter_tables: bad argument");
        try {
            nodes->prov.drifterTables(mapO, num_out, vertices, neighbours, vinv, jacobi);
        } catch (const std::invalid_argument& e) {
            throw bdg_detail::arg_error(std::string("bdg_trinodes_drifter_tables: ") + e.what());
        }
    });
}

// ... and of the curved solver's (bdg_sw2d_curved_enable_drifters): the same with the side tables of the listed elements
int bdg_trinodes_curved_drifter_tables(const bdg_trinodes* nodes, const int* curved_els, int num_curved, const int* mapO, int num_out,
                                       double* vertices, int* neighbours, double* vinv, double* jacobi, int* curved_slot,
                                       double* modal) {
    return guard([&] {
        if (!nodes || !vertices || !neighbours || !vinv || !jacobi || !curved_slot || num_out < 0 || (num_out > 0 && !mapO) ||
            num_curved < 0 || (num_curved > 0 && (!curved_els || !modal)))
            throw bdg_detail::arg_error("bdg_trinodes_curved_drifter_tables: bad argument");
        try {
            nodes->prov.curvedDrifterTables(curved_els, num_curved, mapO, num_out, vertices, neighbours, vinv, jacobi, curved_slot, modal);
        } catch (const std::invalid_argument& e) {
            throw bdg_detail::arg_error(std::string("bdg_trinodes_curved_drifter_tables: ") + e.what());
        }
    });
}

// ---- set-up of the drifters (bdg_sw2dq_enable_drifters): bilinear map, neighbour table, barycentric weights
int bdg_quadnodes_drifter_tables(const bdg_quadnodes* nodes, const int* mapO, int num_out, double* bilinear, int* neighbours,
                                 double* bary) {
    return guard([&] {
        const std::string fn = "bdg_quadnodes_drifter_tables";
        if (!nodes || !bilinear || !neighbours || !bary || num_out < 0 || (num_out > 0 && !mapO))
            throw bdg_detail::arg_error(fn + ": bad argument");
        const auto& p = nodes->prov;
        const int N = p.get_NOrder(), Nq = N + 1, Np = p.get_NumLocalPoints(), K = p.get_NumElements(), NFN = 4 * Nq;
        const real_matrix_type& x = p.get_xGrid(), &y = p.get_yGrid();
        const real_vector_type& r1d = p.get_r1d();
        const int c00 = 0, c10 = Nq * N, c01 = N, c11 = Np - 1;
        for (int k = 0; k < K; ++k) {
            double* b = bilinear + static_cast<size_t>(8) * k;
            const real_matrix_type* g[2] = {&x, &y};
            for (int c = 0; c < 2; ++c) {
                const double v00 = (*g[c])(c00, k), v10 = (*g[c])(c10, k), v01 = (*g[c])(c01, k), v11 = (*g[c])(c11, k);
                b[4 * c + 0] = (v00 + v10 + v01 + v11) / 4;
                b[4 * c + 1] = (v10 - v00 + v11 - v01) / 4;
                b[4 * c + 2] = (v01 - v00 + v11 - v10) / 4;
                b[4 * c + 3] = (v00 - v10 - v01 + v11) / 4;
            }
            // a mesh whose nodes have left this map (deformed coordinates) is not bilinear: the drifters cannot follow it
            const double size = std::max(std::hypot(b[1], b[5]), std::hypot(b[2], b[6]));
            for (int j = 0; j < Nq; ++j)
                for (int i = 0; i < Nq; ++i) {
                    const double r = r1d(j), s = r1d(i);
                    const double ex = b[0] + b[1] * r + b[2] * s + b[3] * r * s - x(Nq * j + i, k);
                    const double ey = b[4] + b[5] * r + b[6] * s + b[7] * r * s - y(Nq * j + i, k);
                    if (!(std::hypot(ex, ey) <= 1e-10 * size))
                        throw bdg_detail::arg_error(fn + ": the nodes of element " + std::to_string(k) + " differ from the bilinear map of "
                                                    "its corners; drifters need bilinear elements");
                }
        }
        // faces in Fmask order (s = -1, r = +1, s = +1, r = -1), which is the mesh's face order
        const index_vector_type& E2E = p.get_MeshManager().get_EToE();
        std::vector<char> open(static_cast<size_t>(4) * K, 0);
        for (int i = 0; i < num_out; ++i) {
            if (mapO[i] < 0 || mapO[i] >= NFN * K) throw bdg_detail::arg_error(fn + ": open-boundary node index out of range");
            open[static_cast<size_t>(mapO[i] / NFN) * 4 + mapO[i] % NFN / Nq] = 1;
        }
        const index_vector_type& vmapM = p.get_vmapM(), &vmapP = p.get_vmapP();
        for (int k = 0; k < K; ++k)
            for (int f = 0; f < 4; ++f) {
                const int k2 = E2E(4 * k + f);
                // (a boundary face is its own neighbour in EToE and maps its nodes onto themselves)
                const size_t g = (static_cast<size_t>(k) * 4 + f) * Nq;
                const bool boundary = k2 == k && vmapP(g) == vmapM(g);
                neighbours[static_cast<size_t>(f) * K + k] = boundary ? (open[static_cast<size_t>(k) * 4 + f] ? -2 : -1) : k2;
            }
        for (int a = 0; a < Nq; ++a) {
            double c = 1;
            for (int b = 0; b < Nq; ++b)
                if (b != a) c *= r1d(a) - r1d(b);
            bary[a] = 1 / c;
        }
    });
}

int bdg_quadnodes_write_vtu(const bdg_quadnodes* nodes, const char* path, const double* field, const char* field_name) {
    return guard([&] {
        if (!nodes || !path || !field || !field_name) throw bdg_detail::arg_error("bdg_quadnodes_write_vtu: NULL argument");
        const auto& p = nodes->prov;
        const int Np = p.get_NumLocalPoints(), K = p.get_NumElements();
        real_matrix_type f(Np, K);
        std::copy(field, field + static_cast<size_t>(Np) * K, f.data());
        blitzdg::VtkOutputter(p).writeFieldToFile(path, f, field_name);
    });
}

int bdg_write_vtu_quads(const char* path, const double* x, const double* y, const double* field, int num_quads,
                        const char* field_name) {
    return guard([&] {
        if (!path || !x || !y || !field || !field_name || num_quads < 0)
            throw bdg_detail::arg_error("bdg_write_vtu_quads: bad argument");
        real_matrix_type xm(4, num_quads), ym(4, num_quads), fm(4, num_quads);
        const size_t n = static_cast<size_t>(4) * num_quads;
        std::copy(x, x + n, xm.data());
        std::copy(y, y + n, ym.data());
        std::copy(field, field + n, fm.data());
        blitzdg::VtkOutputter::writeQuads(path, xm, ym, fm, field_name);
    });
}

int bdg_trinodes_set_coordinates(bdg_trinodes* nodes, const double* x, const double* y) {
    return guard([&] {
        if (!nodes || !x || !y) throw bdg_detail::arg_error("bdg_trinodes_set_coordinates: NULL argument");
        nodes->prov.setCoordinates(x, y);
    });
}

int bdg_trinodes_dims(const bdg_trinodes* nodes, int* order, int* np, int* nfp, int* K) {
    return guard([&] {
        if (!nodes) throw bdg_detail::arg_error("bdg_trinodes_dims: nodes is NULL");
        if (order) *order = nodes->prov.get_NOrder();
        if (np) *np = nodes->prov.get_NumLocalPoints();
        if (nfp) *nfp = nodes->prov.get_NumFacePoints();
        if (K) *K = nodes->prov.get_NumElements();
    });
}

int bdg_trinodes_table(const bdg_trinodes* nodes, int which, bdg_table* out) {
    return guard([&] {
        if (!nodes || !out) throw bdg_detail::arg_error("bdg_trinodes_table: NULL argument");
        const TriangleNodesProvisioner& p = nodes->prov;
        switch (which) {
        case BDG_TRI_R: view(out, p.get_rGrid()); break;
        case BDG_TRI_S: view(out, p.get_sGrid()); break;
        case BDG_TRI_X: view(out, p.get_xGrid()); break;
        case BDG_TRI_Y: view(out, p.get_yGrid()); break;
        case BDG_TRI_V: view(out, p.get_V()); break;
        case BDG_TRI_VINV: view(out, p.get_Vinv()); break;
        case BDG_TRI_DR: view(out, p.get_Dr()); break;
        case BDG_TRI_DS: view(out, p.get_Ds()); break;
        case BDG_TRI_DRW: view(out, p.get_Drw()); break;
        case BDG_TRI_DSW: view(out, p.get_Dsw()); break;
        case BDG_TRI_LIFT: view(out, p.get_Lift()); break;
        case BDG_TRI_FILTER: view(out, p.get_Filter()); break;
        case BDG_TRI_J: view(out, p.get_J()); break;
        case BDG_TRI_RX: view(out, p.get_rx()); break;
        case BDG_TRI_RY: view(out, p.get_ry()); break;
        case BDG_TRI_SX: view(out, p.get_sx()); break;
        case BDG_TRI_SY: view(out, p.get_sy()); break;
        case BDG_TRI_NX: view(out, p.get_nx()); break;
        case BDG_TRI_NY: view(out, p.get_ny()); break;
        case BDG_TRI_FSCALE: view(out, p.get_Fscale()); break;
        case BDG_TRI_FMASK: view(out, p.get_Fmask()); break;
        case BDG_TRI_FX: view(out, p.get_Fx()); break;
        case BDG_TRI_FY: view(out, p.get_Fy()); break;
        case BDG_TRI_VMAPM: view(out, p.get_vmapM()); break;
        case BDG_TRI_VMAPP: view(out, p.get_vmapP()); break;
        case BDG_TRI_MAPP: view(out, p.get_mapP()); break;
        case BDG_TRI_VMAPB: view(out, p.get_vmapB()); break;
        case BDG_TRI_MAPB: view(out, p.get_mapB()); break;
        case BDG_TRI_GATHER: view(out, p.get_gather()); break;
        case BDG_TRI_SCATTER: view(out, p.get_scatter()); break;
        default: throw bdg_detail::arg_error("bdg_trinodes_table: unknown table id");
        }
    });
}

int bdg_trinodes_bcmap_num_tags(const bdg_trinodes* nodes) {
    return nodes ? static_cast<int>(nodes->prov.get_bcMap().size()) : -1;
}

int bdg_trinodes_bcmap_tags(const bdg_trinodes* nodes, int* tags, int capacity) {
    return guard([&] {
        if (!nodes || !tags) throw bdg_detail::arg_error("bdg_trinodes_bcmap_tags: NULL argument");
        std::vector<int> keys;
        for (const auto& kv : nodes->prov.get_bcMap()) keys.push_back(kv.first);
        std::sort(keys.begin(), keys.end());
        if (static_cast<int>(keys.size()) > capacity) throw bdg_detail::arg_error("bdg_trinodes_bcmap_tags: capacity too small");
        std::copy(keys.begin(), keys.end(), tags);
    });
}

int bdg_trinodes_bcmap_nodes(const bdg_trinodes* nodes, int tag, const int** out, int* count) {
    return guard([&] {
        if (!nodes || !out || !count) throw bdg_detail::arg_error("bdg_trinodes_bcmap_nodes: NULL argument");
        const auto& map = nodes->prov.get_bcMap();
        const auto it = map.find(tag);
        if (it == map.end()) { *out = nullptr; *count = 0; return; }
        *out = it->second.data();
        *count = static_cast<int>(it->second.size());
    });
}

// ------------------------------------------------------------------ quadrilateral nodes
// The bdg_trinodes_* shape over QuadNodesProvisioner. Tables use the BDG_TRI_* ids; the ones a quadrilateral
// provisioner does not build are refused.
int bdg_quadnodes_create(int order, const bdg_mesh* mesh, bdg_quadnodes** out) {
    return guard([&] {
        if (!mesh || !out) throw bdg_detail::arg_error("bdg_quadnodes_create: NULL argument");
        if (mesh->mgr.get_NumElements() < 1) throw bdg_detail::arg_error("bdg_quadnodes_create: mesh is empty");
        if (mesh->mgr.get_NumFaces() != 4)
            throw bdg_detail::arg_error("bdg_quadnodes_create: the mesh holds triangles (use bdg_trinodes_create)");
        if (order < 1) throw bdg_detail::arg_error("bdg_quadnodes_create: order must be >= 1");
        *out = new bdg_quadnodes{QuadNodesProvisioner(order, mesh->mgr)};
    });
}

void bdg_quadnodes_destroy(bdg_quadnodes* nodes) { delete nodes; }

int bdg_quadnodes_build_filter(bdg_quadnodes* nodes, double Nc, int s) {
    return guard([&] {
        if (!nodes) throw bdg_detail::arg_error("bdg_quadnodes_build_filter: nodes is NULL");
        nodes->prov.buildFilter(Nc, s);
        nodes->hasFilter = true;
    });
}

int bdg_quadnodes_build_bchash(bdg_quadnodes* nodes, const int* bctype, int n) {
    return guard([&] {
        if (!nodes || !bctype) throw bdg_detail::arg_error("bdg_quadnodes_build_bchash: NULL argument");
        index_vector_type bc(n);
        std::copy(bctype, bctype + n, bc.begin());
        nodes->prov.buildBCHash(bc);
    });
}

int bdg_quadnodes_dims(const bdg_quadnodes* nodes, int* order, int* np, int* nfp, int* K) {
    return guard([&] {
        if (!nodes) throw bdg_detail::arg_error("bdg_quadnodes_dims: nodes is NULL");
        if (order) *order = nodes->prov.get_NOrder();
        if (np) *np = nodes->prov.get_NumLocalPoints();
        if (nfp) *nfp = nodes->prov.get_NumFacePoints();
        if (K) *K = nodes->prov.get_NumElements();
    });
}

int bdg_quadnodes_table(const bdg_quadnodes* nodes, int which, bdg_table* out) {
    return guard([&] {
        if (!nodes || !out) throw bdg_detail::arg_error("bdg_quadnodes_table: NULL argument");
        const QuadNodesProvisioner& p = nodes->prov;
        switch (which) {
        case BDG_TRI_R: view(out, p.get_rGrid()); break;
        case BDG_TRI_S: view(out, p.get_sGrid()); break;
        case BDG_TRI_X: view(out, p.get_xGrid()); break;
        case BDG_TRI_Y: view(out, p.get_yGrid()); break;
        case BDG_TRI_V: view(out, p.get_V()); break;
        case BDG_TRI_VINV: view(out, p.get_Vinv()); break;
        case BDG_TRI_DR: view(out, p.get_Dr()); break;
        case BDG_TRI_DS: view(out, p.get_Ds()); break;
        case BDG_TRI_LIFT: view(out, p.get_Lift()); break;
        case BDG_TRI_FILTER: view(out, p.get_Filter()); break;
        case BDG_TRI_J: view(out, p.get_J()); break;
        case BDG_TRI_RX: view(out, p.get_rx()); break;
        case BDG_TRI_RY: view(out, p.get_ry()); break;
        case BDG_TRI_SX: view(out, p.get_sx()); break;
        case BDG_TRI_SY: view(out, p.get_sy()); break;
        case BDG_TRI_NX: view(out, p.get_nx()); break;
        case BDG_TRI_NY: view(out, p.get_ny()); break;
        case BDG_TRI_FSCALE: view(out, p.get_Fscale()); break;
        case BDG_TRI_FMASK: view(out, p.get_Fmask()); break;
        case BDG_TRI_VMAPM: view(out, p.get_vmapM()); break;
        case BDG_TRI_VMAPP: view(out, p.get_vmapP()); break;
        case BDG_TRI_MAPP: view(out, p.get_mapP()); break;
        case BDG_TRI_VMAPB: view(out, p.get_vmapB()); break;
        case BDG_TRI_MAPB: view(out, p.get_mapB()); break;
        default: throw bdg_detail::arg_error("bdg_quadnodes_table: table not built for quadrilaterals");
        }
    });
}

int bdg_quadnodes_bcmap_num_tags(const bdg_quadnodes* nodes) {
    return nodes ? static_cast<int>(nodes->prov.get_bcMap().size()) : -1;
}

int bdg_quadnodes_bcmap_tags(const bdg_quadnodes* nodes, int* tags, int capacity) {
    return guard([&] {
        if (!nodes || !tags) throw bdg_detail::arg_error("bdg_quadnodes_bcmap_tags: NULL argument");
        std::vector<int> keys;
        for (const auto& kv : nodes->prov.get_bcMap()) keys.push_back(kv.first);
        std::sort(keys.begin(), keys.end());
        if (static_cast<int>(keys.size()) > capacity) throw bdg_detail::arg_error("bdg_quadnodes_bcmap_tags: capacity too small");
        std::copy(keys.begin(), keys.end(), tags);
    });
}

int bdg_quadnodes_bcmap_nodes(const bdg_quadnodes* nodes, int tag, const int** out, int* count) {
    return guard([&] {
        if (!nodes || !out || !count) throw bdg_detail::arg_error("bdg_quadnodes_bcmap_nodes: NULL argument");
        const auto& map = nodes->prov.get_bcMap();
        const auto it = map.find(tag);
        if (it == map.end()) { *out = nullptr; *count = 0; return; }
        *out = it->second.data();
        *count = static_cast<int>(it->second.size());
    });
}

// ------------------------------------------------------------------ Gauss face / cubature contexts

int bdg_trinodes_build_gauss_face_nodes(bdg_trinodes* nodes, int NGauss, bdg_gaussctx** out) {
    return guard([&] {
        if (!nodes || !out) throw bdg_detail::arg_error("bdg_trinodes_build_gauss_face_nodes: NULL argument");
        if (NGauss < 1) throw bdg_detail::arg_error("bdg_trinodes_build_gauss_face_nodes: NGauss must be >= 1");
        *out = new bdg_gaussctx{nodes->prov.buildGaussFaceNodes(NGauss)};
    });
}

void bdg_gaussctx_destroy(bdg_gaussctx* ctx) { delete ctx; }
int bdg_gaussctx_ngauss(const bdg_gaussctx* ctx) { return ctx ? ctx->ctx.NGauss() : -1; }

int bdg_gaussctx_table(const bdg_gaussctx* ctx, int which, bdg_table* out) {
    return guard([&] {
        if (!ctx || !out) throw bdg_detail::arg_error("bdg_gaussctx_table: NULL argument");
        const GaussFaceContext2D& g = ctx->ctx;
        switch (which) {
        case BDG_GAUSS_NX: view(out, g.nx()); break;
        case BDG_GAUSS_NY: view(out, g.ny()); break;
        case BDG_GAUSS_SJ: view(out, g.sJ()); break;
        case BDG_GAUSS_J: view(out, g.Jac()); break;
        case BDG_GAUSS_RX: view(out, g.rx()); break;
        case BDG_GAUSS_RY: view(out, g.ry()); break;
        case BDG_GAUSS_SX: view(out, g.sx()); break;
        case BDG_GAUSS_SY: view(out, g.sy()); break;
        case BDG_GAUSS_X: view(out, g.x()); break;
        case BDG_GAUSS_Y: view(out, g.y()); break;
        case BDG_GAUSS_W: view(out, g.W()); break;
        case BDG_GAUSS_INTERP: view(out, g.Interp()); break;
        case BDG_GAUSS_MAPM: view(out, g.mapM()); break;
        case BDG_GAUSS_MAPP: view(out, g.mapP()); break;
        default: throw bdg_detail::arg_error("bdg_gaussctx_table: unknown table id");
        }
    });
}

int bdg_gaussctx_bcmap_num_tags(const bdg_gaussctx* ctx) { return ctx ? static_cast<int>(ctx->ctx.bcMap().size()) : -1; }

int bdg_gaussctx_bcmap_tags(const bdg_gaussctx* ctx, int* tags, int capacity) {
    return guard([&] {
        if (!ctx || (!tags && capacity > 0)) throw bdg_detail::arg_error("bdg_gaussctx_bcmap_tags: NULL argument");
        std::vector<int> keys;
        for (const auto& kv : ctx->ctx.bcMap()) keys.push_back(kv.first);
        std::sort(keys.begin(), keys.end());
        if (static_cast<int>(keys.size()) > capacity) throw bdg_detail::arg_error("bdg_gaussctx_bcmap_tags: capacity too small");
        std::copy(keys.begin(), keys.end(), tags);
    });
}

int bdg_gaussctx_bcmap_nodes(const bdg_gaussctx* ctx, int tag, const int** out, int* count) {
    return guard([&] {
        if (!ctx || !out || !count) throw bdg_detail::arg_error("bdg_gaussctx_bcmap_nodes: NULL argument");
        const auto it = ctx->ctx.bcMap().find(tag);
        if (it == ctx->ctx.bcMap().end()) { *out = nullptr; *count = 0; return; }
        *out = it->second.data();
        *count = static_cast<int>(it->second.size());
    });
}

int bdg_trinodes_build_cubature_volume_mesh(bdg_trinodes* nodes, int NCubature, bdg_cubctx** out) {
    return guard([&] {
        if (!nodes || !out) throw bdg_detail::arg_error("bdg_trinodes_build_cubature_volume_mesh: NULL argument");
        if (NCubature < 1) throw bdg_detail::arg_error("bdg_trinodes_build_cubature_volume_mesh: NCubature must be >= 1");
        *out = new bdg_cubctx{nodes->prov.buildCubatureVolumeMesh(NCubature)};
    });
}

int bdg_cubature_rule_num_points(int NCubature) {
    int n = -1;
    guard([&] { n = TriangleCubatureRules(NCubature).NumCubaturePoints(); });
    return n;
}

int bdg_cubature_rule(int NCubature, double* r, double* s, double* w) {
    return guard([&] {
        if (!r || !s || !w) throw bdg_detail::arg_error("bdg_cubature_rule: NULL argument");
        const TriangleCubatureRules rule(NCubature);
        const real_vector_type rr = rule.rCoord(), ss = rule.sCoord(), ww = rule.weights();
        for (index_type i = 0; i < rule.NumCubaturePoints(); ++i) { r[i] = rr(i); s[i] = ss(i); w[i] = ww(i); }
    });
}

void bdg_cubctx_destroy(bdg_cubctx* ctx) { delete ctx; }
int bdg_cubctx_num_points(const bdg_cubctx* ctx) { return ctx ? ctx->ctx.NumCubaturePoints() : -1; }
int bdg_cubctx_order(const bdg_cubctx* ctx) { return ctx ? ctx->ctx.NCubature() : -1; }

int bdg_cubctx_table(const bdg_cubctx* ctx, int which, bdg_table* out) {
    return guard([&] {
        if (!ctx || !out) throw bdg_detail::arg_error("bdg_cubctx_table: NULL argument");
        const CubatureContext2D& c = ctx->ctx;
        auto view3 = [&](const real_tensor3_type& t) {
            *out = {t.data(), t.length(0) * t.length(1), t.length(2), BDG_F64};
        };
        switch (which) {
        case BDG_CUB_R: view(out, c.r()); break;
        case BDG_CUB_S: view(out, c.s()); break;
        case BDG_CUB_WEIGHTS: view(out, c.w()); break;
        case BDG_CUB_V: view(out, c.V()); break;
        case BDG_CUB_RX: view(out, c.rx()); break;
        case BDG_CUB_RY: view(out, c.ry()); break;
        case BDG_CUB_SX: view(out, c.sx()); break;
        case BDG_CUB_SY: view(out, c.sy()); break;
        case BDG_CUB_J: view(out, c.Jac()); break;
        case BDG_CUB_DR: view(out, c.Dr()); break;
        case BDG_CUB_DS: view(out, c.Ds()); break;
        case BDG_CUB_MM: view3(c.MM()); break;
        case BDG_CUB_MMCHOL: view3(c.MMChol()); break;
        case BDG_CUB_X: view(out, c.x()); break;
        case BDG_CUB_Y: view(out, c.y()); break;
        case BDG_CUB_W: view(out, c.W()); break;
        default: throw bdg_detail::arg_error("bdg_cubctx_table: unknown table id");
        }
    });
}

// ------------------------------------------------------------------ 1-D nodes

int bdg_nodes1d_create(int order, int K, double xmin, double xmax, bdg_nodes1d** out) {
    return guard([&] {
        if (!out || order < 1 || K < 1 || !(xmax > xmin)) throw bdg_detail::arg_error("bdg_nodes1d_create: bad argument");
        *out = new bdg_nodes1d{Nodes1DProvisioner(order, K, xmin, xmax)};
    });
}

void bdg_nodes1d_destroy(bdg_nodes1d* nodes) { delete nodes; }

int bdg_nodes1d_build_nodes(bdg_nodes1d* nodes) {
    return guard([&] {
        if (!nodes) throw bdg_detail::arg_error("bdg_nodes1d_build_nodes: nodes is NULL");
        nodes->prov.buildNodes();
    });
}

int bdg_nodes1d_compute_jacobian(bdg_nodes1d* nodes) {
    return guard([&] {
        if (!nodes) throw bdg_detail::arg_error("bdg_nodes1d_compute_jacobian: nodes is NULL");
        nodes->prov.computeJacobian();
    });
}

int bdg_nodes1d_map_i(const bdg_nodes1d* nodes) { return nodes ? nodes->prov.get_mapI() : -1; }
int bdg_nodes1d_map_o(const bdg_nodes1d* nodes) { return nodes ? nodes->prov.get_mapO() : -1; }

int bdg_nodes1d_table(const bdg_nodes1d* nodes, int which, bdg_table* out) {
    return guard([&] {
        if (!nodes || !out) throw bdg_detail::arg_error("bdg_nodes1d_table: NULL argument");
        const Nodes1DProvisioner& p = nodes->prov;
        switch (which) {
        case BDG_N1D_R: view(out, p.get_rGrid()); break;
        case BDG_N1D_X: view(out, p.get_xGrid()); break;
        case BDG_N1D_V: view(out, p.get_V()); break;
        case BDG_N1D_VINV: view(out, p.get_Vinv()); break;
        case BDG_N1D_DR: view(out, p.get_Dr()); break;
        case BDG_N1D_LIFT: view(out, p.get_Lift()); break;
        case BDG_N1D_J: view(out, p.get_J()); break;
        case BDG_N1D_RX: view(out, p.get_rx()); break;
        case BDG_N1D_NX: view(out, p.get_nx()); break;
        case BDG_N1D_FMASK: view(out, p.get_Fmask()); break;
        case BDG_N1D_FX: view(out, p.get_Fx()); break;
        case BDG_N1D_FSCALE: view(out, p.get_Fscale()); break;
        case BDG_N1D_ETOV: view(out, p.get_EToV()); break;
        case BDG_N1D_ETOE: view(out, p.get_EToE()); break;
        case BDG_N1D_ETOF: view(out, p.get_EToF()); break;
        case BDG_N1D_VMAPM: view(out, p.get_vmapM()); break;
        case BDG_N1D_VMAPP: view(out, p.get_vmapP()); break;
        default: throw bdg_detail::arg_error("bdg_nodes1d_table: unknown table id");
        }
    });
}

int bdg_lserk4_num_stages(void) { return LSERK4::numStages; }
const double* bdg_lserk4_a(void) { return LSERK4::rk4a; }
const double* bdg_lserk4_b(void) { return LSERK4::rk4b; }

int bdg_vandermonde1d(const double* r, int num_points, int num_cols, double* V, double* Vinv) {
    return guard([&] {
        if (!r || !V || num_points < 1 || num_cols < 1) throw bdg_detail::arg_error("bdg_vandermonde1d: bad argument");
        if (Vinv && num_points != num_cols)
            throw bdg_detail::arg_error("bdg_vandermonde1d: the inverse needs a square matrix (num_points == num_cols)");
        real_vector_type rv(num_points);
        std::copy(r, r + num_points, rv.data());
        real_matrix_type Vm(num_points, num_cols), Vi(num_cols, num_cols);
        blitzdg::VandermondeBuilders().computeVandermondeMatrix(rv, Vm, Vi, Vinv != nullptr);
        std::copy(Vm.data(), Vm.data() + static_cast<size_t>(num_points) * num_cols, V);
        if (Vinv) std::copy(Vi.data(), Vi.data() + static_cast<size_t>(num_cols) * num_cols, Vinv);
    });
}

int bdg_nodes1d_advec_rhs(bdg_nodes1d* nodes, const double* u, double c, double* rhs) {
    return guard([&] {
        if (!nodes || !u || !rhs) throw bdg_detail::arg_error("bdg_nodes1d_advec_rhs: NULL argument");
        auto& p = nodes->prov;
        const int Np = p.get_NumLocalPoints(), K = p.get_NumElements();
        real_matrix_type um(Np, K), out(Np, K);
        std::copy(u, u + static_cast<size_t>(Np) * K, um.data());
        blitzdg::advec1d::computeRHS(um, c, p, out);
        std::copy(out.data(), out.data() + static_cast<size_t>(Np) * K, rhs);
    });
}

int bdg_advec1d_run(int order, int K, double xmin, double xmax, double c, double cfl, double final_time,
                    double* max_error, int* num_steps) {
    return guard([&] {
        if (!max_error || order < 1 || K < 1 || c == 0.0) throw bdg_detail::arg_error("bdg_advec1d_run: bad argument");
        index_type steps = 0;
        *max_error = advec1d::run(order, K, xmin, xmax, c, cfl, final_time, &steps);
        if (num_steps) *num_steps = steps;
    });
}

int bdg_nodes1d_burgers_rhs(bdg_nodes1d* nodes, const double* u, double t, double c, double alpha, double nu, double* rhs) {
    return guard([&] {
        if (!nodes || !u || !rhs) throw bdg_detail::arg_error("bdg_nodes1d_burgers_rhs: NULL argument");
        if (alpha == 0.0 || nu <= 0.0) throw bdg_detail::arg_error("bdg_nodes1d_burgers_rhs: need alpha != 0 and nu > 0");
        auto& p = nodes->prov;
        const int Np = p.get_NumLocalPoints(), K = p.get_NumElements();
        real_matrix_type um(Np, K), out(Np, K);
        std::copy(u, u + static_cast<size_t>(Np) * K, um.data());
        blitzdg::burgers1d::computeRHS(um, p.get_xGrid(), t, c, alpha, nu, p, out);
        std::copy(out.data(), out.data() + static_cast<size_t>(Np) * K, rhs);
    });
}

int bdg_burgers1d_run(int order, int K, double xmin, double xmax, double alpha, double nu, double c, double cfl, double final_time,
                      double* max_error, int* num_steps) {
    return guard([&] {
        if (!max_error || order < 1 || K < 1 || c == 0.0 || alpha == 0.0 || nu <= 0.0)
            throw bdg_detail::arg_error("bdg_burgers1d_run: bad argument");
        index_type steps = 0;
        *max_error = burgers1d::run(order, K, xmin, xmax, alpha, nu, c, cfl, final_time, &steps);
        if (num_steps) *num_steps = steps;
    });
}

// The numbering and the renumbering rule of the sw2d solvers (element_order.hpp) for callers without a GPU.
int bdg_element_order(const int* EToE, int num_elements, int patch, int* perm) {
    return guard([&] {
        if (!EToE || !perm || num_elements < 1) throw bdg_detail::arg_error("bdg_element_order: bad argument");
        const std::vector<int> p = blitzdg::element_order::renumbering(EToE, num_elements, 1, 1, patch);
        std::copy(p.begin(), p.end(), perm);
    });
}

int bdg_element_order_wanted(const int* EToE, int num_elements, int order) {
    int wanted = -1;
    guard([&] {
        if (!EToE || num_elements < 1 || order < 1) throw bdg_detail::arg_error("bdg_element_order_wanted: bad argument");
        wanted = blitzdg::element_order::renumberingWanted(EToE, num_elements, 1, 1, order) ? 1 : 0;
    });
    return wanted;
}

} // extern "C"
