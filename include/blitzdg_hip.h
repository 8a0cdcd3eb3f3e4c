/* blitzdg_hip.h -- C ABI of the MI355X-native blitzdg hot path.
 *
 * One shared library (libblitzdg_hip.so) with two groups of entry points:
 *
 *  (1) Host setup handles (CPU): mesh, 2-D triangle nodes provisioner, 1-D nodes
 *      provisioner. They build exactly the tables the reference's C++ classes
 *      build and export them as borrowed (pointer, rows, cols) views. This is the
 *      seam the reference crosses with boost::python in src/pyblitzdg/pyblitzdg.cpp
 *      :59-201 (MeshManager, TriangleNodesProvisioner/DGContext2D,
 *      Nodes1DProvisioner, LSERK4); blitzdg_amd/pyblitzdg.py binds it with ctypes.
 *
 *  (2) The device-resident sw2d solver (HIP, gfx950): right-hand-side evaluation
 *      and Runge-Kutta stage updates of the 2-D shallow-water nodal DG scheme.
 *      bdg_sw2d_rhs replaces blitzdg::sw2d::computeRHS
 *      (reference src/sw2d-simple/main.cpp:181-356, decl SW2d.hpp:15);
 *      bdg_sw2d_step_lserk4 replaces the LSERK4 stage loop
 *      (src/advec1d/main.cpp:92-102 with include/LSERK4.hpp:15-29);
 *      bdg_sw2d_step_rk2 replaces the midpoint-RK2 + filter loop body
 *      (src/sw2d-simple/main.cpp:132-151); bdg_sw2d_compute_dt replaces the
 *      time-step/blow-up reductions (src/sw2d-simple/main.cpp:98-109,153-167).
 *
 * Conventions: every (rows, K) field/table is row-major fp64 with K (the element
 * index) contiguous, as in the reference (include/Types.hpp:16-18); index tables
 * are int32 and use the reference's column-wise node numbering n + Np*k.
 * Every function returns 0 on success or a BDG_ERR_* code; bdg_last_error()
 * returns a thread-local message. No exceptions cross this boundary. A handle
 * must be used from one host thread at a time.
 */
#ifndef BLITZDG_HIP_H
#define BLITZDG_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BDG_OK 0
#define BDG_ERR_ARGUMENT 1  /* null pointer, bad size, unsupported order ...   */
#define BDG_ERR_RUNTIME 2   /* I/O or setup failure (message has the details) */
#define BDG_ERR_HIP 3       /* a HIP call failed / no usable device            */
#define BDG_ERR_UNSTABLE 4  /* NaN or |eta| > 1e8 detected ("A numerical instability has occurred!") */

typedef struct bdg_mesh bdg_mesh;
typedef struct bdg_trinodes bdg_trinodes;
typedef struct bdg_quadnodes bdg_quadnodes;
typedef struct bdg_nodes1d bdg_nodes1d;
typedef struct bdg_gaussctx bdg_gaussctx;
typedef struct bdg_cubctx bdg_cubctx;
typedef struct bdg_sw2d bdg_sw2d;
typedef struct bdg_sw2dq bdg_sw2dq;

const char* bdg_last_error(void);
int bdg_version(void);

/* ---------------------------------------------------------------- tables */

/* dtype codes of a table view */
#define BDG_F64 0
#define BDG_I32 1

/* Borrowed view of a host table; valid until the owning handle is destroyed or rebuilt. */
typedef struct bdg_table {
    const void* data;
    int rows;   /* 1-D tables: rows = length, cols = 1 */
    int cols;
    int dtype;  /* BDG_F64 or BDG_I32 */
} bdg_table;

/* ---------------------------------------------------------------- MeshManager
 * reference: include/MeshManager.hpp:23-232, src/MeshManager.cpp */
enum {
    BDG_MESH_VERTICES = 0, /* (Nv, 3) f64 */
    BDG_MESH_ELEMENTS = 1, /* (K, 3) i32, CCW */
    BDG_MESH_ETOE = 2,     /* (K, 3) i32 */
    BDG_MESH_ETOF = 3,     /* (K, 3) i32 */
    BDG_MESH_BCTYPE = 4,   /* (K, 3) i32: 0 interior, 3 wall ... */
    BDG_MESH_EPART = 5,    /* (K) i32, after bdg_mesh_partition */
    BDG_MESH_NPART = 6     /* (Nv) i32, after bdg_mesh_partition */
};
int bdg_mesh_create(bdg_mesh** out);
void bdg_mesh_destroy(bdg_mesh* mesh);
int bdg_mesh_read(bdg_mesh* mesh, const char* gmsh_path);                 /* readMesh   */
int bdg_mesh_write(const bdg_mesh* mesh, const char* gmsh_path);          /* Gmsh 2.2 ASCII, what readMesh takes */
/* binary cache of a mesh with its connectivity, BC table and partition maps (MeshManager::writeCache / readCache; the
 * reference has none: SURVEY 8f.2). read_cache refuses files whose magic, version, sizes, index ranges or checksum do not fit. */
int bdg_mesh_write_cache(const bdg_mesh* mesh, const char* cache_path);
int bdg_mesh_read_cache(bdg_mesh* mesh, const char* cache_path);
int bdg_mesh_build(bdg_mesh* mesh, const int* etov, int num_elements,     /* buildMesh  */
                   const double* vert, int num_verts, int dim);
int bdg_mesh_build_box(bdg_mesh* mesh, int nx, int ny, double x0, double x1, double y0, double y1,
                       unsigned long long shuffle_seed);                  /* synthetic box, K = 2*nx*ny */
int bdg_mesh_set_bctype(bdg_mesh* mesh, const int* bctype, int n);        /* setBCType  */
int bdg_mesh_partition(bdg_mesh* mesh, int num_partitions);               /* partitionMesh */
/* buildMesh of quadrangles: etov is (num_elements, 4); a clockwise quadrangle (a, b, c, d) is stored as (a, d, c, b) */
int bdg_mesh_build_quads(bdg_mesh* mesh, const int* etov, int num_elements, const double* vert, int num_verts, int dim);
int bdg_mesh_num_faces(const bdg_mesh* mesh); /* 3: triangles, 4: quadrangles (the mesh tables have this many columns) */
int bdg_mesh_num_elements(const bdg_mesh* mesh);
int bdg_mesh_num_verts(const bdg_mesh* mesh);
int bdg_mesh_table(const bdg_mesh* mesh, int which, bdg_table* out);

/* ---------------------------------------------------------------- TriangleNodesProvisioner / DGContext2D
 * reference: include/TriangleNodesProvisioner.hpp:32-427, include/DGContext2D.hpp:9-258 */
enum {
    BDG_TRI_R = 0, BDG_TRI_S, BDG_TRI_X, BDG_TRI_Y, BDG_TRI_V, BDG_TRI_VINV, BDG_TRI_DR, BDG_TRI_DS,
    BDG_TRI_DRW, BDG_TRI_DSW, BDG_TRI_LIFT, BDG_TRI_FILTER, BDG_TRI_J, BDG_TRI_RX, BDG_TRI_RY, BDG_TRI_SX,
    BDG_TRI_SY, BDG_TRI_NX, BDG_TRI_NY, BDG_TRI_FSCALE, BDG_TRI_FMASK, BDG_TRI_FX, BDG_TRI_FY,
    BDG_TRI_VMAPM, BDG_TRI_VMAPP, BDG_TRI_MAPP, BDG_TRI_VMAPB, BDG_TRI_MAPB, BDG_TRI_GATHER, BDG_TRI_SCATTER
};
int bdg_trinodes_create(int order, const bdg_mesh* mesh, bdg_trinodes** out); /* mesh must outlive it */
void bdg_trinodes_destroy(bdg_trinodes* nodes);
int bdg_trinodes_build_filter(bdg_trinodes* nodes, double Nc, int s);
int bdg_trinodes_build_bchash(bdg_trinodes* nodes, const int* bctype, int n); /* appends, as the reference */
int bdg_trinodes_set_coordinates(bdg_trinodes* nodes, const double* x, const double* y);
int bdg_trinodes_dims(const bdg_trinodes* nodes, int* order, int* np, int* nfp, int* num_elements);
int bdg_trinodes_table(const bdg_trinodes* nodes, int which, bdg_table* out);
/* BCmap: number of tags; tag list; node list of one tag (borrowed). */
int bdg_trinodes_bcmap_num_tags(const bdg_trinodes* nodes);
int bdg_trinodes_bcmap_tags(const bdg_trinodes* nodes, int* tags, int capacity);
int bdg_trinodes_bcmap_nodes(const bdg_trinodes* nodes, int tag, const int** nodes_out, int* count);

/* ---------------------------------------------------------------- QuadNodesProvisioner / DGContext2D
 * reference: include/QuadNodesProvisioner.hpp:90-206, src/QuadNodesProvisioner.cpp. Same shape as bdg_trinodes_*;
 * bdg_quadnodes_table takes the BDG_TRI_* ids (DRW, DSW, FX, FY, GATHER, SCATTER are not built for quadrilaterals).
 * The mesh must hold quadrangles and outlive the handle. */
int bdg_quadnodes_create(int order, const bdg_mesh* mesh, bdg_quadnodes** out);
void bdg_quadnodes_destroy(bdg_quadnodes* nodes);
int bdg_quadnodes_build_filter(bdg_quadnodes* nodes, double Nc, int s); /* the reference's construction, quirk included */
int bdg_quadnodes_build_bchash(bdg_quadnodes* nodes, const int* bctype, int n); /* appends, as the reference */
int bdg_quadnodes_dims(const bdg_quadnodes* nodes, int* order, int* np, int* nfp, int* num_elements);
int bdg_quadnodes_table(const bdg_quadnodes* nodes, int which, bdg_table* out);
int bdg_quadnodes_bcmap_num_tags(const bdg_quadnodes* nodes);
int bdg_quadnodes_bcmap_tags(const bdg_quadnodes* nodes, int* tags, int capacity);
int bdg_quadnodes_bcmap_nodes(const bdg_quadnodes* nodes, int tag, const int** nodes_out, int* count);

/* Output step after the path (reference TriangleNodesProvisioner::splitElements,
 * src/TriangleNodesProvisioner.cpp:1154-1264, and VtkOutputter, include/VtkOutputter.hpp:30-99).
 * split_count = N^2 linear triangles per element. split_operators: IM (Np, Np) interpolation to the
 * equispaced lattice and 3*N^2 lattice-point indices. split_elements: xnew, ynew, fieldnew as
 * (3, N^2*K). write_vtu: one field to a *.vtu file (raw appended binary; no VTK library). */
int bdg_trinodes_split_count(const bdg_trinodes* nodes);
int bdg_trinodes_split_operators(const bdg_trinodes* nodes, double* IM, int* local_triangles);
int bdg_trinodes_split_elements(const bdg_trinodes* nodes, const double* field, double* xnew, double* ynew,
                                double* fieldnew);
int bdg_trinodes_write_vtu(const bdg_trinodes* nodes, const char* path, const double* field,
                           const char* field_name);
/* The same on quadrilaterals (reference QuadNodesProvisioner::splitElements, src/QuadNodesProvisioner.cpp:721-838, and the
 * VTK_QUAD branch of include/VtkOutputter.hpp:111-141). split_count = N^2 small quadrilaterals per element. split_operators: IM
 * (Np, Np) interpolation to the equispaced lattice (point n (N+1) + m at r = -1 + 2m/N, s = -1 + 2n/N), its 1-D factor I1
 * (N+1, N+1) (Gauss-Lobatto -> equispaced Lagrange interpolation; IM(n (N+1) + m, (N+1) j + i) = I1(m, j) I1(n, i)) and
 * 4*N^2 lattice-point indices, corners (n,m), (n,m+1), (n+1,m), (n+1,m+1). split_elements: xnew, ynew, fieldnew as (4, N^2*K).
 * write_vtu: one field to a *.vtu file of VTK_QUAD cells, each listing its four own points in the order 0, 2, 3, 1. */
int bdg_quadnodes_split_count(const bdg_quadnodes* nodes);
int bdg_quadnodes_split_operators(const bdg_quadnodes* nodes, double* IM, double* I1, int* local_quads);
int bdg_quadnodes_split_elements(const bdg_quadnodes* nodes, const double* field, double* xnew, double* ynew,
                                 double* fieldnew);
int bdg_quadnodes_write_vtu(const bdg_quadnodes* nodes, const char* path, const double* field,
                            const char* field_name);
/* Writes small quadrilaterals ((4, num_quads) x, y, field; one column per quadrilateral, corners as split_elements) as a *.vtu. */
int bdg_write_vtu_quads(const char* path, const double* x, const double* y, const double* field, int num_quads,
                        const char* field_name);

/* ---------------------------------------------------------------- GaussFaceContext2D / CubatureContext2D
 * reference: TriangleNodesProvisioner::buildGaussFaceNodes (src/TriangleNodesProvisioner.cpp:207-381,
 * include/GaussFaceContext2D.hpp:68-84) and ::buildCubatureVolumeMesh (:81-205,
 * include/CubatureContext2D.hpp:75-96); python names at src/pyblitzdg/pyblitzdg.cpp:116-117, 124-158.
 * The contexts own their tables (built from the provisioner's CURRENT coordinates) and outlive it.
 * Gauss tables are (3*NGauss, K), Interp (3*NGauss, Np), mapM/mapP (3*NGauss*K) flat ids g + 3*NGauss*k.
 * Cubature tables are (Ncub, K), V/Dr/Ds (Ncub, Np), r/s/w (Ncub); MM and MMChol are the reference's
 * (Np, Np, K) tensors viewed as (Np*Np, K). build_cubature_volume_mesh also recomputes the provisioner's
 * nodal J, rx, ry, sx, sy from its current coordinates, as the reference does. The cubature rule is the
 * reference's tabulated symmetric rule for degrees 1..28 (36 points at degree 12) and a computed conical-product
 * rule beyond its table (include/blitzdg/TriangleCubatureRules.hpp). */
enum {
    BDG_GAUSS_NX = 0, BDG_GAUSS_NY, BDG_GAUSS_SJ, BDG_GAUSS_J, BDG_GAUSS_RX, BDG_GAUSS_RY, BDG_GAUSS_SX,
    BDG_GAUSS_SY, BDG_GAUSS_X, BDG_GAUSS_Y, BDG_GAUSS_W, BDG_GAUSS_INTERP, BDG_GAUSS_MAPM, BDG_GAUSS_MAPP
};
enum {
    BDG_CUB_R = 0, BDG_CUB_S, BDG_CUB_WEIGHTS, BDG_CUB_V, BDG_CUB_RX, BDG_CUB_RY, BDG_CUB_SX, BDG_CUB_SY,
    BDG_CUB_J, BDG_CUB_DR, BDG_CUB_DS, BDG_CUB_MM, BDG_CUB_MMCHOL, BDG_CUB_X, BDG_CUB_Y, BDG_CUB_W
};
int bdg_trinodes_build_gauss_face_nodes(bdg_trinodes* nodes, int NGauss, bdg_gaussctx** out);
void bdg_gaussctx_destroy(bdg_gaussctx* ctx);
int bdg_gaussctx_ngauss(const bdg_gaussctx* ctx);
int bdg_gaussctx_table(const bdg_gaussctx* ctx, int which, bdg_table* out);
int bdg_gaussctx_bcmap_num_tags(const bdg_gaussctx* ctx);
int bdg_gaussctx_bcmap_tags(const bdg_gaussctx* ctx, int* tags, int capacity);
int bdg_gaussctx_bcmap_nodes(const bdg_gaussctx* ctx, int tag, const int** nodes_out, int* count);
int bdg_trinodes_build_cubature_volume_mesh(bdg_trinodes* nodes, int NCubature, bdg_cubctx** out);
void bdg_cubctx_destroy(bdg_cubctx* ctx);
int bdg_cubctx_num_points(const bdg_cubctx* ctx);
int bdg_cubctx_order(const bdg_cubctx* ctx);
int bdg_cubctx_table(const bdg_cubctx* ctx, int which, bdg_table* out);
/* TriangleCubatureRules (reference include/TriangleCubatureRules.hpp:1807-1830): number of points of the rule of
 * degree NCubature (-1: bad degree), and its rCoord / sCoord / weights copied into caller arrays of that length. */
int bdg_cubature_rule_num_points(int NCubature);
int bdg_cubature_rule(int NCubature, double* r, double* s, double* w);

/* ---------------------------------------------------------------- Nodes1DProvisioner
 * reference: include/Nodes1DProvisioner.hpp:25-302 */
enum {
    BDG_N1D_R = 0, BDG_N1D_X, BDG_N1D_V, BDG_N1D_VINV, BDG_N1D_DR, BDG_N1D_LIFT, BDG_N1D_J, BDG_N1D_RX,
    BDG_N1D_NX, BDG_N1D_FMASK, BDG_N1D_FX, BDG_N1D_FSCALE, BDG_N1D_ETOV, BDG_N1D_ETOE, BDG_N1D_ETOF,
    BDG_N1D_VMAPM, BDG_N1D_VMAPP
};
int bdg_nodes1d_create(int order, int num_elements, double xmin, double xmax, bdg_nodes1d** out);
void bdg_nodes1d_destroy(bdg_nodes1d* nodes);
int bdg_nodes1d_build_nodes(bdg_nodes1d* nodes);
int bdg_nodes1d_compute_jacobian(bdg_nodes1d* nodes);
int bdg_nodes1d_map_i(const bdg_nodes1d* nodes);
int bdg_nodes1d_map_o(const bdg_nodes1d* nodes);
int bdg_nodes1d_table(const bdg_nodes1d* nodes, int which, bdg_table* out);

/* LSERK4 coefficients (reference include/LSERK4.hpp:15-29); 5 entries each. */
int bdg_lserk4_num_stages(void);
const double* bdg_lserk4_a(void);
const double* bdg_lserk4_b(void);

/* VandermondeBuilders::buildVandermondeMatrix_numpy (reference include/VandermondeBuilders.hpp:76-105, Python name
 * VandermondeBuilder.buildVandermondeMatrix, src/pyblitzdg/pyblitzdg.cpp:92-93): V(i, j) = P_j^(0,0)(r_i), the orthonormal
 * Legendre polynomials at the num_points entries of r, j = 0 .. num_cols - 1 (the reference: num_cols = order + 1, or
 * num_points when order < 0). V is (num_points, num_cols) row-major; with Vinv != NULL (needs num_points == num_cols)
 * the inverse is written there too. Host only. */
int bdg_vandermonde1d(const double* r, int num_points, int num_cols, double* V, double* Vinv);

/* advec1d: CPU plumbing config (reference src/advec1d/main.cpp:35-122). Runs the
 * LSERK4 loop on the host to t >= final_time and returns the max-norm error
 * against the translated Gaussian. No GPU involved. */
/* advec1d::computeRHS(u, c, nodes1D, RHS) (reference src/advec1d/main.cpp:126-188; Python twin
 * advec1d.py:12-39) on the host: u, rhs are (Np, K). buildNodes and computeJacobian must have run. */
int bdg_nodes1d_advec_rhs(bdg_nodes1d* nodes, const double* u, double c, double* rhs);
int bdg_advec1d_run(int order, int num_elements, double xmin, double xmax, double c, double cfl,
                    double final_time, double* max_error, int* num_steps);

/* burgers1d: the second 1-D solver on Nodes1DProvisioner + LSERK4 (reference src/burgers1d/main.cpp:28-115 driver, :129-226
 * RHS). Host only. rhs: burgers1d::computeRHS(u, x, t, c, alpha, nu, nodes1D, RHS) with x the provisioner's own grid;
 * run: the driver loop to t >= final_time, max-norm error against the travelling wave Burgers2. */
int bdg_nodes1d_burgers_rhs(bdg_nodes1d* nodes, const double* u, double t, double c, double alpha, double nu, double* rhs);
int bdg_burgers1d_run(int order, int num_elements, double xmin, double xmax, double alpha, double nu, double c, double cfl,
                      double final_time, double* max_error, int* num_steps);

/* ---------------------------------------------------------------- sw2d device solver */

/* Host tables a solver is created from (all borrowed for the duration of the call). */
typedef struct bdg_sw2d_desc {
    int order;          /* N: 1..BDG_SW2D_MAX_ORDER                                   */
    int num_elements;   /* K                                                          */
    const double* Dr;   /* (Np, Np)                                                   */
    const double* Ds;   /* (Np, Np)                                                   */
    const double* Lift; /* (Np, 3*Nfp)                                                */
    const double* Filter; /* (Np, Np) or NULL (no filter available)                   */
    const double* rx; const double* sx; const double* ry; const double* sy; /* (Np, K) */
    const double* nx; const double* ny; const double* Fscale;               /* (3*Nfp, K) */
    const int* vmapM;   /* (3*Nfp*K) volume node of each face node, n + Np*k; may be NULL */
    const int* vmapP;   /* (3*Nfp*K) neighbour node of each face node                 */
    const int* mapW;    /* BCmap[3]: flat face-node indices of reflective-wall nodes  */
    int num_wall;
    double g;           /* gravitational acceleration                                 */
    int device;         /* HIP device ordinal                                         */
    int flags;          /* BDG_SW2D_* bits                                            */
    /* ---- optional "variant D" physics of the reference's Python RHS (swhelpers/rhs.py:178-311);
     * all zero / NULL gives variant A above. Straight-sided elements only. */
    int num_fields;     /* 0 or 3: h, hu, hv;  4: + passive tracer hN (F4 = hN u, G4 = hN v)      */
    int sources;        /* nonzero: RHS2 += f hv - CD|u|u - g h zx;  RHS3 -= f hu - CD|u|v;  RHS3 -= g h zy */
    const double* zx;   /* (Np, K) bed slope or NULL (= 0)                            */
    const double* zy;
    const double* coriolis; /* (Np, K) Coriolis parameter f, or NULL: coriolis_const    */
    double coriolis_const;
    double drag;        /* CD                                                         */
} bdg_sw2d_desc;

#define BDG_SW2D_MAX_ORDER 8 /* 7 and 8: straight-sided (affine) geometry only */
#define BDG_SW2D_REORDER 1u /* renumber elements internally for gather locality (results are
                               returned in the caller's numbering either way)         */
#define BDG_SW2D_KEEP_ORDER 4u /* never renumber (default: renumber when the mean face-neighbour
                               distance exceeds 4*sqrt(K) slots, e.g. a shuffled mesh, or, at N <= 4,
                               when over a tenth of the faces have their neighbour more than 1 MiB of
                               stage traffic away, e.g. a wide box row by row). Required
                               for bdg_sw2d_set_partition, whose element ranges are in caller order */
#define BDG_SW2D_NODAL_GEOMETRY 2u /* always read rx..sy, nx, ny, Fscale per node (general path).
                               Default: if they are constant per element / per face to round-off
                               (straight-sided elements: everything the reference's provisioner
                               builds), one value per element / face is kept instead.      */

int bdg_device_count(void); /* HIP devices visible to this process (0 if none / no driver) */
int bdg_sw2d_create(const bdg_sw2d_desc* desc, bdg_sw2d** out);
/* Convenience: take every table from a nodes provisioner (wall nodes = BCmap[3]). */
int bdg_sw2d_create_from_nodes(const bdg_trinodes* nodes, double g, int device, int flags, bdg_sw2d** out);
void bdg_sw2d_destroy(bdg_sw2d* s);

/* State I/O: host (Np, K) row-major arrays in the caller's element numbering. */
int bdg_sw2d_set_state(bdg_sw2d* s, const double* h, const double* hu, const double* hv);
int bdg_sw2d_get_state(bdg_sw2d* s, double* h, double* hu, double* hv);
/* Still-water depth H used only by the eta = h - H blow-up check; default: none (check h). */
int bdg_sw2d_set_bathymetry(bdg_sw2d* s, const double* H);

/* Output step: the drivers' primitive fields eta = h - H (h if no bathymetry was set), u = hu/h,
 * v = hv/h of the resident state as host (Np, K) arrays; with IM != NULL ((Np, Np), from
 * bdg_trinodes_split_operators) they are interpolated to each element's equispaced lattice on the
 * device first (what splitElements does before a *.vtu is written). NULL outputs are skipped. */
int bdg_sw2d_output_fields(bdg_sw2d* s, const double* IM, double* eta, double* u, double* v);
/* Four-field solvers: the tracer concentration N = hN / h (what the reference's sw2d.py writes out), same
 * optional lattice interpolation. */
int bdg_sw2d_output_tracer(bdg_sw2d* s, const double* IM, double* tracer);
/* Writes linear triangles ((3, num_triangles) x, y, field; one column per triangle) as a *.vtu. */
int bdg_write_vtu_triangles(const char* path, const double* x, const double* y, const double* field,
                            int num_triangles, const char* field_name);

/* Drop-in for computeRHS: host fields in, host RHS out (upload, one kernel, download).
 * Does not disturb the resident state. filter != 0 applies Filter to the result. */
int bdg_sw2d_rhs(bdg_sw2d* s, const double* h, const double* hu, const double* hv, double* rhs1,
                 double* rhs2, double* rhs3, int filter);

/* Four-field forms for solvers created with num_fields = 4 (hN: tracer). The three-field
 * functions above refuse such a solver and vice versa. */
int bdg_sw2d_set_state4(bdg_sw2d* s, const double* h, const double* hu, const double* hv, const double* hN);
int bdg_sw2d_get_state4(bdg_sw2d* s, double* h, double* hu, double* hv, double* hN);
int bdg_sw2d_rhs4(bdg_sw2d* s, const double* h, const double* hu, const double* hv, const double* hN,
                  double* rhs1, double* rhs2, double* rhs3, double* rhs4, int filter);
int bdg_sw2d_num_fields(const bdg_sw2d* s);

/* ---- "variant B": the physics of the reference's C++ sw2d driver,
 * computeRHS(fields, numParams, physParams, DGContext2D, t) -- src/sw2d/main.cpp:279-484:
 * still-water depth H with star states at the faces, open-boundary nodes (BCmap[2]) driven by
 *   hP = HM + tide_amplitude cos(2 pi t / tide_period) 1/2 (tanh(tide_ramp (t - tide_period)) + 1),
 * one global Lax-Friedrichs speed, and the sources RHS2 += g h Hx - CD u|u| + f hv,
 * RHS3 += g h Hy - CD v|u| - f hu. After this call every RHS / stepping entry point of a 3-field
 * straight-sided solver evaluates variant B at the solver's model time (bdg_sw2d_set_time; the
 * steppers advance it by dt per step, both Heun evaluations at the old level as main.cpp:211-236).
 * sponge: (Np, K) coefficient of hu /= 1 + c hu^2 used by bdg_sw2d_step_ssprk2 instead of the
 * scalar. Hx, Hy are the caller's (bdg_trinodes_bed_slopes builds them as main.cpp:128-133). */
typedef struct bdg_sw2d_vb_desc {
    const double* H;       /* (Np, K)                                    */
    const double* Hx;      /* (Np, K)                                    */
    const double* Hy;      /* (Np, K)                                    */
    const int* mapO;       /* flat face-node indices of open-boundary nodes, or NULL */
    int num_out;
    double drag;           /* physParams.CD                              */
    double coriolis;       /* physParams.f                               */
    double tide_amplitude; /* reference: 3.0                             */
    double tide_period;    /* reference: 3600*12.42                      */
    double tide_ramp;      /* reference: 0.15/3600                       */
    const double* sponge;  /* (Np, K) or NULL                            */
} bdg_sw2d_vb_desc;
int bdg_sw2d_enable_variant_b(bdg_sw2d* s, const bdg_sw2d_vb_desc* desc);
/* Variant B with a passive tracer hN as a fourth field (the reference's tidal driver has none; the definition is the one of
 * bdg_sw2dq_enable_variant_b4). Concentrations are formed from the depths before the star states, NM = hN-/h-,
 * NP = hN+/h+; a wall node takes NP = NM, an open-boundary node NP = n_open (it wins where a node is both); the star tracer is
 * hM* NM, hP* NP, so a uniform concentration stays uniform over a discontinuous bed; F4 = hN* hu* / h*, G4 = hN* hv* / h*, the
 * Lax-Friedrichs term with variant B's one global speed, which the tracer does not enter; no source term. n_open_count is 1
 * (one concentration for every open-boundary node) or desc->num_out (n_open[i] belongs to mapO[i]; with num_out = 0 a count of
 * 0 is accepted and n_open is not read); anything else, a NULL handle, descriptor or n_open is BDG_ERR_ARGUMENT, and so is a
 * three-field solver, a solver created with sources, a second call, and a call after the solver's first evaluation; a refusal
 * changes nothing. Once, on a solver created with num_fields = 4 and sources = 0: afterwards the four-field calls
 * (bdg_sw2d_rhs4, _set_state4 / _get_state4) and every stepping entry evaluate the three-field variant-B launches exactly as a
 * three-field solver does, each followed by the tracer pass (sw2d_vb_tracer_kernel.hpp); hN is stepped as h is (never sponged),
 * the filter applies to all four right-hand sides. Orders 1 to 8, both geometry forms, partitioned solvers included.
 * bdg_sw2d_enable_variant_b keeps refusing four-field solvers. */
int bdg_sw2d_enable_variant_b4(bdg_sw2d* s, const bdg_sw2d_vb_desc* desc, const double* n_open, int n_open_count);
/* Diffusion, sources and decay of the passive tracer of a four-field solver (tests/tridiff_ref.py):
 *   d(hN)/dt = (advection, as before) + div(kappa h grad N) + S - k hN,   N = hN / h,
 * local DG with central fluxes and no penalty. A face node without a neighbour (vmapP == vmapM: walls and the open boundary
 * alike) is a boundary node with zero diffusive flux; the tracer crosses the open boundary by advection only. kappa_field: (Np, K)
 * diffusivity or NULL (then the scalar kappa); source: (Np, K) S, hN per second, or NULL; decay: k >= 0. Once, before the solver's
 * first evaluation, on a solver created with num_fields = 4: variant A's four-field form, variant D with or without sources, or
 * variant B with a tracer (after bdg_sw2d_enable_variant_b4). From then on every evaluation's launches are followed on the same
 * stream by the two passes of sw2d_diffusion_kernel.hpp, which add T to plane 3 of what the evaluation wrote (the right-hand
 * side, or the LSERK / RK2 / Heun stage update); planes 0-2 and every existing kernel are untouched; a filtered evaluation adds
 * Filter T. BDG_ERR_ARGUMENT, nothing changed: a NULL descriptor, three fields, kappa < 0 or not finite (scalar or any entry),
 * decay < 0 or not finite, a source that is not finite, a second call, after the first evaluation, a solver with a partition set
 * (bdg_sw2d_set_partition on a diffusing solver is refused as well). bdg_sw2d_compute_dt and bdg_sw2d_run_adaptive then return
 * min(advective dt, cfl * dt_diff), dt_diff = 4 / (max kappa (N+1)^4 max(Fscale)^2) (infinite for kappa = 0);
 * bdg_sw2d_diffusion_dt returns dt_diff (BDG_ERR_ARGUMENT without diffusion). */
typedef struct bdg_sw2d_diffusion_desc {
    double kappa;              /* used when kappa_field is NULL                */
    const double* kappa_field; /* (Np, K) or NULL                              */
    const double* source;      /* (Np, K) or NULL                              */
    double decay;              /* k >= 0                                       */
} bdg_sw2d_diffusion_desc;
int bdg_sw2d_enable_tracer_diffusion(bdg_sw2d* s, const bdg_sw2d_diffusion_desc* desc);
int bdg_sw2d_diffusion_dt(const bdg_sw2d* s, double* dt_diff);
/* Horizontal eddy viscosity on the momentum of a triangle solver, constant or Smagorinsky (the definition is
 * restated in tests/triviscosity_ref.py). With u = hu / h and v = hv / h at every node,
 *   d(hu)/dt += div(nu h grad u),  d(hv)/dt += div(nu h grad v),
 *   nu = nu0 + Cs^2 D^2 |S|,  |S| = sqrt(2 u_x^2 + 2 v_y^2 + (u_y + v_x)^2),  D^2 = 2 J / (N+1)^2,
 * in the tracer diffusion's discretisation: local DG, central fluxes, no penalty; a face node with vmapP == vmapM (walls and the
 * open boundary alike) carries no viscous stress (free slip). The gradients in |S| are the ones that diffuse, lifts included.
 * nu: nu0 >= 0, used when nu_field is NULL; nu_field: (Np, K) nu0 >= 0 or NULL; smagorinsky: Cs >= 0 (0: off). Once, before the
 * solver's first evaluation, on any solver kind: three or four fields, with or without sources, variant B with or without a
 * tracer, with or without bdg_sw2d_enable_tracer_diffusion, in either order. From then on every evaluation's launches are
 * followed on the same stream by the two passes of sw2d_viscosity_kernel.hpp, which add the terms to planes 1 and 2 of what the
 * evaluation wrote (a filtered evaluation adds their filtered form); planes 0 and 3 and every existing kernel are untouched. A
 * Heun step with a sponge is q1 = sponge(q + dt (R + T)): the stage launches run with the sponge off and the viscosity's update
 * makes the division. BDG_ERR_ARGUMENT, nothing changed: a NULL handle or descriptor, nu or smagorinsky negative or not finite
 * (scalar or any entry), both zero, a second call, after the first evaluation, a solver with a partition set
 * (bdg_sw2d_set_partition on a viscous solver is refused as well). bdg_sw2d_compute_dt and bdg_sw2d_run_adaptive then return
 * min(advective dt, cfl * dt_visc, cfl * dt_diff if the tracer diffuses), dt_visc = 4 / (max nu (N+1)^4 max(Fscale)^2) with max nu
 * over the nodes of the CURRENT state (Cs > 0: one launch and a fixed-order reduction; Cs = 0: max nu0 from set-up).
 * bdg_sw2d_viscosity_dt returns dt_visc; bdg_sw2d_eddy_viscosity writes the (Np, K) field nu of the current state (both
 * BDG_ERR_ARGUMENT without viscosity). bdg_sw2d_device_bytes counts four flux planes, the plane of nu, the plane of nu0 if it is a
 * field and, per-node geometry with a Filter, two planes of unfiltered terms. */
typedef struct bdg_sw2d_viscosity_desc {
    double nu;              /* used when nu_field is NULL                   */
    const double* nu_field; /* (Np, K) or NULL                              */
    double smagorinsky;     /* Cs >= 0                                      */
} bdg_sw2d_viscosity_desc;
int bdg_sw2d_enable_viscosity(bdg_sw2d* s, const bdg_sw2d_viscosity_desc* desc);
int bdg_sw2d_viscosity_dt(bdg_sw2d* s, double* dt_visc);
int bdg_sw2d_eddy_viscosity(bdg_sw2d* s, double* nu);
int bdg_sw2d_set_time(bdg_sw2d* s, double t);
int bdg_sw2d_get_time(const bdg_sw2d* s, double* t);
/* The global Lax-Friedrichs speed of the most recent variant-B evaluation. */
int bdg_sw2d_global_speed(bdg_sw2d* s, double* lam);
/* Host helpers for the variant-B driver set-up: Hx, Hy = Filter (rx Dr H + sx Ds H, ry Dr H + sy Ds H)
 * (main.cpp:128-133; buildFilter must have been called), and buildSpongeCoeff (main.cpp:516-556). */
int bdg_trinodes_bed_slopes(const bdg_trinodes* nodes, const double* H, double* Hx, double* Hy);
int bdg_trinodes_sponge_coeff(const bdg_trinodes* nodes, const int* mapO, int num_out, double strength,
                              double radius, double* coeff);

/* ---------------------------------------------------------------- quadrilateral sw2d solver (HIP, gfx950)
 * The reference script sw2dquads.py: sw2dComputeRHS (:24-133; local Lax-Friedrichs flux with one speed per face,
 * reflective walls on mapW, strong form) and its midpoint-RK2 + filter loop (:183-213), plus LSERK4 stages.
 * Dr, Ds and Lift must have the Gauss-Lobatto tensor form of QuadNodesProvisioner to 1e-13 max|entry| (create
 * refuses anything else: the kernel only keeps their 1-D factors); Filter stays a dense (Np, Np) matrix.
 * Tables as bdg_sw2d_desc with Nfp = order + 1 and 4 faces: Lift (Np, 4 Nfp), nx, ny, Fscale (4 Nfp, K). */
typedef struct bdg_sw2dq_desc {
    int order;          /* 1..BDG_SW2DQ_MAX_ORDER                                   */
    int num_elements;
    const double* Dr;   /* (Np, Np), Np = (order + 1)^2                             */
    const double* Ds;
    const double* Lift; /* (Np, 4 Nfp)                                              */
    const double* Filter; /* (Np, Np) or NULL (then no filtered modes)              */
    const double* rx;   /* (Np, K)                                                  */
    const double* sx;
    const double* ry;
    const double* sy;
    const double* nx;   /* (4 Nfp, K)                                               */
    const double* ny;
    const double* Fscale;
    const int* vmapM;   /* 4 Nfp K, checked against the Gauss-Lobatto face numbering; NULL = that numbering */
    const int* vmapP;   /* 4 Nfp K                                                  */
    const int* mapW;    /* reflective-wall face nodes (BCmap[3])                    */
    int num_wall;
    double g;
    int device;
    int flags;          /* BDG_SW2DQ_*                                              */
} bdg_sw2dq_desc;

#define BDG_SW2DQ_MAX_ORDER 12 /* 9..12: tiles of 8 elements; triangles and curved elements stop at 8 */
#define BDG_SW2DQ_GENERAL_GEOMETRY 1u /* always read rx..sy per node and nx, ny, Fscale per face node. Default: if
                               every element is a parallelogram (metric terms constant per element, normals and
                               Fscale per face, to 1e-10 relative), 16 values per element are kept instead. */

int bdg_sw2dq_create(const bdg_sw2dq_desc* desc, bdg_sw2dq** out);
/* every table from a quadrilateral provisioner (wall nodes = BCmap[3]; Filter if buildFilter was called) */
int bdg_sw2dq_create_from_nodes(const bdg_quadnodes* nodes, double g, int device, int flags, bdg_sw2dq** out);
void bdg_sw2dq_destroy(bdg_sw2dq* s);
int bdg_sw2dq_set_state(bdg_sw2dq* s, const double* h, const double* hu, const double* hv); /* also zeroes the LSERK residual */
int bdg_sw2dq_get_state(bdg_sw2dq* s, double* h, double* hu, double* hv);
/* host fields in, host RHS out; does not disturb the resident state. filter != 0: Filter applied to the RHS */
int bdg_sw2dq_rhs(bdg_sw2dq* s, const double* h, const double* hu, const double* hv, double* rhs1, double* rhs2,
                  double* rhs3, int filter);
/* The script's loop body: q1 = q + dt/2 F R(q); q += dt F R(q1) (F = Filter if filter != 0, else identity).
 * After the steps, BDG_ERR_UNSTABLE if max|h| > 1e8 or h has a NaN (the script's check). */
int bdg_sw2dq_step_rk2(bdg_sw2dq* s, double dt, int num_steps, int filter);
/* LSERK4 stages (stage i = count % 5, count reset by set_state), same blow-up check at the end */
int bdg_sw2dq_lserk4_stages(bdg_sw2dq* s, double dt, int num_stages);
/* HIP-event milliseconds per LSERK4 stage (kind 0) or per RK2 + filter step (kind 1), averaged over count
 * (kind 2: see bdg_sw2dq_time_speed) */
int bdg_sw2dq_time(bdg_sw2dq* s, int kind, double dt, int count, float* ms);
int bdg_sw2dq_synchronize(bdg_sw2dq* s);
size_t bdg_sw2dq_device_bytes(const bdg_sw2dq* s);
int bdg_sw2dq_uses_parallelogram_geometry(const bdg_sw2dq* s);
/* Four fields and sources: the reference's Python right-hand side (swhelpers/rhs.py:178-311, fluxes of swhelpers/flux.py)
 * on quadrilaterals: passive tracer hN as a fourth field, and optionally Coriolis f, quadratic drag CD and bed slope zx, zy
 * (RHS2 += f hv - CD |u| u - g h zx; RHS3 -= f hu - CD |u| v; RHS3 -= g h zy, the reference's signs). num_fields is 3 (what
 * bdg_sw2dq_create builds) or 4. A four-field solver is driven by the *4 calls below and by step_rk2, lserk4_stages, time,
 * compute_dt and the partition calls (one exchanged record is then 4 Np doubles); the three-field set_state / get_state / rhs
 * are refused on it with BDG_ERR_ARGUMENT, and the *4 calls and set_sources on a three-field solver. */
int bdg_sw2dq_create_fields(const bdg_sw2dq_desc* desc, int num_fields, bdg_sw2dq** out);
int bdg_sw2dq_create_from_nodes_fields(const bdg_quadnodes* nodes, double g, int device, int flags, int num_fields,
                                       bdg_sw2dq** out);
int bdg_sw2dq_num_fields(const bdg_sw2dq* s);
/* zx, zy: (Np, K); Coriolis: f_array (Np, K), or f_scalar where f_array is NULL; CD scalar. Once, before the solver's first
 * evaluation (rhs4, a step, a stage, a timing): afterwards BDG_ERR_ARGUMENT. A solver without this call compiles no source term. */
int bdg_sw2dq_set_sources(bdg_sw2dq* s, const double* zx, const double* zy, double f_scalar, const double* f_array, double CD);
int bdg_sw2dq_set_state4(bdg_sw2dq* s, const double* h, const double* hu, const double* hv, const double* hN);
int bdg_sw2dq_get_state4(bdg_sw2dq* s, double* h, double* hu, double* hv, double* hN);
int bdg_sw2dq_rhs4(bdg_sw2dq* s, const double* h, const double* hu, const double* hv, const double* hN, double* rhs1, double* rhs2,
                   double* rhs3, double* rhs4, int filter);
/* The drivers' time step from the resident state: dt = CFL / ((N+1)^2 * 0.5 * speed), speed = max over face nodes of
 * |Fscale| (sqrt(u^2 + v^2) + sqrt(g h)) (a device reduction in IEEE-exact operations). Either kind of solver. After comm_init
 * the maximum covers the owned elements and is all-reduced, so every rank gets the same dt. BDG_ERR_UNSTABLE on NaN. */
int bdg_sw2dq_compute_dt(bdg_sw2dq* s, double cfl, double* dt, double* speed);
/* Output step: the drivers' primitive fields eta = h - H (h where H is NULL; H: host (Np, K)), u = hu / h, v = hv / h and, on a
 * four-field solver, N = hN / h of the resident state as host (Np, K) arrays, all from ONE kernel launch that reads h once.
 * With lattice != NULL (I1, (N+1, N+1), from bdg_quadnodes_split_operators) they are interpolated on the device to each
 * element's equispaced lattice first (what splitElements does before a *.vtu is written), I1 applied along r and then along s,
 * each sum in ascending order and without contraction. NULL outputs are skipped; N != NULL on a three-field solver is
 * BDG_ERR_ARGUMENT. After set_partition only the owned elements are computed and only the columns [0, num_owned) of the
 * outputs are written. The values pass through device memory that is free between steps; the state is not disturbed. */
int bdg_sw2dq_output_fields(bdg_sw2dq* s, const double* H, const double* lattice, double* eta, double* u, double* v, double* N);
/* HIP-event milliseconds of that launch alone (every field of the solver; H, lattice as above), averaged over count */
int bdg_sw2dq_time_output(bdg_sw2dq* s, const double* H, const double* lattice, int count, float* ms);
/* Element-partitioned runs, as bdg_sw2d_curved_set_partition and friends (same argument order, refusals and error codes):
 * the solver's mesh is ordered [elements without a ghost neighbour: num_interior | partition-boundary elements: up to
 * num_owned | ghosts: up to K]; set_partition refuses (BDG_ERR_ARGUMENT) a bad range, an element of [0, num_interior) whose
 * gather reaches a ghost or that is in the send list, and any call after comm_init. */
int bdg_sw2dq_set_partition(bdg_sw2dq* s, int num_interior, int num_owned, const int* send_elements, int num_send);
/* The RCCL communicator (bdg_comm_unique_id) and the neighbour tables: peer i is sent the elements send_elements[send_start[i]
 * .. + send_count[i]) and its recv_count[i] elements arrive in ghost slots recv_start[i] .. (relative to num_owned); one record
 * of 3 Np (four fields: 4 Np) doubles per element. Refused before set_partition, a second time, or with peer ranges that do not fit. */
int bdg_sw2dq_comm_init(bdg_sw2dq* s, int rank, int world, const void* unique_id, const int* peer_ranks, const int* send_start,
                        const int* send_count, const int* recv_start, const int* recv_count, int num_peers);
/* one ghost refresh of the state (intermediate = 0) or of the RK2 intermediate / other LSERK4 buffer (1), on the solver's stream */
int bdg_sw2dq_exchange(bdg_sw2dq* s, int intermediate);
/* bdg_sw2dq_step_rk2 with the ghosts of q refreshed before the predictor and those of q1 before the corrector. With interior
 * elements the interior range runs on the solver's stream beside the exchange, and the partition-boundary range after it on the
 * exchange stream (two chains joined by events); without (or with BDG_SW2DQ_NO_OVERLAP set) the exchange and then every owned
 * element run in stream order. Ghost elements are not evaluated: the ghost columns bdg_sw2dq_get_state returns hold whatever
 * was last received. The blow-up check covers the owned columns and is all-reduced, so every rank returns BDG_ERR_UNSTABLE
 * together. */
int bdg_sw2dq_step_rk2_exchanged(bdg_sw2dq* s, double dt, int num_steps, int filter);
/* bdg_sw2dq_lserk4_stages with an exchange of the state in front of every stage; schedule and check as above */
int bdg_sw2dq_lserk4_stages_exchanged(bdg_sw2dq* s, double dt, int num_stages);
/* drains both streams, meets every rank (an 8-byte all-reduce), drains again */
int bdg_sw2dq_barrier(bdg_sw2dq* s);
/* ---- "variant B" on quadrilaterals: the tidal driver's right-hand side (src/sw2d/main.cpp:279-484; the text above
 * bdg_sw2d_vb_desc) on a three-field quadrilateral solver, orders 1 to 12, both geometry forms. The descriptor has the
 * triangle one's fields: H, Hx, Hy, sponge are host (Np, K); mapO holds flat face-node indices k * 4 Nfp + face node, as mapW
 * (QuadNodesProvisioner's BCmap[2] after buildBCHash); an open-boundary node wins over a wall node where a node is both.
 * Once, before the solver's first evaluation (afterwards BDG_ERR_ARGUMENT, as set_sources); a four-field solver refuses it
 * with BDG_ERR_ARGUMENT and stays usable. From then on bdg_sw2dq_rhs, step_rk2, lserk4_stages, time and their _exchanged
 * forms evaluate variant B at the solver's model time: every evaluation is the speed pass (global Lax-Friedrichs speed,
 * main.cpp:400-414, left on the device) and the stage launch that reads it. RK2 and Heun steps evaluate twice at the old
 * time level and advance the time by dt; LSERK4 freezes the tide over its five stages and advances after the last.
 * Quirks kept as on triangles: the momentum rescale hMstar (huM / hMstar) is NaN for a dry star state, and the
 * hydrostatic correction of main.cpp:420-421 is identically zero. bdg_sw2dq_compute_dt is unchanged. */
typedef struct bdg_sw2dq_vb_desc {
    const double* H;       /* (Np, K)                                    */
    const double* Hx;      /* (Np, K)                                    */
    const double* Hy;      /* (Np, K)                                    */
    const int* mapO;       /* flat face-node indices of open-boundary nodes, or NULL */
    int num_out;
    double drag;           /* physParams.CD                              */
    double coriolis;       /* physParams.f                               */
    double tide_amplitude; /* reference: 3.0                             */
    double tide_period;    /* reference: 3600*12.42                      */
    double tide_ramp;      /* reference: 0.15/3600                       */
    const double* sponge;  /* (Np, K) or NULL                            */
} bdg_sw2dq_vb_desc;
int bdg_sw2dq_enable_variant_b(bdg_sw2dq* s, const bdg_sw2dq_vb_desc* desc);
int bdg_sw2dq_set_time(bdg_sw2dq* s, double t);
int bdg_sw2dq_get_time(const bdg_sw2dq* s, double* t);
/* The global Lax-Friedrichs speed of the most recent variant-B evaluation (on a partition: the all-rank maximum). */
int bdg_sw2dq_global_speed(bdg_sw2dq* s, double* lam);
/* Heun / SSP-RK2 of the tidal driver (main.cpp:211-236), variant B only (BDG_ERR_ARGUMENT without):
 * q1 = sp(q + dt R(q)); q = sp((q + q1 + dt R(q1))/2), sp(x) = x/(1 + c x^2) on hu, hv, the division fused into the stage
 * store; c is the descriptor's sponge array where it has one, else sponge_coeff (0: plain Heun). Blow-up check as step_rk2. */
int bdg_sw2dq_step_ssprk2(bdg_sw2dq* s, double dt, int num_steps, int filter, double sponge_coeff);
/* On a partition every variant-B evaluation is: the speed pass over the owned elements (it needs no current ghosts), one
 * 8-byte all-reduce (maximum) on the solver's stream, the exchange, then every owned element, in stream order. These
 * evaluations are not overlapped: the all-rank speed has to exist before any element starts (as the triangle solver's). */
int bdg_sw2dq_step_ssprk2_exchanged(bdg_sw2dq* s, double dt, int num_steps, int filter, double sponge_coeff);
/* HIP-event milliseconds of the speed pass alone on the resident state, averaged over count; bdg_sw2dq_time takes kind 2
 * (one unfiltered Heun step with the sponge of the last bdg_sw2dq_step_ssprk2) on a variant-B solver. */
int bdg_sw2dq_time_speed(bdg_sw2dq* s, int count, float* ms);
/* Variant B with a passive tracer: the same physics on a FOUR-field solver (bdg_sw2dq_create_fields), hN as a fourth equation
 * (csrc/hip/sw2d_quadb4_kernel.hpp; the reference's tidal driver has none, the definition is tests/quadrefB4.py). The face
 * concentrations are formed from the depths before the star states, NM = hNM / hM, NP = hNP / hP; a wall node takes NP = NM and an
 * open-boundary node NP = n_open (it wins where a node is both); the star tracer is hM* NM, hP* NP, so a uniform concentration
 * stays uniform over a discontinuous bed; fluxes (hN* hu) / h*, (hN* hv) / h* with the same global speed, which the tracer does
 * not enter; no source term. n_open_count is 1 (one concentration for every open-boundary node) or desc->num_out (n_open[i]
 * belongs to mapO[i]; with num_out = 0 a count of 0 is accepted and n_open is not read); anything else, a NULL handle,
 * descriptor or n_open is BDG_ERR_ARGUMENT, and so is a second call. Once, on a four-field solver
 * before its first evaluation and without a bdg_sw2dq_set_sources call (variant B brings its own sources; set_sources is
 * refused afterwards); a refusal changes nothing. From then on bdg_sw2dq_rhs4, step_rk2, step_ssprk2 (hN is stepped as h is:
 * the sponge division touches hu and hv only), lserk4_stages, time and the _exchanged forms (one record is 4 Np doubles)
 * evaluate it, the speed pass in front as on three fields; set_time, get_time, global_speed, time_speed, the monitor (int hN,
 * gauge N, the descriptor's H by default) and output_fields work as there. bdg_sw2dq_enable_variant_b still refuses four fields. */
int bdg_sw2dq_enable_variant_b4(bdg_sw2dq* s, const bdg_sw2dq_vb_desc* desc, const double* n_open, int n_open_count);
/* Diffusion, sources and decay of the passive tracer of a four-field quadrilateral solver: bdg_sw2d_enable_tracer_diffusion's
 * term and descriptor (tests/tridiff_ref.py, tests/quaddiff_ref.py),
 *   d(hN)/dt = (advection, as before) + div(kappa h grad N) + S - k hN,   N = hN / h,
 * local DG with central fluxes and no penalty; a face node with vmapP == vmapM (walls and the open boundary alike) carries no
 * diffusive flux. Once, before the solver's first evaluation, on a solver created with four fields: plain, with
 * bdg_sw2dq_set_sources, or variant B with a tracer (after bdg_sw2dq_enable_variant_b4). Orders 1 to 12, both geometry forms.
 * From then on the stage launch of every evaluation is followed on the same stream by the two passes of
 * sw2d_quad_diffusion_kernel.hpp, which evaluate T from the stage's input state and add it to plane 3 of what the stage wrote
 * (the right-hand side, or the RK2 / LSERK4 / Heun stage update); a filtered evaluation adds Filter T. The input state of a
 * stage is never one of its output buffers (bdg_sw2dq_step_rk2 and _step_ssprk2 evaluate the state into the intermediate one
 * and back, bdg_sw2dq_lserk4_stages into the other of two buffers), which is what the passes rest on. Planes 0-2, the global
 * speed and every existing kernel are untouched. BDG_ERR_ARGUMENT, nothing changed: a NULL descriptor, three fields, kappa,
 * decay or a source entry negative or not finite, a second call, after the first evaluation, a solver with a partition set
 * (bdg_sw2dq_set_partition on a diffusing solver is refused as well). bdg_sw2dq_compute_dt then returns
 * min(advective dt, cfl * dt_diff), dt_diff = 4 / (max kappa (N+1)^4 max|Fscale|^2) (infinite for kappa = 0);
 * bdg_sw2dq_diffusion_dt returns dt_diff (BDG_ERR_ARGUMENT without diffusion). bdg_sw2dq_device_bytes counts the two flux planes
 * and the planes of kappa and S. */
int bdg_sw2dq_enable_tracer_diffusion(bdg_sw2dq* s, const bdg_sw2d_diffusion_desc* desc);
int bdg_sw2dq_diffusion_dt(const bdg_sw2dq* s, double* dt_diff);
/* Host helpers of the tidal set-up, argument lists as the bdg_trinodes_* ones: Hx, Hy = Filter (rx Dr H + sx Ds H,
 * ry Dr H + sy Ds H) (main.cpp:128-133; bdg_quadnodes_build_filter first), and buildSpongeCoeff (main.cpp:517-553). */
int bdg_quadnodes_bed_slopes(const bdg_quadnodes* nodes, const double* H, double* Hx, double* Hy);
int bdg_quadnodes_sponge_coeff(const bdg_quadnodes* nodes, const int* mapO, int num_out, double strength, double radius,
                               double* coeff);
/* ---- run monitor: conservation diagnostics and gauges recorded on the device during the stepping calls, with no host round
 * trip and no state download (csrc/hip/sw2d_monitor_kernel.hpp). Host set-up, from a quadrilateral provisioner:
 * quadrature_weights: w (Np, K), w[(N+1) j + i, k] = w1[j] w1[i] J[(N+1) j + i, k], w1 the 1-D Gauss-Lobatto weights (the row
 * sums of the 1-D mass matrix). locate_points: for each (x[p], y[p]) the element that contains it and its reference
 * coordinates, by Newton iteration on the element's own nodal map (either geometry form); |r|, |s| <= 1 + 1e-10 counts as
 * inside, a point on a shared edge or vertex goes to the lowest element index, a point in no element gets element -1.
 * lagrange_basis: basis (n, N+1), the 1-D Lagrange basis of the Gauss-Lobatto points at r[p] (barycentric formula; an
 * abscissa that equals a node bit for bit gives the exact unit vector): what the gauges interpolate with. */
int bdg_quadnodes_quadrature_weights(const bdg_quadnodes* nodes, double* w);
int bdg_quadnodes_locate_points(const bdg_quadnodes* nodes, const double* x, const double* y, int n, int* element, double* r,
                                double* s);
int bdg_quadnodes_lagrange_basis(const bdg_quadnodes* nodes, const double* r, int n, double* basis);
/* One record is `width` doubles, width = 10 + 3 num_gauges (four fields: 11 + 4 num_gauges):
 *   [t, int h, int hu, int hv, (int hN,) E, min h, max h, max|hu|, max|hv|, NaN count, then per gauge eta, u, v (, N)]
 * t: the model time of the sample (bdg_sw2dq_get_time). Integrals: sum of w f over the nodes of the elements [0, K) (after
 * set_partition: the owned ones). E = int (hu^2 + hv^2) / (2 h) + g (h - H)^2 / 2, H = 0 without one. Extrema skip NaNs; the NaN
 * count covers every field of the state. Gauges: eta = h - H, u = hu / h, v = hv / h (N = hN / h) formed at the nodes of the
 * gauge's element and interpolated along r and then along s, each sum in ascending order and without contraction (the rule
 * of bdg_sw2dq_output_fields), so a gauge on a node is that node's output value bit for bit. The summation order of the
 * integrals is fixed (a fixed grid, a fixed element range per workgroup, an LDS tree, partials added in ascending order; no
 * floating-point atomics): equal states give equal records bit for bit. */
typedef struct bdg_sw2dq_monitor_desc {
    const double* weights;      /* (Np, K), bdg_quadnodes_quadrature_weights */
    const double* H;            /* (Np, K) or NULL (a variant-B solver then uses its descriptor's H) */
    int num_gauges;             /* may be 0 */
    const int* gauge_element;   /* caller's numbering, each in [0, K) */
    const double* gauge_r;      /* reference coordinates, |r|, |s| <= 1 + 1e-10 (bdg_quadnodes_locate_points) */
    const double* gauge_s;
    int stride;                 /* sample after every stride-th completed step, >= 1 */
    int capacity;               /* records held on the device, >= 1 */
} bdg_sw2dq_monitor_desc;
/* Once per solver. BDG_ERR_ARGUMENT, changing nothing, for a NULL handle or descriptor or weights, a gauge element outside
 * [0, K), |r| or |s| above 1 + 1e-10, stride < 1, capacity < 1, and a second call. From then on step_rk2, step_ssprk2,
 * lserk4_stages (a step is the fifth stage) and their _exchanged forms take a record after every stride-th completed step
 * (counted over calls; set_state, set_state4 and monitor_reset restart the count), two launches on the solver's stream
 * behind the step and no host wait. A stepping call that would take more records than the capacity has left returns
 * BDG_ERR_ARGUMENT before it launches anything. bdg_sw2dq_time* take no samples. Without this call no stepping call
 * launches anything it did not launch before. */
int bdg_sw2dq_enable_monitor(bdg_sw2dq* s, const bdg_sw2dq_monitor_desc* desc);
int bdg_sw2dq_monitor_sample(bdg_sw2dq* s);            /* one record of the resident state now */
int bdg_sw2dq_monitor_count(const bdg_sw2dq* s, int* n);
/* records [first, first + count) as count x width doubles; synchronises the solver's stream */
int bdg_sw2dq_monitor_read(bdg_sw2dq* s, int first, int count, double* records);
int bdg_sw2dq_monitor_width(const bdg_sw2dq* s, int* width);
int bdg_sw2dq_monitor_reset(bdg_sw2dq* s);             /* count = 0, step counter = 0 */
/* Partitioned runs: the reduction covers the owned elements, and a gauge whose element is a ghost (>= num_owned) is not
 * evaluated, its entries stay 0: pass each gauge to the rank that owns its element and any ghost element to the others.
 * monitor_reduce is the one collective (after comm_init): it all-reduces the stored records that no earlier call has
 * reduced, in place on the solver's stream: sum for the integrals, E, the gauges and the NaN count, minimum / maximum for
 * the extrema, t left alone. Call it once before reading, not per sample. */
int bdg_sw2dq_monitor_reduce(bdg_sw2dq* s);
/* ---- drifters: points that move with the velocity (hu / h, hv / h) of the resident state, followed from element to element
 * and recorded on the device, one launch per advance on the solver's stream and no host wait
 * (csrc/hip/sw2d_quad_drifter_kernel.hpp and sw2d_drifter_driver.hpp, which state the algorithm). Single domain and bilinear elements only.
 * Host set-up, from a quadrilateral provisioner: bilinear (K, 8), per element xc, ax, bx, cx, yc, ay, by, cy of the map
 * x(r, s) = xc + ax r + bx s + cx r s of its four corner nodes; neighbours (4, K), the element across each face (faces in
 * Fmask order: s = -1, r = +1, s = +1, r = -1), -1 for a wall, -2 for an open boundary face: a boundary face with a node in
 * mapO (the list of bdg_sw2dq_enable_variant_b; may be empty); bary (N+1), the barycentric weights of the Gauss-Lobatto
 * points. BDG_ERR_ARGUMENT for a mesh whose nodes differ from the bilinear map of their element's corners by more than 1e-10
 * of the element's size. */
int bdg_quadnodes_drifter_tables(const bdg_quadnodes* nodes, const int* mapO, int num_out, double* bilinear, int* neighbours,
                                 double* bary);
typedef struct bdg_sw2dq_drifter_desc {
    int count;                  /* number of drifters, >= 1 */
    const int* element;         /* initial positions: element in [0, K) and reference coordinates, |r|, |s| <= 1 + 1e-10 */
    const double* r;            /* (bdg_quadnodes_locate_points) */
    const double* s;
    const double* bilinear;     /* (K, 8), (4, K), (N+1): bdg_quadnodes_drifter_tables */
    const int* neighbours;
    const double* bary;
    int stride;                 /* record after every stride-th advance, >= 1 */
    int capacity;               /* records held on the device, >= 1 */
} bdg_sw2dq_drifter_desc;
/* Status of a drifter: 0 moving, 1 exited through an open face (frozen there), 2 lost (frozen where it was: the search ran
 * out of hops, its Newton iteration failed or the velocity was not finite), + 4 once it has touched a wall (it slides along it).
 * enable_drifters: once per solver; computes x, y from the map and samples the velocity of the resident state (set_state
 * first). BDG_ERR_ARGUMENT, changing nothing, for a NULL or incomplete descriptor, count, stride or capacity < 1, an element
 * outside [0, K), a point outside its element, a neighbour entry outside [-2, K), a second call, and a solver with a partition
 * set; bdg_sw2dq_set_partition in turn refuses a solver that has drifters. From then on step_rk2, step_ssprk2 and
 * lserk4_stages (a step is the fifth stage) advance the drifters by that step's dt after every completed step (Heun: the
 * velocity sampled before the step and the one of the new state), behind the monitor's sample if there is one, and store a
 * record with t = the model time after every stride-th advance; a call that would take more records than the capacity has left
 * returns BDG_ERR_ARGUMENT before it launches anything. set_state and set_state4 sample the velocity again.
 * drifters_advance: num_steps advances by dt in the resident state as it is (steady flows); the records' time moves on by dt per
 * advance, the model time does not. drifters_time: average device milliseconds of `count` such advances, no records taken.
 * drifters_state: the current x, y, element, r, s, status (count entries each; any may be NULL). drifters_count: records
 * taken and drifters. drifters_read: records [first, first + num): t (num), x, y, status (num x count each, record-major; any
 * may be NULL); synchronises the solver's stream. drifters_reset drops the records only. */
int bdg_sw2dq_enable_drifters(bdg_sw2dq* s, const bdg_sw2dq_drifter_desc* desc);
int bdg_sw2dq_drifters_advance(bdg_sw2dq* s, double dt, int num_steps);
int bdg_sw2dq_drifters_time(bdg_sw2dq* s, double dt, int count, float* ms);
int bdg_sw2dq_drifters_state(bdg_sw2dq* s, double* x, double* y, int* element, double* r, double* sref, int* status);
int bdg_sw2dq_drifters_count(const bdg_sw2dq* s, int* num_records, int* num_drifters);
int bdg_sw2dq_drifters_read(bdg_sw2dq* s, int first, int num, double* t, double* x, double* y, int* status);
int bdg_sw2dq_drifters_reset(bdg_sw2dq* s);

/* Resident time stepping (state stays in HBM). */
int bdg_sw2d_step_lserk4(bdg_sw2d* s, double dt, int num_steps);          /* 5 fused stages per step */
int bdg_sw2d_lserk4_stages(bdg_sw2d* s, double dt, int num_stages);       /* stage i = count % 5      */
int bdg_sw2d_step_rk2(bdg_sw2d* s, double dt, int num_steps, int filter); /* midpoint RK2            */
/* SSP-RK2 (Heun) of the variant-B driver, reference src/sw2d/main.cpp:211-235:
 * q1 = sp(q + dt R(q)); q = sp((q + q1 + dt R(q1))/2), sp(x) = x/(1 + sponge_coeff x^2) on hu, hv
 * (sponge_coeff = 0: plain Heun). */
int bdg_sw2d_step_ssprk2(bdg_sw2d* s, double dt, int num_steps, int filter, double sponge_coeff);
/* dt = CFL / ((N+1)^2 * 0.5 * max_i |Fscale_i| * (|u|+sqrt(g h))[vmapM_i]); also returns
 * max|eta| (or max|h|) and BDG_ERR_UNSTABLE on NaN / > 1e8. */
int bdg_sw2d_compute_dt(bdg_sw2d* s, double cfl, double* dt, double* eta_max);
/* Reference driver loop body (src/sw2d-simple/main.cpp:121-171): RK2 step with
 * filter, blow-up check, adaptive dt; runs until t >= final_time or max_steps. */
int bdg_sw2d_run_adaptive(bdg_sw2d* s, double cfl, double final_time, int max_steps, int filter,
                          double* t_inout, double* dt_inout, int* steps_done);

/* ---- multi-GPU: element partition with a ghost layer (no reference analogue; the reference
 * only computes METIS partition vectors, src/MeshManager.cpp:491-544, and never uses them).
 * The solver is created on a LOCAL mesh whose elements are ordered
 *   [ interior | partition-boundary | ghost ]            (ghost = owned by another rank)
 * Only [0, num_owned) are updated; ghost state is refreshed each stage by the caller:
 *   pack (device buffer of num_send*3*Np doubles, element-major) -> exchange (RCCL, caller's
 *   job) -> unpack into the ghost slots, while the interior elements are already computing. */
int bdg_sw2d_set_partition(bdg_sw2d* s, int num_interior, int num_owned, const int* send_elements,
                           int num_send);
int bdg_sw2d_halo_doubles_per_element(const bdg_sw2d* s);
int bdg_sw2d_halo_pack(bdg_sw2d* s, void* send_buffer_device);
int bdg_sw2d_halo_unpack(bdg_sw2d* s, const void* recv_buffer_device);
/* One LSERK4 stage over part of the owned elements: 0 = interior only (does not advance the
 * stage), 1 = partition-boundary elements then advance, 2 = all owned elements then advance. */
int bdg_sw2d_lserk4_stage_part(bdg_sw2d* s, double dt, int part);
/* Native transport: RCCL point-to-point over xGMI, driven entirely from this library (bound
 * with dlopen on first use). Rank 0 creates a 128-byte id and hands it to every rank by any
 * means; each rank then gives its neighbour list: for peer i, it sends the elements
 * send_elements[send_start[i] .. +send_count[i]) (of bdg_sw2d_set_partition) and receives
 * recv_count[i] ghost elements into ghost slots recv_start[i].. (relative to num_owned).
 * A peer may be this rank itself (loop-back: the send range is delivered to the receive range on
 * the same device) -- used to rehearse the per-stage schedule of an N-way split on one GPU. */
int bdg_comm_unique_id(void* id_out, int capacity);
int bdg_sw2d_comm_init(bdg_sw2d* s, int rank, int world, const void* unique_id, const int* peer_ranks,
                       const int* send_start, const int* send_count, const int* recv_start,
                       const int* recv_count, int num_peers);
/* num_stages LSERK4 stages with the ghost exchange overlapped with the interior elements:
 * pack -> {grouped ncclSend/ncclRecv on the comm stream || interior kernel} -> unpack -> boundary.
 * Ghost elements are inputs of a stage only: after this call (and after bdg_sw2d_group_lserk4_stages)
 * the ghost columns returned by bdg_sw2d_get_state / read by bdg_sw2d_rhs_resident and the output
 * functions are UNDEFINED -- they hold whatever an earlier stage received, or, where the boundary kernel
 * reads the received records directly, their initial values. Owned columns are exact. The next
 * exchanged stage refreshes the ghosts before it reads them. */
int bdg_sw2d_lserk4_stages_exchanged(bdg_sw2d* s, double dt, int num_stages);
/* The drivers' two-evaluation schemes in a partitioned run (bdg_sw2d_step_rk2 / bdg_sw2d_step_ssprk2 with an
 * exchange in front of EACH evaluation, of the state that evaluation reads): midpoint RK2 + filter of the sw2d.py /
 * sw2d-simple drivers (three or four fields, sources) and Heun + sponge of the variant-B driver. With variant B
 * enabled every evaluation -- here and in bdg_sw2d_lserk4_stages_exchanged -- also reduces the one global
 * Lax-Friedrichs speed (reference src/sw2d/main.cpp:414) over all ranks: a speed pass over the owned elements and
 * one 8-byte ncclAllReduce(max) on the solver's stream; these paths are not overlapped with computation, because
 * no element of an evaluation can start before the speed is known. Results equal the single-domain run bit for bit. */
int bdg_sw2d_step_rk2_exchanged(bdg_sw2d* s, double dt, int num_steps, int filter);
int bdg_sw2d_step_ssprk2_exchanged(bdg_sw2d* s, double dt, int num_steps, int filter, double sponge_coeff);
/* In-process alternative to RCCL: all parts of the split are handles of THIS process (one per GPU
 * of the node, or several on one GPU). bdg_sw2d_local_peers takes the same neighbour tables as
 * bdg_sw2d_comm_init; bdg_sw2d_group_lserk4_stages then advances parts[0..n) (parts[r] = rank r)
 * together with the same overlapped schedule, the exchange being device-to-device copies out of the
 * neighbours' send buffers. */
int bdg_sw2d_local_peers(bdg_sw2d* s, int rank, const int* peer_ranks, const int* send_start,
                         const int* send_count, const int* recv_start, const int* recv_count, int num_peers);
int bdg_sw2d_group_lserk4_stages(bdg_sw2d** parts, int num_parts, double dt, int num_stages);
/* bdg_sw2d_compute_dt with the maxima reduced over all ranks (one 8-byte all-reduce each). */
int bdg_sw2d_compute_dt_global(bdg_sw2d* s, double cfl, double* dt, double* eta_max);
int bdg_sw2d_allreduce_max(bdg_sw2d* s, double value, double* out);
int bdg_sw2d_allreduce_sum(bdg_sw2d* s, double value, double* out); /* e.g. total mass over all ranks */
/* Drains this rank's streams, meets every other rank, drains again. */
int bdg_sw2d_barrier(bdg_sw2d* s);
/* RHS of the resident state (owned elements valid; ghosts must be current) to host arrays. */
int bdg_sw2d_rhs_resident(bdg_sw2d* s, double* rhs1, double* rhs2, double* rhs3);

int bdg_sw2d_synchronize(bdg_sw2d* s);
/* Runs num_stages LSERK4 stages bracketed by HIP events on the solver's own stream and
 * returns the average device time per stage-kernel launch in milliseconds. */
int bdg_sw2d_time_lserk4_stages(bdg_sw2d* s, double dt, int num_stages, float* ms_per_launch);
/* Bytes of HBM the solver holds; algorithmic bytes per element per fused stage. */
/* Measurement aids. bdg_probe_stream_triad: STREAM triad (a = b + s*c, 16 B per lane) over three
 * arrays of bytes_per_array each; returns GB/s -- the practical HBM roof of the device.
 * bdg_sw2d_probe_stage_traffic: a launch with the stage kernel's own row accesses and read/write
 * mix but no gathers and no arithmetic; its time is the memory-system floor for that pattern. */
int bdg_probe_stream_triad(int device, size_t bytes_per_array, int repeats, double* gbps);
int bdg_sw2d_probe_stage_traffic(bdg_sw2d* s, int repeats, float* ms_per_launch);
/* 1 if the solver runs the affine-geometry kernels, 0 for the per-node-geometry kernels. */
int bdg_sw2d_uses_affine_geometry(const bdg_sw2d* s);
/* 1 if the solver renumbered the elements internally (I/O stays in the caller's numbering). */
int bdg_sw2d_is_renumbered(const bdg_sw2d* s);
/* The numbering a renumbering solver gives a triangle mesh, from its face-neighbour table alone (no GPU):
 * EToE is (num_elements, 3) row-major, a boundary face naming its own element; perm[caller element] = slot.
 * patch <= 0: breadth-first from element 0 (the solvers' numbering); patch > 0: compact patches of that many
 * elements grown over the face graph, slots by caller index inside a patch (a solver's with BDG_SW2D_ORDER_PATCH=patch). */
int bdg_element_order(const int* EToE, int num_elements, int patch, int* perm);
/* 1 if a solver of this order created without BDG_SW2D_REORDER / BDG_SW2D_KEEP_ORDER renumbers this mesh,
 * 0 if it keeps the caller's order, -1 on a bad argument. */
int bdg_element_order_wanted(const int* EToE, int num_elements, int order);
size_t bdg_sw2d_device_bytes(const bdg_sw2d* s);
/* The tile of elements workgroup `block` of a stage launch of `grid` one-tile workgroups takes (no GPU): workgroups go to the
 * eight XCDs round robin, each XCD owns one contiguous chunk of tiles and walks it from its low end (back = 0) or from its
 * high end (back = 1). The same function the stage kernels call. Whole-mesh stage launches of a solver alternate the
 * direction (BDG_SW2D_SWEEP=forward at creation: always 0); bdg_sw2d_backward_launches: how many of the solver's launches
 * so far walked from the high end (-1: no solver). */
unsigned bdg_stage_tile(unsigned block, unsigned grid, unsigned back);
long long bdg_sw2d_backward_launches(const bdg_sw2d* s);
/* The raw stream (hipStream_t) launches are issued on, for callers that interleave their own work. */
void* bdg_sw2d_stream(bdg_sw2d* s);

/* ---- run monitor of the triangle solver: conservation diagnostics and gauges recorded on the device during the stepping
 * calls, with no host round trip and no state download (csrc/hip/sw2d_monitor_kernel.hpp), the counterpart of the
 * bdg_sw2dq_* group above with the same record layout. Host set-up, from a triangle provisioner (none of the three touches
 * a GPU; BDG_ERR_ARGUMENT for a NULL handle or argument):
 * quadrature_weights: w (Np, K), w[n, k] = m[n] J[n, k], m the column sums of the reference mass matrix Vinv^T Vinv (the
 * provisioner's current J): sum w f is exact for f in P^N on a straight-sided element.
 * locate_points: for each (x[p], y[p]) the element that contains it and its reference coordinates, by Newton iteration on
 * the element's own nodal map (one step on straight-sided elements; deformed coordinates after set_coordinates work too);
 * r >= -1 - 1e-10, s >= -1 - 1e-10, r + s <= 1e-10 counts as inside, a point on a shared edge or vertex goes to the lowest
 * element index, a point in no element gets element -1 (r = s = 0). Candidates come from a uniform grid over the mesh.
 * interpolation_rows: rows (n, Np), rows[p, :] = P(r[p], s[p]) Vinv, P the orthonormal basis row of the provisioner's
 * Vandermonde matrix: the nodal Lagrange basis at the point, what the gauges interpolate with; a point that equals a
 * reference node bit for bit gives the exact unit vector. */
int bdg_trinodes_quadrature_weights(const bdg_trinodes* nodes, double* w);
int bdg_trinodes_locate_points(const bdg_trinodes* nodes, const double* x, const double* y, int n, int* element, double* r,
                               double* s);
int bdg_trinodes_interpolation_rows(const bdg_trinodes* nodes, const double* r, const double* s, int n, double* rows);
/* One record is `width` = 7 + fields + fields * num_gauges doubles:
 *   t, int h, int hu, int hv, (int hN,) E, min h, max h, max|hu|, max|hv|, NaN count, then per gauge eta, u, v (, N)
 * t = the model time (bdg_sw2d_get_time); E = int (hu^2 + hv^2) / (2h) + g (h - H)^2 / 2; the NaN count covers every
 * field; eta = h - H, u = hu / h, v = hv / h, N = hN / h are formed at the nodes of the gauge's element exactly as
 * bdg_sw2d_output_fields forms them and interpolated as sum_n row[n] f[n] over ascending n from 0.0, so a gauge on a node
 * is that node's output value (IM = NULL) bit for bit. H: the descriptor's if given, else the solver's resident one
 * (bdg_sw2d_set_bathymetry or variant B), else 0. The summation order of the integrals is fixed (a fixed grid, a fixed
 * range of device slots per workgroup, each thread its elements and their nodes in ascending order with acc = acc + w f, an
 * LDS tree, partials added in ascending order; no floating-point atomics): equal states give equal records bit for bit.
 * A solver that renumbered its elements (bdg_sw2d_is_renumbered) sums in the order of its device slots: the weights are
 * uploaded through the renumbering, and the records of a renumbered and a BDG_SW2D_KEEP_ORDER solver agree to the summation
 * bound, not bit for bit. Gauge elements are given in the caller's numbering. These weights serve straight-sided
 * solvers; bdg_sw2d_curved has cubature weights and per-element mass matrices and takes the weights its own monitor states
 * (bdg_sw2d_curved_enable_monitor below). */
typedef struct bdg_sw2d_monitor_desc {
    const double* weights;      /* (Np, K), bdg_trinodes_quadrature_weights */
    const double* H;            /* (Np, K) or NULL (the solver's resident H if it has one) */
    int num_gauges;             /* may be 0 */
    const int* gauge_element;   /* caller numbering, each in [0, K) */
    const double* gauge_row;    /* (num_gauges, Np), bdg_trinodes_interpolation_rows */
    int stride;                 /* sample after every stride-th completed step, >= 1 */
    int capacity;               /* records held on the device, >= 1 */
} bdg_sw2d_monitor_desc;
/* Once per solver. BDG_ERR_ARGUMENT, changing nothing, for a NULL handle or descriptor or weights, a gauge list without
 * elements or rows, a gauge element outside [0, K), stride < 1, capacity < 1, and a second call. From then on step_lserk4,
 * lserk4_stages (a step is the fifth stage), step_rk2, step_ssprk2, run_adaptive and the _exchanged forms take a record
 * after every stride-th completed step (counted over calls; set_state, set_state4 and monitor_reset restart the count),
 * two launches on the solver's stream behind the step and no host wait. A stepping call that would take more records than
 * the capacity has left returns BDG_ERR_ARGUMENT before it launches anything; run_adaptive, whose step count is not known in
 * advance (with or without max_steps), checks before each step and stops with that error, steps_done telling the steps it
 * made. lserk4_stage_part, group_lserk4_stages,
 * time_lserk4_stages, probe_stage_traffic and the RHS calls take no records. Without this call no stepping call launches
 * anything it did not launch before. */
int bdg_sw2d_enable_monitor(bdg_sw2d* s, const bdg_sw2d_monitor_desc* desc);
int bdg_sw2d_monitor_sample(bdg_sw2d* s);            /* one record of the resident state now */
int bdg_sw2d_monitor_count(const bdg_sw2d* s, int* n);
/* records [first, first + count) as count x width doubles; synchronises the solver's stream */
int bdg_sw2d_monitor_read(bdg_sw2d* s, int first, int count, double* records);
int bdg_sw2d_monitor_width(const bdg_sw2d* s, int* width);
int bdg_sw2d_monitor_reset(bdg_sw2d* s);             /* count = 0, step counter = 0 */
/* Partitioned runs: the reduction covers the owned elements, and a gauge whose element is a ghost (>= num_owned) is not
 * evaluated, its entries stay 0: pass each gauge to the rank that owns its element and any ghost element to the others.
 * monitor_reduce is the one collective (after comm_init): it all-reduces the stored records that no earlier call has
 * reduced, in place on the solver's stream: sum for the integrals, E, the gauges and the NaN count, minimum / maximum for
 * the extrema, t left alone. Call it once before reading, not per sample. */
int bdg_sw2d_monitor_reduce(bdg_sw2d* s);
/* Average device milliseconds of one sample (both launches), `count` of them bracketed by events on the solver's stream;
 * takes no records (the launches write a scratch record). */
int bdg_sw2d_monitor_time(bdg_sw2d* s, int count, float* ms);

/* ---- drifters of the triangle solver: points that move with the velocity (hu / h, hv / h) of the resident state, followed
 * from element to element and recorded on the device, one launch per advance on the solver's stream and no host wait
 * (csrc/hip/sw2d_drifter_kernel.hpp and sw2d_drifter_driver.hpp, which state the algorithm); the counterpart of the bdg_sw2dq_*drifter* group above with
 * the same statuses and record layout. Single domain and straight-sided (affine) elements only.
 * Host set-up, from a triangle provisioner (no GPU): vertices (K, 8), per element x0, y0, x1, y1, x2, y2 of its corner nodes
 * and two pad entries; the vertices are in face order: face 0 (s = -1) runs from vertex 0 to 1, face 1 (r + s = 0) from 1 to 2,
 * face 2 (r = -1) from 2 to 0. neighbours (3, K): the element across each face, -1 for a wall, -2 for an open boundary face: a
 * boundary face with a node in mapO (the list of bdg_sw2d_enable_variant_b, flat face-node numbering (3 k + f) Nfp + i; may be
 * empty). vinv (Np, Np): the provisioner's inverse Vandermonde matrix. jacobi (N + 2, N + 1, 3): the three-term recurrences
 * p_0 = A_0, p_n = (A_n x + B_n) p_{n-1} + C_n p_{n-2} of sqrt(2) P_n^(0,0) (row 0) and of the orthonormal Jacobi polynomials
 * P_n^(2i+1,0) (row i + 1, i = 0..N), n <= N, entries (A, B, C): the device evaluates the orthonormal simplex basis P(r, s) of
 * the provisioner and the rows P(r, s) Vinv from them without square roots. BDG_ERR_ARGUMENT for a NULL argument, a mapO
 * entry out of range, a mesh on which a node lies off the affine map of its element's corners by more than 1e-10 of the
 * element's size (deformed or blended elements), and an element whose signed area is not positive and finite. */
int bdg_trinodes_drifter_tables(const bdg_trinodes* nodes, const int* mapO, int num_out, double* vertices, int* neighbours,
                                double* vinv, double* jacobi);
typedef struct bdg_sw2d_drifter_desc {
    int count;                  /* number of drifters, >= 1 */
    const int* element;         /* initial positions: element in [0, K), caller numbering, and reference coordinates with */
    const double* r;            /* -1 - s, r + s, -1 - r <= 1e-10 (bdg_trinodes_locate_points) */
    const double* s;
    const double* vertices;     /* (K, 8), (3, K), (Np, Np), (N + 2, N + 1, 3): bdg_trinodes_drifter_tables */
    const int* neighbours;
    const double* vinv;
    const double* jacobi;
    int stride;                 /* record after every stride-th advance, >= 1 */
    int capacity;               /* records held on the device, >= 1 */
} bdg_sw2d_drifter_desc;
/* Status of a drifter: 0 moving, 1 exited through an open face (frozen there), 2 lost (frozen where it was: the search ran
 * out of hops or a coordinate or the velocity was not finite), + 4 once it has touched a wall (it slides along it; in a corner
 * it rests on the vertex).
 * enable_drifters: once per solver; computes x, y from the map and samples the velocity of the resident state (set_state
 * first). BDG_ERR_ARGUMENT, changing nothing, for a NULL or incomplete descriptor, count, stride or capacity < 1, an element
 * outside [0, K), a point outside its element, a neighbour entry outside [-2, K), a second call, and a solver with a partition
 * set; bdg_sw2d_set_partition in turn refuses a solver that has drifters. From then on step_lserk4, lserk4_stages (a step is
 * the fifth stage), step_rk2, step_ssprk2 and run_adaptive advance the drifters by that step's dt after every completed step
 * (Heun: the velocity sampled before the step and the one of the new state), behind the monitor's sample if there is one, and
 * store a record with t = the model time after every stride-th advance; a call that would take more records than the capacity
 * has left returns BDG_ERR_ARGUMENT before it launches anything (run_adaptive checks before every step, as for the monitor).
 * set_state and set_state4 sample the velocity again. A solver that renumbered its elements keeps the drifters' elements and
 * the neighbour table in its device slots; everything passed or read here is in the caller's numbering, and nothing in a
 * drifter's arithmetic depends on the numbering.
 * drifters_advance: num_steps advances by dt in the resident state as it is (steady flows); the records' time moves on by dt per
 * advance, the model time does not. drifters_time: average device milliseconds of `count` such advances, no records taken.
 * drifters_state: the current x, y, element, r, s, status (count entries each; any may be NULL). drifters_count: records
 * taken and drifters. drifters_read: records [first, first + num): t (num), x, y, status (num x count each, record-major; any
 * may be NULL); synchronises the solver's stream. drifters_reset drops the records only.
 * (Curved elements: bdg_sw2d_curved_enable_drifters below.) */
int bdg_sw2d_enable_drifters(bdg_sw2d* s, const bdg_sw2d_drifter_desc* desc);
int bdg_sw2d_drifters_advance(bdg_sw2d* s, double dt, int num_steps);
int bdg_sw2d_drifters_time(bdg_sw2d* s, double dt, int count, float* ms);
int bdg_sw2d_drifters_state(bdg_sw2d* s, double* x, double* y, int* element, double* r, double* sref, int* status);
int bdg_sw2d_drifters_count(const bdg_sw2d* s, int* num_records, int* num_drifters);
int bdg_sw2d_drifters_read(bdg_sw2d* s, int first, int num, double* t, double* x, double* y, int* status);
int bdg_sw2d_drifters_reset(bdg_sw2d* s);

/* ---- field statistics of the triangle and the quadrilateral solver: per node, over the samples of a run, the sums of
 * eta, u, v (mean group), the envelopes etaMax, hMin, speedMax (envelope group) and, for up to four periods T_j, the sums of
 * f cos(omega_j t) and f sin(omega_j t), omega_j = 2 pi / T_j (harmonic group), accumulated on the device with one launch
 * per sample on the solver's stream, no host wait and no state download (csrc/hip/sw2d_stats_kernel.hpp, which states the
 * arithmetic: eta = h - H, u = hu / h, v = hv / h by the rule of output_fields; acc = acc + f c with one multiply and one
 * add; fmax / fmin skip NaNs; speed = sqrt(u u + v v); the envelopes start from -inf, +inf, 0). H: the descriptor's if given,
 * else the solver's resident one (set_bathymetry or variant B), else 0. t is the model time of the sample, and cos / sin are
 * formed on the host in double; the host keeps one row t, c_1, s_1, .. c_m, s_m per sample, exactly what the kernel was
 * given, from which a caller forms the normal equations of a harmonic fit (blitzdg_amd/_records.py: harmonicFit). A group
 * that is off allocates and moves nothing. hN of a four-field solver is not analysed. */
typedef struct bdg_field_stats_desc {
    const double* H;            /* (Np, K) or NULL */
    int stride;                 /* sample after every stride-th completed step, >= 1 */
    int num_periods;            /* 0 .. 4 */
    double periods[4];          /* seconds, each > 0 */
    int mean;                   /* nonzero: the mean group */
    int envelope;               /* nonzero: the envelope group */
} bdg_field_stats_desc;
/* `which` of field_stats_read. SUM: index = field (0 eta, 1 u, 2 v); ETA_MAX, H_MIN, SPEED_MAX: index = 0; COS, SIN: index =
 * 3 j + field for period j. */
enum { BDG_FIELD_STATS_SUM = 0, BDG_FIELD_STATS_ETA_MAX = 1, BDG_FIELD_STATS_H_MIN = 2, BDG_FIELD_STATS_SPEED_MAX = 3,
       BDG_FIELD_STATS_COS = 4, BDG_FIELD_STATS_SIN = 5 };
/* enable_field_stats: once per solver. BDG_ERR_ARGUMENT, changing nothing (device_bytes included), for a NULL handle or
 * descriptor, a second call, stride < 1, num_periods outside [0, 4], a period <= 0, a descriptor with every group off, and a
 * solver with a partition or a transport set; set_partition, comm_init and local_peers in turn refuse a solver that has field
 * statistics (the _exchanged steppers take no samples). From then on the stepping
 * calls that feed the monitor take a sample after every stride-th completed step (counted over calls; set_state and
 * set_state4 restart the count and leave the accumulators alone), behind the monitor's sample and in front of the drifters'
 * advance. field_stats_sample: one sample of the resident state now. field_stats_count: samples taken and num_periods.
 * field_stats_read: one accumulator plane as (Np, K) doubles in the caller's numbering; synchronises the solver's stream;
 * BDG_ERR_ARGUMENT for a group that is off and for an index outside it. field_stats_samples: rows [first, first + count) of the
 * sample log, 1 + 2 num_periods doubles each. field_stats_reset: accumulators as after enable, log empty, step count 0.
 * field_stats_time: average device milliseconds of one sample, `count` of them into scratch accumulators that live for the
 * call: neither the accumulators nor the log change. */
int bdg_sw2d_enable_field_stats(bdg_sw2d* s, const bdg_field_stats_desc* desc);
int bdg_sw2d_field_stats_sample(bdg_sw2d* s);
int bdg_sw2d_field_stats_count(const bdg_sw2d* s, int* samples, int* num_periods);
int bdg_sw2d_field_stats_read(bdg_sw2d* s, int which, int index, double* plane);
int bdg_sw2d_field_stats_samples(const bdg_sw2d* s, int first, int count, double* rows);
int bdg_sw2d_field_stats_reset(bdg_sw2d* s);
int bdg_sw2d_field_stats_time(bdg_sw2d* s, int count, float* ms);
int bdg_sw2dq_enable_field_stats(bdg_sw2dq* s, const bdg_field_stats_desc* desc);
int bdg_sw2dq_field_stats_sample(bdg_sw2dq* s);
int bdg_sw2dq_field_stats_count(const bdg_sw2dq* s, int* samples, int* num_periods);
int bdg_sw2dq_field_stats_read(bdg_sw2dq* s, int which, int index, double* plane);
int bdg_sw2dq_field_stats_samples(const bdg_sw2dq* s, int first, int count, double* rows);
int bdg_sw2dq_field_stats_reset(bdg_sw2dq* s);
int bdg_sw2dq_field_stats_time(bdg_sw2dq* s, int count, float* ms);

/* ---------------------------------------------------------------- sw2d, curved / over-integrated RHS
 * reference: swhelpers.rhs.sw2dComputeRHS_curved(h, hu, hv, hN, zx, zy, g, H, f, CD, ctx, cub_ctx, gauss_ctx,
 * curvedEls, J, gmapM, gmapP) (swhelpers/rhs.py:6-176), driven by sw2d_curved.py:246-277 (RHS, Filter, midpoint
 * RK2). The function is pure in its context arguments, and so is this solver: every table is an input (any
 * cubature rule, any Gauss-node map -- periodic rewiring included), borrowed for the duration of create.
 * Four fields always (h, hu, hv, hN). H is an argument of the reference function that it never uses
 * (rhs.py:16, :73-75 form cub_H / gauss_H and drop them); it is therefore not part of this interface.
 * Host code above this seam: blitzdg_amd/swhelpers/rhs.py (same 17-argument signature). */
typedef struct bdg_sw2d_curved bdg_sw2d_curved;
typedef struct bdg_sw2d_curved_desc {
    int order;            /* N: 1..8                                                          */
    int num_elements;     /* K                                                                */
    int num_cub;          /* cubature points per element (cub_ctx.V.shape[0])                 */
    int num_gauss;        /* Gauss points per face (gauss_ctx.NGauss)                         */
    const double* V;      /* (Np, Np) ctx.V: the straight elements' mass inverse is V V^T     */
    const double* Filter; /* (Np, Np) ctx.filter or NULL                                      */
    const double* J;      /* (Np, K) nodal Jacobian as the driver forms it (sw2d_curved.py:112-118) */
    const double* cubV; const double* cubDr; const double* cubDs;     /* (Ncub, Np) cub_ctx.V, Dr, Ds   */
    const double* cubW; const double* cubrx; const double* cubry;     /* (Ncub, K)  cub_ctx.W, rx, ry   */
    const double* cubsx; const double* cubsy;                         /* (Ncub, K)  cub_ctx.sx, sy      */
    const double* gaussInterp;                                        /* (3 NGauss, Np) gauss_ctx.Interp */
    const double* gaussW; const double* gaussnx; const double* gaussny; /* (3 NGauss, K) gauss_ctx.W, nx, ny */
    const int* gmapM;     /* (3 NGauss K) flat Gauss ids g + 3 NGauss k                       */
    const int* gmapP;
    const int* gmapW;     /* gauss_ctx.BCmap[3]: flat ids of reflective-wall Gauss nodes      */
    int num_wall;
    const int* curvedEls; /* elements that take their own cubature mass matrix                */
    int num_curved;
    const double* MMChol; /* (Np, Np, K) cub_ctx.MMChol; only the columns of curvedEls are read; may be NULL if none */
    const double* zx;     /* (Np, K) or NULL (= 0)                                            */
    const double* zy;
    const double* coriolis; /* (Np, K) f, or NULL: coriolis_const                             */
    double coriolis_const;
    const double* drag;   /* (Np, K) CD (an array in sw2d_curved.py:176-192), or NULL: drag_const */
    double drag_const;
    double g;
    int device;
    int flags;            /* 0                                                                */
} bdg_sw2d_curved_desc;
/* Size limit of one solver: device tables are addressed with 32-bit byte offsets, so max(5 Np, 16 ceil(num_cub / 16),
 * 192 ceil(num_gauss / 16)) * ld * 8 must stay below 4 GiB (ld = num_elements rounded up to 64): 2.8 million elements at
 * N = 4 with the builders' default rules, 2.5 million at N = 8. BDG_ERR_ARGUMENT beyond it: partition the mesh. */
int bdg_sw2d_curved_create(const bdg_sw2d_curved_desc* desc, bdg_sw2d_curved** out);
/* What bdg_sw2d_curved_create would decide for this descriptor, from its host tables alone: no device is touched, so it runs
 * on a machine without a GPU (desc->device is ignored). The same functions build the tables in both calls. The first
 * min(n, 8) of
 *   out[0] form           0 general, 1 nodal-trace (bdg_sw2d_curved_form), after BDG_SW2D_CURVED_GENERAL
 *   out[1] identity_m     1 when gmapM is the identity
 *   out[2] num_curved     distinct elements of curvedEls
 *   out[3] num_affine     straight elements the general form holds compressed (BDG_SW2D_CURVED_NO_AFFINE: 0)
 *   out[4] num_affine_nt  straight elements the nodal-trace form holds compressed (0 on the general form)
 *   out[5] kref           element whose cubature weights the general form's compression refers to (-1: none)
 *   out[6] kref_nt        likewise for the nodal-trace form
 *   out[7] order_tiles    tiles in the nodal-trace form's tile order (0: mesh order)
 * Refusals carry the texts of bdg_sw2d_curved_create. */
#define BDG_SW2D_CURVED_PLAN_FIELDS 8
int bdg_sw2d_curved_plan(const bdg_sw2d_curved_desc* desc, int* out, int n);
void bdg_sw2d_curved_destroy(bdg_sw2d_curved* s);
/* The reference function itself: host (Np, K) fields in, host RHS out; filter != 0 returns Filter * RHS
 * (what the driver applies next, sw2d_curved.py:250-253). The resident state is not disturbed. */
int bdg_sw2d_curved_rhs(bdg_sw2d_curved* s, const double* h, const double* hu, const double* hv, const double* hN,
                        double* rhs1, double* rhs2, double* rhs3, double* rhs4, int filter);
int bdg_sw2d_curved_set_state(bdg_sw2d_curved* s, const double* h, const double* hu, const double* hv, const double* hN);
int bdg_sw2d_curved_get_state(bdg_sw2d_curved* s, double* h, double* hu, double* hv, double* hN);
/* num_steps of the driver's loop body (sw2d_curved.py:246-277) on the resident state: RHS, filter, predictor
 * q1 = q + dt/2 RHS, RHS(q1), filter, corrector q += dt RHS. */
int bdg_sw2d_curved_step_rk2(bdg_sw2d_curved* s, double dt, int num_steps, int filter);
/* num_stages fused LSERK4 stages on the resident state (stage index continues across calls). */
int bdg_sw2d_curved_lserk4_stages(bdg_sw2d_curved* s, double dt, int num_stages);
/* As step_rk2, timed with HIP events on the solver's stream: milliseconds per RHS evaluation
 * (Gauss-trace kernel + stage kernel + curved-element kernel), two evaluations per step. */
int bdg_sw2d_curved_time_rk2(bdg_sw2d_curved* s, double dt, int num_steps, int filter, float* ms_per_rhs);
int bdg_sw2d_curved_synchronize(bdg_sw2d_curved* s);
/* Element-partitioned runs (blitzdg_amd.sw2d_curved.DistributedSw2dCurved; no reference analogue, the reference is
 * single-process): the solver is created on a rank-local mesh [owned elements | ghost elements], and the caller refreshes the
 * ghost columns before every RHS evaluation. Columns [first, first + count) of all 4 Np rows of the resident state
 * (which = 0) or of the RK2 intermediate state (which = 1), as a (4 Np, count) row-major host array: */
int bdg_sw2d_curved_get_elements(bdg_sw2d_curved* s, int which, int first, int count, double* out);
int bdg_sw2d_curved_set_elements(bdg_sw2d_curved* s, int which, int first, int count, const double* in);
/* One half of the driver's step (sw2d_curved.py:246-277), so that a ghost exchange fits between the two evaluations:
 * phase 0 -- predictor, intermediate = state + dt/2 RHS(state); phase 1 -- corrector, state += dt RHS(intermediate). */
int bdg_sw2d_curved_rk2_phase(bdg_sw2d_curved* s, double dt, int phase, int filter);
/* The same exchange driven by this library over RCCL (point-to-point over xGMI; bound with dlopen on first use, as for
 * bdg_sw2d_comm_init, whose id -- bdg_comm_unique_id -- and neighbour tables it takes): the solver's mesh is ordered
 * [elements without a ghost neighbour: num_interior | partition-boundary elements: up to num_owned | ghosts: up to K]; peer i is
 * sent the elements send_elements[send_start[i] .. + send_count[i]) and its recv_count[i] elements arrive in ghost slots
 * recv_start[i] .. (relative to num_owned); one record of 4 Np doubles per element. step_rk2_exchanged = num_steps times
 * {exchange(state), predictor, exchange(intermediate), corrector}; on the nodal-trace form the interior elements of an
 * evaluation run on the solver's stream beside the exchange and the partition-boundary elements on a second stream (two chains
 * joined by events, as bdg_sw2d_lserk4_stages_exchanged), ghost elements are not evaluated, and the ghost columns bdg_sw2d_curved_
 * get_state returns afterwards are whatever was last received. exchange: one refresh by itself (which as above). barrier: drains
 * the streams, meets every rank (an 8-byte all-reduce), drains again. */
int bdg_sw2d_curved_set_partition(bdg_sw2d_curved* s, int num_interior, int num_owned, const int* send_elements, int num_send);
int bdg_sw2d_curved_comm_init(bdg_sw2d_curved* s, int rank, int world, const void* unique_id, const int* peer_ranks,
                              const int* send_start, const int* send_count, const int* recv_start, const int* recv_count,
                              int num_peers);
int bdg_sw2d_curved_step_rk2_exchanged(bdg_sw2d_curved* s, double dt, int num_steps, int filter);
int bdg_sw2d_curved_lserk4_stages_exchanged(bdg_sw2d_curved* s, double dt, int num_stages); /* bdg_sw2d_curved_lserk4_stages, an exchange in front of every stage */
int bdg_sw2d_curved_exchange(bdg_sw2d_curved* s, int which);
int bdg_sw2d_curved_barrier(bdg_sw2d_curved* s);
size_t bdg_sw2d_curved_device_bytes(const bdg_sw2d_curved* s);
/* Compulsory HBM bytes of one RHS evaluation with the tables as this solver holds them (per element, averaged). */
double bdg_sw2d_curved_bytes_per_element(const bdg_sw2d_curved* s);
/* Which kernels serve this solver: 1 = the nodal-trace form (one stage launch per evaluation; the neighbours' Gauss traces
 * are products of their face-node values: needs gmapM = identity, a gmapP that pairs whole faces and an Interp whose face
 * rows vanish off the face nodes -- what buildGaussFaceNodes produces, periodic rewiring included), 0 = the general form
 * (Gauss-trace planes; any map). Decided at creation; BDG_SW2D_CURVED_GENERAL=1 forces 0. -1: NULL handle. */
int bdg_sw2d_curved_form(const bdg_sw2d_curved* s);
/* Which kernel instance this solver's evaluations launch (with the filter fused or not), as the launch path itself decides it:
 * the first min(n, 8) of
 *   out[0] form          0 general, 1 nodal-trace (bdg_sw2d_curved_form)
 *   out[1] streamed      nodal-trace: 1 when the operator image is streamed through LDS, 0 when it is resident (-1: general)
 *   out[2] image_in_lds  general: 1 when the stage kernel holds the operator image in LDS, 0 when it reads it from global
 *                        memory (-1: nodal-trace)
 *   out[3] fb            16-row blocks per face
 *   out[4] live_steps    nodal-trace: live 4-row steps of a face's last block in the compiled shape (4: every step) (-1: general)
 *   out[5] waves         register budget: waves per SIMD the instance is compiled for
 *   out[6] mapm          general: 1 when the interior traces are gathered through a rewired gmapM
 *   out[7] lds_bytes     dynamic LDS of the stage launch
 * No GPU work, nothing is launched. BDG_SW2D_CURVED_STREAM and BDG_SW2D_CURVED_WAVES are read once per process, by the first
 * launch or by this call, whichever comes first. */
#define BDG_SW2D_CURVED_KERNEL_INFO_FIELDS 8
int bdg_sw2d_curved_kernel_info(const bdg_sw2d_curved* s, int filter, int* out, int n);

/* ---- The rest of the reference driver's loop (sw2d_curved.py:231-302) on the resident state: the time step recomputed after
 * every step, the blow-up check, and the six output fields. Kernels: csrc/hip/sw2d_curved_driver_kernel.hpp. A solver on which
 * enable_driver was never called launches exactly what it launched before these calls existed. */
typedef struct bdg_sw2d_curved_driver_desc {
    const double* Fscale;   /* (3 Nfp, K)  ctx.Fscale */
    const int*    vmapM;    /* (3 Nfp K)   ctx.vmapM, flat, node + Np k */
    const double* c;        /* (Np, K) wave speed of the dt formula, or NULL: c_const */
    double        c_const;
    const double* H;        /* (Np, K) or NULL: eta = h */
    const double* Dr; const double* Ds;              /* (Np, Np) */
    const double* rx; const double* sx; const double* ry; const double* sy;   /* (Np, K) */
} bdg_sw2d_curved_driver_desc;
/* Validated on the host before the device is touched: vmapM[j + 3 Nfp k] must be a node of element k, and its local part the
 * same list of 3 Nfp face nodes in every element (that list is what the device gets). BDG_ERR_ARGUMENT, and nothing changed, for
 * a NULL required pointer or a vmapM that fails either check. A second call replaces the tables. The calls below return
 * BDG_ERR_ARGUMENT until this one has succeeded. */
int bdg_sw2d_curved_enable_driver(bdg_sw2d_curved* s, const bdg_sw2d_curved_driver_desc* d);
/* dt = cfl / max_{j,k} ( ((N+1)^2 0.5 |Fscale[j,k]|) (c[n_j,k] + sqrt(u[n_j,k]^2 + v[n_j,k]^2)) ),  u = hu / h, v = hv / h, n_j the
 * face-node list, over the owned elements ([0, num_owned) after set_partition, else all), in that association with contraction
 * off and correctly rounded division and square root: the NumPy expression of sw2d_curved.py:281 on the downloaded state, bit
 * for bit. h_max = max|h|. BDG_ERR_UNSTABLE (dt and h_max still stored) when an owned h or a speed is NaN or h_max > 1e8. */
int bdg_sw2d_curved_compute_dt(bdg_sw2d_curved* s, double cfl, double* dt, double* h_max);
/* The script's loop in the script's order:
 *   while t < final_time and (max_steps <= 0 or done < max_steps):
 *       RK2 + filter step with dt;  t += dt;  dt = compute_dt (BDG_ERR_UNSTABLE on blow-up);  ++done;  t, dt written back
 * The last step is not clipped to final_time (the script does not clip it either). One small device-to-host copy per step.
 * BDG_ERR_ARGUMENT on a solver with a communicator (bdg_sw2d_curved_comm_init): there is no rank-global dt. */
int bdg_sw2d_curved_run_adaptive(bdg_sw2d_curved* s, double cfl, double final_time, int max_steps, int filter,
                                 double* t_inout, double* dt_inout, int* steps_done);
/* eta = h - H, u = hu / h, v = hv / h, B = hN / h, h and vort = (rx Dr v + sx Ds v) - (ry Dr u + sy Ds u) of the resident state as
 * (Np, K) arrays, one launch for all the non-NULL ones; only the owned columns are written. IM == NULL: nodal values (the five
 * pointwise fields equal the expressions on the downloaded state bit for bit). Otherwise every field is multiplied by the
 * (Np, Np) matrix of TriangleNodesProvisioner::splitOperators. Every sum runs over ascending node index from 0.0. */
int bdg_sw2d_curved_output_fields(bdg_sw2d_curved* s, const double* IM, double* eta, double* u, double* v,
                                  double* B, double* h, double* vort);
/* Average device milliseconds (HIP events on the solver's stream, after 10 untimed launches) of `count` dt passes (which = 0) or
 * output launches of all six fields (which = 1; IM as above). */
int bdg_sw2d_curved_time_driver(bdg_sw2d_curved* s, int which, const double* IM, int count, float* ms);

/* ---- model time, run monitor, field statistics and drifters of the curved solver: the groups of bdg_sw2d_* above with the same
 * record layouts, statuses and refusals (csrc/hip/run_records.hpp). Single domain only: every enable_* call refuses a solver
 * with a partition or a communicator set, and set_partition and comm_init refuse a solver that has any of the three; the
 * host-staged halves (rk2_phase) feed nothing. With nothing enabled every stepping call launches exactly what it did before.
 * The columns of the state are the caller's elements: nothing is renumbered.
 * Model time: + dt per completed step of step_rk2 (and time_rk2), per completed five-stage step of lserk4_stages; run_adaptive
 * starts it from its t_inout and adds each step's dt. Only the records read it. */
int bdg_sw2d_curved_set_time(bdg_sw2d_curved* s, double t);
int bdg_sw2d_curved_get_time(const bdg_sw2d_curved* s, double* t);
/* Run monitor: four fields, so a record is t, int h, int hu, int hv, int hN, E, min h, max h, max|hu|, max|hv|, NaN count, then
 * per gauge eta, u, v, N. weights (Np, K): on the elements of curvedEls w[:, k] = cubV^T cubW[:, k], the column sums 1^T M_k of
 * the element's mass matrix, which is the mass its Cholesky solve conserves; m[n] J[n, k] (bdg_trinodes_quadrature_weights) on
 * the others (blitzdg_amd/sw2d_curved.py: quadratureWeights). gauge_row from bdg_trinodes_interpolation_rows at the (r, s)
 * bdg_trinodes_locate_points gives on the deformed coordinates. H: the descriptor's if given, else the one
 * bdg_sw2d_curved_enable_driver was given, else 0. Records after every stride-th completed step of step_rk2, lserk4_stages and
 * run_adaptive (which checks the room before each step); a call that would overflow the capacity is refused before it launches
 * anything. */
int bdg_sw2d_curved_enable_monitor(bdg_sw2d_curved* s, const bdg_sw2d_monitor_desc* desc);
int bdg_sw2d_curved_monitor_sample(bdg_sw2d_curved* s);
int bdg_sw2d_curved_monitor_count(const bdg_sw2d_curved* s, int* n);
int bdg_sw2d_curved_monitor_read(bdg_sw2d_curved* s, int first, int count, double* records);
int bdg_sw2d_curved_monitor_width(const bdg_sw2d_curved* s, int* width);
int bdg_sw2d_curved_monitor_reset(bdg_sw2d_curved* s);
int bdg_sw2d_curved_monitor_time(bdg_sw2d_curved* s, int count, float* ms);
/* Field statistics: bdg_sw2d_enable_field_stats and its group, H by the monitor's rule. */
int bdg_sw2d_curved_enable_field_stats(bdg_sw2d_curved* s, const bdg_field_stats_desc* desc);
int bdg_sw2d_curved_field_stats_sample(bdg_sw2d_curved* s);
int bdg_sw2d_curved_field_stats_count(const bdg_sw2d_curved* s, int* samples, int* num_periods);
int bdg_sw2d_curved_field_stats_read(bdg_sw2d_curved* s, int which, int index, double* plane);
int bdg_sw2d_curved_field_stats_samples(const bdg_sw2d_curved* s, int first, int count, double* rows);
int bdg_sw2d_curved_field_stats_reset(bdg_sw2d_curved* s);
int bdg_sw2d_curved_field_stats_time(bdg_sw2d_curved* s, int count, float* ms);
/* Drifters through curved elements and along curved walls (csrc/hip/sw2d_curved_drifter_kernel.hpp states the algorithm).
 * Host set-up: bdg_trinodes_drifter_tables with the affine check on the elements NOT listed in curved_els alone, and the side
 * tables of the listed ones: curved_slot (K): -1, or the element's row in modal; modal (num_curved, 6, Np): the modal
 * coefficients (Vinv times the nodal values) of x, y, Dr x, Ds x, Dr y, Ds y of the provisioner's current coordinates. vertices
 * of a listed element are its corner nodes. BDG_ERR_ARGUMENT also for a curved_els entry out of range or listed twice and for a
 * listed element with a nodal Jacobian that is not positive. modal may be NULL when num_curved is 0. */
int bdg_trinodes_curved_drifter_tables(const bdg_trinodes* nodes, const int* curved_els, int num_curved, const int* mapO, int num_out,
                                       double* vertices, int* neighbours, double* vinv, double* jacobi, int* curved_slot,
                                       double* modal);
typedef struct bdg_sw2d_curved_drifter_desc {
    int count;                  /* the fields of bdg_sw2d_drifter_desc ... */
    const int* element;
    const double* r;
    const double* s;
    const double* vertices;
    const int* neighbours;
    const double* vinv;
    const double* jacobi;
    int stride;
    int capacity;
    const int* curved_slot;     /* ... and (K), (num_curved, 6, Np): bdg_trinodes_curved_drifter_tables */
    const double* modal;
    int num_curved;
} bdg_sw2d_curved_drifter_desc;
/* The calls of the bdg_sw2d_*drifters* group: advanced after every completed step of step_rk2, lserk4_stages and run_adaptive,
 * sampled again by set_state. BDG_ERR_ARGUMENT also for a curved_slot entry outside [-1, num_curved). */
int bdg_sw2d_curved_enable_drifters(bdg_sw2d_curved* s, const bdg_sw2d_curved_drifter_desc* desc);
int bdg_sw2d_curved_drifters_advance(bdg_sw2d_curved* s, double dt, int num_steps);
int bdg_sw2d_curved_drifters_time(bdg_sw2d_curved* s, double dt, int count, float* ms);
int bdg_sw2d_curved_drifters_state(bdg_sw2d_curved* s, double* x, double* y, int* element, double* r, double* sref, int* status);
int bdg_sw2d_curved_drifters_count(const bdg_sw2d_curved* s, int* num_records, int* num_drifters);
int bdg_sw2d_curved_drifters_read(bdg_sw2d_curved* s, int first, int num, double* t, double* x, double* y, int* status);
int bdg_sw2d_curved_drifters_reset(bdg_sw2d_curved* s);

/* ---------------------------------------------------------------- elliptic solver on straight-sided triangles
 * A u = sigma u - div(kappa grad u) = f in Hesthaven and Warburton's stabilised central flux form (DESIGN.md 3.12 states it; the
 * sign is opposite to an operator that returns the Laplacian), applied by two HIP passes, and conjugate gradients in the mass
 * inner product <u, v> = sum_k J_k u_k^T (V V^T)^-1 v_k with alpha, beta and the residual norm resident in device memory.
 * A face node is INTERIOR (vmapP != vmapM), DIRICHLET (a boundary node listed in mapD) or NEUMANN (any other boundary node).
 * Tables as bdg_sw2d_desc, plus Vinv (Np, Np) and J (Np, K); vmapM is required (it tells boundary nodes from interior ones).
 * kappa_elements: one value per element or NULL (then `kappa` everywhere); tau = tau_scale Np max(Fscale) / 2 max(kappa)
 * (tau_scale 0 is read as 1). flags: BDG_SW2D_REORDER / BDG_SW2D_KEEP_ORDER as for bdg_sw2d_create.
 * BDG_ERR_ARGUMENT, before a GPU is touched: a NULL argument or table, an order outside 1..8, BDG_SW2D_NODAL_GEOMETRY or tables
 * that are not those of straight-sided elements, kappa <= 0 or not finite (scalar or any entry), sigma < 0, tau_scale < 0, a
 * mapD entry that is not a boundary face node. All vectors are host (Np, K) row-major arrays in the caller's numbering. */
typedef struct bdg_poisson2d bdg_poisson2d;
typedef struct bdg_poisson2d_desc {
    int order;
    int num_elements;
    const double* Dr; const double* Ds; const double* Lift; const double* Vinv;
    const double* rx; const double* sx; const double* ry; const double* sy; const double* J; /* (Np, K) */
    const double* nx; const double* ny; const double* Fscale;                                /* (3*Nfp, K) */
    const int* vmapM; const int* vmapP;
    const int* mapD;    /* flat face-node indices (3 Nfp k + j) of the Dirichlet nodes */
    int num_dirichlet;
    double kappa;
    const double* kappa_elements;
    double sigma;
    double tau_scale;
    int device;
    int flags;
} bdg_poisson2d_desc;
typedef struct bdg_poisson2d_result {
    int iterations;
    double relative_residual; /* |r| / |b| in the mass norm, r the recursive residual, b = f - A(0; g, qn) */
    int converged;
    int projected;            /* 1: sigma = 0 and no Dirichlet node; means of b, r and the solution were removed */
} bdg_poisson2d_result;
int bdg_poisson2d_create(const bdg_poisson2d_desc* desc, bdg_poisson2d** out);
/* Every table from a nodes provisioner; mapD NULL with num_dirichlet < 0: BCmap[Wall] + BCmap[Dirichlet]. */
int bdg_poisson2d_create_from_nodes(const bdg_trinodes* nodes, const int* mapD, int num_dirichlet, double kappa,
                                    const double* kappa_elements, double sigma, double tau_scale, int device, int flags,
                                    bdg_poisson2d** out);
void bdg_poisson2d_destroy(bdg_poisson2d* s);
int bdg_poisson2d_set_shift(bdg_poisson2d* s, double sigma);
/* g, qn: (3 Nfp, K) Dirichlet values and outward normal fluxes kappa du/dn (only the entries at nodes of their kind are read);
 * either may be NULL (zero); both NULL clears the data. */
int bdg_poisson2d_set_boundary_data(bdg_poisson2d* s, const double* g, const double* qn);
/* out = A u, with_data != 0: A(u; g, qn). */
int bdg_poisson2d_apply(bdg_poisson2d* s, const double* u, double* out, int with_data);
int bdg_poisson2d_mass_dot(bdg_poisson2d* s, const double* u, const double* v, double* value);
/* Solves A(x; g, qn) = f from x_inout: the data enter b = f - A(0; g, qn) and r0 = b - A x0 once, the iteration runs with the
 * homogeneous operator; the host reads the residual norm every check_every iterations (and at max_iterations), so the
 * iteration count is a multiple of check_every unless max_iterations ends it. b = 0 returns x = 0 in zero iterations.
 * max_iterations <= 0: Np K. BDG_ERR_ARGUMENT for rel_tol <= 0 or check_every < 1; BDG_ERR_UNSTABLE for a residual norm that is
 * not finite. */
int bdg_poisson2d_solve(bdg_poisson2d* s, const double* f, double* x_inout, double rel_tol, int max_iterations, int check_every,
                        bdg_poisson2d_result* result);
/* Device milliseconds per operator application / per iteration of the loop (no host reads), averaged over count. */
int bdg_poisson2d_time_apply(bdg_poisson2d* s, int count, float* ms);
int bdg_poisson2d_time_iterations(bdg_poisson2d* s, int count, float* ms);
size_t bdg_poisson2d_device_bytes(const bdg_poisson2d* s);

/* ---- the same solver on quadrilaterals in parallelogram form: the two passes and the mass product in the
 * tensor form of the quadrilateral kernels, orders 1..12, behind the same handle -- every bdg_poisson2d_* call above serves both
 * families. The descriptor is bdg_poisson2d_desc with the tables of a QuadNodesProvisioner: Np = (N+1)^2, nx / ny / Fscale
 * (4*Nfp, K), vmapM / vmapP and mapD in the face-node numbering 4 Nfp k + j, Vinv = V1^-1 (x) V1^-1; boundary data planes are
 * (4 Nfp, K). flags: BDG_SW2D_REORDER renumbers the elements breadth-first (all I/O stays in the caller's numbering); without it,
 * and with BDG_SW2D_KEEP_ORDER, the caller's order is kept, as bdg_sw2dq_* keeps it.
 * BDG_ERR_ARGUMENT, before a GPU is touched, for what bdg_poisson2d_create refuses and for: an order outside 1..12; a mesh that is
 * not in parallelogram form (rx, sx, ry, sy, J constant per element, nx, ny, Fscale per face, to 1e-10 relative: on a general
 * bilinear quadrilateral M A is not symmetric, so conjugate gradients does not apply); Dr, Ds, Lift or Vinv that do not have the
 * tensor form of the Gauss-Lobatto element. */
int bdg_poisson2d_create_quad(const bdg_poisson2d_desc* desc, bdg_poisson2d** out);
/* Every table from a quadrilateral nodes provisioner; mapD NULL with num_dirichlet < 0: BCmap[Wall] + BCmap[Dirichlet]. */
int bdg_poisson2d_create_from_quadnodes(const bdg_quadnodes* nodes, const int* mapD, int num_dirichlet, double kappa,
                                        const double* kappa_elements, double sigma, double tau_scale, int device, int flags,
                                        bdg_poisson2d** out);

#ifdef __cplusplus
}
#endif
#endif /* BLITZDG_HIP_H */
