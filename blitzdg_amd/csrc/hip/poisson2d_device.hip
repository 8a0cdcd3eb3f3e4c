// poisson2d_device.hip -- the elliptic solver behind the bdg_poisson2d_* calls of include/blitzdg_hip.h: A u = sigma u -
// div(kappa grad u) on straight-sided triangles (the two passes of poisson2d_kernel.hpp, per-order objects poisson2d_order.hip)
// and conjugate gradients in the mass inner product whose scalars live in device memory.
//
// Tables are laid out the way the straight sw2d solver lays out its own (sw2d_device.hip): fp64 planes of ld = K rounded up to 64
// elements per nodal row, 13 numbers of affine geometry per element, int32 gather offsets n' ld + slot(k'), elements renumbered
// internally by the same rule (element_order.hpp) with all I/O in the caller's numbering. On top of them: J_k, kappa_k, one
// byte per face node for its kind, the reference mass matrix's rows, and the weights J M 1. The host builds all of them for both
// element families in host/poisson_tables.cpp (its element-table checks are host/element_tables.cpp, shared with the sw2d solvers);
// createFrom() here allocates and uploads them, through the row transposes of row_transfer.hpp.
//
// HBM layout (planes of Np ld doubles): x, r, s = J M r, two search directions (the fused first pass writes the new one beside
// the old), A p, w = J M A p, the two flux planes; (3 Nfp, ld) data planes g and qn once data is set.
//
// One iteration is six launches (DESIGN.md 3.12 gives the reason for each launch boundary):
//   gradient (p = r + beta p fused in)  ->  divergence  ->  mass product w = J M A p with the partials of p . w
//   ->  finish: alpha  ->  x += alpha p, r -= alpha A p, s -= alpha w with the partials of r . s  ->  finish: beta, <r, r>
// and the host reads <r, r> every check_every iterations.
//
// The same handle serves quadrilaterals in parallelogram form (bdg_poisson2d_create_quad): it then holds
// the launch table of poisson2d_quad_order.hip (a PoissonKernelTable as well), 16 numbers of geometry per element, (4 Nfp,
// ld) index, kind and data planes, the tensor ops image and the 1-D mass matrix; the mass product then writes one partial per
// tile of QuadElem<N>::E elements (tileElems). The loop, its vector kernels, the finishers and the projection are shared and
// launch exactly what they launched for triangles.
#include "../host/capi_internal.hpp"
#include "../host/poisson_tables.hpp"
#include "poisson2d_launch.hpp"
#include "poisson2d_quad_launch.hpp"
#include "row_transfer.hpp"
#include <algorithm>
#include <cmath>
#include <memory>
#include <string>
#include <vector>

namespace bdg_dev {

const PoissonKernelTable* poisson_kernel_table_order1();
const PoissonKernelTable* poisson_kernel_table_order2();
const PoissonKernelTable* poisson_kernel_table_order3();
const PoissonKernelTable* poisson_kernel_table_order4();
const PoissonKernelTable* poisson_kernel_table_order5();
const PoissonKernelTable* poisson_kernel_table_order6();
const PoissonKernelTable* poisson_kernel_table_order7();
const PoissonKernelTable* poisson_kernel_table_order8();

const PoissonKernelTable* poisson_kernel_table(int order) {
    switch (order) {
    case 1: return poisson_kernel_table_order1();
    case 2: return poisson_kernel_table_order2();
    case 3: return poisson_kernel_table_order3();
    case 4: return poisson_kernel_table_order4();
    case 5: return poisson_kernel_table_order5();
    case 6: return poisson_kernel_table_order6();
    case 7: return poisson_kernel_table_order7();
    case 8: return poisson_kernel_table_order8();
    default: return nullptr;
    }
}

#define BDG_PQ_DECL(n) \
    const PoissonKernelTable* poisson_quad_kernel_table_order##n(); \
    int poisson_quad_tile_elements_order##n();
BDG_PQ_DECL(1) BDG_PQ_DECL(2) BDG_PQ_DECL(3) BDG_PQ_DECL(4) BDG_PQ_DECL(5) BDG_PQ_DECL(6)
BDG_PQ_DECL(7) BDG_PQ_DECL(8) BDG_PQ_DECL(9) BDG_PQ_DECL(10) BDG_PQ_DECL(11) BDG_PQ_DECL(12)
#undef BDG_PQ_DECL

#define BDG_PQ_CASES(fn) \
    case 1: return fn##1(); case 2: return fn##2(); case 3: return fn##3(); case 4: return fn##4(); \
    case 5: return fn##5(); case 6: return fn##6(); case 7: return fn##7(); case 8: return fn##8(); \
    case 9: return fn##9(); case 10: return fn##10(); case 11: return fn##11(); case 12: return fn##12();

const PoissonKernelTable* poisson_quad_kernel_table(int order) {
    switch (order) {
    BDG_PQ_CASES(poisson_quad_kernel_table_order)
    default: return nullptr;
    }
}

int poisson_quad_tile_elements(int order) {
    switch (order) {
    BDG_PQ_CASES(poisson_quad_tile_elements_order)
    default: return 0;
    }
}
#undef BDG_PQ_CASES

// a reproducible nonzero right-hand side for bdg_poisson2d_time_iterations: values in (0.5, 1.5) at the nodes of real elements
__global__ void poisson2d_fill_kernel(double* __restrict__ u, long long n, long long ld, int K) {
    const long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned h = static_cast<unsigned>(i) * 2654435761u;
    u[i] = (i % ld < K) ? 0.5 + static_cast<double>(h >> 8) / 16777216.0 : 0.0;
}

} // namespace bdg_dev

using bdg_detail::arg_error;
using bdg_detail::guard;
using bdg_detail::hip_error;
using bdg_detail::unstable_error;
using bdg_dev::DevBuf;
using bdg_dev::hipCheck;

namespace {
constexpr int kBlock = 256;   // threads of a flat vector kernel
constexpr int kItems = 4;     // entries per thread of the reducing ones
} // namespace

struct bdg_poisson2d {
    const bdg_dev::PoissonKernelTable* kt = nullptr;
    int N = 0, Np = 0, Nfp = 0, NFN = 0, K = 0, device = 0;
    int tileElems = 64;                 // elements per partial of the mass product: a wave of triangles, a tile of quadrilaterals
    long long ld = 0;
    double sigma = 0.0, tau = 0.0, area = 0.0;
    bool hasDirichlet = false, hasData = false;
    hipStream_t stream = nullptr;
    size_t bytes = 0;
    DevBuf<double> ageo, jac, kap, ops, mass, wts, q, x, r, s, dirA, dirB, Ap, w, gData, qnData, partial, scal, stage;
    DevBuf<int> vmapP, perm, istage;
    DevBuf<unsigned char> kind, bstage;
    std::vector<int> permHost;          // caller element -> device slot (empty = identity)
    unsigned long long launches = 0;    // whole-mesh operator launches so far: their tile sweep alternates (sw2d_stage_tile.hpp)

    ~bdg_poisson2d() {
        if (stream) (void)hipStreamDestroy(stream);
    }
    void use() const { hipCheck(hipSetDevice(device), "hipSetDevice"); }
    size_t planeSize() const { return static_cast<size_t>(Np) * static_cast<size_t>(ld); }
    long long planeEntries() const { return static_cast<long long>(Np) * ld; }
    bool singular() const { return sigma == 0.0 && !hasDirichlet; }
    int tiles() const { return (K + tileElems - 1) / tileElems; }
    int flatBlocks() const { return static_cast<int>((planeEntries() + kBlock - 1) / kBlock); }
    int reduceBlocks() const { return static_cast<int>((planeEntries() + kBlock * kItems - 1) / (kBlock * kItems)); }

    // host (rows, K) caller order <-> device planes (padded / renumbered): row_transfer.hpp
    bdg_dev::RowLayout rowLayout() const { return {K, ld, perm.p, stream}; }
    void uploadRows(const double* host, double* dev, int rows) { bdg_dev::uploadRows(rowLayout(), host, dev, stage.p, rows); }
    void downloadRows(const double* dev, double* host, int rows) { bdg_dev::downloadRows(rowLayout(), dev, host, stage.p, rows); }

    bdg_dev::PoissonParams params(const double* u, double* out) {
        bdg_dev::PoissonParams p{};
        p.u = u;
        p.scal = scal.p;
        p.q = q.p;
        p.out = out;
        p.ageo = ageo.p;
        p.vmapP = vmapP.p;
        p.kind = kind.p;
        p.kap = kap.p;
        p.g = gData.p;
        p.qn = qnData.p;
        p.sigma = sigma;
        p.tau = tau;
        p.ld = ld;
        p.kbegin = 0;
        p.kend = K;
        return p;
    }
    int nextSweep() { return static_cast<int>(launches++ & 1ull); }

    // out = A u (A(u; g, qn) with data); u and out are device planes
    void applyPlanes(const double* u, double* out, bool data) {
        bdg_dev::PoissonParams p = params(u, out);
        p.sweepBack = nextSweep();
        hipCheck(kt->gradient(data, false, p, ops.p, stream), "poisson2d_gradient_kernel");
        p.sweepBack = nextSweep();
        hipCheck(kt->divergence(data, p, u, ops.p, stream), "poisson2d_divergence_kernel");
    }
    void finish(int count, int what) {
        hipLaunchKernelGGL((bdg_dev::poisson2d_finish_kernel<kBlock>), dim3(1), dim3(kBlock), 0, stream, partial.p, count, what, area,
                           scal.p);
        hipCheck(hipGetLastError(), "poisson2d_finish_kernel");
    }
    // wdst = J M v (where given) and scal <- u . (J M v) the way `what` says
    void massDot(const double* u, const double* v, double* wdst, int what) {
        hipCheck(kt->mass(u, v, wdst, mass.p, jac.p, partial.p, ld, 0, K, stream), "poisson2d_mass_kernel");
        finish(tiles(), what);
    }
    void axpy(double* y, double a, const double* xv) {
        hipLaunchKernelGGL((bdg_dev::poisson2d_axpy_kernel<kBlock>), dim3(flatBlocks()), dim3(kBlock), 0, stream, y, a, xv,
                           planeEntries());
        hipCheck(hipGetLastError(), "poisson2d_axpy_kernel");
    }
    // u -= its mass-weighted mean; sv (may be nullptr) = J M u follows
    void removeMean(double* u, double* sv) {
        hipLaunchKernelGGL((bdg_dev::poisson2d_weighted_sum_kernel<kBlock, kItems>), dim3(reduceBlocks()), dim3(kBlock), 0, stream,
                           wts.p, u, partial.p, planeEntries());
        hipCheck(hipGetLastError(), "poisson2d_weighted_sum_kernel");
        finish(reduceBlocks(), bdg_dev::PF_MEAN);
        hipLaunchKernelGGL((bdg_dev::poisson2d_shift_kernel<kBlock>), dim3(flatBlocks()), dim3(kBlock), 0, stream, u, sv, wts.p, scal.p,
                           planeEntries(), ld, K);
        hipCheck(hipGetLastError(), "poisson2d_shift_kernel");
    }
    double readScalar(int which) {
        double v = 0.0;
        hipCheck(hipMemcpyAsync(&v, scal.p + which, sizeof(double), hipMemcpyDeviceToHost, stream), "D2H copy");
        hipCheck(hipStreamSynchronize(stream), "scalar sync");
        return v;
    }
    // one iteration of the loop: dirCur holds the previous direction on entry, the new one on return
    double* dirCur = nullptr;
    double* dirAlt = nullptr;
    void iterate() {
        bdg_dev::PoissonParams p = params(r.p, Ap.p);
        p.pold = dirCur;
        p.pnew = dirAlt;
        p.sweepBack = nextSweep();
        hipCheck(kt->gradient(false, true, p, ops.p, stream), "poisson2d_gradient_kernel");
        std::swap(dirCur, dirAlt);
        p.sweepBack = nextSweep();
        hipCheck(kt->divergence(false, p, dirCur, ops.p, stream), "poisson2d_divergence_kernel");
        massDot(dirCur, Ap.p, w.p, bdg_dev::PF_ALPHA);
        hipLaunchKernelGGL((bdg_dev::poisson2d_cg_update_kernel<kBlock, kItems>), dim3(reduceBlocks()), dim3(kBlock), 0, stream, x.p,
                           r.p, s.p, dirCur, Ap.p, w.p, scal.p, partial.p, planeEntries());
        hipCheck(hipGetLastError(), "poisson2d_cg_update_kernel");
        finish(reduceBlocks(), bdg_dev::PF_BETA);
    }
    void startLoop() {
        dirCur = dirA.p;
        dirAlt = dirB.p;
        dirA.zero(stream);
        dirB.zero(stream);
    }
};

namespace {

namespace pt = blitzdg::poisson_tables;
using pt::requireSigma;
static_assert(int(pt::kInterior) == bdg_dev::PK_INTERIOR && int(pt::kDirichlet) == bdg_dev::PK_DIRICHLET &&
                  int(pt::kNeumann) == bdg_dev::PK_NEUMANN, "poisson_tables.hpp writes the kind bytes the kernels read");
static_assert(pt::kMaxOrder[pt::kQuadrilaterals] == bdg_dev::kPoissonQuadMaxOrder, "poisson_tables.hpp admits the compiled orders");

// The handle of host tables `t`: allocations and uploads. tileElems: elements per partial of the family's mass product.
bdg_poisson2d* createFrom(const pt::Tables& t, const bdg_dev::PoissonKernelTable* kt, int tileElems, double sigma, int device) {
    auto s = std::unique_ptr<bdg_poisson2d>(new bdg_poisson2d());
    s->kt = kt;
    s->N = t.N; s->Np = t.Np; s->Nfp = t.Nfp; s->NFN = t.NFN; s->K = t.K; s->ld = t.ld;
    s->tileElems = tileElems;
    s->device = device;
    s->sigma = sigma;
    s->tau = t.tau;
    s->area = t.area;
    s->hasDirichlet = t.hasDirichlet;
    s->permHost = t.perm;

    s->use();
    hipCheck(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking), "hipStreamCreate");
    hipStream_t st = s->stream;
    const size_t pl = s->planeSize(), ld = static_cast<size_t>(t.ld), nFaceNodes = static_cast<size_t>(t.NFN) * t.K;
    for (DevBuf<double>* b : {&s->x, &s->r, &s->s, &s->dirA, &s->dirB, &s->Ap, &s->w, &s->wts}) b->alloc(pl, s->bytes, st);
    s->q.alloc(2 * pl, s->bytes, st);
    s->ageo.alloc(t.geoRows * ld, s->bytes, st);
    s->jac.alloc(ld, s->bytes, st);
    s->kap.alloc(ld, s->bytes, st);
    s->vmapP.alloc(t.NFN * ld, s->bytes, st);
    s->kind.alloc(t.NFN * ld, s->bytes, st);
    s->stage.alloc(static_cast<size_t>(std::max(t.Np, t.NFN)) * t.K, s->bytes);
    s->istage.alloc(nFaceNodes, s->bytes);
    s->bstage.alloc(nFaceNodes, s->bytes);
    s->partial.alloc(static_cast<size_t>(std::max(s->tiles(), s->reduceBlocks())), s->bytes, st);
    s->scal.alloc(bdg_dev::PS_COUNT, s->bytes, st);
    if (!s->permHost.empty()) s->perm.upload(s->permHost, s->bytes, "perm upload");

    for (int r = 0; r < t.geoRows; ++r) s->uploadRows(t.geo[r], s->ageo.p + r * ld, 1);
    s->uploadRows(t.jac, s->jac.p, 1);
    s->uploadRows(t.kap.data(), s->kap.p, 1);
    s->uploadRows(t.wts.data(), s->wts.p, t.Np);
    s->ops.upload(t.ops, s->bytes, "ops upload");
    s->mass.upload(t.mass, s->bytes, "mass upload");
    bdg_dev::uploadRows(s->rowLayout(), t.kinds.data(), s->kind.p, s->bstage.p, t.NFN);
    bdg_dev::uploadRows(s->rowLayout(), t.offP.data(), s->vmapP.p, s->istage.p, t.NFN);
    s->istage.release();
    s->bstage.release();
    return s.release();
}

// Host tables, then the device: every refusal that needs no device comes first.
bdg_poisson2d* create(const bdg_poisson2d_desc& d, pt::Family family) {
    const bool quad = family == pt::kQuadrilaterals;
    const bdg_dev::PoissonKernelTable* kt = quad ? bdg_dev::poisson_quad_kernel_table(d.order) : bdg_dev::poisson_kernel_table(d.order);
    std::vector<int> fmask;
    if (kt)
        for (int f = 0; f < (quad ? 4 : 3); ++f)
            for (int n = 0; n < kt->Nfp; ++n) fmask.push_back(kt->fmask(f, n));
    const pt::Tables t = pt::build(d, family, fmask);

    const std::string fn = quad ? "bdg_poisson2d_create_quad" : "bdg_poisson2d_create";
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        throw hip_error(fn + ": no HIP device available (the elliptic solver has no CPU fallback)");
    if (d.device < 0 || d.device >= ndev) throw arg_error(fn + ": device ordinal out of range");
    return createFrom(t, kt, quad ? bdg_dev::poisson_quad_tile_elements(d.order) : 64, d.sigma, d.device);
}

// The descriptor of a provisioner's tables (TriangleNodesProvisioner or QuadNodesProvisioner), and the solver from it. Without a
// mapD and with num_dirichlet < 0 the Dirichlet nodes are the provisioner's wall and Dirichlet nodes.
template <class Provisioner>
bdg_poisson2d* createFromProvisioner(const Provisioner& p, pt::Family family, const int* mapD, int num_dirichlet, double kappa,
                                     const double* kappa_elements, double sigma, double tau_scale, int device, int flags) {
    bdg_poisson2d_desc d{};
    d.order = p.get_NOrder();
    d.num_elements = p.get_NumElements();
    d.Dr = p.get_Dr().data(); d.Ds = p.get_Ds().data(); d.Lift = p.get_Lift().data(); d.Vinv = p.get_Vinv().data();
    d.rx = p.get_rx().data(); d.sx = p.get_sx().data(); d.ry = p.get_ry().data(); d.sy = p.get_sy().data();
    d.J = p.get_J().data();
    d.nx = p.get_nx().data(); d.ny = p.get_ny().data(); d.Fscale = p.get_Fscale().data();
    d.vmapM = p.get_vmapM().data(); d.vmapP = p.get_vmapP().data();
    std::vector<int> walls;
    if (!mapD && num_dirichlet < 0) {
        const auto& bc = p.get_bcMap();
        for (int tag : {static_cast<int>(blitzdg::BCTag::Wall), static_cast<int>(blitzdg::BCTag::Dirichlet)}) {
            const auto it = bc.find(tag);
            if (it != bc.end()) walls.insert(walls.end(), it->second.begin(), it->second.end());
        }
        d.mapD = walls.data();
        d.num_dirichlet = static_cast<int>(walls.size());
    } else {
        d.mapD = mapD;
        d.num_dirichlet = num_dirichlet;
    }
    d.kappa = kappa; d.kappa_elements = kappa_elements; d.sigma = sigma; d.tau_scale = tau_scale;
    d.device = device; d.flags = flags;
    return create(d, family);
}

void requireSolver(const bdg_poisson2d* s, const char* fn) {
    if (!s) throw arg_error(std::string(fn) + ": solver handle is NULL");
}

} // namespace

extern "C" {

int bdg_poisson2d_create(const bdg_poisson2d_desc* desc, bdg_poisson2d** out) {
    return guard([&] {
        if (!desc || !out) throw arg_error("bdg_poisson2d_create: NULL argument");
        *out = create(*desc, pt::kTriangles);
    });
}

int bdg_poisson2d_create_from_nodes(const bdg_trinodes* nodes, const int* mapD, int num_dirichlet, double kappa,
                                    const double* kappa_elements, double sigma, double tau_scale, int device, int flags,
                                    bdg_poisson2d** out) {
    return guard([&] {
        if (!nodes || !out) throw arg_error("bdg_poisson2d_create_from_nodes: NULL argument");
        *out = createFromProvisioner(nodes->prov, pt::kTriangles, mapD, num_dirichlet, kappa, kappa_elements, sigma, tau_scale, device,
                                     flags);
    });
}

int bdg_poisson2d_create_quad(const bdg_poisson2d_desc* desc, bdg_poisson2d** out) {
    return guard([&] {
        if (!desc || !out) throw arg_error("bdg_poisson2d_create_quad: NULL argument");
        *out = create(*desc, pt::kQuadrilaterals);
    });
}

int bdg_poisson2d_create_from_quadnodes(const bdg_quadnodes* nodes, const int* mapD, int num_dirichlet, double kappa,
                                        const double* kappa_elements, double sigma, double tau_scale, int device, int flags,
                                        bdg_poisson2d** out) {
    return guard([&] {
        if (!nodes || !out) throw arg_error("bdg_poisson2d_create_from_quadnodes: NULL argument");
        *out = createFromProvisioner(nodes->prov, pt::kQuadrilaterals, mapD, num_dirichlet, kappa, kappa_elements, sigma, tau_scale,
                                     device, flags);
    });
}

void bdg_poisson2d_destroy(bdg_poisson2d* s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    delete s;
}

int bdg_poisson2d_set_shift(bdg_poisson2d* s, double sigma) {
    return guard([&] {
        requireSolver(s, "bdg_poisson2d_set_shift");
        requireSigma(sigma, "bdg_poisson2d_set_shift");
        s->sigma = sigma;
    });
}

int bdg_poisson2d_set_boundary_data(bdg_poisson2d* s, const double* g, const double* qn) {
    return guard([&] {
        requireSolver(s, "bdg_poisson2d_set_boundary_data");
        s->use();
        if (!g && !qn) {
            s->hasData = false;
            return;
        }
        const size_t fplane = static_cast<size_t>(s->NFN) * s->ld;
        if (!s->gData.p) s->gData.alloc(fplane, s->bytes);
        if (!s->qnData.p) s->qnData.alloc(fplane, s->bytes);
        s->gData.zero(s->stream);
        s->qnData.zero(s->stream);
        if (g) s->uploadRows(g, s->gData.p, s->NFN);
        if (qn) s->uploadRows(qn, s->qnData.p, s->NFN);
        hipCheck(hipStreamSynchronize(s->stream), "boundary data sync");
        s->hasData = true;
    });
}

int bdg_poisson2d_apply(bdg_poisson2d* s, const double* u, double* out, int with_data) {
    return guard([&] {
        requireSolver(s, "bdg_poisson2d_apply");
        if (!u || !out) throw arg_error("bdg_poisson2d_apply: NULL field");
        s->use();
        s->uploadRows(u, s->dirA.p, s->Np);
        s->applyPlanes(s->dirA.p, s->Ap.p, with_data != 0 && s->hasData);
        s->downloadRows(s->Ap.p, out, s->Np);
    });
}

int bdg_poisson2d_mass_dot(bdg_poisson2d* s, const double* u, const double* v, double* value) {
    return guard([&] {
        requireSolver(s, "bdg_poisson2d_mass_dot");
        if (!u || !v || !value) throw arg_error("bdg_poisson2d_mass_dot: NULL argument");
        s->use();
        s->uploadRows(u, s->dirA.p, s->Np);
        s->uploadRows(v, s->dirB.p, s->Np);
        s->massDot(s->dirA.p, s->dirB.p, nullptr, bdg_dev::PF_SUM);
        *value = s->readScalar(bdg_dev::PS_SUM);
    });
}

int bdg_poisson2d_solve(bdg_poisson2d* s, const double* f, double* x_inout, double rel_tol, int max_iterations, int check_every,
                        bdg_poisson2d_result* result) {
    return guard([&] {
        const char* fn = "bdg_poisson2d_solve";
        requireSolver(s, fn);
        if (!f || !x_inout || !result) throw arg_error(std::string(fn) + ": NULL argument");
        if (!(rel_tol > 0.0)) throw arg_error(std::string(fn) + ": rel_tol must be > 0");
        if (check_every < 1) throw arg_error(std::string(fn) + ": check_every must be >= 1");
        const long long cap = static_cast<long long>(s->Np) * s->K;
        const int maxIt = max_iterations > 0 ? max_iterations : static_cast<int>(std::min<long long>(cap, 2147483647LL));
        s->use();
        const bool singular = s->singular();
        *result = bdg_poisson2d_result{0, 0.0, 1, singular ? 1 : 0};
        const size_t total = static_cast<size_t>(s->Np) * s->K;

        // ---- b = f - A(0; g, qn), its mean removed in the singular case; s = J M b, <b, b>
        s->uploadRows(f, s->r.p, s->Np);
        if (s->hasData) {
            s->dirA.zero(s->stream);
            s->applyPlanes(s->dirA.p, s->Ap.p, true);
            s->axpy(s->r.p, -1.0, s->Ap.p);
        }
        if (singular) s->removeMean(s->r.p, nullptr);
        s->massDot(s->r.p, s->r.p, s->s.p, bdg_dev::PF_START);
        const double bb = s->readScalar(bdg_dev::PS_RR);
        if (!std::isfinite(bb)) throw unstable_error(std::string(fn) + ": the right-hand side is not finite");
        if (bb == 0.0) {
            std::fill(x_inout, x_inout + total, 0.0);
            return;
        }
        // ---- r0 = b - A x0 (x0 = 0: r0 = b)
        bool startsAtZero = true;
        for (size_t i = 0; i < total && startsAtZero; ++i) startsAtZero = x_inout[i] == 0.0;
        if (startsAtZero) {
            s->x.zero(s->stream);
        } else {
            s->uploadRows(x_inout, s->x.p, s->Np);
            s->applyPlanes(s->x.p, s->Ap.p, false);
            s->axpy(s->r.p, -1.0, s->Ap.p);
            if (singular) s->removeMean(s->r.p, nullptr);
            s->massDot(s->r.p, s->r.p, s->s.p, bdg_dev::PF_START);
        }
        s->startLoop();
        double rr = startsAtZero ? bb : s->readScalar(bdg_dev::PS_RR);
        int it = 0;
        bool converged = std::sqrt(std::max(rr, 0.0) / bb) <= rel_tol;
        while (!converged && it < maxIt) {
            s->iterate();
            ++it;
            if (it % check_every == 0 || it == maxIt) {
                if (singular) {
                    s->removeMean(s->r.p, nullptr);
                    s->massDot(s->r.p, s->r.p, s->s.p, bdg_dev::PF_REBETA);
                }
                rr = s->readScalar(bdg_dev::PS_RR);
                if (!std::isfinite(rr)) throw unstable_error(std::string(fn) + ": the residual norm is not finite");
                converged = std::sqrt(std::max(rr, 0.0) / bb) <= rel_tol;
            }
        }
        if (singular) s->removeMean(s->x.p, nullptr);
        s->downloadRows(s->x.p, x_inout, s->Np);
        result->iterations = it;
        result->relative_residual = std::sqrt(std::max(rr, 0.0) / bb);
        result->converged = converged ? 1 : 0;
    });
}

int bdg_poisson2d_time_apply(bdg_poisson2d* s, int count, float* ms) {
    return guard([&] {
        requireSolver(s, "bdg_poisson2d_time_apply");
        if (count < 1 || !ms) throw arg_error("bdg_poisson2d_time_apply: count < 1 or NULL result");
        s->use();
        hipLaunchKernelGGL(bdg_dev::poisson2d_fill_kernel, dim3(s->flatBlocks()), dim3(kBlock), 0, s->stream, s->dirA.p,
                           s->planeEntries(), s->ld, s->K);
        hipCheck(hipGetLastError(), "poisson2d_fill_kernel");
        s->applyPlanes(s->dirA.p, s->Ap.p, false); // warm-up
        *ms = bdg_dev::timePerRun(s->stream, count, [&] { s->applyPlanes(s->dirA.p, s->Ap.p, false); });
    });
}

int bdg_poisson2d_time_iterations(bdg_poisson2d* s, int count, float* ms) {
    return guard([&] {
        requireSolver(s, "bdg_poisson2d_time_iterations");
        if (count < 1 || !ms) throw arg_error("bdg_poisson2d_time_iterations: count < 1 or NULL result");
        s->use();
        hipLaunchKernelGGL(bdg_dev::poisson2d_fill_kernel, dim3(s->flatBlocks()), dim3(kBlock), 0, s->stream, s->r.p,
                           s->planeEntries(), s->ld, s->K);
        hipCheck(hipGetLastError(), "poisson2d_fill_kernel");
        s->x.zero(s->stream);
        s->massDot(s->r.p, s->r.p, s->s.p, bdg_dev::PF_START);
        s->startLoop();
        s->iterate(); // warm-up
        *ms = bdg_dev::timePerRun(s->stream, count, [&] { s->iterate(); });
    });
}

size_t bdg_poisson2d_device_bytes(const bdg_poisson2d* s) { return s ? s->bytes : 0; }

} // extern "C"
