// poisson2d_device.hip -- the elliptic solver behind the bdg_poisson2d_* calls of include/blitzdg_hip.h: A u = sigma u -
// div(kappa grad u) on straight-sided triangles (the two passes of poisson2d_kernel.hpp, per-order objects poisson2d_order.hip)
// and conjugate gradients in the mass inner product whose scalars live in device memory.
//
// Tables are set up the way the straight sw2d solver sets up its own (sw2d_device.hip): fp64 planes of ld = K rounded up to 64
// elements per nodal row, 13 numbers of affine geometry per element, int32 gather offsets n' ld + slot(k'), elements renumbered
// internally by the same rule (element_order.hpp) with all I/O in the caller's numbering. On top of them: J_k, kappa_k, one
// byte per face node for its kind, the reference mass matrix's rows, and the weights J M 1.
//
// HBM layout (planes of Np ld doubles): x, r, s = J M r, two search directions (the fused first pass writes the new one beside
// the old), A p, w = J M A p, the two flux planes; (3 Nfp, ld) data planes g and qn once data is set.
//
// One iteration is six launches (DESIGN.md 3.12 gives the reason for each launch boundary):
//   gradient (p = r + beta p fused in)  ->  divergence  ->  mass product w = J M A p with the partials of p . w
//   ->  finish: alpha  ->  x += alpha p, r -= alpha A p, s -= alpha w with the partials of r . s  ->  finish: beta, <r, r>
// and the host reads <r, r> every check_every iterations.
//
// The same handle serves quadrilaterals in parallelogram form (bdg_poisson2d_create_quad): createQuadSolver fills
// it with the launch table of poisson2d_quad_order.hip (a PoissonKernelTable as well), 16 numbers of geometry per element, (4 Nfp,
// ld) index, kind and data planes, the tensor ops image and the 1-D mass matrix; the mass product then writes one partial per
// tile of QuadElem<N>::E elements (tileElems). The loop, its vector kernels, the finishers and the projection are shared and
// launch exactly what they launched for triangles.
#include "../host/capi_internal.hpp"
#include "../host/element_order.hpp"
#include "../host/parallel_for.hpp"
#include "device_buffer.hpp"
#include "poisson2d_launch.hpp"
#include "poisson2d_quad_launch.hpp"
#include <algorithm>
#include <atomic>
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

// (rows, K) caller-order image <-> padded, optionally renumbered device planes. perm[k_caller] = device slot (NULL = identity).
template <typename T>
__global__ void poisson2d_scatter_rows_kernel(const T* __restrict__ src, T* __restrict__ dst, int rows, int K, long long ld,
                                              const int* __restrict__ perm) {
    const long long t = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (t >= static_cast<long long>(rows) * K) return;
    const long long r = t / K, k = t % K;
    dst[r * ld + (perm ? perm[k] : k)] = src[t];
}

template <typename T>
__global__ void poisson2d_gather_rows_kernel(const T* __restrict__ src, T* __restrict__ dst, int rows, int K, long long ld,
                                             const int* __restrict__ perm) {
    const long long t = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (t >= static_cast<long long>(rows) * K) return;
    const long long r = t / K, k = t % K;
    dst[t] = src[r * ld + (perm ? perm[k] : k)];
}

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

    template <typename T>
    void uploadRowsT(const T* host, T* dev, T* staging, int rows) {
        const size_t n = static_cast<size_t>(rows) * K;
        hipCheck(hipMemcpyAsync(staging, host, n * sizeof(T), hipMemcpyHostToDevice, stream), "H2D copy");
        hipLaunchKernelGGL((bdg_dev::poisson2d_scatter_rows_kernel<T>), dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0,
                           stream, staging, dev, rows, K, ld, perm.p);
        hipCheck(hipGetLastError(), "poisson2d_scatter_rows_kernel");
        hipCheck(hipStreamSynchronize(stream), "upload sync"); // the staging buffer is reused
    }
    void uploadRows(const double* host, double* dev, int rows) { uploadRowsT<double>(host, dev, stage.p, rows); }
    void downloadRows(const double* dev, double* host, int rows) {
        const size_t n = static_cast<size_t>(rows) * K;
        hipLaunchKernelGGL((bdg_dev::poisson2d_gather_rows_kernel<double>), dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0,
                           stream, dev, stage.p, rows, K, ld, perm.p);
        hipCheck(hipGetLastError(), "poisson2d_gather_rows_kernel");
        hipCheck(hipMemcpyAsync(host, stage.p, n * sizeof(double), hipMemcpyDeviceToHost, stream), "D2H copy");
        hipCheck(hipStreamSynchronize(stream), "download sync");
    }

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

// The straight solver's test (sw2d_device.hip): metric terms constant per element, face terms constant per face, to 1e-8.
bool geometryIsAffine(const bdg_poisson2d_desc& d, int Np, int Nfp, int K) {
    const double tol = 1e-8;
    std::atomic<bool> ok{true};
    blitzdg::detail::parallelFor(K, [&](int k) {
        const double scale = std::fabs(d.rx[k]) + std::fabs(d.sx[k]) + std::fabs(d.ry[k]) + std::fabs(d.sy[k]);
        for (int n = 1; n < Np; ++n) {
            const size_t o = static_cast<size_t>(n) * K + k;
            if (std::fabs(d.rx[o] - d.rx[k]) > tol * scale || std::fabs(d.sx[o] - d.sx[k]) > tol * scale ||
                std::fabs(d.ry[o] - d.ry[k]) > tol * scale || std::fabs(d.sy[o] - d.sy[k]) > tol * scale ||
                std::fabs(d.J[o] - d.J[k]) > tol * std::fabs(d.J[k]))
                ok = false;
        }
        for (int f = 0; f < 3; ++f) {
            const size_t o0 = static_cast<size_t>(f) * Nfp * K + k;
            for (int n = 1; n < Nfp; ++n) {
                const size_t o = o0 + static_cast<size_t>(n) * K;
                if (std::fabs(d.nx[o] - d.nx[o0]) > tol || std::fabs(d.ny[o] - d.ny[o0]) > tol ||
                    std::fabs(d.Fscale[o] - d.Fscale[o0]) > tol * std::fabs(d.Fscale[o0]))
                    ok = false;
            }
        }
    });
    return ok;
}

void requireSigma(double sigma, const char* fn) {
    if (!(sigma >= 0.0) || !std::isfinite(sigma)) throw arg_error(std::string(fn) + ": sigma must be finite and >= 0");
}

bdg_poisson2d* createSolver(const bdg_poisson2d_desc& d) {
    const char* fn = "bdg_poisson2d_create";
    if (d.order < 1 || d.order > 8) throw arg_error(std::string(fn) + ": order must be 1..8");
    if (d.flags & BDG_SW2D_NODAL_GEOMETRY)
        throw arg_error(std::string(fn) + ": per-node geometry is not supported (straight-sided triangles only)");
    if (!d.kappa_elements && (!(d.kappa > 0.0) || !std::isfinite(d.kappa)))
        throw arg_error(std::string(fn) + ": kappa must be finite and > 0");
    requireSigma(d.sigma, fn);
    if (!(d.tau_scale >= 0.0) || !std::isfinite(d.tau_scale)) throw arg_error(std::string(fn) + ": tau_scale must be finite and >= 0");
    if (d.num_elements < 1) throw arg_error(std::string(fn) + ": num_elements must be >= 1");
    if (!d.Dr || !d.Ds || !d.Lift || !d.Vinv || !d.rx || !d.sx || !d.ry || !d.sy || !d.J || !d.nx || !d.ny || !d.Fscale ||
        !d.vmapM || !d.vmapP)
        throw arg_error(std::string(fn) + ": a required table pointer is NULL");
    if (d.num_dirichlet < 0 || (d.num_dirichlet > 0 && !d.mapD)) throw arg_error(std::string(fn) + ": bad Dirichlet-node list");
    const bdg_dev::PoissonKernelTable* kt = bdg_dev::poisson_kernel_table(d.order);
    if (!kt) throw arg_error(std::string(fn) + ": no kernels compiled for this order");

    const int Np = kt->Np, Nfp = kt->Nfp, NFN = 3 * Nfp, K = d.num_elements;
    const long long ld = (static_cast<long long>(K) + 63) / 64 * 64;
    // Lane addresses are a wave-uniform row pointer plus a 32-bit unsigned BYTE offset (8 * node offset).
    if (static_cast<long long>(Np) * ld * 8 > 4294967295LL)
        throw arg_error(std::string(fn) + ": Np*K exceeds 2^29 nodes (32-bit byte offsets within a plane)");
    double kappaMax = 0.0;
    if (d.kappa_elements) {
        for (int k = 0; k < K; ++k) {
            if (!(d.kappa_elements[k] > 0.0) || !std::isfinite(d.kappa_elements[k]))
                throw arg_error(std::string(fn) + ": every kappa must be finite and > 0");
            kappaMax = std::max(kappaMax, d.kappa_elements[k]);
        }
    } else {
        kappaMax = d.kappa;
    }

    // ---- the index tables, on the host
    const size_t nFaceNodes = static_cast<size_t>(NFN) * K;
    const long long totalNodes = static_cast<long long>(Np) * K;
    for (int k = 0; k < K; ++k)
        for (int f = 0; f < 3; ++f)
            for (int n = 0; n < Nfp; ++n)
                if (d.vmapM[(static_cast<size_t>(k) * 3 + f) * Nfp + n] != kt->fmask(f, n) + Np * k)
                    throw arg_error(std::string(fn) + ": vmapM does not follow the warp&blend face-node ordering (Fmask) these "
                                                      "kernels are specialised for");
    for (size_t i = 0; i < nFaceNodes; ++i)
        if (d.vmapP[i] < 0 || d.vmapP[i] >= totalNodes) throw arg_error(std::string(fn) + ": vmapP entry out of range");
    std::vector<unsigned char> kinds(nFaceNodes); // (NFN, K) rows
    for (int k = 0; k < K; ++k)
        for (int j = 0; j < NFN; ++j) {
            const size_t i = static_cast<size_t>(k) * NFN + j;
            kinds[static_cast<size_t>(j) * K + k] = d.vmapP[i] == d.vmapM[i] ? bdg_dev::PK_NEUMANN : bdg_dev::PK_INTERIOR;
        }
    for (int i = 0; i < d.num_dirichlet; ++i) {
        const int m = d.mapD[i];
        if (m < 0 || static_cast<size_t>(m) >= nFaceNodes) throw arg_error(std::string(fn) + ": Dirichlet-node index out of range");
        unsigned char& e = kinds[static_cast<size_t>(m % NFN) * K + m / NFN];
        if (e == bdg_dev::PK_INTERIOR) throw arg_error(std::string(fn) + ": a mapD entry is not a boundary face node");
        e = bdg_dev::PK_DIRICHLET;
    }
    if (!geometryIsAffine(d, Np, Nfp, K))
        throw arg_error(std::string(fn) + ": the geometry tables are not those of straight-sided elements");
    double fscaleMax = 0.0, area = 0.0;
    for (size_t i = 0; i < nFaceNodes; ++i) fscaleMax = std::max(fscaleMax, std::fabs(d.Fscale[i]));
    // reference mass matrix M = Vinv^T Vinv and its column sums (the nodal quadrature weights)
    std::vector<double> M(static_cast<size_t>(Np) * Np, 0.0), colsum(Np, 0.0);
    for (int i = 0; i < Np; ++i)
        for (int j = 0; j < Np; ++j) {
            double sum = 0.0;
            for (int m = 0; m < Np; ++m) sum += d.Vinv[m * Np + i] * d.Vinv[m * Np + j];
            M[static_cast<size_t>(i) * Np + j] = sum;
        }
    for (int i = 0; i < Np; ++i)
        for (int j = 0; j < Np; ++j) colsum[i] += M[static_cast<size_t>(j) * Np + i];
    std::vector<double> wtsHost(static_cast<size_t>(Np) * K);
    for (int i = 0; i < Np; ++i)
        for (int k = 0; k < K; ++k) wtsHost[static_cast<size_t>(i) * K + k] = colsum[i] * d.J[k];
    for (int k = 0; k < K; ++k) {
        if (!(d.J[k] > 0.0)) throw arg_error(std::string(fn) + ": J must be positive");
        double a = 0.0;
        for (int i = 0; i < Np; ++i) a += colsum[i];
        area += a * d.J[k];
    }

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        throw hip_error(std::string(fn) + ": no HIP device available (the elliptic solver has no CPU fallback)");
    if (d.device < 0 || d.device >= ndev) throw arg_error(std::string(fn) + ": device ordinal out of range");

    auto s = std::unique_ptr<bdg_poisson2d>(new bdg_poisson2d());
    s->kt = kt;
    s->N = d.order; s->Np = Np; s->Nfp = Nfp; s->NFN = NFN; s->K = K; s->ld = ld;
    s->device = d.device;
    s->sigma = d.sigma;
    s->tau = (d.tau_scale > 0.0 ? d.tau_scale : 1.0) * Np * fscaleMax / 2.0 * kappaMax;
    s->area = area;
    s->hasDirichlet = d.num_dirichlet > 0;

    namespace eo = blitzdg::element_order;
    const bool reorder = (d.flags & BDG_SW2D_REORDER) != 0 ||
                         (!(d.flags & BDG_SW2D_KEEP_ORDER) && eo::renumberingWanted(d.vmapP, K, Np, Nfp, d.order));
    if (reorder) s->permHost = eo::renumbering(d.vmapP, K, Np, Nfp, eo::patchSetting());

    s->use();
    hipCheck(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking), "hipStreamCreate");
    hipStream_t st = s->stream;
    const size_t pl = s->planeSize();
    for (DevBuf<double>* b : {&s->x, &s->r, &s->s, &s->dirA, &s->dirB, &s->Ap, &s->w, &s->wts}) b->alloc(pl, s->bytes, st);
    s->q.alloc(2 * pl, s->bytes, st);
    s->ageo.alloc(13 * static_cast<size_t>(ld), s->bytes, st);
    s->jac.alloc(static_cast<size_t>(ld), s->bytes, st);
    s->kap.alloc(static_cast<size_t>(ld), s->bytes, st);
    s->vmapP.alloc(static_cast<size_t>(NFN) * ld, s->bytes, st);
    s->kind.alloc(static_cast<size_t>(NFN) * ld, s->bytes, st);
    s->stage.alloc(static_cast<size_t>(std::max(Np, NFN)) * K, s->bytes);
    s->istage.alloc(nFaceNodes, s->bytes);
    s->bstage.alloc(nFaceNodes, s->bytes);
    s->partial.alloc(static_cast<size_t>(std::max(s->tiles(), s->reduceBlocks())), s->bytes, st);
    s->scal.alloc(bdg_dev::PS_COUNT, s->bytes, st);
    if (!s->permHost.empty()) s->perm.upload(s->permHost, s->bytes, "perm upload");

    // ---- geometry: one metric value per element, one normal / scale per face (row 0 of each table, first node of each face)
    s->uploadRows(d.rx, s->ageo.p, 1);
    s->uploadRows(d.sx, s->ageo.p + ld, 1);
    s->uploadRows(d.ry, s->ageo.p + 2 * ld, 1);
    s->uploadRows(d.sy, s->ageo.p + 3 * ld, 1);
    for (int f = 0; f < 3; ++f) {
        const size_t row = static_cast<size_t>(f) * Nfp * K;
        s->uploadRows(d.nx + row, s->ageo.p + (4 + f) * ld, 1);
        s->uploadRows(d.ny + row, s->ageo.p + (7 + f) * ld, 1);
        s->uploadRows(d.Fscale + row, s->ageo.p + (10 + f) * ld, 1);
    }
    s->uploadRows(d.J, s->jac.p, 1);
    {
        std::vector<double> kapHost(K, d.kappa);
        if (d.kappa_elements) kapHost.assign(d.kappa_elements, d.kappa_elements + K);
        s->uploadRows(kapHost.data(), s->kap.p, 1);
    }
    s->uploadRows(wtsHost.data(), s->wts.p, Np);
    s->uploadRowsT<unsigned char>(kinds.data(), s->kind.p, s->bstage.p, NFN);

    // ---- operator rows: VnOps image, row i = {Dr[i][m], Ds[i][m]} for m < Np, then Lift[i][j]
    {
        const int ROW = 2 * Np + NFN;
        std::vector<double> img(static_cast<size_t>(ROW) * Np);
        for (int i = 0; i < Np; ++i) {
            for (int m = 0; m < Np; ++m) {
                img[static_cast<size_t>(i) * ROW + 2 * m] = d.Dr[i * Np + m];
                img[static_cast<size_t>(i) * ROW + 2 * m + 1] = d.Ds[i * Np + m];
            }
            for (int j = 0; j < NFN; ++j) img[static_cast<size_t>(i) * ROW + 2 * Np + j] = d.Lift[i * NFN + j];
        }
        s->ops.upload(img, s->bytes, "ops upload");
        s->mass.upload(M, s->bytes, "mass upload");
    }

    // ---- gather offsets: reference numbering (n' + Np k') -> n' ld + slot(k'), as (NFN, K) rows
    {
        std::vector<int> rows(nFaceNodes);
        const int* perm = s->permHost.empty() ? nullptr : s->permHost.data();
        for (int k = 0; k < K; ++k)
            for (int j = 0; j < NFN; ++j) {
                const int v = d.vmapP[static_cast<size_t>(k) * NFN + j];
                const int n2 = v % Np, k2 = v / Np;
                rows[static_cast<size_t>(j) * K + k] = static_cast<int>(n2 * ld + (perm ? perm[k2] : k2));
            }
        s->uploadRowsT<int>(rows.data(), s->vmapP.p, s->istage.p, NFN);
    }
    s->istage.release();
    s->bstage.release();
    return s.release();
}

// ---- the quadrilateral family: the same handle, filled for poisson2d_quad_kernel.hpp

// D1 | l0 | lN from Dr = D1 (x) I, Ds = I (x) D1 and the face-wise lift, each held to 1e-13 max|entry| as sw2d_quad_device.hip does.
std::vector<double> quadTensorOps(const std::string& fn, int N, const double* Dr, const double* Ds, const double* Lift) {
    const int Nq = N + 1, Np = Nq * Nq, NFN = 4 * Nq;
    std::vector<double> ops(static_cast<size_t>(Nq) * Nq + 2 * Nq);
    double* D1 = ops.data();
    double* l0 = D1 + Nq * Nq;
    double* lN = l0 + Nq;
    for (int j = 0; j < Nq; ++j)
        for (int m = 0; m < Nq; ++m) D1[j * Nq + m] = Dr[static_cast<size_t>(Nq * j) * Np + Nq * m];
    for (int i = 0; i < Nq; ++i) l0[i] = Lift[static_cast<size_t>(i) * NFN];
    for (int j = 0; j < Nq; ++j) lN[j] = Lift[static_cast<size_t>(Nq * j) * NFN + Nq];
    double maxD = 0.0, maxL = 0.0, errD = 0.0, errL = 0.0;
    for (size_t i = 0; i < static_cast<size_t>(Np) * Np; ++i) maxD = std::max({maxD, std::fabs(Dr[i]), std::fabs(Ds[i])});
    for (size_t i = 0; i < static_cast<size_t>(Np) * NFN; ++i) maxL = std::max(maxL, std::fabs(Lift[i]));
    for (int j = 0; j < Nq; ++j)
        for (int i = 0; i < Nq; ++i) {
            const size_t row = static_cast<size_t>(Nq * j + i);
            for (int jj = 0; jj < Nq; ++jj)
                for (int ii = 0; ii < Nq; ++ii) {
                    const int col = Nq * jj + ii;
                    errD = std::max(errD, std::fabs(Dr[row * Np + col] - (ii == i ? D1[j * Nq + jj] : 0.0)));
                    errD = std::max(errD, std::fabs(Ds[row * Np + col] - (jj == j ? D1[i * Nq + ii] : 0.0)));
                }
            for (int q = 0; q < Nq; ++q) {
                errL = std::max(errL, std::fabs(Lift[row * NFN + q] - (q == j ? l0[i] : 0.0)));
                errL = std::max(errL, std::fabs(Lift[row * NFN + Nq + q] - (q == i ? lN[j] : 0.0)));
                errL = std::max(errL, std::fabs(Lift[row * NFN + 2 * Nq + q] - (q == j ? lN[i] : 0.0)));
                errL = std::max(errL, std::fabs(Lift[row * NFN + 3 * Nq + q] - (q == i ? l0[j] : 0.0)));
            }
        }
    if (!(maxD > 0.0) || !(maxL > 0.0) || !(errD <= 1e-13 * maxD) || !(errL <= 1e-13 * maxL))
        throw arg_error(fn + ": Dr, Ds and Lift are not the tensor operators of the Gauss-Lobatto quadrilateral (D1 (x) I, I (x) D1, "
                             "face-wise lifts); the quadrilateral kernels have no dense-operator form");
    return ops;
}

// M = Vinv^T Vinv (Np, Np) and its 1-D factor M1 (Nq, Nq) with M = M1 (x) M1, held to 1e-12 max|entry|.
void quadMassFactors(const std::string& fn, int N, const double* Vinv, std::vector<double>& M, std::vector<double>& M1) {
    const int Nq = N + 1, Np = Nq * Nq;
    M.assign(static_cast<size_t>(Np) * Np, 0.0);
    for (int m = 0; m < Np; ++m)
        for (int i = 0; i < Np; ++i) {
            const double a = Vinv[static_cast<size_t>(m) * Np + i];
            for (int j = 0; j < Np; ++j) M[static_cast<size_t>(i) * Np + j] += a * Vinv[static_cast<size_t>(m) * Np + j];
        }
    if (!(M[0] > 0.0)) throw arg_error(fn + ": Vinv does not give a positive definite mass matrix");
    const double m00 = std::sqrt(M[0]);
    M1.assign(static_cast<size_t>(Nq) * Nq, 0.0);
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
}

// Breadth-first numbering from the face-neighbour graph of a quadrilateral mesh: perm[k] = device slot.
std::vector<int> quadBfsOrder(const int* vmapP, int K, int Np, int Nq) {
    std::vector<int> perm(K, -1), frontier, nextFrontier;
    int next = 0;
    for (int seed = 0; seed < K; ++seed) {
        if (perm[seed] >= 0) continue;
        perm[seed] = next++;
        frontier.assign(1, seed);
        while (!frontier.empty()) {
            nextFrontier.clear();
            for (int k : frontier)
                for (int f = 0; f < 4; ++f) {
                    const int k2 = vmapP[(static_cast<size_t>(k) * 4 + f) * Nq] / Np;
                    if (perm[k2] < 0) {
                        perm[k2] = next++;
                        nextFrontier.push_back(k2);
                    }
                }
            frontier.swap(nextFrontier);
        }
    }
    return perm;
}

bdg_poisson2d* createQuadSolver(const bdg_poisson2d_desc& d) {
    const std::string fn = "bdg_poisson2d_create_quad";
    if (d.order < 1 || d.order > bdg_dev::kPoissonQuadMaxOrder)
        throw arg_error(fn + ": order must be 1.." + std::to_string(bdg_dev::kPoissonQuadMaxOrder));
    if (d.flags & BDG_SW2D_NODAL_GEOMETRY)
        throw arg_error(fn + ": per-node geometry is not supported (quadrilaterals in parallelogram form only)");
    if (!d.kappa_elements && (!(d.kappa > 0.0) || !std::isfinite(d.kappa))) throw arg_error(fn + ": kappa must be finite and > 0");
    requireSigma(d.sigma, fn.c_str());
    if (!(d.tau_scale >= 0.0) || !std::isfinite(d.tau_scale)) throw arg_error(fn + ": tau_scale must be finite and >= 0");
    if (d.num_elements < 1) throw arg_error(fn + ": num_elements must be >= 1");
    if (!d.Dr || !d.Ds || !d.Lift || !d.Vinv || !d.rx || !d.sx || !d.ry || !d.sy || !d.J || !d.nx || !d.ny || !d.Fscale ||
        !d.vmapM || !d.vmapP)
        throw arg_error(fn + ": a required table pointer is NULL");
    if (d.num_dirichlet < 0 || (d.num_dirichlet > 0 && !d.mapD)) throw arg_error(fn + ": bad Dirichlet-node list");
    const bdg_dev::PoissonKernelTable* kt = bdg_dev::poisson_quad_kernel_table(d.order);
    if (!kt) throw arg_error(fn + ": no kernels compiled for this order");

    const int N = d.order, Nq = N + 1, Np = kt->Np, NFN = 4 * Nq, K = d.num_elements;
    const long long ld = (static_cast<long long>(K) + 63) / 64 * 64;
    if (static_cast<long long>(Np) * ld >= (1LL << 31)) throw arg_error(fn + ": Np*K exceeds 2^31 nodes (32-bit gather offsets)");
    double kappaMax = 0.0;
    if (d.kappa_elements) {
        for (int k = 0; k < K; ++k) {
            if (!(d.kappa_elements[k] > 0.0) || !std::isfinite(d.kappa_elements[k]))
                throw arg_error(fn + ": every kappa must be finite and > 0");
            kappaMax = std::max(kappaMax, d.kappa_elements[k]);
        }
    } else {
        kappaMax = d.kappa;
    }
    const std::vector<double> opsHost = quadTensorOps(fn, N, d.Dr, d.Ds, d.Lift);
    std::vector<double> M, M1;
    quadMassFactors(fn, N, d.Vinv, M, M1);

    // ---- the index tables, on the host
    const size_t nFaceNodes = static_cast<size_t>(NFN) * K;
    const long long totalNodes = static_cast<long long>(Np) * K;
    for (int k = 0; k < K; ++k)
        for (int f = 0; f < 4; ++f)
            for (int n = 0; n < Nq; ++n)
                if (d.vmapM[(static_cast<size_t>(k) * 4 + f) * Nq + n] != kt->fmask(f, n) + Np * k)
                    throw arg_error(fn + ": vmapM is not the Gauss-Lobatto face numbering (faces s=-1, r=+1, s=+1, r=-1)");
    for (size_t i = 0; i < nFaceNodes; ++i)
        if (d.vmapP[i] < 0 || d.vmapP[i] >= totalNodes) throw arg_error(fn + ": vmapP entry out of range");
    std::vector<unsigned char> kinds(nFaceNodes); // (NFN, K) rows
    for (int k = 0; k < K; ++k)
        for (int j = 0; j < NFN; ++j) {
            const size_t i = static_cast<size_t>(k) * NFN + j;
            kinds[static_cast<size_t>(j) * K + k] = d.vmapP[i] == d.vmapM[i] ? bdg_dev::PK_NEUMANN : bdg_dev::PK_INTERIOR;
        }
    for (int i = 0; i < d.num_dirichlet; ++i) {
        const int m = d.mapD[i];
        if (m < 0 || static_cast<size_t>(m) >= nFaceNodes) throw arg_error(fn + ": Dirichlet-node index out of range");
        unsigned char& e = kinds[static_cast<size_t>(m % NFN) * K + m / NFN];
        if (e == bdg_dev::PK_INTERIOR) throw arg_error(fn + ": a mapD entry is not a boundary face node");
        e = bdg_dev::PK_DIRICHLET;
    }

    // ---- geometry: the parallelogram form of sw2d_quad_device.hip (metric terms and J constant per element, nx, ny, Fscale per
    // face, to 1e-10 relative), 16 numbers per element, and J_k
    std::vector<double> ag(static_cast<size_t>(16) * K), jacHost(K);
    {
        std::atomic<bool> para{true}, positive{true};
        const double* met[4] = {d.rx, d.sx, d.ry, d.sy};
        const double* fg[3] = {d.nx, d.ny, d.Fscale};
        blitzdg::detail::parallelFor(K, [&](int k) {
            double scale = 0.0;
            for (int a = 0; a < 4; ++a)
                for (int n = 0; n < Np; ++n) scale = std::max(scale, std::fabs(met[a][static_cast<size_t>(n) * K + k]));
            for (int a = 0; a < 5; ++a) {
                const double* tab = a < 4 ? met[a] : d.J;
                double mean = 0.0;
                for (int n = 0; n < Np; ++n) mean += tab[static_cast<size_t>(n) * K + k];
                mean /= Np;
                const double sc = a < 4 ? scale : std::fabs(mean);
                for (int n = 0; n < Np; ++n)
                    if (!(std::fabs(tab[static_cast<size_t>(n) * K + k] - mean) <= 1e-10 * sc)) para = false;
                if (a < 4) ag[static_cast<size_t>(a) * K + k] = mean;
                else jacHost[k] = mean;
            }
            if (!(jacHost[k] > 0.0)) positive = false;
            for (int c = 0; c < 3; ++c)
                for (int f = 0; f < 4; ++f) {
                    double mean = 0.0, sc = 0.0;
                    for (int n = 0; n < Nq; ++n) {
                        const double v = fg[c][static_cast<size_t>(f * Nq + n) * K + k];
                        mean += v;
                        sc = std::max(sc, std::fabs(v));
                    }
                    mean /= Nq;
                    if (c < 2) sc = 1.0;
                    for (int n = 0; n < Nq; ++n)
                        if (!(std::fabs(fg[c][static_cast<size_t>(f * Nq + n) * K + k] - mean) <= 1e-10 * sc)) para = false;
                    ag[static_cast<size_t>(4 + 4 * c + f) * K + k] = mean;
                }
        });
        if (!para)
            throw arg_error(fn + ": the mesh is not in parallelogram form (metric terms constant per element to 1e-10). On a general "
                                 "bilinear quadrilateral the variable metric does not commute with the mass matrix, M A is not "
                                 "symmetric and conjugate gradients has no licence (DESIGN.md 3.13)");
        if (!positive) throw arg_error(fn + ": J must be positive");
    }
    double fscaleMax = 0.0;
    for (size_t i = 0; i < nFaceNodes; ++i) fscaleMax = std::max(fscaleMax, std::fabs(d.Fscale[i]));
    std::vector<double> colsum(Np, 0.0);
    for (int i = 0; i < Np; ++i)
        for (int j = 0; j < Np; ++j) colsum[i] += M[static_cast<size_t>(j) * Np + i];
    std::vector<double> wtsHost(static_cast<size_t>(Np) * K);
    for (int i = 0; i < Np; ++i)
        for (int k = 0; k < K; ++k) wtsHost[static_cast<size_t>(i) * K + k] = colsum[i] * jacHost[k];
    double area = 0.0, refArea = 0.0;
    for (int i = 0; i < Np; ++i) refArea += colsum[i];
    for (int k = 0; k < K; ++k) area += refArea * jacHost[k];

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        throw hip_error(fn + ": no HIP device available (the elliptic solver has no CPU fallback)");
    if (d.device < 0 || d.device >= ndev) throw arg_error(fn + ": device ordinal out of range");

    auto s = std::unique_ptr<bdg_poisson2d>(new bdg_poisson2d());
    s->kt = kt;
    s->N = N; s->Np = Np; s->Nfp = Nq; s->NFN = NFN; s->K = K; s->ld = ld;
    s->tileElems = bdg_dev::poisson_quad_tile_elements(N);
    s->device = d.device;
    s->sigma = d.sigma;
    s->tau = (d.tau_scale > 0.0 ? d.tau_scale : 1.0) * Np * fscaleMax / 2.0 * kappaMax;
    s->area = area;
    s->hasDirichlet = d.num_dirichlet > 0;
    // Sw2dQuadSolver never renumbers: the caller's order stays unless BDG_SW2D_REORDER asks for the breadth-first one
    if ((d.flags & BDG_SW2D_REORDER) != 0 && !(d.flags & BDG_SW2D_KEEP_ORDER)) s->permHost = quadBfsOrder(d.vmapP, K, Np, Nq);

    s->use();
    hipCheck(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking), "hipStreamCreate");
    hipStream_t st = s->stream;
    const size_t pl = s->planeSize();
    for (DevBuf<double>* b : {&s->x, &s->r, &s->s, &s->dirA, &s->dirB, &s->Ap, &s->w, &s->wts}) b->alloc(pl, s->bytes, st);
    s->q.alloc(2 * pl, s->bytes, st);
    s->ageo.alloc(16 * static_cast<size_t>(ld), s->bytes, st);
    s->jac.alloc(static_cast<size_t>(ld), s->bytes, st);
    s->kap.alloc(static_cast<size_t>(ld), s->bytes, st);
    s->vmapP.alloc(static_cast<size_t>(NFN) * ld, s->bytes, st);
    s->kind.alloc(static_cast<size_t>(NFN) * ld, s->bytes, st);
    s->stage.alloc(static_cast<size_t>(std::max({Np, NFN, 16})) * K, s->bytes);
    s->istage.alloc(nFaceNodes, s->bytes);
    s->bstage.alloc(nFaceNodes, s->bytes);
    s->partial.alloc(static_cast<size_t>(std::max(s->tiles(), s->reduceBlocks())), s->bytes, st);
    s->scal.alloc(bdg_dev::PS_COUNT, s->bytes, st);
    if (!s->permHost.empty()) s->perm.upload(s->permHost, s->bytes, "perm upload");

    s->uploadRows(ag.data(), s->ageo.p, 16);
    s->uploadRows(jacHost.data(), s->jac.p, 1);
    {
        std::vector<double> kapHost(K, d.kappa);
        if (d.kappa_elements) kapHost.assign(d.kappa_elements, d.kappa_elements + K);
        s->uploadRows(kapHost.data(), s->kap.p, 1);
    }
    s->uploadRows(wtsHost.data(), s->wts.p, Np);
    s->uploadRowsT<unsigned char>(kinds.data(), s->kind.p, s->bstage.p, NFN);
    s->ops.upload(opsHost, s->bytes, "ops upload");
    s->mass.upload(M1, s->bytes, "mass upload");

    // ---- gather offsets: reference numbering (n' + Np k') -> n' ld + slot(k'), as (NFN, K) rows; a boundary node gathers itself
    {
        std::vector<int> rows(nFaceNodes);
        const int* perm = s->permHost.empty() ? nullptr : s->permHost.data();
        for (int k = 0; k < K; ++k)
            for (int j = 0; j < NFN; ++j) {
                const int v = d.vmapP[static_cast<size_t>(k) * NFN + j];
                const int n2 = v % Np, k2 = v / Np;
                rows[static_cast<size_t>(j) * K + k] = static_cast<int>(n2 * ld + (perm ? perm[k2] : k2));
            }
        s->uploadRowsT<int>(rows.data(), s->vmapP.p, s->istage.p, NFN);
    }
    s->istage.release();
    s->bstage.release();
    return s.release();
}

void requireSolver(const bdg_poisson2d* s, const char* fn) {
    if (!s) throw arg_error(std::string(fn) + ": solver handle is NULL");
}

} // namespace

extern "C" {

int bdg_poisson2d_create(const bdg_poisson2d_desc* desc, bdg_poisson2d** out) {
    return guard([&] {
        if (!desc || !out) throw arg_error("bdg_poisson2d_create: NULL argument");
        *out = createSolver(*desc);
    });
}

int bdg_poisson2d_create_from_nodes(const bdg_trinodes* nodes, const int* mapD, int num_dirichlet, double kappa,
                                    const double* kappa_elements, double sigma, double tau_scale, int device, int flags,
                                    bdg_poisson2d** out) {
    return guard([&] {
        if (!nodes || !out) throw arg_error("bdg_poisson2d_create_from_nodes: NULL argument");
        const blitzdg::TriangleNodesProvisioner& p = nodes->prov;
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
        *out = createSolver(d);
    });
}

int bdg_poisson2d_create_quad(const bdg_poisson2d_desc* desc, bdg_poisson2d** out) {
    return guard([&] {
        if (!desc || !out) throw arg_error("bdg_poisson2d_create_quad: NULL argument");
        *out = createQuadSolver(*desc);
    });
}

int bdg_poisson2d_create_from_quadnodes(const bdg_quadnodes* nodes, const int* mapD, int num_dirichlet, double kappa,
                                        const double* kappa_elements, double sigma, double tau_scale, int device, int flags,
                                        bdg_poisson2d** out) {
    return guard([&] {
        if (!nodes || !out) throw arg_error("bdg_poisson2d_create_from_quadnodes: NULL argument");
        const blitzdg::QuadNodesProvisioner& p = nodes->prov;
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
        *out = createQuadSolver(d);
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
