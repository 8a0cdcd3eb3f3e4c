// Host tables of the curved / over-integrated sw2d solver (curved_tables.hpp). Layouts: sw2d_curved_kernel.hpp
// (CurvedOps), sw2d_curved_nt_kernel.hpp (CurvedOpsNT). Reference: swhelpers/rhs.py:6-176.
#include "curved_tables.hpp"
#include "capi_internal.hpp"
#include "parallel_for.hpp"
#include <algorithm>
#include <atomic>
#include <cmath>

namespace blitzdg {
namespace curved_tables {
namespace {

using bdg_detail::arg_error;
using Desc = bdg_sw2d_curved_desc;

size_t at2(int row, int K, int k) { return static_cast<size_t>(row) * K + k; }

std::vector<double> matmul(const double* A, const double* B, int n, int m, int c) { // (n,m) (m,c)
    std::vector<double> C(static_cast<size_t>(n) * c, 0.0);
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < m; ++k) {
            const double a = A[static_cast<size_t>(i) * m + k];
            for (int j = 0; j < c; ++j) C[static_cast<size_t>(i) * c + j] += a * B[static_cast<size_t>(k) * c + j];
        }
    return C;
}

// ---- validation and index maps
void buildMaps(const Desc& d, Tables& t) {
    const int Np = t.Np, K = t.K, NG = t.ng, NG3 = 3 * NG, fb = t.fb, CR = 16 * t.ncb, GR = 48 * fb;
    const long long ld = t.ld, nG = static_cast<long long>(NG3) * K;
    // lane addresses are a row pointer plus an unsigned 32-bit BYTE offset within one plane (the state, trace and coefficient
    // arrays are reached through ONE descriptor each: 4 state / trace planes, up to 5 coefficient planes)
    if (static_cast<long long>(std::max({5 * Np, CR, 4 * GR})) * ld * 8 > 4294967295LL)
        throw arg_error("bdg_sw2d_curved_create: a table exceeds 4 GiB (32-bit byte offsets): partition the mesh");
    for (long long i = 0; i < nG; ++i) {
        if (d.gmapP[i] < 0 || d.gmapP[i] >= nG || d.gmapM[i] < 0 || d.gmapM[i] >= nG)
            throw arg_error("bdg_sw2d_curved_create: gmapM / gmapP entry out of range");
        t.identityM = t.identityM && d.gmapM[i] == i;
    }
    auto devOffset = [&](int v) { // flat id g + 3NG k -> padded row * ld + k
        const int k2 = v / NG3, g2 = v % NG3, f2 = g2 / NG, l2 = g2 % NG;
        return static_cast<int>((16ll * fb * f2 + l2) * ld + k2);
    };
    t.offP.assign(static_cast<size_t>(GR) * K, 0);
    if (!t.identityM) t.offM.assign(static_cast<size_t>(GR) * K, 0);
    t.maxNeighbour.assign(static_cast<size_t>(K), 0);
    detail::parallelFor(K, [&](int k) {
        int m = k;
        for (int gI = 0; gI < NG3; ++gI) {
            const size_t at = at2(16 * fb * (gI / NG) + gI % NG, K, k);
            t.offP[at] = devOffset(d.gmapP[static_cast<size_t>(k) * NG3 + gI]);
            if (!t.identityM) t.offM[at] = devOffset(d.gmapM[static_cast<size_t>(k) * NG3 + gI]);
            m = std::max(m, d.gmapP[static_cast<size_t>(k) * NG3 + gI] / NG3);
        }
        t.maxNeighbour[static_cast<size_t>(k)] = m;
    });
    for (int i = 0; i < d.num_wall; ++i) {
        const int w = d.gmapW[i];
        if (w < 0 || w >= nG) throw arg_error("bdg_sw2d_curved_create: wall Gauss-node index out of range");
        int& e = t.offP[at2(16 * fb * (w % NG3 / NG) + w % NG, K, w / NG3)];
        if (e >= 0) e = -(e + 1);
    }
    t.slotOf.assign(static_cast<size_t>(ld), -1);
    for (int i = 0; i < d.num_curved; ++i) {
        const int k = d.curvedEls[i];
        if (k < 0 || k >= K) throw arg_error("bdg_sw2d_curved_create: curvedEls entry out of range");
        if (t.slotOf[k] < 0) { // the reference takes set(curvedEls)
            t.slotOf[k] = static_cast<int>(t.curved.size());
            t.curved.push_back(k);
        }
    }
    t.sideLd = (static_cast<long long>(t.curved.size()) + 63) / 64 * 64;
    for (size_t i = 0; i < static_cast<size_t>(Np) * K; ++i)
        if (!(d.J[i] > 0.0)) throw arg_error("bdg_sw2d_curved_create: nodal Jacobian J must be positive");
}

// ---- straight-sided elements
std::vector<char> classifyStraight(const Desc& d, const Tables& t) {
    const int Np = t.Np, K = t.K, Ncub = t.ncub, NG = t.ng;
    const double* geo[4] = {d.cubrx, d.cubry, d.cubsx, d.cubsy};
    std::vector<char> level(static_cast<size_t>(K), kNotStraight);
    detail::parallelFor(K, [&](int k) {
        double scale = 0.0;
        for (int g = 0; g < 4; ++g) scale = std::max(scale, std::fabs(geo[g][k]));
        for (int g = 0; g < 4; ++g)
            for (int i = 1; i < Ncub; ++i)
                if (std::fabs(geo[g][at2(i, K, k)] - geo[g][k]) > 1e-10 * scale) return;
        level[k] = kCubStraight;
        const double j0 = d.J[k];
        for (int m = 1; m < Np; ++m)
            if (std::fabs(d.J[at2(m, K, k)] - j0) > 1e-10 * std::fabs(j0)) return;
        for (int f = 0; f < 3; ++f) {
            const size_t r0 = at2(f * NG, K, k);
            for (int ig = 1; ig < NG; ++ig)
                if (std::fabs(d.gaussnx[r0 + static_cast<size_t>(ig) * K] - d.gaussnx[r0]) > 1e-10 ||
                    std::fabs(d.gaussny[r0 + static_cast<size_t>(ig) * K] - d.gaussny[r0]) > 1e-10) return;
        }
        level[k] = kStraight;
    });
    return level;
}

// W[., k] = ratio * wr[.] with ratio = W[0, k] / wr[0] > 0 (rows of stride K from w); 0.0: not proportional
double proportional(const double* w, int K, int n, const double* wr) {
    const double ratio = w[0] / wr[0];
    if (!(ratio > 0.0)) return 0.0;
    for (int i = 1; i < n; ++i)
        if (!(std::fabs(w[static_cast<size_t>(i) * K] - ratio * wr[i]) <= 1e-10 * std::fabs(ratio * wr[i]))) return 0.0;
    return ratio;
}

// The general form's compression: every unlisted cubature-straight element whose weights are a multiple of kref's.
void compressGeneral(const Desc& d, const std::vector<char>& level, Tables& t) {
    const int K = t.K, Ncub = t.ncub;
    const double* geo[4] = {d.cubrx, d.cubry, d.cubsx, d.cubsy};
    for (int k = 0; k < K && t.kref < 0; ++k)
        if (level[k] >= kCubStraight && d.cubW[k] > 0.0) t.kref = k;
    if (t.kref < 0) return;
    t.wref.assign(static_cast<size_t>(16) * t.ncb, 0.0);
    t.cubAffine.assign(static_cast<size_t>(4) * K, 0.0);
    t.affineEl.assign(static_cast<size_t>(t.ld), 0);
    for (int i = 0; i < Ncub; ++i) t.wref[i] = d.cubW[at2(i, K, t.kref)];
    std::atomic<int> counted{0};
    detail::parallelChunks(K, [&](int kBegin, int kEnd) {
        int mine = 0;
        for (int k = kBegin; k < kEnd; ++k) {
            if (t.slotOf[k] >= 0 || level[k] < kCubStraight) continue; // elements of curvedEls keep the general path
            const double ratio = proportional(d.cubW + k, K, Ncub, t.wref.data());
            if (ratio == 0.0) continue;
            t.affineEl[k] = 1;
            for (int g = 0; g < 4; ++g) t.cubAffine[at2(g, K, k)] = ratio * geo[g][k];
            ++mine;
        }
        counted += mine;
    });
    t.numAffine = counted;
    for (long long k = K; k < t.ld; ++k) t.affineEl[k] = t.affineEl[K - 1]; // (padding lanes repeat the last element)
}

// The nodal-trace form's: unlisted fully straight elements whose cubature and Gauss weights are multiples of krefNT's.
// e[0..3] = ratio (rx, ry, sx, sy), then (nx, ny, weight ratio) per face, e[13] = 1 / J. Sets bit 3 of faceFlags.
void compressNodalTrace(const Desc& d, const std::vector<char>& level, Tables& t) {
    const int K = t.K, Ncub = t.ncub, NG = t.ng;
    const double* geo[4] = {d.cubrx, d.cubry, d.cubsx, d.cubsy};
    t.elAffine.assign(static_cast<size_t>(14) * K, 0.0);
    t.gaussWref.assign(static_cast<size_t>(16) * t.fb, 0.0);
    t.wrefNT.assign(static_cast<size_t>(16) * t.ncb, 0.0);
    for (int k = 0; k < K && t.krefNT < 0; ++k)
        if (t.slotOf[k] < 0 && level[k] == kStraight && d.cubW[k] > 0.0 && d.gaussW[k] > 0.0) t.krefNT = k;
    if (t.krefNT < 0) return;
    std::vector<double> gw(static_cast<size_t>(NG));
    for (int i = 0; i < Ncub; ++i) t.wrefNT[i] = d.cubW[at2(i, K, t.krefNT)];
    for (int ig = 0; ig < NG; ++ig) { gw[ig] = d.gaussW[at2(ig, K, t.krefNT)]; t.gaussWref[ig] = 0.5 * gw[ig]; }
    std::atomic<int> counted{0};
    detail::parallelChunks(K, [&](int kBegin, int kEnd) {
        int mine = 0;
        double e[14];
        for (int k = kBegin; k < kEnd; ++k) {
            if (t.slotOf[k] >= 0 || level[k] != kStraight) continue;
            const double ratio = proportional(d.cubW + k, K, Ncub, t.wrefNT.data());
            bool ok = ratio != 0.0;
            for (int g = 0; g < 4; ++g) e[g] = ratio * geo[g][k];
            for (int f = 0; f < 3 && ok; ++f) {
                const size_t r0 = at2(f * NG, K, k);
                const double sf = proportional(d.gaussW + r0, K, NG, gw.data());
                ok = sf != 0.0;
                e[4 + 3 * f] = d.gaussnx[r0]; e[5 + 3 * f] = d.gaussny[r0]; e[6 + 3 * f] = sf;
            }
            if (!ok) continue;
            e[13] = 1.0 / d.J[k];
            t.faceFlags[k] |= 8;
            for (int i = 0; i < 14; ++i) t.elAffine[at2(i, K, k)] = e[i];
            ++mine;
        }
        counted += mine;
    });
    t.numAffineNT = counted;
}

// ---- face structure of the nodal-trace form (sw2d_curved_nt_kernel.hpp), or false when the context lacks it:
//  (1) gmapM is the identity; (2) every row block of Interp that belongs to a face is zero outside N + 1 columns (its face
//  nodes); (3) gmapP pairs whole faces, in the same or in the opposite direction, and the paired faces' interpolation
//  columns agree at the paired Gauss points under one permutation of their face nodes; (4) a face's Gauss points are all
//  walls or none; (5) the image fits the kernel's LDS plan. Fills nodeP, faceNodes and the wall bits of faceFlags.
bool faceStructure(const Desc& d, const KernelSizes& ks, Tables& t) {
    const int Np = t.Np, K = t.K, NG = t.ng, NG3 = 3 * NG, Nfp = t.N + 1, KE = ks.ntOff[2];
    const long long ld = t.ld;
    if (!t.identityM || !ks.ntFits) return false;
    if (4ll * 16 * t.ncb * ld * 8 > 4294967295LL) return false; // the cubature planes behind ONE descriptor
    const double* I = d.gaussInterp; // (3 NG, Np)
    std::vector<std::vector<int>> nodes(3);
    for (int f = 0; f < 3; ++f) {
        for (int m = 0; m < Np; ++m) {
            double big = 0.0;
            for (int ig = 0; ig < NG; ++ig) big = std::max(big, std::fabs(I[static_cast<size_t>(f * NG + ig) * Np + m]));
            if (big > 1e-9) nodes[f].push_back(m);
            else if (big > 1e-12) return false; // neither a face node nor nothing
        }
        if (static_cast<int>(nodes[f].size()) != Nfp) return false;
    }
    auto IF = [&](int f, int ig, int i) { return I[static_cast<size_t>(f * NG + ig) * Np + nodes[f][i]]; };
    // (3) node pairing of (f, f2, direction): perm[i] = i2 with IF(f, ig, i) == IF(f2, ig2(ig), i2) for every ig
    std::vector<int> perm(static_cast<size_t>(18) * Nfp, -1), permState(18, 0); // 0 not tried, 1 found, -1 none
    auto pairing = [&](int f, int f2, int rev) -> const int* {
        const int id = (f * 3 + f2) * 2 + rev;
        int* out = perm.data() + static_cast<size_t>(id) * Nfp;
        if (permState[id] == 0) {
            std::vector<char> used(Nfp, 0);
            bool ok = true;
            for (int i = 0; i < Nfp && ok; ++i) {
                int found = -1;
                for (int i2 = 0; i2 < Nfp && found < 0; ++i2) {
                    if (used[i2]) continue;
                    double worst = 0.0;
                    for (int ig = 0; ig < NG; ++ig) worst = std::max(worst, std::fabs(IF(f, ig, i) - IF(f2, rev ? NG - 1 - ig : ig, i2)));
                    if (worst < 1e-11) found = i2;
                }
                if (found < 0) ok = false;
                else { used[found] = 1; out[i] = found; }
            }
            permState[id] = ok ? 1 : -1;
        }
        return permState[id] == 1 ? out : nullptr;
    };
    t.rowsP = 3 * KE * 4;
    t.nodeP.assign(static_cast<size_t>(t.rowsP) * K, 0);
    t.faceFlags.assign(static_cast<size_t>(ld), 0);
    std::vector<int> wallCount(static_cast<size_t>(3) * K, 0);
    for (int i = 0; i < d.num_wall; ++i) ++wallCount[static_cast<size_t>(d.gmapW[i] / NG3) * 3 + (d.gmapW[i] % NG3) / NG];
    for (int k = 0; k < K; ++k)
        for (int f = 0; f < 3; ++f) {
            const int* gp = d.gmapP + static_cast<size_t>(k) * NG3 + f * NG;
            const int k2 = gp[0] / NG3, f2 = (gp[0] % NG3) / NG, l0 = gp[0] % NG;
            int rev;
            if (l0 == 0 && (NG == 1 || gp[NG - 1] % NG == NG - 1)) rev = 0;
            else if (l0 == NG - 1) rev = 1;
            else return false;
            for (int ig = 0; ig < NG; ++ig)
                if (gp[ig] != k2 * NG3 + f2 * NG + (rev ? NG - 1 - ig : ig)) return false;
            const int* pm = pairing(f, f2, rev);
            const int wc = wallCount[static_cast<size_t>(k) * 3 + f];
            if (!pm || (wc != 0 && wc != NG)) return false;
            if (wc) t.faceFlags[k] |= 1 << f;
            for (int i = 0; i < KE * 4; ++i) // padding rows: an own node (the column of GE is zero)
                t.nodeP[at2(f * KE * 4 + i, K, k)] = i < Nfp ? static_cast<int>(nodes[f2][pm[i]] * ld + k2) : k;
        }
    t.faceNodes.resize(static_cast<size_t>(t.rowsP));
    for (int f = 0; f < 3; ++f)
        for (int i = 0; i < KE * 4; ++i) t.faceNodes[static_cast<size_t>(f) * KE * 4 + i] = nodes[f][i < Nfp ? i : 0];
    return true;
}

// ---- order of the tiles: positions [n x / 8, n (x + 1) / 8) of the list are XCD x's (sw2d_curved_nt_kernel); each eighth gets
//      an eighth of the general tiles (in mesh order, first), then straight-sided ones (in mesh order). Empty: mesh order.
std::vector<int> tileOrder(const std::vector<int>& faceFlags, int K) {
    const int ntiles = (K + 15) / 16;
    std::vector<int> general, straight, order;
    for (int t = 0; t < ntiles; ++t) {
        bool allStraight = true;
        for (int k = 16 * t; k < std::min(K, 16 * t + 16); ++k) allStraight = allStraight && (faceFlags[k] & 8);
        (allStraight ? straight : general).push_back(t);
    }
    const long long G = static_cast<long long>(general.size()), S = static_cast<long long>(straight.size());
    if (G == 0 || S == 0 || ntiles < 64) return {};
    long long gi = 0, si = 0;
    for (long long x = 0; x < 8; ++x) {
        const long long cx = ntiles * (x + 1) / 8 - ntiles * x / 8;
        long long gq = std::min({G * (x + 1) / 8 - G * x / 8, cx, G - gi}), sq = cx - gq;
        if (sq > S - si) { sq = S - si; gq = cx - sq; }
        for (long long i = 0; i < gq; ++i) order.push_back(general[static_cast<size_t>(gi + i)]);
        for (long long i = 0; i < sq; ++i) order.push_back(straight[static_cast<size_t>(si + i)]);
        gi += gq; si += sq;
    }
    if (gi != G || si != S || static_cast<int>(order.size()) != ntiles) return {};
    return order;
}

// ---- operator image in MFMA A-tile order: entry l of a tile = A[row l & 15][step column l >> 4]. faceNodes == nullptr: the
//      general form's layout (CurvedOps), else the nodal-trace form's (CurvedOpsNT), whose Gauss tiles hold face-node columns.
std::vector<double> operatorImage(const Desc& d, const KernelSizes& ks, const Tables& t, const std::vector<double>& M,
                                  const std::vector<double>& MF, const int* faceNodes) {
    const int Np = t.Np, Ncub = t.ncub, NG = t.ng, ncb = t.ncb, fb = t.fb, Nfp = t.N + 1, KV = ks.KV, MT = ks.MT;
    const bool nt = faceNodes != nullptr;
    const int VCH = ks.ntOff[0], SCH = ks.ntOff[1], KE = ks.ntOff[2], offSurf = ks.ntOff[3], offMass = ks.ntOff[4];
    const int* off = ks.opsOff;
    const int offM = nt ? offMass : off[4], offMF = nt ? offMass + MT * KV : off[5], offF = nt ? offMass + 2 * MT * KV : off[6];
    const double* I = d.gaussInterp;
    std::vector<double> img(static_cast<size_t>(nt ? ks.ntTiles : ks.opsTiles) * 64, 0.0);
    for (int l = 0; l < 64; ++l) {
        const int i = l & 15, sc = l >> 4;
        auto at = [&](int tile) -> double& { return img[static_cast<size_t>(tile) * 64 + l]; };
        for (int rb = 0; rb < ncb; ++rb) {
            for (int c = 0; c < KV; ++c) {
                const int row = 16 * rb + i, m = 4 * c + sc;
                if (row < Ncub && m < Np) at(nt ? rb * VCH + c : off[0] + rb * KV + c) = d.cubV[static_cast<size_t>(row) * Np + m];
            }
            for (int r = 0; r < MT; ++r)
                for (int reg = 0; reg < 4; ++reg) {
                    const int node = 16 * r + i, cp = 16 * rb + 4 * reg + sc;
                    if (node >= Np || cp >= Ncub) continue;
                    at(nt ? rb * VCH + KV + r * 4 + reg : off[1] + (r * ncb + rb) * 4 + reg) = d.cubDr[static_cast<size_t>(cp) * Np + node];
                    at(nt ? rb * VCH + KV + 4 * MT + r * 4 + reg : off[2] + (r * ncb + rb) * 4 + reg) = d.cubDs[static_cast<size_t>(cp) * Np + node];
                }
        }
        for (int gb = 0; gb < 3 * fb; ++gb) {
            const int f = gb / fb, b = gb % fb;
            for (int c = 0; c < (nt ? KE : KV); ++c) { // Interp: face-node columns (nodal-trace) or every node
                const int local = 16 * b + i, m = 4 * c + sc;
                if (local >= NG || m >= (nt ? Nfp : Np)) continue;
                at(nt ? offSurf + gb * SCH + c : off[7] + gb * KV + c) = I[static_cast<size_t>(f * NG + local) * Np + (nt ? faceNodes[f * KE * 4 + m] : m)];
            }
            for (int r = 0; r < MT; ++r)
                for (int reg = 0; reg < 4; ++reg) {
                    const int node = 16 * r + i, local = 16 * b + 4 * reg + sc;
                    if (node < Np && local < NG)
                        at(nt ? offSurf + gb * SCH + KE + r * 4 + reg : off[3] + (r * 3 * fb + gb) * 4 + reg) = -I[static_cast<size_t>(f * NG + local) * Np + node];
                }
        }
        for (int r = 0; r < MT; ++r)
            for (int c = 0; c < KV; ++c) {
                const int node = 16 * r + i, m = 4 * c + sc;
                if (node >= Np || m >= Np) continue;
                at(offM + r * KV + c) = M[static_cast<size_t>(node) * Np + m];
                if (d.Filter) {
                    at(offMF + r * KV + c) = MF[static_cast<size_t>(node) * Np + m];
                    at(offF + r * KV + c) = d.Filter[static_cast<size_t>(node) * Np + m];
                }
            }
    }
    return img;
}

// ---- inverse mass matrix of every listed element from its upper Cholesky factor U (M = U^T U): W = U^-1 by back
//      substitution, Minv = W W^T (the reference solves U^T y = b, U x = y per evaluation, rhs.py:157-162)
std::vector<double> inverseMass(const Desc& d, const Tables& t) {
    const int Np = t.Np, K = t.K;
    std::vector<double> minv(static_cast<size_t>(Np) * Np * t.curved.size(), 0.0);
    std::atomic<bool> badDiagonal{false};
    detail::parallelChunks(static_cast<int>(t.curved.size()), [&](int cBegin, int cEnd) {
        std::vector<double> U(static_cast<size_t>(Np) * Np), W(static_cast<size_t>(Np) * Np);
        for (int c = cBegin; c < cEnd; ++c) {
            for (int i = 0; i < Np; ++i)
                for (int jj = 0; jj < Np; ++jj) U[static_cast<size_t>(i) * Np + jj] = d.MMChol[(static_cast<size_t>(i) * Np + jj) * K + t.curved[c]];
            std::fill(W.begin(), W.end(), 0.0);
            for (int jj = 0; jj < Np; ++jj) { // column jj of W: U w = e_jj, from row jj upwards
                if (!(U[static_cast<size_t>(jj) * Np + jj] > 0.0)) { badDiagonal = true; break; }
                W[static_cast<size_t>(jj) * Np + jj] = 1.0 / U[static_cast<size_t>(jj) * Np + jj];
                for (int i = jj - 1; i >= 0; --i) {
                    double sum = 0.0;
                    for (int m = i + 1; m <= jj; ++m) sum += U[static_cast<size_t>(i) * Np + m] * W[static_cast<size_t>(m) * Np + jj];
                    W[static_cast<size_t>(i) * Np + jj] = -sum / U[static_cast<size_t>(i) * Np + i];
                }
            }
            double* out = minv.data() + static_cast<size_t>(c) * Np * Np;
            for (int i = 0; i < Np; ++i)
                for (int jj = i; jj < Np; ++jj) {
                    double sum = 0.0;
                    for (int m = jj; m < Np; ++m) sum += W[static_cast<size_t>(i) * Np + m] * W[static_cast<size_t>(jj) * Np + m];
                    out[static_cast<size_t>(i) * Np + jj] = out[static_cast<size_t>(jj) * Np + i] = sum;
                }
        }
    }, 8);
    if (badDiagonal) throw arg_error("bdg_sw2d_curved_create: MMChol has a non-positive diagonal entry on an element of curvedEls");
    return minv;
}

} // namespace

void validate(const Desc& d) {
    if (d.num_elements < 1 || d.num_cub < 1 || d.num_gauss < 1) throw arg_error("bdg_sw2d_curved_create: bad sizes");
    if (d.num_gauss > 32) throw arg_error("bdg_sw2d_curved_create: at most 32 Gauss points per face");
    if (!d.V || !d.J || !d.cubV || !d.cubDr || !d.cubDs || !d.cubW || !d.cubrx || !d.cubry || !d.cubsx || !d.cubsy ||
        !d.gaussInterp || !d.gaussW || !d.gaussnx || !d.gaussny || !d.gmapM || !d.gmapP)
        throw arg_error("bdg_sw2d_curved_create: a required table pointer is NULL");
    if (d.num_wall < 0 || (d.num_wall > 0 && !d.gmapW)) throw arg_error("bdg_sw2d_curved_create: bad wall-node list");
    if (d.num_curved < 0 || (d.num_curved > 0 && (!d.curvedEls || !d.MMChol)))
        throw arg_error("bdg_sw2d_curved_create: curvedEls given without MMChol (or a negative count)");
}

Tables build(const Desc& d, const KernelSizes& ks, const Switches& sw) {
    validate(d);
    Tables t;
    t.N = d.order; t.Np = ks.Np; t.K = d.num_elements;
    t.ncub = d.num_cub; t.ncb = (d.num_cub + 15) / 16; t.ng = d.num_gauss; t.fb = (d.num_gauss + 15) / 16;
    t.ld = (static_cast<long long>(t.K) + 63) / 64 * 64;
    buildMaps(d, t);
    const std::vector<char> level = sw.noAffine ? std::vector<char>(static_cast<size_t>(t.K), kNotStraight) : classifyStraight(d, t);
    compressGeneral(d, level, t);
    t.useNT = !sw.general && faceStructure(d, ks, t);
    if (t.useNT) {
        std::vector<int>().swap(t.offP);
        std::vector<int>().swap(t.offM);
        compressNodalTrace(d, level, t);
        for (long long k = t.K; k < t.ld; ++k) t.faceFlags[k] = t.faceFlags[t.K - 1]; // padding lanes repeat the last element
        if (!sw.noTileOrder) t.tileOrder = tileOrder(t.faceFlags, t.K);
    }
    if (!t.curved.empty()) t.minv = inverseMass(d, t);
    std::vector<double> Vt(static_cast<size_t>(t.Np) * t.Np);
    for (int i = 0; i < t.Np; ++i)
        for (int jj = 0; jj < t.Np; ++jj) Vt[static_cast<size_t>(i) * t.Np + jj] = d.V[static_cast<size_t>(jj) * t.Np + i];
    const std::vector<double> M = matmul(d.V, Vt.data(), t.Np, t.Np, t.Np);
    const std::vector<double> MF = d.Filter ? matmul(d.Filter, M.data(), t.Np, t.Np, t.Np) : std::vector<double>();
    t.ops = operatorImage(d, ks, t, M, MF, nullptr);
    if (t.useNT) t.opsNT = operatorImage(d, ks, t, M, MF, t.faceNodes.data());
    t.bytesPerElement = bytesPerElement(d, t);
    return t;
}

void weightedGeometry(const Desc& d, int g, std::vector<double>& out) {
    const double* geo[4] = {d.cubrx, d.cubry, d.cubsx, d.cubsy};
    out.resize(static_cast<size_t>(d.num_cub) * d.num_elements);
    detail::parallelFor(static_cast<long long>(out.size()), [&](long long i) { out[i] = d.cubW[i] * geo[g][i]; }, 1 << 16);
}

void inverseJacobian(const Desc& d, int Np, std::vector<double>& out) {
    out.resize(static_cast<size_t>(Np) * d.num_elements);
    for (size_t i = 0; i < out.size(); ++i) out[i] = 1.0 / d.J[i];
}

double bytesPerElement(const Desc& d, const Tables& t) {
    const int Np = t.Np, Ncub = t.ncub, NG3 = 3 * t.ng, Nfp = t.N + 1, KE = (Nfp + 3) / 4;
    if (t.useNT) { // state in, update in / out, the neighbours' face nodes, node map + flags, geometry (14 numbers on straight elements), sources
        const double fa = static_cast<double>(t.numAffineNT) / t.K;
        return 8.0 * (4 * Np + 4 * Np + 4 * 3 * Nfp + (1.0 - fa) * (4 * Ncub + 3 * NG3 + Np) + fa * 14 + (d.zx ? Np : 0) +
                      (d.zy ? Np : 0) + (d.coriolis ? Np : 0) + (d.drag ? Np : 0)) +
               4.0 * (3 * KE * 4 + 3);
    }
    // state in, RHS out, cubature geometry (4 Ncub per general element, 4 per straight one), Gauss geometry, 1/J, sources,
    // state again in the trace kernel, traces out and in (the exterior side; the interior side too when gmapM is not the identity)
    const double fa = static_cast<double>(t.numAffine) / t.K;
    return 8.0 * (4 * Np + 4 * Np + (1.0 - fa) * 4 * Ncub + fa * 4 + 3 * NG3 + Np + (d.zx ? Np : 0) + (d.zy ? Np : 0) +
                  (d.coriolis ? Np : 0) + (d.drag ? Np : 0) + 4 * Np + (t.identityM ? 2 : 3) * 4 * NG3) +
           4.0 * (NG3 * (t.identityM ? 1 : 2) + 2);
}

} // namespace curved_tables
} // namespace blitzdg
