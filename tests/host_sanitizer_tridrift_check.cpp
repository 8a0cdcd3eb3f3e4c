// Stand-alone driver of the triangle drifters' host set-up (TriangleNodesProvisioner::drifterTables), built with
// -fsanitize=address,undefined by tests/test_tri_drifter_setup.py and run on the CPU:
//   host_tridrift_check
#include "blitzdg/MeshManager.hpp"
#include "blitzdg/TriangleNodesProvisioner.hpp"
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <vector>

using namespace blitzdg;

int main() {
    int bad = 0;
    for (unsigned long long seed : {0ULL, 9ULL}) {
        MeshManager mesh;
        mesh.buildBoxMesh(7, 5, -1.0, 1.0, -1.0, 1.0, seed);
        for (int N : {1, 4, 8}) {
            TriangleNodesProvisioner nodes(N, mesh);
            const int Np = nodes.get_NumLocalPoints(), Nfp = nodes.get_NumFacePoints(), K = nodes.get_NumElements();
            std::vector<double> vert(static_cast<size_t>(8) * K), vinv(static_cast<size_t>(Np) * Np), jac(static_cast<size_t>(N + 2) * (N + 1) * 3);
            std::vector<int> neigh(static_cast<size_t>(3) * K);
            nodes.drifterTables(nullptr, 0, vert.data(), neigh.data(), vinv.data(), jac.data());
            // the box has 2 (7 + 5) wall faces, every other face names a neighbour that names this element back
            int walls = 0;
            double area = 0;
            for (int k = 0; k < K; ++k) {
                const double* v = &vert[static_cast<size_t>(8) * k];
                area += 0.5 * ((v[2] - v[0]) * (v[5] - v[1]) - (v[4] - v[0]) * (v[3] - v[1]));
                for (int f = 0; f < 3; ++f) {
                    const int nb = neigh[static_cast<size_t>(f) * K + k];
                    if (nb == -1) { ++walls; continue; }
                    if (nb < 0 || nb >= K) { ++bad; continue; }
                    bool back = false;
                    for (int g = 0; g < 3; ++g) back = back || neigh[static_cast<size_t>(g) * K + nb] == k;
                    bad += !back;
                }
            }
            bad += walls != 2 * (7 + 5);
            bad += !(std::fabs(area - 4.0) < 1e-12);
            // every face node of element 3 open: its boundary faces (if any) become -2, nothing else changes
            std::vector<int> mapO;
            for (int i = 0; i < 3 * Nfp; ++i) mapO.push_back(3 * 3 * Nfp + i);
            std::vector<int> neigh2(neigh.size());
            nodes.drifterTables(mapO.data(), static_cast<int>(mapO.size()), vert.data(), neigh2.data(), vinv.data(), jac.data());
            for (size_t i = 0; i < neigh.size(); ++i)
                bad += neigh2[i] != ((static_cast<int>(i) % K == 3 && neigh[i] == -1) ? -2 : neigh[i]);
            // the refusals throw and write nothing out of bounds
            const int out = 3 * Nfp * K;
            try { nodes.drifterTables(&out, 1, vert.data(), neigh2.data(), vinv.data(), jac.data()); ++bad; } catch (const std::invalid_argument&) {}
            std::vector<double> x(static_cast<size_t>(Np) * K), y(x.size());
            for (int n = 0; n < Np; ++n)
                for (int k = 0; k < K; ++k) {
                    x[static_cast<size_t>(n) * K + k] = -nodes.get_xGrid()(n, k); // mirrored: every area negative
                    y[static_cast<size_t>(n) * K + k] = nodes.get_yGrid()(n, k);
                }
            nodes.setCoordinates(x.data(), y.data());
            try { nodes.drifterTables(nullptr, 0, vert.data(), neigh2.data(), vinv.data(), jac.data()); ++bad; } catch (const std::invalid_argument&) {}
            std::printf("seed=%llu N=%d K=%d area=%.15g walls=%d\n", seed, N, K, area, walls);
        }
    }
    std::printf(bad ? "host tridrift check FAILED (%d)\n" : "host tridrift check ok\n", bad);
    return bad ? 1 : 0;
}
