// Stand-alone driver of the triangle run monitor's host set-up (TriangleNodesProvisioner::quadratureWeights, locatePoints,
// interpolationRows), built with -fsanitize=address,undefined by tests/test_tri_monitor_setup.py and run on the CPU:
//   host_trimon_check
#include "blitzdg/MeshManager.hpp"
#include "blitzdg/TriangleNodesProvisioner.hpp"
#include <cmath>
#include <cstdio>
#include <vector>

using namespace blitzdg;

int main() {
    int bad = 0;
    for (unsigned long long seed : {0ULL, 9ULL}) {
        MeshManager mesh;
        mesh.buildBoxMesh(7, 5, -1.0, 1.0, -1.0, 1.0, seed);
        for (int N : {1, 4, 8}) {
            TriangleNodesProvisioner nodes(N, mesh);
            const int Np = nodes.get_NumLocalPoints(), K = nodes.get_NumElements();
            real_matrix_type w;
            nodes.quadratureWeights(w);
            double area = 0;
            for (int n = 0; n < Np; ++n)
                for (int k = 0; k < K; ++k) area += w(n, k);
            bad += !(std::fabs(area - 4.0) < 1e-12);
            // every node of every element and a few points outside: located, and the round trip closes
            std::vector<double> x, y;
            for (int k = 0; k < K; ++k)
                for (int n = 0; n < Np; ++n) {
                    x.push_back(nodes.get_xGrid()(n, k));
                    y.push_back(nodes.get_yGrid()(n, k));
                }
            for (double far : {1e3, -1e3, 1e300}) {
                x.push_back(far);
                y.push_back(-far);
            }
            const int n = static_cast<int>(x.size());
            std::vector<int> el(n);
            std::vector<double> r(n), s(n), rows(static_cast<size_t>(n) * Np);
            nodes.locatePoints(x.data(), y.data(), n, el.data(), r.data(), s.data());
            nodes.locatePoints(nullptr, nullptr, 0, nullptr, nullptr, nullptr);
            nodes.interpolationRows(nullptr, nullptr, 0, nullptr);
            for (int p = n - 3; p < n; ++p) {
                bad += el[p] != -1;
                r[p] = s[p] = -1.0; // a vertex, for the rows below
            }
            nodes.interpolationRows(r.data(), s.data(), n, rows.data());
            for (int p = 0; p < n - 3; ++p) {
                if (el[p] < 0 || el[p] > p / Np) { ++bad; continue; } // the lowest element that holds the node
                double px = 0, py = 0;
                for (int m = 0; m < Np; ++m) {
                    px += rows[static_cast<size_t>(p) * Np + m] * nodes.get_xGrid()(m, el[p]);
                    py += rows[static_cast<size_t>(p) * Np + m] * nodes.get_yGrid()(m, el[p]);
                }
                bad += !(std::fabs(px - x[p]) < 1e-10 && std::fabs(py - y[p]) < 1e-10);
            }
            // on a node: the unit vector
            std::vector<double> unit(static_cast<size_t>(Np) * Np);
            nodes.interpolationRows(nodes.get_rGrid().data(), nodes.get_sGrid().data(), Np, unit.data());
            for (int a = 0; a < Np; ++a)
                for (int b = 0; b < Np; ++b) bad += unit[static_cast<size_t>(a) * Np + b] != (a == b ? 1.0 : 0.0);
            std::printf("seed=%llu N=%d K=%d area=%.15g located=%d\n", seed, N, K, area, n);
        }
    }
    std::printf(bad ? "host trimon check FAILED (%d)\n" : "host trimon check ok\n", bad);
    return bad ? 1 : 0;
}
