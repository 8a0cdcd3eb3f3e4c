// Stand-alone driver of the run monitor's host set-up (QuadNodesProvisioner::quadratureWeights, locatePoints,
// lagrangeBasis1D), built with -fsanitize=address,undefined by tests/test_quad_monitor_setup.py and run on the CPU:
//   host_monitor_check <quadrangle mesh .msh>
#include "blitzdg/MeshManager.hpp"
#include "blitzdg/QuadNodesProvisioner.hpp"
#include <cmath>
#include <cstdio>
#include <vector>

using namespace blitzdg;

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    MeshManager mesh;
    mesh.readMesh(argv[1]);
    int bad = 0;
    for (int N : {1, 4, 9}) {
        QuadNodesProvisioner nodes(N, mesh);
        const int Nq = N + 1, Np = nodes.get_NumLocalPoints(), K = nodes.get_NumElements();
        real_matrix_type w;
        nodes.quadratureWeights(w);
        double area = 0;
        for (int n = 0; n < Np; ++n)
            for (int k = 0; k < K; ++k) area += w(n, k);
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
        std::vector<double> r(n), s(n), lr(Nq), ls(Nq);
        nodes.locatePoints(x.data(), y.data(), n, el.data(), r.data(), s.data());
        nodes.locatePoints(nullptr, nullptr, 0, nullptr, nullptr, nullptr);
        for (int p = 0; p < n; ++p) {
            if (p >= n - 3) {
                bad += el[p] != -1;
                continue;
            }
            if (el[p] < 0 || el[p] > p / Np) { ++bad; continue; } // the lowest element that holds the node
            nodes.lagrangeBasis1D(r[p], lr.data());
            nodes.lagrangeBasis1D(s[p], ls.data());
            double px = 0, py = 0;
            for (int j = 0; j < Nq; ++j)
                for (int i = 0; i < Nq; ++i) {
                    px += lr[j] * ls[i] * nodes.get_xGrid()(Nq * j + i, el[p]);
                    py += lr[j] * ls[i] * nodes.get_yGrid()(Nq * j + i, el[p]);
                }
            bad += !(std::fabs(px - x[p]) < 1e-10 && std::fabs(py - y[p]) < 1e-10);
        }
        for (int a = 0; a < Nq; ++a) { // on a node: the unit vector
            nodes.lagrangeBasis1D(nodes.get_r1d()(a), lr.data());
            for (int b = 0; b < Nq; ++b) bad += lr[b] != (a == b ? 1.0 : 0.0);
        }
        std::printf("N=%d K=%d area=%.15g located=%d\n", N, K, area, n);
    }
    std::printf(bad ? "host monitor check FAILED (%d)\n" : "host monitor check ok\n", bad);
    return bad ? 1 : 0;
}
