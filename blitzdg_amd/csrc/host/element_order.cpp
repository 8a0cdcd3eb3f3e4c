// Element numberings from the face-neighbour graph, and the renumbering rule (element_order.hpp).
#include "element_order.hpp"
#include "parallel_for.hpp"
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>

namespace blitzdg {
namespace element_order {

// Breadth-first (Cuthill-McKee style) renumbering from the face-neighbour graph:
// neighbours end up within O(sqrt(K)) slots of each other, so the trace gather of
// a wave hits lines its own or nearby waves stream. perm[k] = device slot.
std::vector<int> bfsOrder(const int* vmapP, int K, int Np, int Nfp, int faces) {
    std::vector<int> perm(K, -1);
    int next = 0;
    std::vector<int> frontier, nextFrontier;
    for (int seed = 0; seed < K; ++seed) {
        if (perm[seed] >= 0) continue;
        perm[seed] = next++;
        frontier.assign(1, seed);
        while (!frontier.empty()) {
            nextFrontier.clear();
            for (int k : frontier)
                for (int f = 0; f < faces; ++f) {
                    const int k2 = vmapP[(static_cast<size_t>(k) * faces + f) * Nfp] / Np;
                    if (k2 >= 0 && k2 < K && perm[k2] < 0) {
                        perm[k2] = next++;
                        nextFrontier.push_back(k2);
                    }
                }
            frontier.swap(nextFrontier);
        }
    }
    return perm;
}

// A patch grows breadth-first from its seed until it holds `patch` elements; its still-unassigned
// face neighbours join a FIFO of seeds, and the next patch starts from the first FIFO entry that is
// still free (from the next free element in caller order when the FIFO has run dry: the first patch,
// and every further component of a disconnected mesh). Patches therefore tile the mesh outwards from
// element 0, each next to ones numbered shortly before it. Inside a patch the slots follow the caller's
// index, which on a structured mesh keeps the runs of lane +- 1 neighbours and so the number of cache
// lines one gather instruction touches. Serial: 10^6 elements take 0.08 s (breadth-first: 0.02 s).
std::vector<int> patchOrder(const int* vmapP, int K, int Np, int Nfp, int patch) {
    patch = std::max(1, patch);
    std::vector<int> perm(K, -1);
    std::vector<char> taken(K, 0), queued(K, 0);
    std::vector<int> seeds, members;
    seeds.reserve(K);
    members.reserve(std::min(patch, K));
    size_t head = 0;
    int cursor = 0, next = 0;
    auto neighbour = [&](int k, int f) {
        const int k2 = vmapP[(static_cast<size_t>(k) * 3 + f) * Nfp] / Np;
        return k2 >= 0 && k2 < K ? k2 : k;
    };
    while (next < K) {
        int seed = -1;
        while (head < seeds.size() && seed < 0) {
            const int c = seeds[head++];
            if (!taken[c]) seed = c;
        }
        if (seed < 0) {
            while (taken[cursor]) ++cursor;
            seed = cursor;
        }
        members.assign(1, seed);
        taken[seed] = 1;
        for (size_t i = 0; i < members.size() && static_cast<int>(members.size()) < patch; ++i)
            for (int f = 0; f < 3 && static_cast<int>(members.size()) < patch; ++f) {
                const int k2 = neighbour(members[i], f);
                if (!taken[k2]) {
                    taken[k2] = 1;
                    members.push_back(k2);
                }
            }
        // (an element waits in the FIFO once: it stays there until a patch starts from it or passes it over)
        for (int k : members)
            for (int f = 0; f < 3; ++f) {
                const int k2 = neighbour(k, f);
                if (!taken[k2] && !queued[k2]) {
                    queued[k2] = 1;
                    seeds.push_back(k2);
                }
            }
        std::sort(members.begin(), members.end());
        for (int k : members) perm[k] = next++;
    }
    return perm;
}

int patchSetting() {
    const char* e = std::getenv("BDG_SW2D_ORDER_PATCH");
    return e ? std::atoi(e) : kDefaultPatch;
}

std::vector<int> renumbering(const int* vmapP, int K, int Np, int Nfp, int patch) {
    return patch <= 0 ? bfsOrder(vmapP, K, Np, Nfp, 3) : patchOrder(vmapP, K, Np, Nfp, patch);
}

int stageBytesPerElement(int order) {
    // state read and written at every stage, residual read at four and written at four of the five
    // stages of a step (3 Np doubles each); 13 geometry doubles and 3 face links per element
    const int Np = (order + 1) * (order + 2) / 2;
    return 24 * Np * 18 / 5 + 13 * 8 + 3 * 4;
}

int farWindow(int order, int K) {
    if (order > 4) return 0;
    const long long bytes = stageBytesPerElement(order);
    const long long l2 = 4ll << 20;
    return K * bytes > l2 ? static_cast<int>((1ll << 20) / bytes) : 0;
}

bool renumberingWanted(const int* vmapP, int K, int Np, int Nfp, int order) {
    const int window = farWindow(order, K);
    std::atomic<long long> total{0}, far{0};        // integers: the same sums whatever the number of workers
    detail::parallelChunks(K, [&](int kBegin, int kEnd) {
        long long mine = 0, mineFar = 0;
        for (int k = kBegin; k < kEnd; ++k)
            for (int f = 0; f < 3; ++f) {
                const long long dist = std::llabs(static_cast<long long>(vmapP[(static_cast<size_t>(k) * 3 + f) * Nfp] / Np) - k);
                mine += dist;
                mineFar += dist > window;
            }
        total += mine;
        far += mineFar;
    });
    const double sum = static_cast<double>(total.load());
    if (sum / (3.0 * K) > 4.0 * std::sqrt(static_cast<double>(K))) return true;
    return window > 0 && 10 * far.load() > 3ll * K;
}

} // namespace element_order
} // namespace blitzdg
