// sw2d_launch_host.hpp -- host code only: what the per-order launch files of the triangle solvers (sw2d_order.hip,
// sw2d_curved_order.hip) share besides the dispatchers.
#pragma once
#include "sw2d_dispatch.hpp"
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>

// names of the per-order entry points: BDG_CAT(kernel_table_order, BDG_ORDER)
#define BDG_CAT2(a, b) a##b
#define BDG_CAT(a, b) BDG_CAT2(a, b)

namespace bdg_dev {

// A kernel may claim more than 64 KB of dynamic LDS only once its limit was raised.
template <class Kernel>
hipError_t allowDynamicLds(Kernel kern, size_t bytes) {
    if (bytes <= 64 * 1024) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(bytes));
}

// One array behind ONE 32-bit buffer descriptor: `fields` planes of Np rows of ld doubles
inline bool fitsOneDescriptor(long long fields, int Np, long long ld) { return fields * Np * ld * 8 <= 4294967295LL; }

#ifdef BDG_PHASE_CLOCK
// Profiling build: COLS phase cycles for each of the first ROWS waves / workgroups of the last launch go to
// $BDG_PHASE_CLOCK_FILE when the process exits (the buffer is pinned host memory the kernel writes directly, so nothing of
// HIP is needed at that point). nullptr: no memory.
template <unsigned ROWS, int COLS>
unsigned long long* phaseClockBuffer() {
    static unsigned long long* buf = nullptr;
    if (!buf) {
        if (hipHostMalloc(&buf, ROWS * COLS * sizeof(unsigned long long), hipHostMallocMapped) != hipSuccess) return buf = nullptr;
        std::memset(buf, 0, ROWS * COLS * sizeof(unsigned long long));
        std::atexit([] {
            const char* name = std::getenv("BDG_PHASE_CLOCK_FILE");
            if (FILE* f = name ? std::fopen(name, "w") : nullptr) {
                for (unsigned w = 0; w < ROWS; ++w) {
                    std::fprintf(f, "%u", w);
                    for (int i = 0; i < COLS; ++i) std::fprintf(f, " %llu", buf[w * COLS + i]);
                    std::fprintf(f, "\n");
                }
                std::fclose(f);
            }
        });
    }
    return buf;
}
#endif

} // namespace bdg_dev
