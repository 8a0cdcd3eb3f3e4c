// The run-time to compile-time dispatchers of blitzdg_amd/csrc/hip/sw2d_dispatch.hpp on the host, with a callable that records
// the constants it is reached with. One line per call: dispatcher, arguments, what came back, how often the callable ran and with
// which constants. tests/test_dispatch.py builds this with -fsanitize=address,undefined, runs it and checks every line.
#include "sw2d_dispatch.hpp"
#include <cstdio>
#include <string>

namespace {
int calls = 0, total = 0;
std::string reached;

// what the callable answers: never hipErrorInvalidValue (the dispatchers' own answer), and not the same twice in a row
hipError_t answer() { return (total++ % 2) ? hipErrorNotReady : hipErrorNotSupported; }

struct Record {
    template <class M>
    hipError_t operator()(M) const {
        ++calls;
        reached += std::to_string(M::value);
        return answer();
    }
    template <class M, class F>
    hipError_t operator()(M, F) const {
        static_assert(std::is_same<typename F::value_type, bool>::value, "the filter constant is a std::bool_constant");
        ++calls;
        reached += std::to_string(M::value) + "," + std::to_string(F::value ? 1 : 0);
        return answer();
    }
};

template <class Call>
void line(const char* name, int arg, int filter, Call&& call) {
    calls = 0;
    reached.clear();
    const hipError_t expect = (total % 2) ? hipErrorNotReady : hipErrorNotSupported; // what the callable will answer if it runs
    const hipError_t got = call();
    std::printf("%s arg=%d filter=%d ret=%d calls=%d passed=%d reached=%s\n", name, arg, filter, static_cast<int>(got), calls,
                (calls == 1 && got == expect) ? 1 : 0, reached.c_str());
}
} // namespace

int main() {
    using namespace bdg_dev;
    std::printf("invalid=%d\n", static_cast<int>(hipErrorInvalidValue));
    const int modes[] = {-1, 0, 1, 2, 3, 4, 99}; // every mode of either numbering, one before, one past the last, and 99
    for (int mode : modes) {
        line("forMode", mode, 0, [&] { return forMode(mode, Record{}); });
        for (int filter = 0; filter < 2; ++filter) {
            line("forModeFilter", mode, filter, [&] { return forModeFilter(mode, filter != 0, Record{}); });
            line("curvedForMode", mode, filter, [&] { return curvedForMode(mode, filter != 0, Record{}); });
            line("quadForMode", mode, filter, [&] { return quadForMode<false>(mode, filter != 0, Record{}); });
            line("quadForModeHeun", mode, filter, [&] { return quadForMode<true>(mode, filter != 0, Record{}); });
        }
    }
    for (int order = 0; order <= 9; ++order) line("forOrder8", order, 0, [&] { return forOrder<8>(order, Record{}); });
    for (int order = 0; order <= 13; ++order) line("forOrder12", order, 0, [&] { return forOrder<12>(order, Record{}); });
    std::printf("dispatch ok\n");
    return 0;
}
