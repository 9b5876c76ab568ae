// Stand-alone program over fspann-query-system_amd/host/java_random.hpp (pure host C++17): built by
// tests/test_gt_validate_cpu.py with plain g++ under -fsanitize=address,undefined and run as it is.
//   gt_sampler_test NQ:SAMPLE [NQ:SAMPLE ...]
// prints `anchors A B` (new Random(42).nextInt() twice), then one line per pair: `NQ SAMPLE: v v v ...`, the validator's sample in
// the HashSet's iteration order.
#include <cstdio>
#include <cstdlib>

#include "../../fspann-query-system_amd/host/java_random.hpp"

int main(int argc, char** argv) {
    fspann::jdk::Random r(42);
    const int a = r.nextInt();
    const int b = r.nextInt();
    std::printf("anchors %d %d\n", a, b);
    for (int i = 1; i < argc; i++) {
        char* end = nullptr;
        const long long nq = std::strtoll(argv[i], &end, 10);
        if (!end || *end != ':') { std::fprintf(stderr, "bad pair %s\n", argv[i]); return 2; }
        const long long sample = std::strtoll(end + 1, nullptr, 10);
        const std::vector<int64_t> sel = fspann::jdk::gt_validator_sample(nq, sample);
        std::printf("%lld %lld:", nq, sample);
        for (int64_t v : sel) std::printf(" %lld", static_cast<long long>(v));
        std::printf("\n");
    }
    return 0;
}
