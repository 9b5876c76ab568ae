// java_random.hpp — host model of java.util.Random (the 48-bit LCG of the class itself, JDK 8 .. 21) and of the sample
// GroundtruthValidator.validate draws with it (api/.../GroundtruthValidator.java:112-123).
// Product code (pure host C++17, no HIP): fspann_gt_validator_sample and fspann_gt_validate_dev take the sample from here.
//
//   Random rnd = new Random(42); Set<Integer> sampled = new HashSet<>();
//   while (sampled.size() < effectiveSample) sampled.add(rnd.nextInt(queries.size()));
//   for (int queryIdx : sampled) ...
//
// What is modelled: the seed scramble (seed ^ 0x5DEECE66D) & (2^48 - 1), next(bits), nextInt() and both branches of
// nextInt(bound) (a power-of-two bound takes the high bits of one draw; any other bound runs the rejection loop, whose test
// `u - r + m < 0` is an int overflow).  The set is java.util.HashMap behind HashSet: Integer.hashCode is the value, the table
// starts at 16 with load factor 0.75 and grows as values arrive, and the iteration order is HashMapModel's (java_hashmap.hpp).
// Distinct Integers have distinct hashCodes and the spread h ^ (h >>> 16) is a bijection, so a tree bin never has to order two
// keys of equal hash: KeyOrder is never asked, and a bin that treeifies is walked in the right order by construction.
#pragma once
#include <cstdint>
#include <vector>

#include "java_hashmap.hpp"

namespace fspann {
namespace jdk {

class Random {
  public:
    explicit Random(int64_t seed) : seed_((static_cast<uint64_t>(seed) ^ kMul) & kMask) {}
    // Random.next(bits): the top `bits` bits of the advanced 48-bit state, as a Java int
    int32_t next(int bits) {
        seed_ = (seed_ * kMul + 0xBull) & kMask;
        return static_cast<int32_t>(static_cast<uint32_t>(seed_ >> (48 - bits)));
    }
    int32_t nextInt() { return next(32); }
    // Random.nextInt(bound), bound > 0
    int32_t nextInt(int32_t bound) {
        int32_t r = next(31);
        const int32_t m = bound - 1;
        if ((bound & m) == 0) return static_cast<int32_t>((static_cast<int64_t>(bound) * static_cast<int64_t>(r)) >> 31);
        // for (int u = r; u - (r = u % bound) + m < 0; u = next(31));   — the sum wraps like a Java int
        for (int32_t u = r;; u = next(31)) {
            r = u % bound;
            const uint32_t s = static_cast<uint32_t>(u) - static_cast<uint32_t>(r) + static_cast<uint32_t>(m);
            if (static_cast<int32_t>(s) >= 0) break;
        }
        return r;
    }

  private:
    static constexpr uint64_t kMul = 0x5DEECE66Dull, kMask = (1ull << 48) - 1;
    uint64_t seed_;
};

struct IntegerOrder {      // Integer.compareTo (a tree bin would ask it for two keys of equal hash: there are none)
    int operator()(int32_t a, int32_t b) const { return a < b ? -1 : (a > b ? 1 : 0); }
};

// The validator's sample of min(sample_size, nq) query indices, in the HashSet's iteration order.  0 < nq < 2^31 or the list is
// empty; sample_size <= 0: empty.
inline std::vector<int64_t> gt_validator_sample(int64_t nq, int64_t sample_size) {
    std::vector<int64_t> out;
    if (nq <= 0 || nq > INT32_MAX || sample_size <= 0) return out;
    const int64_t want = sample_size < nq ? sample_size : nq;
    HashMapModel<IntegerOrder> set(16, IntegerOrder{});      // new HashMap<>(): the first put allocates 16 bins, threshold 12
    set.reserve(static_cast<size_t>(want));
    Random rnd(42);
    const int32_t bound = static_cast<int32_t>(nq);
    while (set.size() < want) {
        const int32_t v = rnd.nextInt(bound);
        set.put(v, v, 0);                                    // HashSet.add: map.put(e, PRESENT); Integer.hashCode() is the value
    }
    out.reserve(static_cast<size_t>(want));
    set.for_each([&](int32_t key, int64_t) { out.push_back(key); });
    return out;
}

}  // namespace jdk
}  // namespace fspann
