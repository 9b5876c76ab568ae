// host_staging_check.cpp — the layouts and the transport choice of csrc/host_staging.h as plain host code
// (tests/test_host_staging_cpu.py builds it with AddressSanitizer + UBSan and runs it; no device is touched).  Each of the four
// host-pointer calls is driven with raw byte counts through every combination of nq in {1, 4, 5}, FSPANN_ZERO_COPY on / off, pinned
// block there / missing, block mapped / not; the transport and every piece's offset in the mapped and in the block layout are
// compared with the formulas written out below, which are those of the entry points as they stood before the header existed
// (a(x) = x rounded up to 16, kPin = 1 MiB).
#include "../../fspann-query-system_amd/csrc/host_staging.h"

#include <cstdio>

namespace {

using namespace fspann;
constexpr size_t kPin = size_t(1) << 20;
size_t a(size_t x) { return (x + 15) / 16 * 16; }
size_t mx(size_t x, size_t y) { return x > y ? x : y; }

int checked = 0, wrong = 0;
struct Facts { int64_t nq; bool zc, blk, dev; };
const char* name(Transport t) { return t == Transport::Mapped ? "mapped" : t == Transport::Block ? "block" : "direct"; }

// one case: the transport, the way up's offsets (the same in both layouts) and the way down's offsets, block layout then mapped layout
void expect(const char* call, const char* what, Facts f, Staging& io, StagePolicy pol, Transport want, const size_t* up, int n_up, const size_t* down_block,
            const size_t* down_mapped, int n_down) {
    checked++;
    const Transport got = io.pick(f.nq, pol, {f.zc, f.blk, f.dev});
    bool ok = got == want && io.n_down == n_down;
    int u = 0;
    for (int i = 0; i < io.n_up && ok; i++) {
        if (io.up[i].apart) continue;       // (outside both layouts)
        ok = u < n_up && io.up[i].off == up[u];
        u++;
    }
    ok = ok && u == n_up;
    for (int i = 0; i < n_down && ok; i++) {
        io.t = Transport::Block;
        ok = io.down_off(i) == down_block[i];
        io.t = Transport::Mapped;
        ok = ok && io.down_off(i) == down_mapped[i];
    }
    if (!ok) {
        wrong++;
        std::printf("%s, %s, nq %lld zero_copy %d block %d mapped %d: got %s, want %s (or an offset differs)\n", call, what, static_cast<long long>(f.nq), f.zc, f.blk, f.dev,
                    name(got), name(want));
    }
}

bool zc_ok(Facts f) { return f.nq <= 4 && f.zc && f.blk && f.dev; }

void encode(const char* what, Facts f, size_t qb, size_t cb, size_t hb) {
    const size_t bb = 4 * static_cast<size_t>(f.nq);
    const size_t tot = a(qb) + a(cb) + a(bb) + a(hb);
    const Transport want = (tot <= kPin && zc_ok(f)) ? Transport::Mapped : Transport::Direct;          // never the block
    const size_t up[] = {0}, down_b[] = {0, a(cb), a(cb) + a(bb)}, down_m[] = {a(qb), a(qb) + a(cb), a(qb) + a(cb) + a(bb)};     // q | codes | bad | hashes
    EncodeIo io(nullptr, qb, cb, bb, hb);
    expect("encode", what, f, io, EncodeIo::policy, want, up, 1, down_b, down_m, 3);
}

void route(const char* what, Facts f, size_t cb, size_t ob) {
    const size_t ob_a = a(ob), cnt_a = a(12 * static_cast<size_t>(f.nq));
    const bool block = mx(cb, 2 * ob_a + cnt_a) <= kPin && f.blk;
    const bool mapped = block && a(cb) + 2 * ob_a + cnt_a <= kPin && zc_ok(f);
    const size_t up[] = {0}, down_b[] = {0, ob_a, 2 * ob_a}, down_m[] = {a(cb), a(cb) + ob_a, a(cb) + 2 * ob_a};                  // codes | ids | scores | counts
    RouteIo io(nullptr, cb, ob, 12 * static_cast<size_t>(f.nq));
    expect("route", what, f, io, RouteIo::policy, mapped ? Transport::Mapped : block ? Transport::Block : Transport::Direct, up, 1, down_b, down_m, 3);
}

void refine(const char* what, Facts f, size_t qb, size_t rows_b, size_t ib, size_t ob_d, size_t ob_i, bool store) {
    const size_t nb = 4 * static_cast<size_t>(f.nq);
    const size_t upb = a(qb) + a(ib) + a(nb), downb = a(ob_d) + a(ob_i) + a(2 * nb);
    const bool block = !store && mx(upb, downb) <= kPin && f.blk;                                     // fspann_refine_store: one copy per argument, always
    const bool mapped = block && upb <= 8192 && a(upb) + downb <= kPin && zc_ok(f);
    const size_t up[] = {0, a(qb), a(qb) + a(ib)}, down_b[] = {0, a(ob_d), a(ob_d) + a(ob_i)};        // q | ids | counts (rows apart) | dist | ids | count, scored
    const size_t down_m[] = {a(upb), a(upb) + a(ob_d), a(upb) + a(ob_d) + a(ob_i)};
    RefineIo io(nullptr, qb, nullptr, rows_b, nullptr, ib, nullptr, nb, ob_d, ob_i);
    expect(store ? "refine_store" : "refine", what, f, io, store ? RefineIo::store_policy : RefineIo::policy,
           mapped ? Transport::Mapped : block ? Transport::Block : Transport::Direct, up, 3, down_b, down_m, 3);
}

}  // namespace

int main() {
    for (int64_t nq : {1, 4, 5})
        for (int bits = 0; bits < 8; bits++) {
            const Facts f{nq, (bits & 1) != 0, (bits & 2) != 0, (bits & 4) != 0};
            const size_t n = static_cast<size_t>(nq), bb_a = a(4 * n), cnt_a = a(12 * n), nb2_a = a(8 * n);
            // ---- encode: q, codes, hashes
            encode("small, no hashes (a piece of no bytes)", f, 64 * n, 32 * n, 0);
            encode("sizes that are no multiple of 16", f, 36 * n + 4, 40 * n, 72 * n + 4);
            encode("sum exactly kPin", f, kPin - a(32 * n) - bb_a - a(96 * n), 32 * n, 96 * n);
            encode("sum kPin + 16", f, kPin - a(32 * n) - bb_a - a(96 * n) + 16, 32 * n, 96 * n);
            encode("sum kPin + 16 through one odd byte", f, kPin - a(32 * n) - bb_a - a(96 * n) + 1, 32 * n, 96 * n);
            // ---- route: codes, one list (ids and scores are two of them)
            const size_t cb0 = (kPin - 16 - cnt_a) % 32 == 0 ? 16 : 32;      // so that the two lists share the rest evenly
            const size_t ob_fit = (kPin - cb0 - cnt_a) / 2;
            route("small", f, 32 * n, 256 * n);
            route("a list that is no multiple of 16", f, 32 * n, 4 * 37 * n);
            route("sum exactly kPin", f, cb0, ob_fit);
            route("sum kPin + 16: the block, not mapped", f, cb0 + 16, ob_fit);
            route("codes of kPin bytes: the max test holds, the sum test does not", f, kPin, 256);
            route("codes of kPin + 8 bytes", f, kPin + 8, 256);
            const size_t ob_max = (kPin - cnt_a) / 32 * 16;                   // two lists of whole 16-byte pieces and the counts: kPin or kPin - 16
            route("the largest way down that fits", f, 8, ob_max);
            route("16 bytes more per list", f, 8, ob_max + 16);
            route("cap 140 000: two lists beyond the block", f, 32 * n, 4 * 140000 * n);
            // ---- refine: q, rows (apart), ids, dist, ids out
            for (bool store : {false, true}) {
                refine("small", f, 64 * n, 64 * 64 * n, 256 * n, 80 * n, 40 * n, store);
                refine("sizes that are no multiple of 16", f, 36 * n, 36 * 25 * n, 100 * n, 8 * 3 * n, 4 * 3 * n, store);
                refine("up = 8192", f, 64, 1 << 20, 8192 - 64 - bb_a, 80 * n, 40 * n, store);
                refine("up = 8208", f, 64, 1 << 20, 8208 - 64 - bb_a, 80 * n, 40 * n, store);
                refine("up = 8192, sum exactly kPin", f, 64, 1 << 20, 8192 - 64 - bb_a, kPin - 8192 - a(40 * n) - nb2_a, 40 * n, store);
                refine("up = 8192, sum kPin + 16", f, 64, 1 << 20, 8192 - 64 - bb_a, kPin - 8192 - a(40 * n) - nb2_a + 16, 40 * n, store);
                refine("up exactly kPin", f, 64, 1 << 24, kPin - 64 - bb_a, 80 * n, 40 * n, store);
                refine("up kPin + 16", f, 64, 1 << 24, kPin - 64 - bb_a + 16, 80 * n, 40 * n, store);
                refine("down exactly kPin", f, 64, 1 << 20, 256, kPin - a(40 * n) - nb2_a, 40 * n, store);
                refine("down kPin + 16", f, 64, 1 << 20, 256, kPin - a(40 * n) - nb2_a + 16, 40 * n, store);
            }
        }
    std::printf("%d cases checked, %d wrong\n", checked, wrong);
    return wrong ? 1 : 0;
}
