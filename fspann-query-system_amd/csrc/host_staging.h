// host_staging.h — how a host-pointer entry point (fspann_encode / _route / _refine / _refine_store) moves its arguments: ONE
// description of a call's pieces, which sizes the transports, picks one, and places every piece on it.  Plain host code; the
// layouts and the choice (Staging up to pick(), the four *Io structs) call nothing of HIP (tests/cpp/host_staging_check.cpp).
#pragma once
#include "fspann_common.h"

namespace fspann {
namespace {      // (internal linkage, like the api_*.hip.h it serves: one translation unit per binary includes it)

constexpr size_t kPinBytes = size_t(1) << 20;        // the context's pinned block
// Calls of a handful of queries (QueryService.search is one token per call, ForwardSecureANNSystem.java:636): the kernels read their
// arguments from the pinned block and write their results into it THROUGH THE BUS — no copy command either way, one launch sequence and
// one synchronisation (a copy command costs ~8 us of the stream's time whatever its size; a few KB written by the kernel itself cost
// less).  More queries than this go through the block with one copy each way: thousands of scattered 4-byte stores over PCIe do not.
constexpr int64_t kZeroCopyMaxQ = 4;
constexpr size_t a16(size_t x) { return (x + 15) & ~size_t(15); }      // a piece's room (NOT the Carver's 256: the thresholds count these)

enum class Transport {
    Direct,   // one copy command per argument, from and to the caller's memory
    Block,    // packed into the pinned block, one copy command each way
    Mapped    // the kernels read and write the mapped pinned block themselves: "zero copy"
};
struct StagePolicy { bool block, mapped; size_t mapped_up_max; };       // what a call allows; mapped only with at most so many bytes up
struct PinFacts { bool zero_copy, have_block, have_dev_ptr; };          // FSPANN_ZERO_COPY, the pinned block exists, ... and is mapped

struct Staging {
    struct Piece {
        size_t bytes, off;          // off: among the 16-rounded pieces of its way (up | down); Mapped: the way down follows the way up
        int slot;                   // Direct: ws_io[slot].p + slot_off
        size_t slot_off;
        const void* src;            // the way up: the caller's memory
        bool apart;                 // outside the block on every transport: its own copy command straight from the caller's buffer
    };
    struct Out { int piece; size_t off, bytes; void* dst; };            // a part of a piece on the way down, and where the caller wants it
    Piece up[4] = {}, down[3] = {};
    Out outs[5] = {};
    int n_up = 0, n_down = 0, n_out = 0;
    size_t up_bytes = 0, down_bytes = 0;     // the two ways: sums of 16-rounded pieces
    int block_up = 0, block_down = 1;        // Block: the ws_io slots of the two ways
    Transport t = Transport::Direct;

    int add_up(size_t bytes, int slot, const void* src, size_t slot_off = 0, bool apart = false) {
        up[n_up] = {bytes, up_bytes, slot, slot_off, src, apart};
        if (!apart) up_bytes += a16(bytes);
        return n_up++;
    }
    int add_down(size_t bytes, int slot, size_t slot_off = 0) {
        down[n_down] = {bytes, down_bytes, slot, slot_off, nullptr, false};
        down_bytes += a16(bytes);
        return n_down++;
    }
    void out(int piece, void* dst, size_t bytes, size_t off = 0) { if (dst && bytes) outs[n_out++] = {piece, off, bytes, dst}; }
    size_t down_off(int i) const { return (t == Transport::Mapped ? up_bytes : 0) + down[i].off; }      // in the pinned block

    // The choice.  Mapped: both ways fit the block together, a handful of queries (short ways up only where the policy says so: the
    // kernels fetch them over the bus), zero copy on and the block mapped.  Block: each way fits it.
    Transport pick(int64_t nq, StagePolicy p, PinFacts f) const {
        if (p.mapped && up_bytes <= p.mapped_up_max && up_bytes + down_bytes <= kPinBytes && nq <= kZeroCopyMaxQ && f.zero_copy && f.have_block && f.have_dev_ptr)
            return Transport::Mapped;
        if (p.block && up_bytes <= kPinBytes && down_bytes <= kPinBytes && f.have_block) return Transport::Block;
        return Transport::Direct;
    }

    // ---- at work on a context ----
    // the context's pinned block, allocated at the first call whose sizes qualify for it (none to be had: the call goes Direct)
    void choose(fspann_ctx* c, int64_t nq, StagePolicy p) {
        if (!c->h_pin && pick(nq, p, {c->knob_zero_copy, true, true}) != Transport::Direct) {
            void* block = nullptr;
            if (hipHostMalloc(&block, kPinBytes, hipHostMallocDefault) != hipSuccess) { block = nullptr; (void)hipGetLastError(); }
            else if (hipHostGetDevicePointer(&c->d_pin, block, 0) != hipSuccess) { c->d_pin = nullptr; (void)hipGetLastError(); }
            c->h_pin.reset(block);
        }
        t = pick(nq, p, {c->knob_zero_copy, c->h_pin != nullptr, c->d_pin != nullptr});
    }
    unsigned char* pin(const fspann_ctx* c) const { return static_cast<unsigned char*>(c->h_pin.get()); }
    static size_t grown(size_t need, const Piece& p) { return need > p.slot_off + p.bytes ? need : p.slot_off + p.bytes; }
    // device buffers of this transport, then where a piece lives on the device (a piece of no bytes: nowhere)
    int begin(fspann_ctx* c) {
        int rc;
        if (t == Transport::Block && ((rc = ensure(c, c->ws_io[block_up], up_bytes)) || (rc = ensure(c, c->ws_io[block_down], down_bytes)))) return rc;
        for (int slot = 0; slot < 8; slot++) {
            size_t need = 0;
            for (int i = 0; i < n_up; i++) if (up[i].slot == slot && up[i].bytes && (up[i].apart || t == Transport::Direct)) need = grown(need, up[i]);
            for (int i = 0; i < n_down; i++) if (down[i].slot == slot && down[i].bytes && t == Transport::Direct) need = grown(need, down[i]);
            if (need && (rc = ensure(c, c->ws_io[slot], need))) return rc;
        }
        return FSPANN_OK;
    }
    template <typename T> T* dev(const fspann_ctx* c, const Piece& p, size_t block_off, int block_slot) const {
        if (!p.bytes) return nullptr;
        if (t == Transport::Direct || p.apart) return reinterpret_cast<T*>(static_cast<unsigned char*>(c->ws_io[p.slot].p) + p.slot_off);
        return reinterpret_cast<T*>((t == Transport::Mapped ? static_cast<unsigned char*>(c->d_pin) : static_cast<unsigned char*>(c->ws_io[block_slot].p)) + block_off);
    }
    template <typename T> T* dev_up(const fspann_ctx* c, int i) const { return dev<T>(c, up[i], up[i].off, block_up); }
    template <typename T> T* dev_down(const fspann_ctx* c, int i) const { return dev<T>(c, down[i], down_off(i), block_down); }
    // the way up: packed into the block (and, Block, sent by one copy command), or a copy command per piece
    int send(fspann_ctx* c) {
        if (t != Transport::Direct) {
            for (int i = 0; i < n_up; i++) if (!up[i].apart) std::memcpy(pin(c) + up[i].off, up[i].src, up[i].bytes);
            if (t == Transport::Block) FSP_HIP(hipMemcpyAsync(c->ws_io[block_up].p, pin(c), up_bytes, hipMemcpyHostToDevice, c->stream));
        }
        for (int i = 0; i < n_up; i++)
            if (up[i].bytes && (up[i].apart || t == Transport::Direct)) FSP_HIP(hipMemcpyAsync(dev_up<void>(c, i), up[i].src, up[i].bytes, hipMemcpyHostToDevice, c->stream));
        return FSPANN_OK;
    }
    // the way down, behind the launches: Block one copy command into the block (stream order: the way up has been read by then),
    // Direct one per output into the caller's memory, Mapped none.  The caller synchronises, then ...
    int fetch(fspann_ctx* c) {
        if (t == Transport::Block) FSP_HIP(hipMemcpyAsync(pin(c), c->ws_io[block_down].p, down_bytes, hipMemcpyDeviceToHost, c->stream));
        if (t == Transport::Direct)
            for (int o = 0; o < n_out; o++)
                FSP_HIP(hipMemcpyAsync(outs[o].dst, dev_down<unsigned char>(c, outs[o].piece) + outs[o].off, outs[o].bytes, hipMemcpyDeviceToHost, c->stream));
        return FSPANN_OK;
    }
    // ... reads a piece where it landed on the host (Direct: its first output) and hands the outputs over (Direct: they are in place)
    const void* landed(const fspann_ctx* c, int piece) const {
        if (t != Transport::Direct) return pin(c) + down_off(piece);
        for (int o = 0; o < n_out; o++) if (outs[o].piece == piece) return outs[o].dst;
        return nullptr;
    }
    void unpack(const fspann_ctx* c) const {
        if (t != Transport::Direct) for (int o = 0; o < n_out; o++) std::memcpy(outs[o].dst, pin(c) + down_off(outs[o].piece) + outs[o].off, outs[o].bytes);
    }
};

// The four calls.  Pieces in block order; byte counts as the caller counts them (a piece of none takes no room and is never copied).
struct EncodeIo : Staging {          // q | codes | bad | hashes (optional); no Block: a batch's codes go straight to the caller
    enum { Codes, Bad, Hashes };
    static constexpr StagePolicy policy{false, true, SIZE_MAX};
    EncodeIo(const void* q, size_t qb, size_t codes_b, size_t bad_b, size_t hashes_b) {
        add_up(qb, kIoEncQ, q);
        add_down(codes_b, kIoEncCodes); add_down(bad_b, kIoEncBad); add_down(hashes_b, kIoEncHashes);
    }
};
struct RouteIo : Staging {           // codes | ids | scores (always produced) | count, kept, rawSeen
    enum { Ids, Scores, Counts };
    static constexpr StagePolicy policy{true, true, SIZE_MAX};
    RouteIo(const void* codes, size_t codes_b, size_t list_b, size_t counts_b) {
        add_up(codes_b, kIoRouteCodes, codes);
        add_down(list_b, kIoRouteIds); add_down(list_b, kIoRouteScores); add_down(counts_b, kIoRouteCounts);
        block_up = kIoRouteCodes; block_down = kIoRouteIds;
    }
};
struct RefineIo : Staging {          // q | ids | counts | dist | ids | count, scored; the rows apart.  Direct: the three count arrays share a slot
    enum { Q, Rows, CandIds, CandCount };
    enum { Dist, Ids, Counts };
    // Mapped with short lists only: with thousands of candidate ids every chunk's workgroup would fetch its ids over the bus first
    // (SIFT_P4_FAST, B = 8 000: 439 against 405 us per call); the rows always travel by a copy command (a workgroup reading 256 KB
    // over the bus is slow)
    static constexpr StagePolicy policy{true, true, 8192}, store_policy{false, false, 0};
    RefineIo(const void* q, size_t qb, const void* rows, size_t rows_b, const void* ids, size_t ids_b, const void* counts, size_t nb, size_t dist_b, size_t out_ids_b) {
        add_up(qb, kIoRefQ, q); add_up(rows_b, kIoRefRows, rows, 0, true); add_up(ids_b, kIoRefIds, ids); add_up(nb, kIoRefCounts, counts);
        add_down(dist_b, kIoRefOutDist); add_down(out_ids_b, kIoRefOutIds); add_down(2 * nb, kIoRefCounts, nb);
        block_up = kIoRefQ; block_down = kIoRefOutIds;
    }
    // the caller's outputs, in the order their copy commands are issued
    void outputs(int32_t* out_ids, size_t ids_b, double* out_dist, size_t dist_b, int32_t* out_count, int32_t* scored, size_t nb) {
        out(Ids, out_ids, ids_b); out(Dist, out_dist, dist_b); out(Counts, out_count, nb); out(Counts, scored, nb, nb);
    }
};

}  // namespace
}  // namespace fspann
