// api_encode.hip.h — TokenGen / Setup coding entry points: fspann_encode[_dev], the encode path switch (Coding.H / Coding.C, idx/Coding.java:250-301)
// Part of the single translation unit fspann_api.hip (included there, in order); product code, no CPU fallback.
#pragma once
#include "../../include/fspann_encode_kwaves.h"

namespace {

// Grid of an MFMA tile kernel whose blocks take 32 RT rows x 128 CT projections (z: the slices of the split-k kernel)
inline dim3 mfma_tile_grid(int64_t nq, int P, int RT, int CT, int z = 1) {
    return dim3(static_cast<unsigned>((nq + mfma_tile_q(RT) - 1) / mfma_tile_q(RT)), static_cast<unsigned>((P + mfma_tile_p(CT) - 1) / mfma_tile_p(CT)),
                static_cast<unsigned>(z));
}

// Slices of the split-k MFMA encode for a batch of nq rows (1: the unsplit 32 x 128 tile).  FSPANN_ENCODE_SPLITK forces a count; the
// rule otherwise, settled by measurement (tools/encode_bench.py with SPLITK=..., profiles/notes/encode_splitk.txt): split only while
// the slices together stay at or below one block per two CUs, at most four ways, and no slice shorter than four k tiles.  A slice's
// publish / arrive / join is NOT small: per added slice a 256-block grid pays ~40 us (1 024 x 1 024 x 768: 75 us unsplit, 115 / 138 /
// 176 / 274 us at S = 2 / 3 / 4 / 8; 4 096 x 256 x 960: 91 unsplit, 129 / 152 / 185), so a grid that already has a block per CU is
// never split; 512 x 256 x 960 (32 blocks): 75 us unsplit, 65.9 / 62.5 / 60.8 / 64.7 / 65.2 / 74.7 at S = 2 / 3 / 4 / 6 / 8 / 10.
// Either way S <= ceil(d / 32), and S is then lowered to the number of slices that ceil(KT / S) tiles each actually fill, so no
// slice is empty (KT = 4, S = 3: two slices of two tiles).
inline int encode_splitk_slices(const fspann_ctx* c, int64_t nq) {
    const int KT = (c->cfg.dim + kMfmaKT - 1) / kMfmaKT;
    int S = c->knob_encode_splitk;
    if (S <= 0) {
        const dim3 tiles = mfma_tile_grid(nq, c->P_total, 1, 1);
        const int64_t blocks = static_cast<int64_t>(tiles.x) * tiles.y;
        S = static_cast<int>(std::min<int64_t>(4, static_cast<int64_t>(c->num_cus) / (2 * blocks)));
        S = std::min(S, KT / 4);
    }
    S = std::max(1, std::min(S, KT));
    const int per = (KT + S - 1) / S;
    return (KT + per - 1) / per;
}

// The split-k kernel in place of the small tile (S >= 2 slices).  Work area: one arrival counter per 32 x 128 tile (cleared on the
// stream, like the code words), then [tiles][S] slots of one block's partial (16 KB of accumulators + 32 norms + 32 flags).
// launch_tile, here and below: launch_encode_mfma's launcher (kernel, grid, block, LDS bytes, then what follows the 18 common arguments)
template <typename TIn, typename LaunchTile>
int launch_encode_mfma_splitk(fspann_ctx* c, int64_t nq, int S, LaunchTile launch_tile) {
    const int KT = (c->cfg.dim + kMfmaKT - 1) / kMfmaKT, per = (KT + S - 1) / S;
    const dim3 grid = mfma_tile_grid(nq, c->P_total, 1, 1, S);
    const size_t tiles = static_cast<size_t>(grid.x) * grid.y;
    const size_t ctr_bytes = (tiles * 4 + 255) / 256 * 256;
    int rc = ensure(c, c->ws_splitk, ctr_bytes + tiles * S * kSplitSlotBytes);
    if (rc) return rc;
    unsigned* arrive = static_cast<unsigned*>(c->ws_splitk.p);
    FSP_HIP(hipMemsetAsync(arrive, 0, tiles * 4, c->stream));
    launch_tile(encode_mfma_splitk_kernel<TIn>, grid, dim3(256), 0, per, static_cast<unsigned char*>(c->ws_splitk.p) + ctr_bytes, arrive);
    return FSPANN_OK;
}

// The k-wave kernel in place of the small tile: one workgroup of 4 G waves per 32 x 128 tile, the k tiles dealt to its G groups, the
// join in LDS (no work area, nothing to clear).  G = 4 needs 84 352 B of dynamic LDS: the kernel's ceiling is raised once per context.
template <typename TIn, int G, typename LaunchTile>
int launch_encode_mfma_kwave(fspann_ctx* c, int64_t nq, LaunchTile launch_tile) {
    constexpr size_t lds = encode_kwave_lds(G);
    if (lds > 64 * 1024)
        if (int rc = raise_lds_ceiling(c, encode_mfma_kwave_kernel<TIn, G>, lds)) return rc;
    launch_tile(encode_mfma_kwave_kernel<TIn, G>, mfma_tile_grid(nq, c->P_total, 1, 1), dim3(256 * G), lds);
    return FSPANN_OK;
}

// kwaves: k-groups of the k-wave kernel (fspann_set_encode_kwaves; 0 = off), taken ahead of
// splitk: slices of the dimension (encode_splitk_slices); 1 = the unsplit kernels
template <typename TIn>
int launch_encode_mfma(fspann_ctx* c, int64_t nq, const TIn* q_dev, uint64_t* codes_dev, int32_t* hashes_dev, int32_t* bad_dev, int splitk = 1, int kwaves = 0) {
    const int P = c->P_total, d = c->cfg.dim;
    const int64_t cap = std::max<int64_t>(65536, nq * P / 16);
    int rc = ensure(c, c->ws_fix, 256 + static_cast<size_t>(cap) * 8);
    if (rc) return rc;
    unsigned long long* cnt = static_cast<unsigned long long*>(c->ws_fix.p);
    int64_t* list = reinterpret_cast<int64_t*>(static_cast<char*>(c->ws_fix.p) + 256);
    FSP_HIP(hipMemsetAsync(cnt, 0, 8, c->stream));
    // the code words start clear: the MFMA epilogue ORs in the bits of the pairs it can decide, encode_fix_kernel those of the rest
    FSP_HIP(hipMemsetAsync(codes_dev, 0, static_cast<size_t>(nq) * c->TD * c->W * 8, c->stream));
    unsigned long long* cw = reinterpret_cast<unsigned long long*>(codes_dev);
    // an MFMA tile kernel: the 18 arguments they all begin with, then the kernel's own
    auto launch_tile = [&](auto kernel, dim3 grid, dim3 block, size_t lds, auto... extra) {
        hipLaunchKernelGGL(kernel, grid, block, lds, c->stream, q_dev, nq, d, c->fam->d_alphaT32.get(), c->fam->d_r.get(), c->fam->d_omega.get(), P, c->cfg.m,
                           c->cfg.lambda, c->W, c->TD, hashes_dev, cw, bad_dev, list, cap, cnt, c->fam->alpha_norm_max, extra...);
    };
    // block tile: 64 x 256 for bulk coding (Setup: hundreds of thousands of rows per call); 32 x 128 with tiles in flight for batches
    // of up to a few thousand blocks of the large tile (8 192 x 1 024 x 768: 273 against 327 us; equal at 262 144 rows)
    const int64_t big_blocks = ((nq + 63) / 64) * ((P + 255) / 256);
    if (kwaves == 2 || kwaves == 4) {
        rc = (kwaves == 2) ? launch_encode_mfma_kwave<TIn, 2>(c, nq, launch_tile) : launch_encode_mfma_kwave<TIn, 4>(c, nq, launch_tile);
        if (rc) return rc;
    } else if (splitk > 1) {
        if ((rc = launch_encode_mfma_splitk<TIn>(c, nq, splitk, launch_tile))) return rc;
    } else if (big_blocks >= 16 * static_cast<int64_t>(c->num_cus) && c->knob_mfma_tile != 1) {
        launch_tile(encode_mfma_kernel<TIn, 2, 2>, mfma_tile_grid(nq, P, 2, 2), dim3(256), 0);
    } else {
        launch_tile(encode_mfma_kernel<TIn, 1, 1>, mfma_tile_grid(nq, P, 1, 1), dim3(256), 0);
    }
    FSP_HIP(hipGetLastError());
    // (a wave per kFixG pairs: as many blocks as the list can need, at most four per CU — the waves stride over the tasks)
    const int64_t fix_blocks = std::min<int64_t>(static_cast<int64_t>(c->num_cus) * 4, (cap + kFixG * 4 - 1) / (kFixG * 4));
    hipLaunchKernelGGL((encode_fix_kernel<TIn>), dim3(static_cast<unsigned>(std::max<int64_t>(1, fix_blocks))), dim3(256), 0, c->stream,
                       q_dev, d, c->fam->d_alpha_rows.get(), c->fam->d_r.get(), c->fam->d_omega.get(), P, c->cfg.m, c->cfg.lambda, c->W, c->TD, list, cnt, cap, hashes_dev, cw);
    FSP_HIP(hipGetLastError());
    c->fix_cap_last = static_cast<unsigned long long>(cap);
    return 1;  // caller enqueues the exact kernel guarded by (count > cap): it only runs if the list overflowed
}

template <typename TIn>
int launch_encode(fspann_ctx* c, int64_t nq, const TIn* q_dev, uint64_t* codes_dev, int32_t* hashes_dev,
                  int32_t* bad_dev, double* proj_dev = nullptr) {
    const int m = c->cfg.m;
    const unsigned long long* guard = nullptr;
    unsigned long long guard_cap = 0;
    // auto: the MFMA pre-filter pays from ~5e8 multiply-adds per call (its fixed part: clearing the code words, the exact re-check of the
    // pairs on a bucket edge, four launches).  tools/encode_bench.py, exact vs MFMA: 1 024 x 256 x 128 12 / 31 us, 512 x 256 x 960
    // 48 / 75, 1 024 x 1 024 x 768 132 / 77, 4 096 x 256 x 960 169 / 94, 8 192 x 1 024 x 768 758 / 273, 262 144 x 256 x 128 1 080 / 502.
    // With the split-k kernel (mode 3, exact / MFMA / split-k under its rule, medians of three rounds): 512 x 256 x 960 48 / 75 / 61
    // (S = 4), 1 024 x 1 024 x 768 130 / 75 / 75 (not split), 4 096 x 256 x 960 162 / 91 / 91 (not split).  The split beats the
    // unsplit MFMA path only where the exact kernel beats both, so auto never takes it: mode 3 is opt-in.
    const bool want_mfma = (c->encode_mode == 2) || (c->encode_mode == 3) ||
                           (c->encode_mode == 0 && static_cast<double>(nq) * c->P_total * c->cfg.dim >= 5.0e8);
    if (want_mfma && !proj_dev && c->fam->d_alphaT32.get() && c->W <= 3) {      // (the fused bit-pack epilogue carries three code words: <= 192 bits)
        // mode 3: the dimension split over workgroups where encode_splitk_slices asks for it — query batches only, never Setup's coding
        // (a build in progress: hundreds of thousands of rows per call fill the chip unsplit)
        const int splitk = (c->encode_mode == 3 && c->bld_done < 0) ? encode_splitk_slices(c, nq) : 1;
        // the k-wave kernel (fspann_set_encode_kwaves, opt-in): only where mode 2 or 3 chose this path (never auto), for query batches, and
        // with at least two k tiles to deal out; it goes ahead of mode 3's split over workgroups
        const int kwaves = (c->encode_mode != 0 && c->bld_done < 0 && c->cfg.dim > kMfmaKT) ? c->encode_kwaves : 0;
        c->kwaves_last = 0;
        int rc = launch_encode_mfma<TIn>(c, nq, q_dev, codes_dev, hashes_dev, bad_dev, splitk, kwaves);
        if (rc <= 0) return rc;  // error
        c->kwaves_last = kwaves;
        // the list can only overflow when almost every pair sits on a bucket boundary (degenerate omega): the
        // exact kernel below is enqueued with a device-side guard and returns immediately otherwise.
        guard = static_cast<const unsigned long long*>(c->ws_fix.p);
        guard_cap = c->fix_cap_last;
        c->mfma_last = true;
    } else {
        c->mfma_last = false;
        c->kwaves_last = 0;
    }
    const int tdPerBlock = std::max(1, kEncThreads / m);
    const int gy = (c->TD + tdPerBlock - 1) / tdPerBlock;
    const EncodeArgs<TIn> ea{q_dev, nq, c->cfg.dim, c->fam->d_alphaT.get(), c->fam->d_r.get(), c->fam->d_omega.get(), c->P_total, m, c->cfg.lambda, c->W, c->TD, tdPerBlock,
                             codes_dev, hashes_dev, bad_dev, proj_dev, guard, guard_cap, c->dbg_route};
    // QB queries per block: 8 for bulk coding (index build), 4 for query batches so that
    // a 1024-query batch still fills 256 CUs.
    bool launched = false;
    if constexpr (sizeof(TIn) == 4) {
        // two rows per workgroup when four would leave CUs without one (BASELINE config #3's shard: 512 queries x 256 projections = 128
        // workgroups of four rows: 59.8 -> 48.4 us); FSPANN_ENCODE_QB forces 1 / 2 / 4 / 8 (dev A/B)
        int qb_env = c->knob_encode_qb;
        if (qb_env == 0 && nq >= 2 && ((nq + 3) / 4) * static_cast<int64_t>(gy) < c->num_cus) qb_env = 2;
        if (qb_env == 1 || qb_env == 2) {
            if (qb_env == 1) hipLaunchKernelGGL((encode_exact_kernel<TIn, 1>), dim3(static_cast<unsigned>(nq), gy), dim3(kEncThreads), 0, c->stream, ea);
            else hipLaunchKernelGGL((encode_exact_kernel<TIn, 2>), dim3(static_cast<unsigned>((nq + 1) / 2), gy), dim3(kEncThreads), 0, c->stream, ea);
            launched = true;
        }
    }
    if constexpr (sizeof(TIn) == 4) {       // (8 fp64 query rows per block do not fit the register budget)
        if (!launched && (nq >= 8192 || c->knob_encode_qb == 8)) {
            constexpr int QB = 8;
            hipLaunchKernelGGL((encode_exact_kernel<TIn, QB>), dim3(static_cast<unsigned>((nq + QB - 1) / QB), gy), dim3(kEncThreads), 0, c->stream, ea);
            launched = true;
        }
    }
    if (!launched) {
        // 4 rows per workgroup = 256 workgroups for a 1024-query batch.  Every workgroup reads all of alpha (256 KB) from L2:
        // fewer rows per workgroup (2: 12.8 us, 1: 20 us) cost more in that traffic than the extra waves per SIMD buy, and the
        // loop itself is bound by one dependent fp64 instruction per ~10 cycles of a lone wave (7.8 of 11.4 us, tools/encode_stamps.py).
        constexpr int QB = 4;
        hipLaunchKernelGGL((encode_exact_kernel<TIn, QB>), dim3(static_cast<unsigned>((nq + QB - 1) / QB), gy), dim3(kEncThreads), 0, c->stream, ea);
    }
    FSP_HIP(hipGetLastError());
    return FSPANN_OK;
}

}  // namespace

extern "C" {

// ---- encode -----------------------------------------------------------------------
int fspann_encode_dev(fspann_ctx* c, int64_t nq, const void* q_dev, int dtype, uint64_t* codes_dev,
                      int32_t* hashes_dev, int32_t* bad_dev) {
    CHECK_CTX(c);
    if (!c->fam->have_g) return fail(FSPANN_E_STATE, "GFunctionRegistry not initialized. Build index first.");
    if (nq < 0) return fail(FSPANN_E_ARG, "nq < 0");
    if (nq == 0) return FSPANN_OK;
    if (!q_dev || !codes_dev) return fail(FSPANN_E_NULL, "query vector is null");
    if (dtype == FSPANN_F64) return launch_encode<double>(c, nq, static_cast<const double*>(q_dev), codes_dev, hashes_dev, bad_dev);
    if (dtype == FSPANN_F32) return launch_encode<float>(c, nq, static_cast<const float*>(q_dev), codes_dev, hashes_dev, bad_dev);
    if (int rc = refuse_row_only(dtype, "dtype")) return rc;
    return fail(FSPANN_E_ARG, "unknown dtype %d", dtype);
}

int fspann_encode(fspann_ctx* c, int64_t nq, const void* q, int dtype, uint64_t* codes, int32_t* hashes) {
    CHECK_CTX(c);
    if (!c->fam->have_g) return fail(FSPANN_E_STATE, "GFunctionRegistry not initialized. Build index first.");
    if (nq < 0) return fail(FSPANN_E_ARG, "nq < 0");
    if (nq == 0) return FSPANN_OK;
    if (!q || !codes) return fail(FSPANN_E_NULL, "query vector is null");
    if (int rc = refuse_row_only(dtype, "dtype")) return rc;
    if (dtype != FSPANN_F32 && dtype != FSPANN_F64) return fail(FSPANN_E_ARG, "unknown dtype %d", dtype);
    const size_t esz = dtype == FSPANN_F64 ? 8 : 4;
    const size_t cb = static_cast<size_t>(nq) * c->TD * c->W * 8, bb = static_cast<size_t>(nq) * 4;
    const size_t hb = hashes ? static_cast<size_t>(nq) * c->P_total * 4 : 0;
    return guarded([&]() -> int {
    // a handful of queries (QueryTokenFactory.create is one vector per call): through the mapped pinned block, no copy commands
    EncodeIo io(q, static_cast<size_t>(nq) * c->cfg.dim * esz, cb, bb, hb);
    io.choose(c, nq, EncodeIo::policy);
    std::vector<int32_t> bad_direct(io.t == Transport::Direct ? static_cast<size_t>(nq) : 0);
    io.out(EncodeIo::Codes, codes, cb); io.out(EncodeIo::Bad, io.t == Transport::Direct ? bad_direct.data() : nullptr, bb); io.out(EncodeIo::Hashes, hashes, hb);
    int rc;
    if ((rc = io.begin(c)) || (rc = io.send(c))) return rc;
    rc = fspann_encode_dev(c, nq, io.dev_up<void>(c, 0), dtype, io.dev_down<uint64_t>(c, EncodeIo::Codes), io.dev_down<int32_t>(c, EncodeIo::Hashes),
                           io.dev_down<int32_t>(c, EncodeIo::Bad));
    if (rc || (rc = io.fetch(c))) return rc;
    FSP_HIP(hipStreamSynchronize(c->stream));
    const int32_t* bad = static_cast<const int32_t*>(io.landed(c, EncodeIo::Bad));
    for (int64_t i = 0; i < nq; i++)
        if (bad[i]) return fail(FSPANN_E_ARG, "Vector contains NaN/Inf (query %lld)", (long long)i);  // Coding.java:360
    io.unpack(c);
    return FSPANN_OK;
    });
}

// Encode path selection: 0 = auto (MFMA pre-filter from 5e8 multiply-adds per call — rows x projections x dim —, exact fp64 below),
// 1 = exact fp64 VALU only, 2 = always MFMA fp32 GEMM + exact re-check, 3 = as 2 with the dimension split over workgroups for batches
// that leave CUs idle (encode_mfma_splitk_kernel; where the MFMA path is not eligible it falls back like 2).  All modes produce
// bit-identical hashes and codes.
int fspann_set_encode_mode(fspann_ctx* c, int mode) {
    if (!c) return fail(FSPANN_E_NULL, "ctx is null");
    if (mode < 0 || mode > 3) return fail(FSPANN_E_ARG, "encode mode must be 0, 1, 2 or 3");
    c->encode_mode = mode;
    return FSPANN_OK;
}
// include/fspann_encode_kwaves.h: the k-groups of the k-wave MFMA encode (encode_mfma_kwave_kernel), 0 = off.  It applies where mode
// 2 or 3 chose the MFMA path for a query batch of at least two k tiles (launch_encode); every mode stays bit-identical.
int fspann_set_encode_kwaves(fspann_ctx* c, int groups) {
    CHECK_CTX(c);
    if (groups != 0 && groups != 2 && groups != 4) return fail(FSPANN_E_ARG, "encode k-groups must be 0, 2 or 4");
    c->encode_kwaves = groups;
    return FSPANN_OK;
}
// k-groups the last encode call ran with (0: it ran another kernel)
int fspann_last_encode_kwaves(fspann_ctx* c) {
    CHECK_CTX(c);
    return c->kwaves_last;
}
// (query, projection) pairs the last MFMA-path encode re-checked with the exact kernel (0 for the exact path).
int64_t fspann_last_encode_rechecked(fspann_ctx* c) {
    if (!c) return FSPANN_E_NULL;
    if (!c->mfma_last || !c->ws_fix.p) return 0;
    unsigned long long n = 0;
    if (hipSetDevice(c->device) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess ||
        hipMemcpy(&n, c->ws_fix.p, 8, hipMemcpyDeviceToHost) != hipSuccess) return FSPANN_E_DEVICE;
    return static_cast<int64_t>(n);
}

}  // extern "C"
