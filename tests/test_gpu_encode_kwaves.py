"""GPU: the k-wave MFMA encode (set_encode_kwaves(G) under encode mode 2: the k tiles of one 32 x 128 tile dealt to G groups of
four waves in one workgroup, partials joined in LDS) gives the oracle's sequential fp64 hashes and codes bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _setup(pkg, oracle, T, D, m, lam, d, seed, G):
    rng = np.random.default_rng(seed)
    S = rng.standard_normal((1000, d)).astype(np.float32).astype(np.float64)
    alpha, r, w = oracle.registry_init(S, m, 13, T, D)
    o = oracle.Oracle(T, D, m, lam, d)
    o.set_gfunctions(alpha, r, w)
    ctx = pkg.FspannContext(pkg.PaperRuntimeConfig(tables=T, divisions=D, m=m, lambda_=lam, dim=d), 0)
    ctx.set_gfunctions(alpha, r, w)
    ctx.set_encode_mode(2)
    ctx.set_encode_kwaves(G)                                     # the parent commit has no such call: every test of this file fails here
    return rng, o, ctx, (alpha, r, w)


@pytest.mark.parametrize("G", [2, 4])
@pytest.mark.parametrize("T,D,m,lam,d,nq,runs", [
    (3, 2, 24, 2, 100, 333, True),     # d % 32 != 0, four k tiles; P = 144: a second, partial block of projections; partial last row tile
    (1, 1, 1, 1, 150, 5, True),        # five k tiles: uneven lists, groups idle in the last trip; five rows, one projection
    (3, 1, 7, 3, 33, 70, True),        # two k tiles: at G = 4 two groups run on zeros only; P = 21, P % 4 != 0
    (2, 1, 100, 1, 64, 65, True),      # P = 200, two code words
    (2, 1, 60, 3, 64, 65, True),       # three code words
    (2, 1, 100, 2, 64, 65, False),     # four code words: not eligible
    (8, 1, 8, 2, 960, 200, True),      # BASELINE config #3's dimension: 30 k tiles
    (2, 1, 8, 2, 16, 9, False),        # one k tile: nothing to split, the unsplit kernel runs
])
def test_kwaves_equals_oracle(pkg, oracle, G, T, D, m, lam, d, nq, runs):
    rng, o, ctx, _ = _setup(pkg, oracle, T, D, m, lam, d, T * 7 + d, G)
    with ctx:
        for dt in (np.float32, np.float64):
            Q = (rng.standard_normal((nq, d)) * 2).astype(dt)
            ref_h, ref_c = o.hashes(Q.astype(np.float64)), o.encode(Q.astype(np.float64))
            c2, h2 = ctx.encode(Q, want_hashes=True)
            ran, n_fix = ctx.last_encode_kwaves(), ctx.last_encode_rechecked()
            c3 = ctx.encode(Q)                                   # without the hashes output buffer
            assert np.array_equal(h2, ref_h) and np.array_equal(c2, ref_c) and np.array_equal(c3, ref_c)
            assert ran == (G if runs else 0) and ctx.last_encode_kwaves() == ran
            assert n_fix < 0.01 * h2.size + 8, n_fix            # the guard band is narrow on ordinary data


def test_kwaves_band_uses_whole_row_norm(pkg, oracle):
    """Rows on bucket edges whose k tiles 0 and 2 (groups 0 and 2 at G = 4) are 1e-3 of the others: a guard band taken from one
    group's norm would be a thousand times too narrow.  A constructed pair MUST be re-checked when its distance to the edge is
    under half the band: the fp32 sum is within the band of the exact one by the kernel's own bound, so the edge lies inside
    its interval."""
    T, D, m, lam, d = 4, 1, 16, 2, 128
    rng, o, ctx, (alpha, r, w) = _setup(pkg, oracle, T, D, m, lam, d, 99, 4)
    with ctx:
        rows, must = [], 0
        for i in range(400):
            v = rng.standard_normal(d)
            v[:32] *= 1e-3
            v[64:96] *= 1e-3
            p = rng.integers(0, T * D * m)
            y = float(np.dot(v, alpha.reshape(-1, d)[p]))
            kbucket = rng.integers(-3, 4)
            eps = rng.choice([0.0, 1e-12, -1e-12, 1e-9, -1e-9, 1e-7, -1e-7, 3e-6, -3e-6])
            target = (kbucket + eps) * w.reshape(-1)[p] - r.reshape(-1)[p]
            if abs(y) > 1e-3:
                v = v * (target / y)
                must += abs(eps) * w.reshape(-1)[p] < 0.5 * (d + 4) * 2.0 ** -24 * np.linalg.norm(v)
            rows.append(v)
        Q = np.array(rows)
        c2, h2 = ctx.encode(Q, want_hashes=True)
        n_fix = ctx.last_encode_rechecked()
        print("constructed pairs that must be re-checked:", must, "re-checked:", n_fix)
        assert ctx.last_encode_kwaves() == 4
        assert must >= 200 and n_fix >= must
        assert np.array_equal(h2, o.hashes(Q)) and np.array_equal(c2, o.encode(Q))


def test_kwaves_flags_and_ranges_cross_groups(pkg, oracle):
    T, D, m, lam, d = 2, 1, 8, 2, 128                            # four k tiles, one per group at G = 4
    rng, o, ctx, _ = _setup(pkg, oracle, T, D, m, lam, d, 6, 4)
    with ctx:
        Q = rng.standard_normal((9, d))
        Q[2, 70] = 1e200       # group 2's tile: overflows fp32 -> re-checked exactly, int32 saturation
        Q[3] *= 1e-200         # underflows fp32
        c2, h2 = ctx.encode(Q, want_hashes=True)
        assert ctx.last_encode_kwaves() == 4
        assert np.array_equal(h2, o.hashes(Q)) and np.array_equal(c2, o.encode(Q))
        Q[5, 100] = np.nan     # group 3's tile only
        with pytest.raises(pkg.FspannArgumentError, match="NaN/Inf"):
            ctx.encode(Q)


def test_kwaves_knob(pkg, oracle):
    T, D, m, lam, d = 3, 2, 24, 2, 100
    rng, o, ctx, _ = _setup(pkg, oracle, T, D, m, lam, d, 11, 2)
    with ctx:
        for groups in (3, 8, -1):
            with pytest.raises(pkg.FspannArgumentError):
                ctx.set_encode_kwaves(groups)
        Qa, Qb = rng.standard_normal((70, d)), rng.standard_normal((333, d))
        first, second, third = ctx.encode(Qa), ctx.encode(Qb), ctx.encode(Qa)      # no state is carried between calls
        assert ctx.last_encode_kwaves() == 2                                       # (the refused values changed nothing)
        assert np.array_equal(first, o.encode(Qa)) and np.array_equal(second, o.encode(Qb)) and np.array_equal(third, first)
        ctx.set_encode_kwaves(0)
        assert np.array_equal(ctx.encode(Qa), first) and ctx.last_encode_kwaves() == 0
