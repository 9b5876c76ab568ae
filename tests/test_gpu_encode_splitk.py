"""GPU: the split-k MFMA encode (encode mode 3: the dimension divided over workgroups, partials joined by the last block to
arrive) gives the oracle's sequential fp64 hashes and codes bit for bit.  FSPANN_ENCODE_SPLITK forces the number of slices, so
the join is reached at small dimensions."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _setup(pkg, oracle, T, D, m, lam, d, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    S = (rng.standard_normal((1000, d)) * scale).astype(np.float32).astype(np.float64)
    alpha, r, w = oracle.registry_init(S, m, 13, T, D)
    o = oracle.Oracle(T, D, m, lam, d)
    o.set_gfunctions(alpha, r, w)
    ctx = pkg.FspannContext(pkg.PaperRuntimeConfig(tables=T, divisions=D, m=m, lambda_=lam, dim=d), 0)
    ctx.set_gfunctions(alpha, r, w)
    return rng, o, ctx, (alpha, r, w)


def _split(monkeypatch, pkg, oracle, T, D, m, lam, d, seed, slices):
    monkeypatch.setenv("FSPANN_ENCODE_SPLITK", str(slices))      # read once, when the context is made
    rng, o, ctx, g = _setup(pkg, oracle, T, D, m, lam, d, seed)
    ctx.set_encode_mode(3)                                       # the parent commit refuses mode 3: every test of this file fails here
    return rng, o, ctx, g


@pytest.mark.parametrize("T,D,m,lam,d,nq,slices", [
    (3, 2, 24, 2, 100, 333, 2),    # d % 32 != 0, last slice 36 of 64 dimensions; P = 144: a second, partial block of projections
    (3, 2, 24, 2, 100, 70, 3),     # four k tiles in three slices: two slices of two tiles
    (1, 1, 1, 1, 150, 5, 3),       # five k tiles as 2 + 2 + 1; five rows, one projection
    (3, 1, 7, 3, 33, 70, 8),       # more slices than k tiles: clamped to two, the last one dimension long; P = 21, P % 4 != 0
    (2, 1, 100, 1, 64, 65, 2),     # P = 200, two code words
    (2, 1, 60, 3, 64, 65, 2),      # three code words
    (2, 1, 100, 2, 64, 65, 2),     # four code words: not eligible, falls back like mode 2
    (8, 1, 8, 2, 960, 200, 8),     # BASELINE config #3's dimension: 30 k tiles in eight slices
])
def test_splitk_equals_oracle(monkeypatch, pkg, oracle, T, D, m, lam, d, nq, slices):
    rng, o, ctx, _ = _split(monkeypatch, pkg, oracle, T, D, m, lam, d, T * 7 + d, slices)
    with ctx:
        for dt in (np.float32, np.float64):
            Q = (rng.standard_normal((nq, d)) * 2).astype(dt)
            ref_h, ref_c = o.hashes(Q.astype(np.float64)), o.encode(Q.astype(np.float64))
            c2, h2 = ctx.encode(Q, want_hashes=True)
            c3 = ctx.encode(Q)                                   # without the hashes output buffer
            n_fix = ctx.last_encode_rechecked()
            assert np.array_equal(h2, ref_h) and np.array_equal(c2, ref_c) and np.array_equal(c3, ref_c)
            assert n_fix < 0.01 * h2.size + 8, n_fix            # the guard band is narrow on ordinary data


def test_splitk_band_uses_whole_row_norm(monkeypatch, pkg, oracle):
    """Rows on bucket edges whose first 32 dimensions (slice 0) are 1e-3 of the last 32 (slice 1): a guard band taken from one
    slice's norm would be a thousand times too narrow whenever slice 0 arrives last.  A constructed pair MUST be re-checked when
    its distance to the edge is under half the band: the fp32 sum is within the band of the exact one by the kernel's own bound
    (and within a tenth of it in practice, sqrt(d) against d roundings), so the edge lies inside its interval."""
    T, D, m, lam, d = 4, 1, 16, 2, 64
    rng, o, ctx, (alpha, r, w) = _split(monkeypatch, pkg, oracle, T, D, m, lam, d, 99, 2)
    with ctx:
        rows, must = [], 0
        for i in range(400):
            v = rng.standard_normal(d)
            v[:32] *= 1e-3
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
        assert must >= 200 and n_fix >= must
        assert np.array_equal(h2, o.hashes(Q)) and np.array_equal(c2, o.encode(Q))


def test_splitk_flags_cross_slices(monkeypatch, pkg, oracle):
    T, D, m, lam, d = 2, 1, 8, 2, 96                              # three slices of one k tile
    rng, o, ctx, _ = _split(monkeypatch, pkg, oracle, T, D, m, lam, d, 6, 3)
    with ctx:
        Q = rng.standard_normal((9, d))
        Q[2, 40] = 1e200       # middle slice: overflows fp32 -> re-checked exactly, int32 saturation
        Q[3] *= 1e-200         # underflows fp32
        c2, h2 = ctx.encode(Q, want_hashes=True)
        assert np.array_equal(h2, o.hashes(Q)) and np.array_equal(c2, o.encode(Q))
        Q[5, 90] = np.nan      # last slice only
        with pytest.raises(pkg.FspannArgumentError, match="NaN/Inf"):
            ctx.encode(Q)


def test_splitk_counters_are_rearmed(monkeypatch, pkg, oracle):
    T, D, m, lam, d = 3, 2, 24, 2, 100
    rng, o, ctx, _ = _split(monkeypatch, pkg, oracle, T, D, m, lam, d, 11, 2)
    with ctx:
        Qa, Qb = rng.standard_normal((70, d)), rng.standard_normal((333, d))
        first, second, third = ctx.encode(Qa), ctx.encode(Qb), ctx.encode(Qa)
        assert np.array_equal(first, o.encode(Qa)) and np.array_equal(second, o.encode(Qb)) and np.array_equal(third, first)


def test_encode_mode_3_accepted_4_refused(pkg, oracle):
    _, _, ctx, _ = _setup(pkg, oracle, 2, 1, 8, 2, 16, seed=1)
    with ctx:
        ctx.set_encode_mode(3)
        with pytest.raises(pkg.FspannArgumentError, match="0, 1, 2 or 3"):
            ctx.set_encode_mode(4)
