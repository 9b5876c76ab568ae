"""GPU, full size: exact ground truth over 1 M x 128 SIFT-like BYTES (fspann_groundtruth_typed_dev, FSPANN_U8 base and queries)
for 1 024 byte queries, k = 100, against the oracle over the same values as float32 — ids and squared distances of every
query — and fspann_eval_metrics_typed_dev of that ground truth against itself (recall 1 everywhere)."""
import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.fullsize]


def siftlike(rng, n, d, r=16, noise=6.0):
    """bench.py's SIFT-like generator (integers 0..255 of intrinsic dimension r), as tests/test_gpu_u8_fullsize.py has it."""
    U = (rng.standard_normal((r, d)) / np.sqrt(r)).astype(np.float32)
    def draw(cnt):
        y = rng.standard_normal((cnt, r), dtype=np.float32) @ U
        return np.clip(np.rint(np.float32(64.0) + np.float32(48.0) * y + np.float32(noise) * rng.standard_normal((cnt, d), dtype=np.float32)), 0, 255).astype(np.float32)
    return draw


def test_sift_1m_bytes_groundtruth_and_metrics(pkg, oracle):
    import torch
    dev = torch.device("cuda", 0)
    N = pkg._native
    n, d, nq, k = 1_000_000, 128, 1024, 100
    rng = np.random.default_rng(1)
    draw = siftlike(rng, n, d)
    X8 = draw(n).astype(np.uint8)
    dst = rng.choice(n, 1000, replace=False)
    X8[dst] = X8[rng.integers(0, n, 1000)]                    # 1 000 rows are copies of other rows: exact ties
    Q8 = draw(nq).astype(np.uint8)
    Q8[:24] = X8[rng.integers(0, n, 24)]                      # 24 queries are base rows: distance 0
    with pkg.FspannContext(pkg.PaperRuntimeConfig(tables=1, divisions=1, m=4, lambda_=2, dim=d), 0) as ctx:
        xd, qd = torch.from_numpy(X8).to(dev), torch.from_numpy(Q8).to(dev)
        ids = torch.full((nq, k), -7, dtype=torch.int32, device=dev)
        d2 = torch.full((nq, k), -7.0, dtype=torch.float64, device=dev)
        rec = torch.zeros(nq, dtype=torch.float64, device=dev)
        rat = torch.zeros(nq, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        ctx.groundtruth_typed_dev(n, xd.data_ptr(), N.U8, nq, qd.data_ptr(), N.U8, d, k, ids.data_ptr(), d2.data_ptr())
        ctx.eval_metrics_typed_dev(n, xd.data_ptr(), N.U8, nq, qd.data_ptr(), N.U8, d, k, ids.data_ptr(), k, 0, ids.data_ptr(), k,
                                   rec.data_ptr(), rat.data_ptr())
        ctx.sync()
        ids, d2, rec, rat = ids.cpu().numpy(), d2.cpu().numpy(), rec.cpu().numpy(), rat.cpu().numpy()
    ref_ids, ref_d2 = oracle.groundtruth(X8.astype(np.float32), Q8.astype(np.float32), k)
    bad = np.flatnonzero((ids != ref_ids).any(1) | (d2 != ref_d2).any(1))
    assert bad.size == 0, (bad.size, bad[:8])
    assert (d2[:24, 0] == 0).all()
    assert (rec == 1.0).all()
    ok = ~np.isnan(rat)                                       # a query that IS a base row has d(q, gt_0) = 0: the reference's NaN
    assert not ok[:24].any() and (rat[ok] == 1.0).all()
