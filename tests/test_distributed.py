"""Multi-process (world_size 2, gloo on CPU) tests of the sharding logic used
by the multi-GPU paths: image sharding, the cross-rank log-sum-exp merge of
NLL partials, and gradient averaging for data parallelism.  Compute inside the
ranks comes from the oracle (test infrastructure); what is under test is
iwae_replication_project_amd.distributed."""
import math
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _run(rank, world, rdzv, fn, q):
    try:
        dist.init_process_group("gloo", init_method=rdzv, rank=rank, world_size=world)
    except Exception as e:          # pragma: no cover
        q.put((rank, repr(e)))
        return
    try:
        q.put((rank, fn(rank, world)))
    except Exception as e:          # pragma: no cover
        q.put((rank, repr(e)))
    finally:
        dist.destroy_process_group()


def spawn(fn, world=2):
    """The ranks meet through a file in a fresh directory (a port found free and
    then released can be taken before rank 0 listens on it), and no rank
    outlives the call: a failed rank cannot leave its peer waiting."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with tempfile.TemporaryDirectory() as tmp:
        rdzv = "file://" + os.path.join(tmp, "rendezvous")
        ps = [ctx.Process(target=_run, args=(r, world, rdzv, fn, q), daemon=True) for r in range(world)]
        for p in ps:
            p.start()
        try:
            out = dict(q.get(timeout=120) for _ in ps)
            for p in ps:
                p.join(timeout=60)
        finally:
            for p in ps:
                if p.is_alive():
                    p.terminate()
                    p.join(timeout=60)
    return out


def _model():
    from oracle import iwae_oracle as O
    rng = np.random.default_rng(0)
    spec = O.ModelSpec([16, 8], [8, 16], [8, 4], [8, 32], x_dim=32)
    params = O.glorot_init(spec, rng, out_bias=rng.normal(size=32) * 0.3)
    x = (rng.random((7, 32)) < 0.3).astype(np.float64)
    eps = O.draw_eps(spec, 40, 7, rng)
    return O, spec, params, x, eps


def nll_sample_shard(rank, world):
    """Each rank evaluates its k-range of every image; merge partials."""
    from iwae_replication_project_amd import distributed as D
    O, spec, params, x, eps = _model()
    k = eps[0].shape[0]
    lo, hi = D.shard_range(k, rank, world)
    lw = O.forward(params, spec, x, [e[lo:hi] for e in eps])["lw"]
    m = torch.tensor(lw.max(0))
    s = torch.tensor(np.exp(lw - lw.max(0)).sum(0))
    M, S = D.merge_lse_partials(m, s)
    merged = (M + torch.log(S) - math.log(k)).numpy()
    return merged.tolist()


def nll_image_shard(rank, world):
    from iwae_replication_project_amd import distributed as D
    O, spec, params, x, eps = _model()
    lo, hi = D.shard_range(x.shape[0], rank, world)
    lp = O.L_k_per_image(O.forward(params, spec, x[lo:hi], [e[:, lo:hi] for e in eps])["lw"])
    tot = torch.tensor([lp.sum(), float(hi - lo)], dtype=torch.float64)
    dist.all_reduce(tot)
    return float(-(tot[0] / tot[1]))


def dp_grads(rank, world):
    """Per-rank gradient of the batch-mean VAE loss on its shard, averaged
    across ranks == gradient of the full-batch loss (equal shards)."""
    from iwae_replication_project_amd import distributed as D
    O, spec, params, x, eps = _model()
    x, eps = x[:6], [e[:, :6] for e in eps]
    lo, hi = D.shard_range(6, rank, world)
    _, g = O.objective_and_grads(params, spec, x[lo:hi], [e[:, lo:hi] for e in eps], "VAE", eps[0].shape[0])
    t = torch.tensor(O.flatten_params(spec, g))
    D.allreduce_mean_(t)
    return t.numpy().tolist()


def test_shard_range_partitions_everything():
    from iwae_replication_project_amd.distributed import shard_range
    for n in (0, 1, 7, 10000, 10001):
        for w in (1, 2, 3, 8):
            parts = [shard_range(n, r, w) for r in range(w)]
            assert parts[0][0] == 0 and parts[-1][1] == n
            assert all(parts[i][1] == parts[i + 1][0] for i in range(w - 1))
            sizes = [hi - lo for lo, hi in parts]
            assert max(sizes) - min(sizes) <= 1


def test_sample_sharded_nll_merge_equals_single_process():
    out = spawn(nll_sample_shard)
    O, spec, params, x, eps = _model()
    ref = O.L_k_per_image(O.forward(params, spec, x, eps)["lw"])
    for r in (0, 1):
        assert not isinstance(out[r], str), out[r]
        np.testing.assert_allclose(out[r], ref, rtol=1e-10)


def test_image_sharded_nll_equals_single_process():
    out = spawn(nll_image_shard)
    O, spec, params, x, eps = _model()
    ref = -np.mean(O.L_k_per_image(O.forward(params, spec, x, eps)["lw"]))
    assert out[0] == pytest.approx(ref, rel=1e-12) and out[1] == pytest.approx(ref, rel=1e-12)


def test_data_parallel_gradient_average_equals_full_batch():
    out = spawn(dp_grads)
    O, spec, params, x, eps = _model()
    _, g = O.objective_and_grads(params, spec, x[:6], [e[:, :6] for e in eps], "VAE", eps[0].shape[0])
    ref = O.flatten_params(spec, g)
    for r in (0, 1):
        assert not isinstance(out[r], str), out[r]
        np.testing.assert_allclose(out[r], ref, rtol=1e-10, atol=1e-13)


def dp_grads_unequal(rank, world):
    """Unequal shards (4 + 3 images): the weighted merge sum_r B_r g_r / sum_r B_r
    (what the library's data-parallel step computes from one all-reduce of the
    gradient buffer plus its batch-size tail) equals the full-batch gradient."""
    from iwae_replication_project_amd import distributed as D
    O, spec, params, x, eps = _model()
    lo, hi = D.shard_range(7, rank, world)
    _, g = O.objective_and_grads(params, spec, x[lo:hi], [e[:, lo:hi] for e in eps], "IWAE", eps[0].shape[0])
    t = torch.tensor(np.concatenate([O.flatten_params(spec, g), [0.0]]))
    return D.weighted_grad_merge_(t, hi - lo).numpy().tolist()


def test_data_parallel_weighted_merge_unequal_shards_equals_full_batch():
    out = spawn(dp_grads_unequal)
    O, spec, params, x, eps = _model()
    _, g = O.objective_and_grads(params, spec, x, eps, "IWAE", eps[0].shape[0])
    ref = O.flatten_params(spec, g)
    for r in (0, 1):
        assert not isinstance(out[r], str), out[r]
        np.testing.assert_allclose(out[r], ref, rtol=1e-10, atol=1e-13)
    # the unweighted 1/world average is wrong for unequal shards
    lo = []
    for r in (0, 1):
        a, b = (0, 4) if r == 0 else (4, 7)
        _, gr = O.objective_and_grads(params, spec, x[a:b], [e[:, a:b] for e in eps], "IWAE", eps[0].shape[0])
        lo.append(O.flatten_params(spec, gr))
    assert np.abs((lo[0] + lo[1]) / 2 - ref).max() > 1e-6


# ---- world size 8: the arithmetic of the 8-GPU SCALE run (configs[2] / [4]),
# rehearsed with gloo on CPU before any 8-rank run happens on hardware

def _model8(n_img, k):
    """A small oracle model over n_img images (the sharding arithmetic does not
    depend on the layer widths; the small model keeps 8 ranks' compute short)."""
    from oracle import iwae_oracle as O
    rng = np.random.default_rng(8)
    spec = O.ModelSpec([12, 6], [6, 12], [6, 3], [6, 16], x_dim=16)
    params = O.glorot_init(spec, rng, out_bias=rng.normal(size=16) * 0.3)
    x = (rng.random((n_img, 16)) < 0.3).astype(np.float64)
    eps = O.draw_eps(spec, k, n_img, rng)
    return O, spec, params, x, eps


def nll_image_shard_10k(rank, world):
    """configs[2]: 10,000 test images sharded by image over the ranks (1,250
    each at world 8); each rank's per-image log p(x) and one all-reduce of
    (sum, count) give the mean NLL."""
    from iwae_replication_project_amd import distributed as D
    O, spec, params, x, eps = _model8(10_000, 6)
    lo, hi = D.shard_range(x.shape[0], rank, world)
    lp = O.L_k_per_image(O.forward(params, spec, x[lo:hi], [e[:, lo:hi] for e in eps])["lw"])
    tot = torch.tensor([lp.sum(), float(hi - lo)], dtype=torch.float64)
    dist.all_reduce(tot)
    return [float(-(tot[0] / tot[1])), hi - lo]


def nll_sample_shard_8(rank, world, k=43):
    """The sample-chunk split: k = 43 samples of every image over the ranks
    (ragged: 6 + 6 + 6 + 5 * 5 at world 8), per-image LSE partials merged."""
    from iwae_replication_project_amd import distributed as D
    O, spec, params, x, eps = _model8(9, k)
    lo, hi = D.shard_range(k, rank, world)
    lw = O.forward(params, spec, x, [e[lo:hi] for e in eps])["lw"]
    m = torch.tensor(lw.max(0))
    s = torch.tensor(np.exp(lw - lw.max(0)).sum(0))
    M, S = D.merge_lse_partials(m, s)
    return (M + torch.log(S) - math.log(k)).numpy().tolist()


# configs[4]: 4,096 images over 8 ranks with one ragged shard (the last rank
# holds 509 images, the first 515): the batch-size-weighted merge of one
# all-reduce gives the full-batch gradient of the batch-mean loss
DP8_SHARDS = [515, 512, 512, 512, 512, 512, 512, 509]


def dp_grads_weighted_8(rank, world):
    from iwae_replication_project_amd import distributed as D
    O, spec, params, x, eps = _model8(sum(DP8_SHARDS), 3)
    lo = sum(DP8_SHARDS[:rank])
    hi = lo + DP8_SHARDS[rank]
    _, g = O.objective_and_grads(params, spec, x[lo:hi], [e[:, lo:hi] for e in eps], "IWAE", eps[0].shape[0])
    t = torch.tensor(np.concatenate([O.flatten_params(spec, g), [0.0]]))
    return D.weighted_grad_merge_(t, hi - lo).numpy().tolist()


def test_world8_image_sharded_nll_10k_images():
    out = spawn(nll_image_shard_10k, world=8)
    O, spec, params, x, eps = _model8(10_000, 6)
    ref = -np.mean(O.L_k_per_image(O.forward(params, spec, x, eps)["lw"]))
    for r in range(8):
        assert not isinstance(out[r], str), out[r]
        assert out[r][1] == 1250
        assert out[r][0] == pytest.approx(ref, rel=1e-12)


def test_world8_sample_chunk_lse_merge_ragged():
    out = spawn(nll_sample_shard_8, world=8)
    O, spec, params, x, eps = _model8(9, 43)
    ref = O.L_k_per_image(O.forward(params, spec, x, eps)["lw"])
    from iwae_replication_project_amd.distributed import shard_range
    assert sorted({shard_range(43, r, 8)[1] - shard_range(43, r, 8)[0] for r in range(8)}) == [5, 6]
    for r in range(8):
        assert not isinstance(out[r], str), out[r]
        np.testing.assert_allclose(out[r], ref, rtol=1e-10)


def test_world8_weighted_dp_merge_4096_images_one_ragged_shard():
    out = spawn(dp_grads_weighted_8, world=8)
    O, spec, params, x, eps = _model8(sum(DP8_SHARDS), 3)
    _, g = O.objective_and_grads(params, spec, x, eps, "IWAE", eps[0].shape[0])
    ref = O.flatten_params(spec, g)
    for r in range(8):
        assert not isinstance(out[r], str), out[r]
        np.testing.assert_allclose(out[r], ref, rtol=1e-9, atol=1e-12)
    # the plain 1/world mean of the ranks' gradients is off with the ragged shard
    parts = []
    for r in range(8):
        lo = sum(DP8_SHARDS[:r]); hi = lo + DP8_SHARDS[r]
        _, gr = O.objective_and_grads(params, spec, x[lo:hi], [e[:, lo:hi] for e in eps], "IWAE", 3)
        parts.append(O.flatten_params(spec, gr))
    assert np.abs(np.mean(parts, axis=0) - ref).max() > 1e-9
