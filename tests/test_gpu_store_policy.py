"""Store policy of what a launch leaves to later launches (include/iwae.h
iwae_set_store_policy; the facade's tuning name st_wt): write-through (sc1)
stores of the 16-row engine launches and of the fused update's tiles, and the early finishers' own L2 write-back, change
where a stored line lives and when it reaches memory -- never a bit of a result.

Every case runs three train steps from the same seed and batches under mask 0,
the default mask and 63 (every bit) and compares losses, weights, gradients and
the Adam moments bitwise."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ARCH2 = ([200, 100], [100, 200], [100, 50], [100, 784])
ARCH1 = ([200], [200], [50], [784])
# x_dim 30 and the latent width 6 are no multiple of 4, the hidden widths 24 / 12
# no multiple of 16: scalar tail stores, partial lines
ARCH_ODD = ([24, 12], [12, 24], [24, 6], [24, 30])

MASKS = (0, None, 63)          # None: the library's default mask (no tuning passed)


def _flat(ws):
    return np.concatenate([np.asarray(w, np.float32).ravel() for w in ws])


def _model(arch, loss, k, mask, x_dim=784, **kw):
    from iwae_replication_project_amd import Adam, Flexible_Model
    tune = dict(kw.pop("tuning", {}))
    if mask is not None:
        tune["st_wt"] = mask
    m = Flexible_Model(*arch, dataset_bias=None, loss_function=loss, k=k, seed=29, x_dim=x_dim, tuning=tune, **kw)
    m.compile(Adam(learning_rate=1e-3, epsilon=1e-4))
    return m


def _state(m, losses):
    """What a run computed; the kernel status is clean and no in-launch wait gave up."""
    m.check_kernel_status()
    assert m._lib.iwae_debug_count(m._h, 8) == 0
    mm, vv, st = m.get_optimizer_state()
    return (np.asarray(losses, np.float32), _flat(m.get_weights()), _flat(m.get_gradients()),
            np.asarray(mm, np.float32), np.asarray(vv, np.float32), st)


def _three_steps(arch, loss, k, B, mask, x_dim=784, **kw):
    rng = np.random.default_rng(500 + B + k)
    xs = (rng.random((3, B, x_dim)) < 0.25).astype(np.float32)
    m = _model(arch, loss, k, mask, x_dim=x_dim, **kw)
    losses = [m.train_step(xs[i])[loss] for i in range(3)]
    counts = {i: m._lib.iwae_debug_count(m._h, i) for i in (2, 9, 14)}
    return _state(m, losses), counts


def _assert_same(runs):
    names = ("losses", "weights", "gradients", "adam_m", "adam_v")
    for r in runs[1:]:
        for name, a, b in zip(names, runs[0], r):
            np.testing.assert_array_equal(a, b, err_msg=name)
        assert runs[0][5] == r[5] == 3


@pytest.mark.parametrize("case", ["a", "b", "c", "d"])
def test_store_policy_masks_are_bitwise_equal(case):
    """a: the flagship architecture, B = 6, k = 50 (300 rows): job I' and the
    update as the combined launch with its write-through hand-off (counter 9).
    b: one stochastic layer 784-200-200-50, k = 5, B = 20 (100 rows): job I' and
    upd_kernel as two launches (below the combined launch's 256 rows).
    c: x_dim 30, widths 24 / 12 / 24 / 6, B = 3, k = 7: 21 rows, a ragged second
    row tile, scalar tail stores and partial lines at every store site.
    d: PIWAE (k1 = 5, k2 = 10) on shape a with the backward chain run twice
    (piwae_one 0: the IWAE_{k1 k2} weighting, then MIWAE's for the encoder)."""
    arch, loss, k, B, x_dim, kw = {
        "a": (ARCH2, "IWAE", 50, 6, 784, {}),
        "b": (ARCH1, "IWAE", 5, 20, 784, {}),
        "c": (ARCH_ODD, "IWAE", 7, 3, 30, {}),
        "d": (ARCH2, "PIWAE", 50, 6, 784, dict(k1=5, k2=10, tuning={"piwae_one": 0})),
    }[case]
    runs, counts = zip(*[_three_steps(arch, loss, k, B, mask, x_dim=x_dim, **kw) for mask in MASKS])
    for c in counts:
        assert c == counts[0], counts                  # the same launches under every mask
        assert c[2] > 0 and c[14] > 0, c               # the engine and the fused update ran
        if case == "a":
            assert c[9] > 0, c                         # ... job I' and the update as one launch (counted at capture)
        if case == "b":
            assert c[9] == 0, c                        # ... as two launches
    assert np.isfinite(runs[0][0]).all()
    _assert_same(runs)


def test_store_policy_multi_step_graph_equals_single_calls():
    """e: train_steps over 5 batches (one captured multi-step graph) under mask 63
    against 5 train_step calls under mask 0, the flagship architecture at
    B = 6, k = 50."""
    import torch
    B, k, n = 6, 50, 5
    rng = np.random.default_rng(77)
    xs = (rng.random((n * B, 784)) < 0.25).astype(np.float32)
    m = _model(ARCH2, "IWAE", k, 63)
    la = m.train_steps(torch.from_numpy(xs).to(m.device), B)
    ra = _state(m, list(la))
    f = _model(ARCH2, "IWAE", k, 0)
    rb = _state(f, [f.train_step(xs[i * B:(i + 1) * B])["IWAE"] for i in range(n)])
    for name, a, b in zip(("losses", "weights", "gradients", "adam_m", "adam_v"), ra, rb):
        np.testing.assert_array_equal(a, b, err_msg=name)
    assert ra[5] == rb[5] == n
