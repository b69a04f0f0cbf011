"""The row-chain engine's op loop on the GPU at the shapes of
tests/engine_op_cases.py (idle waves and hand-over, 8 / 9 / 17 column tiles, one
to three k chunks, a split output layer, ragged and full workgroups, image-row
jobs, three layers): one injected-noise train step against the float64 oracle
at the bars of tests/test_gpu_shapes.py -- loss and whole gradient 1e-4
relative, each parameter tensor 5e-4 of its largest entry, Adam as there --
with the launch counters saying the engine (2) and, at 264 rows, the combined
launch (9) ran.  tests/test_engine_op_cases.py shows the reference in float32
stays within a quarter of these bars on the same inputs.

Measured on an MI355X over all cases and losses: loss 1.7e-6, whole gradient
5.8e-5, worst tensor 1.4e-4."""
import functools

import numpy as np
import pytest

import engine_op_cases as E
import pathgrad_ref as R
from oracle import iwae_oracle as O

pytestmark = pytest.mark.gpu

REL = 1e-4
TENSOR = 5e-4
ADAM_ATOL = 6e-5
COUNTERS = (2, 9, 13, 14)
TRAIN = [(n, v[0]) for n in E.CASES for v in E.loss_variants(n)]


def _flat(ws):
    return np.concatenate([np.asarray(w, np.float64).ravel() for w in ws])


@functools.lru_cache(maxsize=None)
def _reference(name, vid):
    out = E.reference_step(name, vid)
    for a in out[1:]:
        a.setflags(write=False)
    return out


def _model(name, vid="IWAE", **kw):
    from iwae_replication_project_amd import Adam, Flexible_Model
    from iwae_replication_project_amd.flexible_iwae import _split, weight_shapes
    he, hd, le, ld, x_dim, B, k, seed = E.CASES[name]
    _, loss, lkw = E.variant(name, vid)
    spec, params, mean, x, eps = E.make(name)
    m = Flexible_Model(he, hd, le, ld, dataset_bias=mean, loss_function=loss, k=k, seed=1, x_dim=x_dim, **lkw, **kw)
    m.set_weights(_split(O.flatten_params(spec, params).astype(np.float32), weight_shapes(m.dense)))
    m.compile(Adam(learning_rate=1e-3, epsilon=1e-4))
    return m, x.astype(np.float32), [e.astype(np.float32) for e in eps]


def _counts(m):
    return {i: int(m._lib.iwae_debug_count(m._h, i)) for i in COUNTERS}


def _advance(m, before):
    return {i: v - before[i] for i, v in _counts(m).items()}


@pytest.mark.parametrize("name,vid", TRAIN, ids=["-".join(c) for c in TRAIN])
def test_train_step_matches_float64_on_the_engine(name, vid):
    _, loss, _ = E.variant(name, vid)
    m, x, eps = _model(name, vid)
    spec, params = E.make(name)[:2]
    c0 = _counts(m)
    loss_gpu = m.train_step(x, eps=eps)[loss]
    m.check_kernel_status()
    adv = _advance(m, c0)
    ref_loss, ref_g, ref_w = _reference(name, vid)
    g, w = _flat(m.get_gradients()), _flat(m.get_weights())
    whole = R.rel_l2(g, ref_g)
    per = [np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)
           for a, b in zip(R.split_tensors(spec, g), R.split_tensors(spec, ref_g))]
    print(f"{name} {vid}: loss rel {abs(loss_gpu - ref_loss) / abs(ref_loss):.2e}, gradient rel-L2 {whole:.2e}, "
          f"worst tensor {max(per):.2e}, post-Adam weights {np.abs(w - ref_w).max():.2e}, counters {adv}")
    assert np.isfinite(loss_gpu) and np.isfinite(g).all()
    assert abs(loss_gpu - ref_loss) <= REL * abs(ref_loss), (loss_gpu, ref_loss)
    assert whole <= REL, whole
    assert max(per) <= TENSOR, per
    # Adam as tests/test_gpu_shapes.py
    w_from_g = O.Adam(1e-3, 0.9, 0.999, 1e-4).apply(O.flatten_params(spec, params), g)
    np.testing.assert_allclose(w, w_from_g, atol=2e-6)
    np.testing.assert_allclose(w, ref_w, atol=max(ADAM_ATOL, 10 * np.abs(g - ref_g).max()))
    assert adv[2] > 0 and adv[13] == 0, adv              # on the engine, not the row-block kernels
    if name == "Et":
        assert adv[9] > 0, adv                            # the combined image-row backward + update launch


def test_device_noise_steps_graph_equals_eager():
    """Two Philox train steps of the one-full-workgroup case, eager and through
    a captured graph: bit-identical losses, weights and Adam state
    (test_gpu_shapes.test_device_noise_steps_graphs_equal_eager)."""
    name = E.GRAPH_CASE
    he, hd, le, ld, x_dim, B, k, seed = E.CASES[name]
    rng = np.random.default_rng(seed + 3)
    xs = (rng.random((2 * B, x_dim)) < 0.3).astype(np.float32)
    runs = []
    for graphs in (False, True):
        m, _, _ = _model(name, use_graphs=graphs)
        m.set_seed(77)
        c0 = _counts(m)
        losses = [m.train_step(xs[i * B:(i + 1) * B])["IWAE"] for i in range(2)]
        m.check_kernel_status()
        assert _advance(m, c0)[2] > 0
        mm, vv, st = m.get_optimizer_state()
        runs.append((np.asarray(losses, np.float32), _flat(m.get_weights()), np.asarray(mm), np.asarray(vv), st))
    assert np.isfinite(runs[0][0]).all()
    w0 = O.flatten_params(*E.make(name)[:2])
    assert np.abs(runs[0][1] - w0).max() > 1e-4            # the steps moved the weights
    for a, b in zip(runs[0][:4], runs[1][:4]):
        np.testing.assert_array_equal(a, b)
    assert runs[0][4] == runs[1][4] == 2
