"""IWAE_STL / IWAE_DREG on the GPU against the float64 reference
(tests/pathgrad_ref.py) on identical injected noise and weights, on the fused
row-block path and the layer-wise path, at the smallest shapes that reach every
branch of the kernels they add to (pathgrad_ref.SHAPES):

  S1   1 layer, 15 sample rows (one partial 16-row tile), d = 6 (not a multiple of 4)
  S2   2 layers, 35 ragged rows: the density job, 4 dL/dh sources at layer 0
  S2w  33 images: the first layer's backward beyond the few-row launches
  S3   3 layers: a middle layer with 4 sources, two density jobs
  S4   d = 70 > 64: second lane pass of the element-wise kernel, more than 16 column quads

Bars: those of test_gpu_parity.py / test_gpu_configs.py (loss and whole
gradient 1e-4 relative, each parameter tensor 5e-4 of its largest entry, Adam
as test_gpu_configs._check).  tests/test_pathgrad_ref.py shows the reference
run in float32 stays within a quarter of them on these very inputs."""
import functools

import numpy as np
import pytest

import pathgrad_ref as R
from oracle import iwae_oracle as O

pytestmark = pytest.mark.gpu

REL = 1e-4
TENSOR = 5e-4
ADAM_ATOL = 6e-5
ARCH1 = ([200], [200], [50], [784])
PATH_COUNTER = {"fused": 11, "layerwise": 12}


def _flat(ws):
    return np.concatenate([np.asarray(w, np.float64).ravel() for w in ws])


@functools.lru_cache(maxsize=None)
def _case(name):
    """(arch, B, k, x_dim, (spec, params, mean, x, eps)) of a named case."""
    if name.startswith("C0-"):
        loss = name[3:]
        return ARCH1, 20, 5, 784, R.make_case(ARCH1, 20, 5, 300 + len(loss), x_dim=784)
    arch, B, k, case = R.shape_case(name)
    return arch, B, k, R.X_DIM, case


@functools.lru_cache(maxsize=None)
def _reference(name, loss):
    """(loss, flat gradient, post-Adam flat weights) in float64, computed once."""
    _, _, _, _, (spec, params, _, x, eps) = _case(name)
    ref_loss, ref_new, ref_g = R.train_step(params, spec, x, eps, loss, O.Adam(1e-3, 0.9, 0.999, 1e-4))
    out = (ref_loss, ref_g, O.flatten_params(spec, ref_new))
    for a in out[1:]:
        a.setflags(write=False)
    return out


def _model(name, loss, **kw):
    from iwae_replication_project_amd import Adam, Flexible_Model
    from iwae_replication_project_amd.flexible_iwae import _split, weight_shapes
    (he, hd, le, ld), B, k, x_dim, (spec, params, mean, x, eps) = _case(name)
    m = Flexible_Model(he, hd, le, ld, dataset_bias=mean, loss_function=loss, k=k, seed=1, x_dim=x_dim, **kw)
    m.set_weights(_split(O.flatten_params(spec, params).astype(np.float32), weight_shapes(m.dense)))
    m.compile(Adam(learning_rate=1e-3, epsilon=1e-4))
    return m, x.astype(np.float32), [e.astype(np.float32) for e in eps]


def _counts(m):
    return [int(m._lib.iwae_debug_count(m._h, i)) for i in (2, 11, 12)]


def _step_and_check(name, loss, **kw):
    """One injected-noise train step against the reference; returns the
    advance of the (engine, row-block path-gradient, layer-wise path-gradient)
    launch counters."""
    m, x, eps = _model(name, loss, **kw)
    spec, params = _case(name)[4][:2]
    c0 = _counts(m)
    loss_gpu = m.train_step(x, eps=eps)[loss]
    m.check_kernel_status()
    adv = [b - a for a, b in zip(c0, _counts(m))]
    ref_loss, ref_g, ref_w = _reference(name, loss)
    g, w = _flat(m.get_gradients()), _flat(m.get_weights())
    whole = R.rel_l2(g, ref_g)
    per = [np.abs(a - b).max() / np.abs(b).max() for a, b in zip(R.split_tensors(spec, g), R.split_tensors(spec, ref_g))]
    print(f"{name} {loss} {kw}: loss rel {abs(loss_gpu - ref_loss) / abs(ref_loss):.2e}, gradient rel-L2 {whole:.2e}, "
          f"worst tensor {max(per):.2e}, counters {adv}")
    assert abs(loss_gpu - ref_loss) <= REL * abs(ref_loss), (loss_gpu, ref_loss)
    assert whole <= REL, whole
    assert max(per) <= TENSOR, per
    # Adam as test_gpu_configs._check: the device Adam on the device gradient (tight), and
    # against the reference weights within the lr/eps = 10 amplification of the gradient error
    w_from_g = O.Adam(1e-3, 0.9, 0.999, 1e-4).apply(O.flatten_params(spec, params), g)
    np.testing.assert_allclose(w, w_from_g, atol=2e-6)
    np.testing.assert_allclose(w, ref_w, atol=max(ADAM_ATOL, 10 * np.abs(g - ref_g).max()))
    return adv


@pytest.mark.parametrize("path", ["fused", "layerwise"])
@pytest.mark.parametrize("loss", R.LOSSES)
@pytest.mark.parametrize("name", list(R.SHAPES))
def test_parity_with_reference(name, loss, path):
    engine, rb, gauss = _step_and_check(name, loss, kernel_path=path)
    adv = {11: rb, 12: gauss}
    mine = PATH_COUNTER[path]
    assert adv[mine] > 0 and adv[23 - mine] == 0 and engine == 0, (engine, rb, gauss)


def test_narrow_model_row_block_backward_iwae():
    """S1 is narrower than every model of the other test files: all its widths
    are below 32, where the row-block backward's LDS row (padded to 64) must be
    wider than the forward's (32).  Plain IWAE on the fused path, against the oracle."""
    m, x, eps = _model("S1", "IWAE", kernel_path="fused")
    spec, params, _, x64, eps64 = _case("S1")[4]
    loss_gpu = m.train_step(x, eps=eps)["IWAE"]
    ref_loss, _, ref_g = O.train_step(params, spec, x64, eps64, "IWAE", _case("S1")[2], O.Adam(1e-3, 0.9, 0.999, 1e-4))
    assert abs(loss_gpu - ref_loss) <= REL * abs(ref_loss)
    assert R.rel_l2(_flat(m.get_gradients()), ref_g) <= REL


@pytest.mark.parametrize("loss", R.LOSSES)
@pytest.mark.parametrize("name", ["S2", "C0"])
def test_auto_path_is_row_block_not_engine(name, loss):
    """Default kernel_path: the row-block kernels, never the bf16x3 engine
    (whose Gaussian backward has no gradient modes)."""
    engine, rb, gauss = _step_and_check("C0-" + loss if name == "C0" else name, loss)
    assert engine == 0 and rb > 0 and gauss == 0, (engine, rb, gauss)


@pytest.mark.parametrize("loss", R.LOSSES)
def test_bound_value_is_iwae_bit_for_bit(loss):
    m, x, eps = _model("S2", loss)
    k = _case("S2")[2]
    want = m.get_L_k(x, k, eps=eps)
    got = m._bound(m._lc(loss, k=k), x, eps)
    assert np.float32(got).tobytes() == np.float32(want).tobytes(), (got, want)


@pytest.mark.parametrize("loss", R.LOSSES)
def test_device_noise_graphs_determinism(loss):
    """Philox noise: two fresh models with one seed end bitwise equal, with and
    without graphs."""
    rng = np.random.default_rng(5)
    B = _case("S2")[1]
    xs = (rng.random((3 * B, R.X_DIM)) < 0.3).astype(np.float32)
    ws = []
    for graphs in (True, True, False):
        m, _, _ = _model("S2", loss, use_graphs=graphs)
        m.set_seed(77)
        losses = m.train_steps(xs, B)
        m.check_kernel_status()
        assert losses.shape == (3,) and np.isfinite(losses).all()
        ws.append(_flat(m.get_weights()))
    assert np.array_equal(ws[0], ws[1])
    assert np.array_equal(ws[0], ws[2])
    w0 = O.flatten_params(*_case("S2")[4][:2])
    assert np.abs(ws[0] - w0).max() > 1e-4       # the steps moved the weights


@pytest.mark.parametrize("loss", R.LOSSES)
def test_forward_backward_then_adam_equals_train_step(loss):
    a, x, eps = _model("S2", loss)
    la = a.train_step(x, eps=eps)[loss]
    b, _, _ = _model("S2", loss)
    xd = b._x(x)
    arr, n, keep = b._eps(eps, xd.shape[0], b.k)
    b._forward_backward(b._lc(), xd, xd.shape[0], arr, n)
    b._apply_adam(1.0)
    b._stream.synchronize()
    assert float(b._loss_buf.item()) == la
    np.testing.assert_array_equal(_flat(a.get_gradients()), _flat(b.get_gradients()))
    np.testing.assert_allclose(_flat(b.get_weights()), _flat(a.get_weights()), atol=2e-6)


def test_unknown_loss_id_still_rejected():
    from iwae_replication_project_amd import _lib
    m, x, eps = _model("S1", "IWAE_STL")
    lc = m._lc()
    lc.loss = 11
    xd = m._x(x)
    rc = m._lib.iwae_train_step(m._h, lc, _lib.fptr(xd), xd.shape[0], None, 0, _lib.fptr(m._loss_buf))
    assert rc == -1                               # IWAE_EINVAL
    assert b"unknown loss_function id 11" in m._lib.iwae_last_error(m._h)
