"""Training with missing pixels on the GPU (iwae_train_step_masked,
iwae_forward_backward_masked, iwae_bound_masked and the facade's mask=...)
against the float64 reference (tests/missing_ref.py) on identical injected
noise and weights, on the fused row-block path and the layer-wise path, at the
smallest shapes that reach each branch of the pixel-masked Bernoulli epilogue
and of the staging (missing_ref.SHAPES):

  M1    1 layer, x_dim 64, 15 sample rows: one partial row tile, two full 32-column tiles
  M2    2 layers, 35 ragged rows, x_row_div = k
  M2w   33 images: beyond the few-row first-layer launches
  M50   x_dim 50, off 4 and off 32: partial column tile, the n < N guard with -1 in range
  M50w  M50 at 33 images: the unmasked step stages x too (the bit-for-bit test)
  M784  784-200-200-50, B 20, k 5: 24.5 column tiles, the GEMM tile shape the real model gets
  M784k the same at k 477, 9540 sample rows: the 128 x 128 tile kernel (from 512 such tiles) with a
        partial row tile, and a train step's output layer on bf16x3 products (from 8192 rows)

Every mask: NaN at the missing entries of x, image 0 entirely missing, image 1
entirely observed, Bernoulli(0.5) elsewhere.  Bars: test_gpu_pathgrad.py's (loss
and whole gradient 1e-4 relative, each tensor 5e-4 of its largest entry, Adam
as its _step_and_check); tests/test_missing_ref.py shows the reference run in
float32 stays within a quarter of them on these very inputs.
tests/test_gpu_step_shapes.py sweeps the masked step over odd widths, x_dim and depths."""
import functools

import numpy as np
import pytest

import missing_ref as M
import pathgrad_ref as R
from oracle import iwae_oracle as O

pytestmark = pytest.mark.gpu

REL = 1e-4
TENSOR = 5e-4
ADAM_ATOL = 6e-5
ALL_LOSSES = ["IWAE", "VAE", "L_alpha", "VAE_V1", "CIWAE", "PIWAE", "IWAE_DREG"]
PARITY = [(n, "IWAE") for n in ("M1", "M2", "M2w", "M50", "M784", "M784k")] + \
         [(n, l) for n in ("M2", "M50") for l in ALL_LOSSES[1:]]


def _flat(ws):
    return np.concatenate([np.asarray(w, np.float64).ravel() for w in ws])


def _bits(m, loss_value):
    """(loss, gradients, weights) as float32 bit patterns."""
    g = np.concatenate([np.asarray(a, np.float32).ravel() for a in m.get_gradients()])
    w = np.concatenate([np.asarray(a, np.float32).ravel() for a in m.get_weights()])
    return np.float32(loss_value).tobytes(), g.tobytes(), w.tobytes()


_case = functools.lru_cache(maxsize=None)(M.shape_case)


def _opt():
    return O.Adam(1e-3, 0.9, 0.999, 1e-4)


@functools.lru_cache(maxsize=None)
def _reference(name, loss):
    """(loss, flat gradient, post-Adam flat weights) in float64, computed once."""
    _, _, k, _, (spec, params, _, x, eps, eps2, mask) = _case(name)
    ref_loss, ref_new, ref_g = M.train_step(params, spec, x, mask, eps, loss, _opt(), **M.loss_kwargs(loss, k, eps2))
    out = (ref_loss, ref_g, O.flatten_params(spec, ref_new))
    for a in out[1:]:
        a.setflags(write=False)
    return out


def _model(name, loss, **kw):
    """(model, x [NaN where missing], mask, eps) as float32 arrays; CIWAE: eps = draw 1 + draw 2."""
    from iwae_replication_project_amd import Adam, Flexible_Model
    from iwae_replication_project_amd.flexible_iwae import _split, weight_shapes
    (he, hd, le, ld), B, k, x_dim, (spec, params, mean, x, eps, eps2, mask) = _case(name)
    lk = {a: b for a, b in M.loss_kwargs(loss, k).items() if a != "eps2"}
    m = Flexible_Model(he, hd, le, ld, dataset_bias=mean, loss_function=loss, k=k, seed=1, x_dim=x_dim, **lk, **kw)
    m.set_weights(_split(O.flatten_params(spec, params).astype(np.float32), weight_shapes(m.dense)))
    m.compile(Adam(learning_rate=1e-3, epsilon=1e-4))
    e = list(eps) + (list(eps2) if loss == "CIWAE" else [])
    return m, x.astype(np.float32), mask.astype(np.float32), [a.astype(np.float32) for a in e]


def _counts(m):
    """(masked Bernoulli launches, engine launches, ring train forwards)"""
    return [int(m._lib.iwae_debug_count(m._h, i)) for i in (21, 2, 4)]


def _step_and_check(name, loss, **kw):
    """One injected-noise masked train step against the reference; returns the
    advance of the counters of _counts."""
    m, x, mask, eps = _model(name, loss, **kw)
    spec, params = _case(name)[4][:2]
    c0 = _counts(m)
    loss_gpu = m.train_step(x, eps=eps, mask=mask)[loss]
    m.check_kernel_status()
    adv = [b - a for a, b in zip(c0, _counts(m))]
    ref_loss, ref_g, ref_w = _reference(name, loss)
    g, w = _flat(m.get_gradients()), _flat(m.get_weights())
    whole, per = R.rel_l2(g, ref_g), M.worst_tensor(spec, g, ref_g)
    print(f"{name} {loss} {kw}: loss rel {abs(loss_gpu - ref_loss) / abs(ref_loss):.2e}, gradient rel-L2 {whole:.2e}, "
          f"worst tensor {per:.2e}, counters {adv}")
    assert abs(loss_gpu - ref_loss) <= REL * abs(ref_loss), (loss_gpu, ref_loss)
    assert whole <= REL, whole
    assert per <= TENSOR, per
    w_from_g = _opt().apply(O.flatten_params(spec, params), g)
    np.testing.assert_allclose(w, w_from_g, atol=2e-6)
    np.testing.assert_allclose(w, ref_w, atol=max(ADAM_ATOL, 10 * np.abs(g - ref_g).max()))
    return adv


# ------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("path", ["fused", "layerwise"])
@pytest.mark.parametrize("name,loss", PARITY, ids=[f"{n}-{l}" for n, l in PARITY])
def test_parity_with_reference(name, loss, path):
    bern, engine, ring = _step_and_check(name, loss, kernel_path=path)
    assert bern > 0 and engine == 0 and ring == 0, (bern, engine, ring)


@pytest.mark.parametrize("path", ["fused", "layerwise"])
def test_parity_exact_f32_main_loop(path):
    """iwae_set_precision(h, 0): the masked epilogue behind the f32 MFMA main loop."""
    bern, engine, ring = _step_and_check("M2", "IWAE", kernel_path=path, precision="f32")
    assert bern > 0 and engine == 0 and ring == 0


@pytest.mark.parametrize("path", ["fused", "layerwise"])
@pytest.mark.parametrize("loss", ["IWAE", "L_alpha"])
def test_fractional_pixels(loss, path):
    """Grey-level observed pixels: the epilogue's logf / log1pf branches (the
    all-binarised fast paths do not apply), with the -1 of a missing pixel
    running through them, in the train step and in the forward-only bound."""
    m, x, mask, eps = _model("M50", loss, kernel_path=path)
    _, _, k, _, (spec, params, _, _, eps64, eps2, mask64) = _case("M50")
    grey = np.random.default_rng(8).random(x.shape).astype(np.float32)
    x64 = M.with_holes(grey.astype(np.float64), mask64)
    kw = M.loss_kwargs(loss, k, eps2)
    ref_loss, _, ref_g = M.train_step(params, spec, x64, mask64, eps64, loss, _opt(), **kw)
    bound = m._bound(m._lc(), x64, eps, mask=mask)
    assert abs(bound + ref_loss) <= REL * abs(ref_loss), (bound, ref_loss)
    got = m.train_step(x64, eps=eps, mask=mask)[loss]
    m.check_kernel_status()
    g = _flat(m.get_gradients())
    print(f"grey {loss} {path}: loss rel {abs(got - ref_loss) / abs(ref_loss):.2e}, gradient rel-L2 {R.rel_l2(g, ref_g):.2e}, "
          f"worst tensor {M.worst_tensor(spec, g, ref_g):.2e}")
    assert abs(got - ref_loss) <= REL * abs(ref_loss), (got, ref_loss)
    assert R.rel_l2(g, ref_g) <= REL
    assert M.worst_tensor(spec, g, ref_g) <= TENSOR


@pytest.mark.parametrize("name", ["M2", "M784"])
def test_auto_path_never_engine_or_ring(name):
    bern, engine, ring = _step_and_check(name, "IWAE")
    assert bern > 0 and engine == 0 and ring == 0, (bern, engine, ring)
    # an unmasked step never counts under id 21; at M784 (BASELINE configs[0]) it runs on the
    # engine, so the zero above is the masked plan's doing
    m, x, mask, eps = _model(name, "IWAE")
    c0 = _counts(m)
    m.train_step(np.where(mask != 0, x, 0), eps=eps)
    adv = [b - a for a, b in zip(c0, _counts(m))]
    assert adv[0] == 0, adv
    if name == "M784":
        assert adv[1] > 0, adv


# --------------------------------------- 2. all observed = the unmasked step
@pytest.mark.parametrize("path", ["fused", "layerwise"])
@pytest.mark.parametrize("name,loss", [("M50w", "IWAE"), ("M50w", "L_alpha"), ("M2", "IWAE"), ("M2", "L_alpha")])
def test_all_ones_mask_is_the_unmasked_step_bit_for_bit(name, loss, path):
    """M50w: both steps stage x (x_dim % 4 != 0, more than 32 images), so they
    differ in the epilogue instantiation alone.  M2: the unmasked row-block
    step's few-row input launch reads the caller's x; it stages the same values
    in the same order, so the bits agree there too."""
    outs = []
    for masked in (False, True):
        m, x, mask, eps = _model(name, loss, kernel_path=path)
        xc = np.where(mask != 0, x, 0).astype(np.float32)
        kw = {"mask": np.ones_like(mask)} if masked else {}
        outs.append(_bits(m, m.train_step(xc, eps=eps, **kw)[loss]))
        m.check_kernel_status()
    assert outs[0][0] == outs[1][0], "loss"
    assert outs[0][1] == outs[1][1], "gradients"
    assert outs[0][2] == outs[1][2], "weights"


# ------------------------------------------------ 3. missing values never leak
@pytest.mark.parametrize("path", ["fused", "layerwise"])
@pytest.mark.parametrize("name,loss", [("M50", "IWAE"), ("M2", "L_alpha"), ("M784", "IWAE")])
def test_missing_values_never_leak(name, loss, path):
    outs = []
    for fill in (np.nan, np.inf, 0.0):
        m, x, mask, eps = _model(name, loss, kernel_path=path)
        outs.append(_bits(m, m.train_step(M.with_holes(x, mask, fill), eps=eps, mask=mask)[loss]))
    assert np.isfinite(np.frombuffer(outs[0][0] + outs[0][1] + outs[0][2], np.float32)).all()
    assert outs[0] == outs[1] and outs[0] == outs[2]


# ------------------------------------------------ 4. two implementations agree
@pytest.mark.parametrize("path", ["auto", "layerwise"])
@pytest.mark.parametrize("name", ["M2", "M50", "M784", "M784k"])
def test_bound_agrees_with_impute_and_reference(name, path):
    """get_L_k(mask=...) runs the masked Bernoulli GEMM epilogue, log_px_observed
    iwae_impute's masked first pass: each within 1e-4 of float64, so within 2e-4
    of each other."""
    m, x, mask, eps = _model(name, "IWAE", kernel_path=path)
    _, _, k, _, (spec, params, _, x64, eps64, _, mask64) = _case(name)
    c0 = _counts(m)
    got = m.get_L_k(x, k, eps=eps, mask=mask)
    assert _counts(m)[0] - c0[0] == 1
    other = float(m.log_px_observed(x, mask, k, eps=eps).double().mean().item())
    ref = M.objective_and_grads(params, spec, x64, mask64, eps64, "IWAE", with_grads=False)[0]
    print(f"{name} {path}: bound {got:.6f}, impute {other:.6f}, reference {ref:.6f}")
    assert abs(got - ref) <= 1e-4 * abs(ref), (got, ref)
    assert abs(got - other) <= 2e-4 * abs(ref), (got, other)


@pytest.mark.parametrize("loss", ["VAE", "L_alpha", "VAE_V1", "CIWAE"])
def test_other_bounds_against_reference(loss):
    m, x, mask, eps = _model("M50", loss)
    _, _, k, _, (spec, params, _, x64, eps64, eps2, mask64) = _case("M50")
    got = m._bound(m._lc(), x, eps, 2 if loss == "CIWAE" else 1, mask=mask)
    ref = M.objective_and_grads(params, spec, x64, mask64, eps64, loss, with_grads=False,
                                **M.loss_kwargs(loss, k, eps2))[0]
    assert abs(got - ref) <= 1e-4 * abs(ref), (got, ref)


# ------------------------------------------------------ 5. graphs and buffers
def _device_noise_inputs(nbatch):
    _, B, _, x_dim, _ = _case("M2")
    rng = np.random.default_rng(5)
    xs = (rng.random((nbatch * B, x_dim)) < 0.3).astype(np.float32)
    ms = np.concatenate([M.make_mask(B, x_dim, 40 + i) for i in range(nbatch)]).astype(np.float32)
    return B, M.with_holes(xs, ms), ms


def test_graph_replay_reads_new_buffers():
    """Device noise, one seed, graphs on and off: the weights agree bit for bit
    after a step on (x1, m1) and after one on (x2, m2) held in other tensors; the
    graph model captures once."""
    import torch
    B, xs, ms = _device_noise_inputs(2)
    models = []
    for graphs in (True, False):
        m, _, _, _ = _model("M2", "IWAE", use_graphs=graphs)
        m.set_seed(77)
        models.append(m)
    c0 = [m.graph_captures() for m in models]
    w0 = _flat(models[0].get_weights())
    for i in range(2):
        ws = []
        for m in models:
            xt = torch.tensor(xs[i * B:(i + 1) * B], device=m.device)       # fresh device tensors per step
            mt = torch.tensor(ms[i * B:(i + 1) * B], device=m.device)
            out = m.train_step(xt, mask=mt)
            m.check_kernel_status()
            assert np.isfinite(out["IWAE"])
            ws.append(_flat(m.get_weights()))
        assert np.array_equal(ws[0], ws[1]), f"step {i}"
    assert np.abs(ws[0] - w0).max() > 1e-4
    assert [m.graph_captures() - c for m, c in zip(models, c0)] == [1, 0]


@pytest.mark.parametrize("graphs", [True, False])
def test_train_steps_equals_single_steps(graphs):
    B, xs, ms = _device_noise_inputs(3)
    a, _, _, _ = _model("M2", "IWAE", use_graphs=graphs)
    a.set_seed(78)
    la = a.train_steps(xs, B, mask=ms)
    a.check_kernel_status()
    b, _, _, _ = _model("M2", "IWAE", use_graphs=graphs)
    b.set_seed(78)
    lb = [b.train_step(xs[i * B:(i + 1) * B], mask=ms[i * B:(i + 1) * B])["IWAE"] for i in range(3)]
    assert la.shape == (3,) and np.isfinite(la).all()
    assert np.asarray(la, np.float32).tobytes() == np.asarray(lb, np.float32).tobytes()
    assert np.array_equal(_flat(a.get_weights()), _flat(b.get_weights()))
    assert a.epoch == 3


def test_fit_permutes_x_and_mask_alike():
    """fit(mask=...) with shuffling: the masked entries hold NaN, so a mask that
    was not permuted with x would let NaN reach the encoder (observed NaN)."""
    B, xs, ms = _device_noise_inputs(3)
    m, _, _, _ = _model("M2", "IWAE")
    hist = m.fit(xs[:3 * B - 2], epochs=2, batch_size=B, seed=3, mask=ms[:3 * B - 2])["IWAE"]
    m.check_kernel_status()
    assert len(hist) == 2 and np.isfinite(hist).all()
    assert np.isfinite(_flat(m.get_weights())).all()


# ------------------------------------ 6. forward_backward_masked + apply_adam
@pytest.mark.parametrize("loss", ["IWAE", "IWAE_DREG"])
def test_forward_backward_then_adam_equals_train_step(loss):
    from iwae_replication_project_amd import _lib
    a, x, mask, eps = _model("M2", loss)
    la = a.train_step(x, eps=eps, mask=mask)[loss]
    b, _, _, _ = _model("M2", loss)
    xd, md = b._x(x), b._mask(mask, x.shape[0])
    arr, n, keep = b._eps(eps, xd.shape[0], b.k)
    b._call(b._lib.iwae_forward_backward_masked(b._h, b._lc(), _lib.fptr(xd), _lib.fptr(md), xd.shape[0], arr, n,
                                                _lib.fptr(b._loss_buf)))
    b._apply_adam(1.0)
    b._stream.synchronize()
    assert float(b._loss_buf.item()) == la
    np.testing.assert_array_equal(_flat(a.get_gradients()), _flat(b.get_gradients()))
    np.testing.assert_allclose(_flat(b.get_weights()), _flat(a.get_weights()), atol=2e-6)


# ----------------------------------------------------- 7. three-step trajectory
@pytest.mark.parametrize("path", ["fused", "layerwise"])
def test_three_step_trajectory(path):
    m, x, _, eps = _model("M2", "IWAE", kernel_path=path)
    _, B, k, x_dim, (spec, params, _, x64, eps64, _, _) = _case("M2")
    opt = _opt()
    x, x64 = np.nan_to_num(x, nan=0.0), np.nan_to_num(x64, nan=0.0)     # each step digs its own holes
    for step in range(3):
        mask = M.make_mask(B, x_dim, 60 + step)
        got = m.train_step(M.with_holes(x, mask), eps=eps, mask=mask.astype(np.float32))["IWAE"]
        ref, params, _ = M.train_step(params, spec, M.with_holes(x64, mask), mask, eps64, "IWAE", opt)
        print(f"step {step}: loss {got:.6f} reference {ref:.6f} rel {abs(got - ref) / abs(ref):.2e}")
        assert abs(got - ref) <= REL * abs(ref), (step, got, ref)
    m.check_kernel_status()


# ------------------------------------------------------------------ 8. errors
def test_errors():
    from iwae_replication_project_amd import _lib
    m, x, mask, eps = _model("M2", "IWAE")
    xd, md = m._x(x), m._mask(mask, x.shape[0])
    B = xd.shape[0]
    out = _lib.fptr(m._loss_buf)
    for fn in (m._lib.iwae_train_step_masked, m._lib.iwae_forward_backward_masked, m._lib.iwae_bound_masked):
        assert fn(m._h, m._lc(), _lib.fptr(xd), None, B, None, 0, out) == -1
        assert b"mask is NULL" in m._lib.iwae_last_error(m._h)
    with pytest.raises(ValueError):
        m.train_step(x, mask=mask[:, :-1])
    with pytest.raises(ValueError):
        m.get_L_k(x, 3, mask=mask[:-1])
    # data parallel (world 2, the caller reduces): refused, and the handle stays usable
    w0 = _flat(m.get_weights())
    m._call(m._lib.iwae_dp_init(m._h, 0, 2, None))
    for fn in (m._lib.iwae_train_step_masked, m._lib.iwae_forward_backward_masked, m._lib.iwae_bound_masked):
        assert fn(m._h, m._lc(), _lib.fptr(xd), _lib.fptr(md), B, None, 0, out) == -1
        assert b"data parallel" in m._lib.iwae_last_error(m._h)
    assert np.array_equal(_flat(m.get_weights()), w0)
    m._call(m._lib.iwae_dp_init(m._h, 0, 1, None))
    assert np.isfinite(m.train_step(x, eps=eps, mask=mask)["IWAE"])
    m.check_kernel_status()


def test_facade_refuses_a_mask_under_data_parallelism():
    m, x, mask, eps = _model("M2", "IWAE")
    m._dp = object()
    with pytest.raises(ValueError):
        m.train_step(x, mask=mask)
    with pytest.raises(ValueError):
        m.train_steps(x, x.shape[0], mask=mask)
    m._dp = None
