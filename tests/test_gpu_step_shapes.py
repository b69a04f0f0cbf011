"""Shape sweep of the reweighted wake-sleep step and the pixel-masked train step
on the GPU: every case of tests/step_shape_cases.py (shape_cases' models -- odd
and tiny widths, x_dim off 4, 1 to 8 stochastic layers, widths either side of
kRbMaxWidth -- and the row-count cases R20p20 .. R32p1 around smallm_rows)
against the float64 references (tests/wakesleep_ref.py, tests/missing_ref.py) on
identical injected noise, dreams, masks and weights, on the "fused" and the
"layerwise" request, with the launch counters pinning which kernels ran
(step_shape_cases.expected, never observed behaviour).

Bars, by import: tests/test_gpu_wakesleep.py's REL, TENSOR, ADAM_ATOL for the
wake-sleep step, tests/test_gpu_missing.py's for the masked step; a tensor
whose float64 gradient is exactly zero must be exactly zero
(missing_ref.worst_tensor).  tests/test_step_shape_cases.py shows the references
run in float32 stay within a quarter of the bars on these very inputs, and that
deliberately wrong references miss them by a factor of 40 at least.

Measured on an MI355X over all cases, coefficient pairs / losses and paths:
wake-sleep values 3.7e-7, whole gradient 4.6e-6, worst tensor 1.7e-5; masked
loss 2.9e-7, whole gradient 4.5e-6, worst tensor 2.1e-5; masked bound 4.1e-6.
With out_x3_rows = 16 on O2w: wake-sleep values 5.1e-8, whole gradient 3.5e-6,
worst tensor 9.0e-6; masked 3.3e-8, 3.7e-6, 8.4e-6 -- the bars hold as they are."""
import numpy as np
import pytest

import missing_ref as M
import pathgrad_ref as PR
import step_shape_cases as SS
import test_gpu_missing as TM
import test_gpu_wakesleep as TW
import wakesleep_ref as W
from oracle import iwae_oracle as O

pytestmark = pytest.mark.gpu

PATHS = ("fused", "layerwise")
MIX = W.COEFS[2]
WS_PARITY = [(n, c, p) for n in SS.WS_CASES for c in SS.WS_COEFS[n] for p in PATHS]
MASKED_PARITY = [(n, l, p) for n in SS.MASKED_CASES for l in SS.MASKED_LOSSES[n] for p in PATHS]
MASKED_IDS = (21, 2, 4, 13)        # masked Bernoulli launches, engine launches, ring train forwards, row-block forwards

_flat, _bits, _values, _counts, _adv = TW._flat, TW._bits, TW._values, TW._counts, TW._adv


def _opt():
    return O.Adam(1e-3, 0.9, 0.999, 1e-4)


def _ws_inputs(name):
    """(x, eps, dreams) of a wake-sleep case as float32 arrays."""
    _, x, eps, dreams = SS.ws_case(name)[4][2:]
    return (x.astype(np.float32), [e.astype(np.float32) for e in eps],
            (dreams[0].astype(np.float32), [v.astype(np.float32) for v in dreams[1]]))


def _ws_model(name, **kw):
    """test_gpu_wakesleep._model at the case's own x_dim."""
    from iwae_replication_project_amd import Adam, Flexible_Model
    from iwae_replication_project_amd.flexible_iwae import _split, weight_shapes
    (he, hd, le, ld), B, k, n, (spec, params, mean, _, _, _) = SS.ws_case(name)
    kw.setdefault("seed", 1)
    knobs = kw.pop("knobs", {})
    m = Flexible_Model(he, hd, le, ld, dataset_bias=mean, loss_function="IWAE", k=k, x_dim=spec.x_dim, **kw)
    m.set_weights(_split(O.flatten_params(spec, params).astype(np.float32), weight_shapes(m.dense)))
    m.compile(Adam(learning_rate=1e-3, epsilon=1e-4))
    for knob, v in knobs.items():
        m.set_tuning(knob, v)
    return (m,) + _ws_inputs(name)


def _ws_step_and_check(name, coef, tag, **kw):
    """One injected wake-sleep step against float64 at the bars; returns (model's counters' advance, values)."""
    m, x, eps, dreams = _ws_model(name, **kw)
    spec, params = SS.ws_case(name)[4][:2]
    c0 = _counts(m)
    got = _values(m.wake_sleep_step(x, coef[0], coef[1], dreams=dreams if coef[1] > 0 else None, eps=eps))
    m.check_kernel_status()
    adv = _adv(m, c0)
    ref_vals, ref_g, ref_w = SS.ws_reference(name, coef)
    g, w = _flat(m.get_gradients()), _flat(m.get_weights())
    vrel = SS.value_errors(got, ref_vals)
    whole, per = PR.rel_l2(g, ref_g), M.worst_tensor(spec, g, ref_g)
    print(f"{name} {coef} {tag}: values rel {[f'{v:.2e}' for v in vrel]}, gradient rel-L2 {whole:.2e}, "
          f"worst tensor {per:.2e}, post-Adam weights {np.abs(w - ref_w).max():.2e}, counters {adv}")
    assert np.isfinite(got).all() and np.isfinite(g).all()
    for a, b in zip(got, ref_vals):
        assert abs(a - b) <= TW.REL * abs(b), (got, ref_vals)          # (an absent phase: exactly 0)
    assert whole <= TW.REL, whole
    assert per <= TW.TENSOR, per
    w_from_g = _opt().apply(O.flatten_params(spec, params), g)
    np.testing.assert_allclose(w, w_from_g, atol=2e-6)
    np.testing.assert_allclose(w, ref_w, atol=max(TW.ADAM_ATOL, 10 * np.abs(g - ref_g).max()))
    return adv, got, g


def _check_ws_counters(name, coef, path, adv):
    """One call; the GM_FIT counter of the path expected() names, one per encoder layer; no engine; no own dreams."""
    e = SS.WS_CASES[name]
    mine = SS.expected(name, e, path, coef)["fit_counter"]
    assert adv[35] == 1 and adv[mine] == len(e[0]) and adv[73 - mine] == 0 and adv[2] == 0 and adv[38] == 0, (adv, mine)


# ------------------------------------------------------- wake-sleep: parity
@pytest.mark.parametrize("name,coef,path", WS_PARITY, ids=[f"{n}-{SS.COEF_ID[c]}-{p}" for n, c, p in WS_PARITY])
def test_wake_sleep_parity_with_reference(name, coef, path):
    """The three values, the whole gradient, every parameter tensor and the post-Adam weights against
    wakesleep_ref.train_step in float64.  A "fused" request on D5, D8 or W512 succeeds and counts under 37."""
    adv, _, _ = _ws_step_and_check(name, coef, path, kernel_path=path)
    _check_ws_counters(name, coef, path, adv)
    if path == "fused" and name in ("D5", "D8", "W512"):
        assert adv[37] == len(SS.WS_CASES[name][0]) and adv[36] == 0, adv


@pytest.mark.parametrize("name", ["D4", "D5", "W511", "W512"])
def test_wake_sleep_automatic_path(name):
    adv, _, _ = _ws_step_and_check(name, MIX, "auto")
    _check_ws_counters(name, MIX, "auto", adv)
    assert (adv[36] > 0) == (name in ("D4", "W511")), adv


# -------------------------------------------------- wake-sleep: bit for bit
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", ["O2", "R40p5"])
def test_wake_sleep_value_is_the_iwae_steps_bit_for_bit(name, path):
    a, x, eps, dreams = _ws_model(name, kernel_path=path)
    b, _, _, _ = _ws_model(name, kernel_path=path)
    la = a.train_step(x, eps=eps)["IWAE"]
    lb = b.wake_sleep_step(x, 0.5, 0.5, dreams=dreams, eps=eps)["IWAE"]
    assert np.isfinite(la) and _bits(la) == _bits(lb), (la, lb)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", ["O2", "R40p5"])
def test_wake_sleep_decoder_gradient_is_the_iwae_steps_bit_for_bit(name, path):
    a, x, eps, _ = _ws_model(name, kernel_path=path)
    a.wake_sleep_step(x, 1.0, 0.0, eps=eps, update=False)
    b, _, _, _ = _ws_model(name, kernel_path=path)
    xd = b._x(x)
    arr, n, keep = b._eps(eps, xd.shape[0], b.k)
    b._forward_backward(b._lc(), xd, xd.shape[0], arr, n)
    b._stream.synchronize()
    ne = PR.enc_size(SS.ws_case(name)[4][0])
    ga, gb = _flat(a.get_gradients()), _flat(b.get_gradients())
    assert np.isfinite(ga).all()
    assert np.array_equal(ga[ne:], gb[ne:])
    assert not np.array_equal(ga[:ne], gb[:ne])


# --------------------------------------- wake-sleep: own dreams, x_dim % 4 != 0
@pytest.mark.parametrize("path", [None, "layerwise"], ids=["auto", "layerwise"])
def test_own_dreams_at_an_odd_x_dim_are_generates_at_that_noise_position(path):
    """test_own_dreams_are_generates_at_that_noise_position on O2's model (x_dim 37: the dream pixels' row
    stride r4(x_dim) = 40 is not x_dim), n = 11."""
    kw = {} if path is None else {"kernel_path": path}
    n, seed = 11, 4242
    assert SS.WS_CASES["O2"][4] % 4 != 0
    a, x, _, _ = _ws_model("O2", seed=seed, **kw)
    ca = _counts(a)
    va = a.wake_sleep_step(x, 0.5, 0.5, n_dream=n, update=False)
    assert _adv(a, ca)[38] == 1
    # twin B: the wake forward's draw, then generate's, from the same seed
    b, _, _, _ = _ws_model("O2", seed=seed, **kw)
    xd = b._x(x)
    b._forward_backward(b._lc(), xd, xd.shape[0], None, 0)
    s = b.sample(n, return_probs=False, return_latents=True)
    dreams = (s["x"].contiguous(), s["h"])
    # twin C: fed x and those dreams at the same seed
    c, _, _, _ = _ws_model("O2", seed=seed, **kw)
    cc = _counts(c)
    vc = c.wake_sleep_step(x, 0.5, 0.5, dreams=dreams, update=False)
    assert _adv(c, cc)[38] == 0
    assert np.isfinite(_values(va)).all() and va["sleep"] != 0.0
    assert _bits(_values(va)) == _bits(_values(vc))
    np.testing.assert_array_equal(_flat(a.get_gradients()), _flat(c.get_gradients()))
    # the noise position afterwards is the twin's
    sa, sb = a.sample(5, return_probs=False), b.sample(5, return_probs=False)
    assert np.array_equal(sa["x"].cpu().numpy(), sb["x"].cpu().numpy())


# ------------------------------------------------- wake-sleep: stale rows
@pytest.mark.parametrize("path", PATHS)
def test_no_stale_dream_rows_across_a_change_of_rows(path):
    """R5p40's shape under the mix leaves 40 dream rows behind 15 wake rows (5 image rows); R20p20's shape
    wake-only then covers them with its 60 wake rows (20 image rows): a fresh model's bits."""
    assert SS.WS_CASES["R5p40"][6] == SS.WS_CASES["R20p20"][6]          # one k
    a, x, eps, _ = _ws_model("R20p20", kernel_path=path)
    x5, eps5, dreams5 = _ws_inputs("R5p40")
    a.wake_sleep_step(x5, 0.5, 0.5, dreams=dreams5, eps=eps5, update=False)
    va = a.wake_sleep_step(x, 1.0, 0.0, eps=eps, update=False)
    a.check_kernel_status()
    b, _, _, _ = _ws_model("R20p20", kernel_path=path)
    vb = b.wake_sleep_step(x, 1.0, 0.0, eps=eps, update=False)
    assert np.isfinite(_values(vb)).all()
    assert _bits(_values(va)) == _bits(_values(vb))
    np.testing.assert_array_equal(_flat(a.get_gradients()), _flat(b.get_gradients()))


# ------------------------------------------------------------ masked: parity
def _masked_counts(m):
    return [int(m._lib.iwae_debug_count(m._h, i)) for i in MASKED_IDS]


def _masked_step_and_check(name, loss, tag, knobs=None, **kw):
    """test_gpu_missing._step_and_check with the row-block forward counter; returns (counters' advance, loss bits, gradient)."""
    m, x, mask, eps = TM._model(name, loss, **kw)
    for knob, v in (knobs or {}).items():
        m.set_tuning(knob, v)
    spec, params = SS.masked_case(name)[4][:2]
    c0 = _masked_counts(m)
    loss_gpu = m.train_step(x, eps=eps, mask=mask)[loss]
    m.check_kernel_status()
    adv = [b - a for a, b in zip(c0, _masked_counts(m))]
    ref_loss, ref_g, ref_w = SS.masked_reference(name, loss)
    g, w = _flat(m.get_gradients()), _flat(m.get_weights())
    whole, per = PR.rel_l2(g, ref_g), M.worst_tensor(spec, g, ref_g)
    print(f"{name} {loss} {tag}: loss rel {abs(loss_gpu - ref_loss) / abs(ref_loss):.2e}, gradient rel-L2 {whole:.2e}, "
          f"worst tensor {per:.2e}, post-Adam weights {np.abs(w - ref_w).max():.2e}, counters {dict(zip(MASKED_IDS, adv))}")
    assert np.isfinite(loss_gpu) and np.isfinite(g).all()
    assert abs(loss_gpu - ref_loss) <= TM.REL * abs(ref_loss), (loss_gpu, ref_loss)
    assert whole <= TM.REL, whole
    assert per <= TM.TENSOR, per
    w_from_g = _opt().apply(O.flatten_params(spec, params), g)
    np.testing.assert_allclose(w, w_from_g, atol=2e-6)
    np.testing.assert_allclose(w, ref_w, atol=max(TM.ADAM_ATOL, 10 * np.abs(g - ref_g).max()))
    return adv, loss_gpu, g


@pytest.mark.parametrize("name,loss,path", MASKED_PARITY, ids=["-".join(c) for c in MASKED_PARITY])
def test_masked_parity_with_reference(name, loss, path):
    (bern, engine, ring, rb), _, _ = _masked_step_and_check(name, loss, path, kernel_path=path)
    exp = SS.expected(name, SS.MASKED_CASES[name], path)
    assert bern > 0 and engine == 0 and ring == 0, (bern, engine, ring)
    assert (rb > 0) == exp["row_block"], (rb, exp)


# ----------------------------------------- masked: the bound, and bit for bit
@pytest.mark.parametrize("path", ["auto", "layerwise"])
@pytest.mark.parametrize("name", SS.BOUND_CASES)
def test_masked_bound_against_reference(name, path):
    m, x, mask, eps = TM._model(name, "IWAE", kernel_path=path)
    _, _, k, _, (spec, params, _, x64, eps64, _, mask64) = SS.masked_case(name)
    c0 = TM._counts(m)
    got = m.get_L_k(x, k, eps=eps, mask=mask)
    m.check_kernel_status()
    assert TM._counts(m)[0] - c0[0] == 1
    ref = M.objective_and_grads(params, spec, x64, mask64, eps64, "IWAE", with_grads=False)[0]
    print(f"{name} {path}: bound {got:.6f}, reference {ref:.6f}, rel {abs(got - ref) / abs(ref):.2e}")
    assert abs(got - ref) <= 1e-4 * abs(ref), (got, ref)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", ["O2", "O2w"])
def test_all_ones_mask_is_the_unmasked_step_bit_for_bit(name, path):
    outs = []
    for masked in (False, True):
        m, x, mask, eps = TM._model(name, "IWAE", kernel_path=path)
        xc = np.where(mask != 0, x, 0).astype(np.float32)
        kw = {"mask": np.ones_like(mask)} if masked else {}
        outs.append(TM._bits(m, m.train_step(xc, eps=eps, **kw)["IWAE"]))
        m.check_kernel_status()
    assert np.isfinite(np.frombuffer(outs[0][0] + outs[0][1] + outs[0][2], np.float32)).all()
    assert outs[0][0] == outs[1][0], "loss"
    assert outs[0][1] == outs[1][1], "gradients"
    assert outs[0][2] == outs[1][2], "weights"


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", ["O2", "D4"])
def test_nan_or_zero_at_the_missing_entries_changes_no_bit(name, path):
    outs = []
    for fill in (np.nan, 0.0):
        m, x, mask, eps = TM._model(name, "IWAE", kernel_path=path)
        outs.append(TM._bits(m, m.train_step(M.with_holes(x, mask, fill), eps=eps, mask=mask)["IWAE"]))
        m.check_kernel_status()
    assert np.isfinite(np.frombuffer(outs[0][0] + outs[0][1] + outs[0][2], np.float32)).all()
    assert outs[0] == outs[1]


# ----------------------------- the output layer on bf16x3 products, 66 rows
@pytest.mark.parametrize("path", ["layerwise", "fused"])
def test_output_layer_on_bf16x3_products_at_a_small_shape(path):
    """set_tuning("out_x3_rows", 16) on O2w (66 sample rows; output Dense 65 -> 66, both off 32: the split
    weight copy is padded): the wake-sleep mix step and the masked IWAE step meet float64 at the usual bars,
    L_theta has the bits of an IWAE train step under the same knob, and the knob at 0 changes a bit of each."""
    name, knob = SS.OUT_X3_CASE, {"out_x3_rows": SS.OUT_X3_ROWS}
    off = {"out_x3_rows": 0}
    assert SS.expected(name, SS.WS_CASES[name], path, out_x3_rows=SS.OUT_X3_ROWS)["out_x3"]
    adv, vals, g = _ws_step_and_check(name, MIX, f"{path} out_x3", kernel_path=path, knobs=knob)
    _check_ws_counters(name, MIX, path, adv)
    m, x, eps, _ = _ws_model(name, kernel_path=path, knobs=knob)
    la = m.train_step(x, eps=eps)["IWAE"]
    assert _bits(la) == _bits(vals[0]), (la, vals[0])
    _, vals0, g0 = _ws_step_and_check(name, MIX, f"{path} out_x3 off", kernel_path=path, knobs=off)
    assert _bits(vals) != _bits(vals0) or not np.array_equal(g, g0)
    (bern, engine, ring, rb), lm, gm = _masked_step_and_check(name, "IWAE", f"{path} out_x3", knobs=knob, kernel_path=path)
    assert bern > 0 and engine == 0 and ring == 0
    _, lm0, gm0 = _masked_step_and_check(name, "IWAE", f"{path} out_x3 off", knobs=off, kernel_path=path)
    assert _bits(lm) != _bits(lm0) or not np.array_equal(gm, gm0)
