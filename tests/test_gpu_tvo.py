"""The thermodynamic variational objective on the GPU (iwae_tvo_step / _grad /
_weights) against the float64 reference (tests/tvo_ref.py) on identical
injected noise and weights, on the fused row-block path and the layer-wise
path, at the smallest shapes that reach every branch (tvo_ref.CASES):

  T1   1 layer, 15 rows (one partial 16-row tile), every width below 32
  T2   2 layers, 35 ragged rows: an upper layer whose input latent is data
  T2w  33 images: beyond the few-row launches of the first layer
  T3   3 layers: a middle layer
  T4   d = 70 > 64: second lane pass of the element-wise kernel
  Tk1  T2's model at k = 1 (a_theta = 1, a_phi = -1)

over the partitions P1 = [0, 1], P5 = tvo_schedule(5), and on T2 also
P2 = [0, 0.3, 1] and P64 (65 equal steps, the largest).

Bars: test_gpu_wakesleep.py's (the three values and the whole gradient 1e-4
relative, each parameter tensor 5e-4 of its largest entry, its Adam check).
tests/test_tvo_ref.py shows the reference run in float32 stays within a
quarter of them on these very inputs.  Every test prints what it measured."""
import functools

import numpy as np
import pytest

import pathgrad_ref as PR
import tvo_ref as T
from oracle import iwae_oracle as O

pytestmark = pytest.mark.gpu

REL = 1e-4
TENSOR = 5e-4
ADAM_ATOL = 6e-5
IDS = (2, 36, 37, 42, 43)          # engine launches; GM_FIT row-block jobs, GM_FIT launches; TVO calls, tvo_kernel launches
FIT_COUNTER = {"fused": 36, "layerwise": 37}
EPS32 = 2.0 ** -23


def _flat(ws):
    return np.concatenate([np.asarray(w, np.float64).ravel() for w in ws])


def _bits(a):
    return np.asarray(a, np.float32).tobytes()


@functools.lru_cache(maxsize=None)
def _case(name):
    return T.case(name)


@functools.lru_cache(maxsize=None)
def _reference(name, part):
    """((L_tvo, L_upper, L_iwae), flat gradient, post-Adam flat weights) in float64, computed once."""
    spec, params, _, x, eps = _case(name)[3]
    vals, new, g = T.train_step(params, spec, x, eps, T.PARTS[part], O.Adam(1e-3, 0.9, 0.999, 1e-4))
    w = O.flatten_params(spec, new)
    g.setflags(write=False)
    w.setflags(write=False)
    return tuple(float(v) for v in vals), g, w


def _model(name, loss="IWAE", **kw):
    from iwae_replication_project_amd import Adam, Flexible_Model
    from iwae_replication_project_amd.flexible_iwae import _split, weight_shapes
    (he, hd, le, ld), B, k, (spec, params, mean, x, eps) = _case(name)
    kw.setdefault("seed", 1)
    m = Flexible_Model(he, hd, le, ld, dataset_bias=mean, loss_function=loss, k=k, x_dim=T.X_DIM, **kw)
    m.set_weights(_split(O.flatten_params(spec, params).astype(np.float32), weight_shapes(m.dense)))
    m.compile(Adam(learning_rate=1e-3, epsilon=1e-4))
    return m, x.astype(np.float32), [e.astype(np.float32) for e in eps]


def _counts(m):
    return {i: int(m._lib.iwae_debug_count(m._h, i)) for i in IDS}


def _adv(m, c0):
    c1 = _counts(m)
    return {i: c1[i] - c0[i] for i in IDS}


def _values(out):
    return (out["TVO"], out["TVO_upper"], out["IWAE"])


# ------------------------------------------------------------------- parity
@pytest.mark.parametrize("path", ["fused", "layerwise"])
@pytest.mark.parametrize("name,part", T.CASE_PARTS)
def test_parity_with_reference(name, part, path):
    m, x, eps = _model(name, kernel_path=path)
    spec, params = _case(name)[3][:2]
    c0 = _counts(m)
    got = _values(m.tvo_step(x, betas=T.PARTS[part], eps=eps))
    m.check_kernel_status()
    adv = _adv(m, c0)
    ref_vals, ref_g, ref_w = _reference(name, part)
    g, w = _flat(m.get_gradients()), _flat(m.get_weights())
    whole = PR.rel_l2(g, ref_g)
    per = [np.abs(a - b).max() / np.abs(b).max() for a, b in zip(PR.split_tensors(spec, g), PR.split_tensors(spec, ref_g))]
    vrel = [abs(a - b) / abs(b) for a, b in zip(got, ref_vals)]
    print(f"{name} {part} {path}: values rel {[f'{v:.2e}' for v in vrel]}, gradient rel-L2 {whole:.2e}, "
          f"worst tensor {max(per):.2e}, counters {adv}")
    for a, b in zip(got, ref_vals):
        assert abs(a - b) <= REL * abs(b), (got, ref_vals)
    assert whole <= REL, whole
    assert max(per) <= TENSOR, per
    w_from_g = O.Adam(1e-3, 0.9, 0.999, 1e-4).apply(O.flatten_params(spec, params), g)
    np.testing.assert_allclose(w, w_from_g, atol=2e-6)
    np.testing.assert_allclose(w, ref_w, atol=max(ADAM_ATOL, 10 * np.abs(g - ref_g).max()))
    # counters: one call, one tvo_kernel launch, the path's own GM_FIT counter once per encoder layer, never the engine
    mine = FIT_COUNTER[path]
    assert adv[42] == 1 and adv[43] == 1 and adv[mine] == spec.L and adv[73 - mine] == 0 and adv[2] == 0, adv


@pytest.mark.parametrize("path", ["fused", "layerwise"])
def test_parity_beyond_one_workgroup(path):
    """T1's model at B = 65, k = 127: 8255 rows, the smallest batch on the far
    side of bound_grid's rule (B > 64 and B k > 8192), where the three batch
    values are summed by the last workgroup to arrive.  Same bars."""
    from iwae_replication_project_amd import Adam, Flexible_Model
    from iwae_replication_project_amd.flexible_iwae import _split, weight_shapes
    (he, hd, le, ld), B, k, (spec, params, mean, x, eps) = T.multi_case()
    betas = T.PARTS["P5"]
    ref_vals, _, ref_g = T.train_step(params, spec, x, eps, betas, O.Adam(1e-3, 0.9, 0.999, 1e-4))
    m = Flexible_Model(he, hd, le, ld, dataset_bias=mean, loss_function="IWAE", k=k, x_dim=T.X_DIM, seed=1,
                       kernel_path=path)
    m.set_weights(_split(O.flatten_params(spec, params).astype(np.float32), weight_shapes(m.dense)))
    m.compile(Adam(learning_rate=1e-3, epsilon=1e-4))
    e32 = [e.astype(np.float32) for e in eps]
    got = [_values(m.tvo_step(x.astype(np.float32), betas=betas, eps=e32, update=False)) for _ in range(2)]
    m.check_kernel_status()
    g = _flat(m.get_gradients())
    whole = PR.rel_l2(g, ref_g)
    per = [np.abs(a - b).max() / np.abs(b).max() for a, b in zip(PR.split_tensors(spec, g), PR.split_tensors(spec, ref_g))]
    vrel = [abs(a - float(b)) / abs(float(b)) for a, b in zip(got[0], ref_vals)]
    print(f"B 65 k 127 P5 {path}: values rel {[f'{v:.2e}' for v in vrel]}, gradient rel-L2 {whole:.2e}, "
          f"worst tensor {max(per):.2e}")
    assert max(vrel) <= REL and whole <= REL and max(per) <= TENSOR
    assert _bits(got[0]) == _bits(got[1])                # the ticket is back at 0: a second call, the same bits


def test_default_path_is_row_block():
    m, x, eps = _model("T2")
    c0 = _counts(m)
    m.tvo_step(x, eps=eps)
    adv = _adv(m, c0)
    assert adv[36] == 2 and adv[37] == 0 and adv[2] == 0 and adv[42] == 1, adv


# ------------------------------------------------ iwae_tvo_weights on its own
def _host_lw(N, k, spread, seed):
    """Uniform over `spread` nats around -300, an image model's range: every
    value of the sandwich then lies in [-400, -200], away from 0, where a
    relative error says nothing."""
    rng = np.random.default_rng(seed)
    return (-300.0 + spread * (rng.random((N, k)) - 0.5)).astype(np.float32)


def _check_weights(got, lw, betas, tag):
    """Device outputs against float64 of the same float32 lw."""
    ref = T.tvo_terms(lw.astype(np.float64).T, betas)
    J = len(betas) - 1
    errs = {}
    for key in ("a_theta", "a_phi"):
        a, r = got[key].cpu().numpy().astype(np.float64), ref[key].T
        errs[key] = float((np.abs(a - r).max(1) / np.abs(r).max(1)).max())
    for key in ("lower", "upper", "iwae"):
        v, r = got[key].cpu().numpy().astype(np.float64), ref[key]
        errs[key] = float((np.abs(v - r) / np.abs(r)).max())
    s_theta = float(np.abs(got["a_theta"].cpu().numpy().astype(np.float64).sum(1) - 1).max())
    s_phi = float(np.abs(got["a_phi"].cpu().numpy().astype(np.float64).sum(1) + 1).max())
    lo, up, iw = (got[key].cpu().numpy().astype(np.float64) for key in ("lower", "upper", "iwae"))
    # each value is max + a term within the spread, summed over J intervals in float32
    tol = (J + 8) * EPS32 * np.abs(lw.astype(np.float64)).max(1)
    gap = float(np.maximum(lo - iw, iw - up).max())
    print(f"{tag}: {', '.join(f'{k_} {v:.2e}' for k_, v in errs.items())}, |sum a_theta - 1| {s_theta:.2e}, "
          f"|sum a_phi + 1| {s_phi:.2e}, sandwich excess {gap:.2e} (allowed {tol.max():.2e})")
    for key, v in errs.items():
        assert v <= 1e-4, (key, v)
    assert s_theta <= 1e-4 and s_phi <= 1e-4
    assert (lo <= iw + tol).all() and (iw <= up + tol).all()


# N = 3 below the multi-workgroup rule; (64, 129) and (65, 126) on its single-workgroup side (N <= 64, N k <= 8192),
# (65, 127) the smallest beyond both
WEIGHT_SHAPES = [(3, 1), (3, 5), (3, 64), (3, 65), (3, 1024), (3, 1025), (64, 129), (65, 126), (65, 127)]


@pytest.mark.parametrize("spread", [4.0, 200.0])
@pytest.mark.parametrize("N,k", WEIGHT_SHAPES)
def test_weights_against_float64(N, k, spread):
    m, _, _ = _model("T1")
    lw = _host_lw(N, k, spread, 100 + k)
    for part in ("P1", "P5", "P64"):
        betas = T.PARTS[part]
        got = m.tvo_bounds(lw, betas, want=("lower", "upper", "iwae", "a_theta", "a_phi"))
        m.check_kernel_status()
        _check_weights(got, lw, betas, f"N {N} k {k} spread {spread:g} {part}")


def test_weights_leave_every_state_alone_and_outputs_are_optional():
    m, x, eps = _model("T2", seed=5)
    ref, _, _ = _model("T2", seed=5)
    lw = _host_lw(5, 7, 4.0, 3)
    c0 = _counts(m)
    full = m.tvo_bounds(lw, T.PARTS["P5"], want=("lower", "upper", "iwae", "a_theta", "a_phi"))
    for key in full:
        one = m.tvo_bounds(lw, T.PARTS["P5"], want=(key,))
        assert list(one) == [key] and _bits(one[key].cpu().numpy()) == _bits(full[key].cpu().numpy())
    adv = _adv(m, c0)
    assert adv[43] == 6 and adv[42] == 0 and adv[2] == 0, adv
    assert np.array_equal(_flat(m.get_weights()), _flat(ref.get_weights()))
    sa, sb = m.sample(4, return_probs=False), ref.sample(4, return_probs=False)
    assert np.array_equal(sa["x"].cpu().numpy(), sb["x"].cpu().numpy())
    # the model's own log weights: the batch means of the sandwich
    lo, up, iw = m.get_L_TVO(x, 6, eps=None)
    print(f"get_L_TVO: lower {lo:.4f} iwae {iw:.4f} upper {up:.4f}")
    assert lo <= iw <= up


@pytest.mark.parametrize("poison", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("k", [5, 1025])
def test_a_non_finite_log_weight_poisons_its_image_only(k, poison):
    m, _, _ = _model("T1")
    lw = _host_lw(3, k, 4.0, 9)
    want = ("lower", "upper", "iwae", "a_theta", "a_phi")
    clean = m.tvo_bounds(lw, T.PARTS["P5"], want=want)
    bad = lw.copy()
    bad[1, k // 2] = poison
    got = m.tvo_bounds(bad, T.PARTS["P5"], want=want)
    m.check_kernel_status()
    for key in want:
        c, g = clean[key].cpu().numpy(), got[key].cpu().numpy()
        assert not np.isfinite(g[1]).any(), key
        assert _bits(g[0]) == _bits(c[0]) and _bits(g[2]) == _bits(c[2]), key


# --------------------------------------------------------- one interval: VAE
@pytest.mark.parametrize("path", ["fused", "layerwise"])
@pytest.mark.parametrize("name", ["T2", "T2w"])
def test_one_interval_decoder_gradient_is_the_vae_steps(name, path):
    a, x, eps = _model(name, kernel_path=path)
    va = a.tvo_step(x, betas=T.PARTS["P1"], eps=eps, update=False)
    b, _, _ = _model(name, loss="VAE", kernel_path=path)
    xd = b._x(x)
    arr, n, keep = b._eps(eps, xd.shape[0], b.k)
    b._forward_backward(b._lc(), xd, xd.shape[0], arr, n)
    b._stream.synchronize()
    ne = PR.enc_size(_case(name)[3][0])
    ga, gb = _flat(a.get_gradients()), _flat(b.get_gradients())
    err = PR.rel_l2(ga[ne:], gb[ne:])
    print(f"{name} {path}: J = 1 decoder gradient vs the VAE step's, rel-L2 {err:.2e}")
    assert err <= REL, err
    assert va["TVO"] >= va["IWAE"] >= va["TVO_upper"]


@pytest.mark.parametrize("path", ["fused", "layerwise"])
def test_grad_then_adam_equals_step(path):
    a, x, eps = _model("T2", kernel_path=path)
    va = a.tvo_step(x, betas=T.PARTS["P5"], eps=eps)
    b, _, _ = _model("T2", kernel_path=path)
    vb = b.tvo_step(x, betas=T.PARTS["P5"], eps=eps, update=False)
    assert b.get_optimizer_state()[2] == 0                   # Adam state moves only in _step
    assert np.array_equal(_flat(b.get_weights()), O.flatten_params(*_case("T2")[3][:2]).astype(np.float32))
    b._apply_adam(1.0)
    b._stream.synchronize()
    assert _bits(_values(va)) == _bits(_values(vb))
    np.testing.assert_array_equal(_flat(a.get_gradients()), _flat(b.get_gradients()))
    np.testing.assert_array_equal(_flat(a.get_weights()), _flat(b.get_weights()))
    assert a.get_optimizer_state()[2] == b.get_optimizer_state()[2] == 1


# ---------------------------------------------------- determinism and state
def test_device_noise_determinism_and_noise_position():
    rng = np.random.default_rng(5)
    B = _case("T2")[1]
    xs = (rng.random((3 * B, T.X_DIM)) < 0.3).astype(np.float32)
    ws, vs = [], []
    for _ in range(2):
        m, _, _ = _model("T2", seed=77)
        v = m.tvo_steps(xs, B, n_part=5)
        m.check_kernel_status()
        assert v.shape == (3, 3) and np.isfinite(v).all()
        assert (v[:, 0] >= v[:, 2]).all() and (v[:, 2] >= v[:, 1]).all()
        ws.append(_flat(m.get_weights()))
        vs.append(v)
    assert np.array_equal(ws[0], ws[1]) and _bits(vs[0]) == _bits(vs[1])
    w0 = O.flatten_params(*_case("T2")[3][:2])
    assert np.abs(ws[0] - w0).max() > 1e-4       # the steps moved the weights
    assert m.epoch == 3
    # one step advances the noise position once, as one forward-backward pass does
    a, x, _ = _model("T2", seed=4242)
    a.tvo_step(x, update=False)
    b, _, _ = _model("T2", seed=4242)
    xd = b._x(x)
    b._forward_backward(b._lc(), xd, xd.shape[0], None, 0)
    sa, sb = a.sample(5, return_probs=False), b.sample(5, return_probs=False)
    assert np.array_equal(sa["x"].cpu().numpy(), sb["x"].cpu().numpy())


def test_captured_train_steps_replay_around_a_tvo_call():
    """A graph-captured train_steps run before and after a TVO step that fits
    the workspace replays: nothing is captured again."""
    m, x, eps = _model("T1")
    rng = np.random.default_rng(6)
    xs = (rng.random((2 * 40, T.X_DIM)) < 0.3).astype(np.float32)        # 40 x 5 = 200 sample rows: room for T1's 15
    m.train_steps(xs, 40)
    caps = m.graph_captures()
    assert caps >= 1
    m.tvo_step(x, eps=eps)
    losses = m.train_steps(xs, 40)
    m.check_kernel_status()
    assert np.isfinite(losses).all()
    assert m.graph_captures() == caps


# ------------------------------------------------------------------- errors
def _fp(a):
    from iwae_replication_project_amd import _lib
    return None if a is None else a.ctypes.data_as(_lib.FP)


def test_every_invalid_argument_is_rejected_before_any_launch():
    from iwae_replication_project_amd import _lib
    m, x, eps = _model("T2", seed=9)
    ref, _, _ = _model("T2", seed=9)
    L = 2
    xd = m._x(x)
    vals = m._scratch.new_zeros(3)
    B, k = xd.shape[0], 5
    X, V = _lib.fptr(xd), _lib.fptr(vals)
    f32 = lambda *v: np.array(v, dtype=np.float32)
    good = f32(0, 0.3, 1)
    long66 = np.linspace(0, 1, 66).astype(np.float32)
    bad_betas = [(f32(0, np.nan, 1), 2), (f32(0, np.inf, 1), 2), (f32(0, 0.5, 0.5, 1), 3), (f32(0, 0.6, 0.4, 1), 3),
                 (f32(0.1, 0.5, 1), 2), (f32(0, 0.5, 0.9), 2), (f32(-0.5, 0, 1), 2), (good, 0), (good, -1), (long66, 65)]
    # (cfg fields, betas, x, B)
    bad = [(None, good, X, B),                              # cfg NULL
           ((k, 2), None, X, B),                            # betas NULL
           ((k, 2), good, None, B),                         # x NULL
           ((0, 2), good, X, B),                            # k < 1
           ((k, 2), good, X, 0),                            # B < 1
           ((1 << 28, 2), good, X, 8)]                      # B k above 2^30
    bad += [((k, J), b, X, B) for b, J in bad_betas]
    arr, ne, keep = m._eps(eps, B, k)
    holes = (_lib.FP * L)(_lib.fptr(keep[0]), None)
    for fn in (m._lib.iwae_tvo_step, m._lib.iwae_tvo_grad):
        for cfgv, b, xp, nb in bad:
            cfg = None if cfgv is None else _lib.IwaeTvoConfig(*cfgv)
            assert fn(m._h, cfg, _fp(b), xp, nb, None, 0, V) == -1, (cfgv, b, nb)
            assert m._lib.iwae_last_error(m._h), cfgv
        cfg = _lib.IwaeTvoConfig(k, 2)
        assert fn(m._h, cfg, _fp(good), X, B, arr, 1, V) == -1          # a wrong n_eps
        assert fn(m._h, cfg, _fp(good), X, B, holes, L, V) == -1        # a NULL eps[i]
    # iwae_tvo_weights
    lw = m._scratch.new_zeros(3 * 5)
    out = m._scratch.new_zeros(3)
    LW, OUT = _lib.fptr(lw), _lib.fptr(out)
    W = m._lib.iwae_tvo_weights
    none5 = (None,) * 5
    outs = (OUT, None, None, None, None)
    assert W(m._h, None, 3, 5, _fp(good), 2, *outs) == -1               # lw NULL
    assert W(m._h, LW, 3, 5, None, 2, *outs) == -1                      # betas NULL
    assert W(m._h, LW, 0, 5, _fp(good), 2, *outs) == -1                 # N < 1
    assert W(m._h, LW, 3, 0, _fp(good), 2, *outs) == -1                 # k < 1
    assert W(m._h, LW, 1, (1 << 20) + 1, _fp(good), 2, *outs) == -1     # k above 2^20
    assert W(m._h, LW, 1 << 11, 1 << 20, _fp(good), 2, *outs) == -1     # N k above 2^30
    assert W(m._h, LW, 3, 5, _fp(good), 2, *none5) == -1                # every output NULL
    for b, J in bad_betas:
        assert W(m._h, LW, 3, 5, _fp(b), J, *outs) == -1, (b, J)
    with pytest.raises(ValueError):
        m.tvo_step(x, betas=[0.0, 0.5, 0.5, 1.0])
    with pytest.raises(ValueError):
        m.tvo_bounds(np.zeros((3, 5), np.float32), good, want=())
    for i in IDS:
        assert int(m._lib.iwae_debug_count(m._h, i)) == 0, i
    # the noise position is where a fresh model's is
    sa, sb = m.sample(4, return_probs=False), ref.sample(4, return_probs=False)
    assert np.array_equal(sa["x"].cpu().numpy(), sb["x"].cpu().numpy())
    assert np.array_equal(_flat(m.get_weights()), _flat(ref.get_weights()))


def test_data_parallel_driver_is_refused():
    m, x, eps = _model("T1")
    m._dp = object()
    try:
        with pytest.raises(ValueError, match="data parallel"):
            m.tvo_step(x)
        with pytest.raises(ValueError, match="data parallel"):
            m.tvo_steps(x, 1)
    finally:
        m._dp = None
