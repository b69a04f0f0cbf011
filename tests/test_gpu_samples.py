"""Sample-axis sweep on the GPU: every case of tests/sample_cases.py (k on both
sides of the lane stride, of the in-launch bound's limits, of the LDS-staged
limit; image counts on both sides of the one-workgroup rule; log-weights spread
beyond float32's exp range; tied medians) against the float64 oracle on
identical injected noise and weights, with the launch counters 15 and 16 pinning
which home of the bound arithmetic ran (sample_cases.expected_bound).

Bars, the project's own (tests/test_gpu_shapes.py): loss and whole gradient
1e-4 relative, each parameter tensor 5e-4 of its largest entry, Adam as
test_gpu_configs._check, log-weights 1e-4 of max|ref|, bounds 1e-4 relative,
log p(x) 1e-3 nats.  tests/test_sample_cases.py shows the reference run in
float32 stays within a quarter of them on these very inputs.

Measured on an MI355X over all cases, losses and paths (763 train steps): loss
6.1e-6, whole gradient 6.1e-5 (K65 on S2, L_power_p with p = 2.5, engine), worst
tensor 1.6e-4 (K1025 on S2, the same loss), post-Adam weights 6.0e-6;
log-weights 2.5e-5 of max|lw|, forward-only bounds 1.4e-5, log p(x) 1.4e-4 nats
(k = 1).  WIDE: gradient 4.0e-5, worst tensor 1.1e-4; TIE: 1.5e-5 and 4.7e-5.

With three loops of a library copy made wrong on purpose -- image_grad's MIWAE
stride over k1 and its squared-softmax stride 128 for 64, bound_kernel's
contrib[] re-sum one image short -- exactly the cases named for them fail:
MIWAE / PIWAE at K130 and K257, IWAE_DREG at K65, K257 and WIDE, everything at
M65, C33 and M1025."""
import functools

import numpy as np
import pytest

import pathgrad_ref as R
import sample_cases as C
from oracle import iwae_oracle as O
from test_gpu_shapes import ADAM_ATOL, LOGPX_ATOL, REL, TENSOR, _flat

pytestmark = pytest.mark.gpu

COUNTERS = (2, 13, 15, 16)
# kernel path, IWAE_KNOB_TC_BOUND
CONFIGS = {"auto": ("auto", 1), "auto_nobound": ("auto", 0), "fused": ("fused", 1), "layerwise": ("layerwise", 1)}
LDS_LAST_K = {"S1": 184, "S2": 184, "S3": 256}    # the largest k whose bound ran in the engine's launch
AUTO_ONLY = ("M1025-S1",)     # 66625 rows: the other paths' f32 GEMM chain adds nothing on the sample axis
TRAIN = [(n, v, c) for n, v in C.CASE_LOSS for c in CONFIGS if n not in AUTO_ONLY or c.startswith("auto")]


@functools.lru_cache(maxsize=None)
def _reference(name, vid):
    out = C.reference_step(name, vid)
    for a in out[1:]:
        a.setflags(write=False)
    return out


def _model(name, vid="IWAE", **kw):
    from iwae_replication_project_amd import Adam, Flexible_Model
    from iwae_replication_project_amd.flexible_iwae import _split, weight_shapes
    he, hd, le, ld, x_dim, B, k, seed = C.CASES[name]
    _, loss, lkw = C.variant(name, vid)
    spec, params, mean, x, eps = C.make(name)
    m = Flexible_Model(he, hd, le, ld, dataset_bias=mean, loss_function=loss, k=k, seed=1, x_dim=x_dim, **lkw, **kw)
    m.set_weights(_split(O.flatten_params(spec, params).astype(np.float32), weight_shapes(m.dense)))
    m.compile(Adam(learning_rate=1e-3, epsilon=1e-4))
    draws = eps + (C.second_draw(name) if loss == "CIWAE" else [])
    return m, x.astype(np.float32), [e.astype(np.float32) for e in draws]


def _counts(m):
    return {i: int(m._lib.iwae_debug_count(m._h, i)) for i in COUNTERS}


def _advance(m, before):
    return {i: v - before[i] for i, v in _counts(m).items()}


def _check_step(m, name, vid, loss_gpu, tag):
    """Loss, gradient (whole and per tensor) and post-Adam weights of a model
    after one train step against float64 (test_gpu_shapes' assertions)."""
    spec, params = C.make(name)[:2]
    ref_loss, ref_g, ref_w = _reference(name, vid)
    g, w = _flat(m.get_gradients()), _flat(m.get_weights())
    whole = R.rel_l2(g, ref_g)
    # (VAE_V1 leaves the decoder's prior layers an exactly zero gradient: 0 / tiny = 0)
    per = [np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)
           for a, b in zip(R.split_tensors(spec, g), R.split_tensors(spec, ref_g))]
    print(f"{tag}: loss rel {abs(loss_gpu - ref_loss) / abs(ref_loss):.2e}, gradient rel-L2 {whole:.2e}, "
          f"worst tensor {max(per):.2e}, post-Adam weights {np.abs(w - ref_w).max():.2e}")
    assert np.isfinite(loss_gpu) and np.isfinite(g).all() and np.isfinite(w).all()      # no NaN, no inf
    assert abs(loss_gpu - ref_loss) <= REL * abs(ref_loss), (loss_gpu, ref_loss)
    assert whole <= REL, whole
    assert max(per) <= TENSOR, per
    # Adam as test_gpu_configs._check
    w_from_g = O.Adam(1e-3, 0.9, 0.999, 1e-4).apply(O.flatten_params(spec, params), g)
    np.testing.assert_allclose(w, w_from_g, atol=2e-6)
    np.testing.assert_allclose(w, ref_w, atol=max(ADAM_ATOL, 10 * np.abs(g - ref_g).max()))


# ------------------------------------- a, c. train step (WIDE and TIE among the cases)
@pytest.mark.parametrize("name,vid,config", TRAIN, ids=["-".join(c) for c in TRAIN])
def test_train_step_matches_float64_in_the_expected_bound_home(name, vid, config):
    """One injected-noise train step against float64, and where its bound was
    computed: counter 15 (bound_kernel launches) stays 0 exactly where
    expected_bound says in-launch -- but for the cases of LDS_FALLBACK, whose
    engine plan leaves the in-launch bound too little LDS -- and is 1 elsewhere;
    counter 16 advances exactly where bound_kernel ran on several workgroups."""
    path, tc_bound = CONFIGS[config]
    _, loss, lkw = C.variant(name, vid)
    m, x, eps = _model(name, vid, kernel_path=path, tuning=dict(tc_bound=tc_bound))
    c0 = _counts(m)
    loss_gpu = m.train_step(x, eps=eps)[loss]
    m.check_kernel_status()
    adv = _advance(m, c0)
    home, groups = C.expected_bound(name, vid, path, bool(tc_bound))
    lds = home == "in-launch" and adv[15] > 0
    print(f"{name} {vid} {config}: expected {home} {groups}, counters {adv}"
          + (f"; LDS condition: bound_kernel ran at k = {C.CASES[name][6]}" if lds else ""))
    _check_step(m, name, vid, loss_gpu, f"{name} {vid} {config}")
    assert (adv[2] > 0) == C.on_engine(name, vid, path), adv
    if home == "in-launch":
        assert lds == (name in C.LDS_FALLBACK), (adv, name)
        assert adv[15] == (1 if lds else 0) and adv[16] == 0, adv
    else:
        assert adv[15] == 1 and adv[16] == (1 if groups > 1 else 0), (adv, groups)


def test_the_in_launch_bound_ran_at_every_named_point():
    """The train-step test pins counter 15 to expected_bound and LDS_FALLBACK:
    by them the in-launch bound ran at K17, K65, K128 and on both sides of B64 /
    K256's limits on some model, and K256 needed the wider S3 for it."""
    def ran(name, vid="IWAE"):
        return C.expected_bound(name, vid)[0] == "in-launch" and name not in C.LDS_FALLBACK
    for pt in ("K17", "K63", "K64", "K65", "K128", "K130", "K256", "B64"):
        assert any(ran(n) for n in C.CASES if C.POINT_OF.get(n) == pt), pt
    assert ran("K65-S2") and ran("K130-S2", "MIWAE") and ran("K17-S1", "L_median") and ran("K128-S1", "PIWAE")
    assert set(C.LDS_FALLBACK) == {"K256-S1"} and ran("K256-S3")
    assert C.MODELS["S3"][0] == [64]
    assert ran("WIDE") and ran("TIE64", "L_median") and ran("TIE65", "L_median")


@pytest.mark.parametrize("model", ["S1", "S2", "S3"])
def test_where_the_lds_condition_takes_the_in_launch_bound_away(model):
    """use_tc_bound's last condition (the engine plan's LDS holds 64 + 8 r4(k)
    floats ahead of its accumulators) by counter 15, k = 132 .. 256 in steps of 4
    on device noise: the in-launch bound is lost once, at a k that depends on the
    model's widths, and not regained.  S1 and S2 (every width pads to 32 columns:
    two LDS buffers of 16 rows x 48 bf16, hi and lo planes, 1536 floats) keep it
    to k = 184 = (1536 - 64) / 8; S3's 64-wide buffers keep it to the limit of 256."""
    from iwae_replication_project_amd import Flexible_Model
    he, le = C.MODELS[model]
    hd, ld = C.S._mirror(he, le, C.X_DIM)
    x = (np.random.default_rng(5).random((2, C.X_DIM)) < 0.3).astype(np.float32)
    ran = []
    for k in range(132, 257, 4):
        m = Flexible_Model(he, hd, le, ld, dataset_bias=np.full(C.X_DIM, 0.3), loss_function="IWAE", k=k, seed=1,
                           x_dim=C.X_DIM)
        c0 = _counts(m)
        assert np.isfinite(m.train_step(x)["IWAE"])
        adv = _advance(m, c0)
        assert adv[2] > 0 and adv[15] in (0, 1)
        ran.append(adv[15] == 0)
    last = max([132 + 4 * i for i, r in enumerate(ran) if r], default=None)
    print(f"{model} {he}: the in-launch bound runs up to k = {last}")
    assert ran == sorted(ran, reverse=True), ran
    assert last == LDS_LAST_K[model], last


# ------------------------------------------------------ b. forward-only bounds
def _bound(m, vid, loss, kw, k, x, eps):
    named = {"IWAE": lambda: m.get_L_k(x, k, eps=eps), "VAE": lambda: m.get_L(x, k, eps=eps),
             "L_median": lambda: m.get_L_median(x, k, eps=eps),
             "CIWAE": lambda: m.get_L_CIWAE(x, k, kw.get("beta"), eps=eps),
             "L_alpha": lambda: m.get_L_alpha(x, k, kw.get("alpha"), eps=eps),
             "L_power_p": lambda: m.get_L_power_p(x, k, kw.get("p"), eps=eps),
             "VAE_V1": lambda: m.get_L_V1(x, k, eps=eps),
             "MIWAE": lambda: m.get_L_MIWAE(x, kw.get("k1"), kw.get("k2"), eps=eps)}
    if loss in named:
        return named[loss]()
    return m._bound(m._lc(loss, k=k, **kw), x, eps)           # PIWAE, IWAE_STL, IWAE_DREG: the value of IWAE


@pytest.mark.parametrize("path", ["auto", "layerwise"])
@pytest.mark.parametrize("name", list(C.CASES))
def test_forward_only_bounds_and_log_weights_match_float64(name, path):
    """iwae_bound through the facade's get_L* / _bound for every loss of the
    case, and get_log_weights: bound_kernel without the gradient outputs, on
    one or several workgroups (counter 16), staged or not (K1025, M1025)."""
    he, hd, le, ld, x_dim, B, k, seed = C.CASES[name]
    m, x, eps = _model(name, C.loss_variants(name)[0][0], kernel_path=path)
    eps = eps[:len(he)]                                         # the first draw
    lw_ref = C.log_weights(name)
    c0 = _counts(m)
    lw = m.get_log_weights(x, k, eps=eps).cpu().numpy()
    adv = _advance(m, c0)
    e_lw = np.abs(lw - lw_ref).max() / np.abs(lw_ref).max()
    print(f"{name} {path}: log-weights {e_lw:.2e} of max|lw|, counters {adv}")
    assert lw.shape == lw_ref.shape and np.isfinite(lw).all()
    assert e_lw <= REL, e_lw
    several = B > 4 * C.BOUND_WAVES and B * k > C.BOUND_ROWS
    assert adv[15] == 1 and adv[16] == (1 if several else 0), adv
    for vid, loss, kw in C.loss_variants(name):
        draws = eps + ([e.astype(np.float32) for e in C.second_draw(name)] if loss == "CIWAE" else [])
        ref = C.reference_bound(name, vid)
        c0 = _counts(m)
        val = _bound(m, vid, loss, kw, k, x, draws)
        adv = _advance(m, c0)
        print(f"{name} {path} {vid}: bound rel {abs(val - ref) / abs(ref):.2e}, counters {adv}")
        assert np.isfinite(val) and abs(val - ref) <= REL * abs(ref), (vid, val, ref)
        assert adv[15] == 1 and adv[16] == (1 if C.expected_bound(name, vid, "layerwise")[1] > 1 else 0), (vid, adv)
    m.check_kernel_status()


# --------------------------------------------------------------- d. rejection
def test_losses_that_need_the_lds_copy_are_rejected_beyond_1024_samples():
    """L_median, MIWAE and PIWAE at k = 1025: ValueError from train_step and
    from the forward-only bound, before any launch (no counter moves, the
    weights and the Adam step stay); the same handle then runs an IWAE step at
    k = 1025 that matches float64.  (k = 1024 is accepted: K1024-S1 above.)"""
    name = "K1025-S1"
    k = C.CASES[name][6]
    m, x, eps = _model(name, "IWAE")
    w0 = _flat(m.get_weights())
    c0 = _counts(m)
    for loss, kw in (("L_median", {}), ("MIWAE", dict(k1=205, k2=5)), ("PIWAE", dict(k1=205, k2=5))):
        assert C.rejected(loss, k)
        m.loss_function, m.k1, m.k2 = loss, kw.get("k1"), kw.get("k2")
        with pytest.raises(ValueError, match="k <= 1024"):
            m.train_step(x, eps=eps)
        with pytest.raises(ValueError, match="k <= 1024"):
            m._bound(m._lc(loss, k=k, **kw), x, eps)
    with pytest.raises(ValueError, match="k <= 1024"):
        m.get_L_median(x, k, eps=eps)
    with pytest.raises(ValueError, match="k <= 1024"):
        m.get_L_MIWAE(x, 205, 5, eps=eps)
    assert _advance(m, c0) == {i: 0 for i in COUNTERS}
    np.testing.assert_array_equal(_flat(m.get_weights()), w0)
    assert m.get_optimizer_state()[2] == 0
    m.loss_function, m.k1, m.k2 = "IWAE", None, None
    ref = C.reference_bound(name, "IWAE")
    assert abs(m.get_L_k(x, k, eps=eps) - ref) <= REL * abs(ref)
    loss_gpu = m.train_step(x, eps=eps)["IWAE"]
    m.check_kernel_status()
    _check_step(m, name, "IWAE", loss_gpu, f"{name} IWAE after the rejections")
    assert m.get_optimizer_state()[2] == 1


# ------------------------------------------- e. NLL reductions at their edges
@pytest.mark.parametrize("path", ["auto", "layerwise"])
@pytest.mark.parametrize("model", ["S1", "S2"])
def test_log_px_matches_float64_at_the_reductions_edges(model, path):
    """log_px on injected noise at k = 1, beside the 64-lane stride, beside the
    weight-ring kernel's kS >= 128 rule and beside lse_kernel's 8 x 256 rows."""
    from iwae_replication_project_amd import Flexible_Model
    from iwae_replication_project_amd.flexible_iwae import _split, weight_shapes
    worst = 0.0
    for k in C.NLL_KS:
        (he, hd, le, ld), (spec, params, mean, x, eps) = C.nll_case(model, k)
        m = Flexible_Model(he, hd, le, ld, dataset_bias=mean, loss_function="IWAE", k=k, seed=1, x_dim=C.X_DIM,
                           kernel_path=path)
        m.set_weights(_split(O.flatten_params(spec, params).astype(np.float32), weight_shapes(m.dense)))
        lp = m.log_px(x.astype(np.float32), k, eps=[e.astype(np.float32) for e in eps]).cpu().numpy()
        m.check_kernel_status()
        err = np.abs(lp - C.nll_reference(model, k)).max()
        worst = max(worst, err)
        print(f"{model} {path} k = {k}: log p(x) {err:.2e} nats")
        assert lp.shape == (C.NLL_B,) and np.isfinite(lp).all()
        assert err <= LOGPX_ATOL, (k, err)
    print(f"{model} {path}: worst log p(x) {worst:.2e} nats")
