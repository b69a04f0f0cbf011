"""The importance-weighted posterior (iwae_posterior, Flexible_Model.posterior /
reconstructed_x_probs_iw): the fused post_kernel pass and the layer-wise pass
against the float64 reference of tests/posterior_ref.py.

Models: the seven architectures of test_gpu_generate with float32-rounded
weights, every Dense KERNEL multiplied by 0.5 (biases kept).  With plain Glorot
weights these untrained models have an effective sample size of about 1, the
weighting is one-hot and the test would be vacuous; with the 0.5 scale ESS / k
spans a few per cent to almost 1.  Every case asserts min w~_ref >= 1e-10 and
1 < ESS_ref < k for every image it uses (k > 1).

Parity under injected noise is in two parts, which together pin the result:
  1. weights: log_px within NLL_TOL; the implied log weights log(w~) + log_px +
     log k within REL * max|lw_ref| (test_log_weights_match_golden's bar); |sum_s
     w~ - 1| <= (k + 8) 2^-23; ess within relative (k + 8) 2^-23 of 1 / sum w~^2
     evaluated in float64 from the returned weights;
  2. combination: h_mean and probs against combine(DEVICE weights, float64 rows),
     per element atol + rtol * sum_s w~_s |v_ref,s| with LATENT_TOL / PROBS_TOL of
     test_gpu_generate (the bars of one row of the same quantities; a convex
     combination of rows keeps them).
The end-to-end error against the reference's own weights is printed, not gated:
it is the log-weight error times the spread of the values, a property of the
first pass.

Worst ratios measured on an MI355X (error / bar over the 79 injected-noise
cases, fused / layer-wise; DESIGN.md s9 has the table): log_px 0.004 / 0.004,
implied log weights 0.007 / 0.007, sum of weights 0.045 / 0.049, ess 0.070 /
0.069, h_mean 0.125 / 0.127, probs 0.066 / 0.065; fused against layer-wise on
device noise (twice the bars) h_mean 0.267, probs 0.005.  End to end against
the reference's own weights: at most 9.5e-5 in a latent mean, 1.8e-6 in a
probability."""
import ctypes
import functools

import numpy as np
import pytest

import group_cases as GC
import posterior_ref as R
from test_gpu_generate import ARCHS, LATENT_TOL, PROBS_TOL
from test_gpu_parity import NLL_TOL, REL, make_model, weights_from_flat

pytestmark = pytest.mark.gpu

PATHS = ("auto", "layerwise")
KS = (1, 17, 130)          # degenerate; straddles a 16-row tile; several partials per image at every RT, ring first pass
NS = (1, 5, 33)            # 33: past the 32-image few-row first layer
SMALL = (0, 1, 2)          # the full grid; the other four run (5, 17) and (3, 130)
GRID = [(ai, N, k) for ai in SMALL for N in NS for k in KS] + \
       [(ai, N, k) for ai in range(len(ARCHS)) if ai not in SMALL for N, k in ((5, 17), (3, 130))]
BIG = 5                    # the configs[1] architecture 784-200-200-100-100-50
EPS23 = 2.0 ** -23


def _spec_params(ai):
    from oracle import iwae_oracle as O
    he, hd, le, ld = ARCHS[ai]
    x_dim = ld[-1]
    rng = np.random.default_rng(100 + ai)
    spec = O.ModelSpec(he, hd, le, ld, x_dim=x_dim)
    params = O.glorot_init(spec, rng, out_bias=O.output_bias_from_mean(rng.uniform(0.02, 0.4, x_dim)))
    params = {n: [(0.5 * w).astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64)]
              for n, (w, b) in params.items()}
    return O, spec, params


@functools.lru_cache(maxsize=None)
def _setup(ai, path):
    O, spec, params = _spec_params(ai)
    he, hd, le, ld = ARCHS[ai]
    m = make_model(he, hd, le, ld, x_dim=spec.x_dim, kernel_path=path)
    m.set_weights(weights_from_flat(m, O.flatten_params(spec, params)))
    return O, spec, params, m


@functools.lru_cache(maxsize=None)
def _case(ai, N, k, seed=None, density=0.3):
    """Inputs and the float64 reference of one case (computed once, shared)."""
    O, spec, params = _spec_params(ai)
    rng = np.random.default_rng(7000 + 100 * ai + 10 * N + k if seed is None else seed)
    x = (rng.random((N, spec.x_dim)) < density).astype(np.float32)
    eps = [rng.standard_normal((k, N, d)).astype(np.float32) for d in spec.n_latent_encoder]
    ref = R.posterior(params, spec, x, eps)
    assert ref["weights"].min() >= 1e-10, ref["weights"].min()
    if k > 1:
        assert (ref["ess"] > 1).all() and (ref["ess"] < k).all(), ref["ess"]
    return x, eps, ref


def _counts(m):
    return [int(m._lib.iwae_debug_count(m._h, i)) for i in (17, 18)]


def _post_plan_fits(ai):
    """post_plan's rule (iwae_model.hip), restated: LDS buffers for the latents a
    stage reads (h_1 .. h_{L-1}; h_1 alone when L = 1), P and Q, each as wide as
    the widest thing it holds (an input's padded K = fan-in + 1 rounded up to 32,
    a tanh output and its reader's padded K, h_1 as f32 in P / Q), row strides of
    8 mod 16 dwords, two bf16 planes, plus one float per row: the plan fits when
    16 rows of that are at most 160 KB."""
    he, hd, le, ld = ARCHS[ai]
    L, x_dim = len(le), ld[-1]
    r32 = lambda v: (v + 31) // 32 * 32
    nl = max(1, L - 1)
    width = [0] * (nl + 2)
    bP, bQ = nl, nl + 1

    def dense(fin, fout, i, o, next_k):
        width[i] = max(width[i], r32(fin + 1))
        if o is not None:
            width[o] = max(width[o], fout, next_k)

    for i in range(1, L):
        H = he[i]
        dense(le[i - 1], H, i - 1, bP, r32(H + 1))
        dense(H, H, bP, bQ, r32(H + 1))
        dense(H, 2 * le[i], bQ, None, 0)
        if i < nl:
            width[i] = max(width[i], r32(le[i] + 1))
    H = hd[L - 1]
    dense(le[0], H, 0, bQ, r32(H + 1))
    dense(H, H, bQ, bP, r32(H + 1))
    dense(H, x_dim, bP, None, 0)
    width[0] = max(width[0], r32(le[0] + 1))
    width[bP], width[bQ] = max(width[bP], le[0]), max(width[bQ], le[0])
    per_row = 0
    for w in width:
        sdw = (max(w, 32) + 1) // 2
        while sdw % 16 != 8:
            sdw += 1
        per_row += 2 * 2 * sdw * 2          # two planes of 2 sdw bf16, 2 bytes each
    return 16 * (per_row + 4) <= 160 * 1024 and nl + 2 <= 12 and 3 * L <= 24


_NLL_FUSED = {}


def _nll_is_fused(ai, m, x):
    """Whether the NLL's first pass runs on the fused kernels for this model
    (counter id 0 counts their launches); asked once per model."""
    if ai not in _NLL_FUSED:
        c0 = int(m._lib.iwae_debug_count(m._h, 0))
        m.log_px(x[:1], 2)
        _NLL_FUSED[ai] = int(m._lib.iwae_debug_count(m._h, 0)) > c0
    return _NLL_FUSED[ai]


def _expect_fused(ai, path, m, x):
    """The rule: post_kernel runs (id 17) when the path is not layer-wise, the
    fused NLL kernel applies to the model and post_plan fits; else the
    layer-wise second pass (id 18)."""
    return path == "auto" and _nll_is_fused(ai, m, x) and _post_plan_fits(ai)


def _np(t):
    return t.cpu().numpy()


def _check_parity(out, ref, k, label):
    """Parts 1 and 2 of the parity; returns the worst ratios (error / bar)."""
    w = _np(out["weights"]).astype(np.float64)
    lpx = _np(out["log_px"]).astype(np.float64)
    ess = _np(out["ess"]).astype(np.float64)
    N = w.shape[0]
    assert w.shape == (N, k) and lpx.shape == (N,) and ess.shape == (N,)
    lw_ref = ref["lw"].T                                        # [N, k]
    # ---- 1. the weights
    r_lpx = np.abs(lpx - ref["log_px"]).max() / NLL_TOL
    assert (w > 0).all()
    implied = np.log(w) + lpx[:, None] + np.log(k)
    r_lw = np.abs(implied - lw_ref).max() / (REL * np.abs(lw_ref).max())
    r_sum = np.abs(w.sum(1) - 1.0).max() / ((k + 8) * EPS23)
    r_ess = np.abs(ess * (w * w).sum(1) - 1.0).max() / ((k + 8) * EPS23)
    # ---- 2. the combination under the device's weights
    hm_ref, p_ref = R.combine(w, ref["cache"])
    hm_abs, p_abs = R.combine_abs(w, ref["cache"])
    r_h = 0.0
    for hd, hr, ha in zip(out["h_mean"], hm_ref, hm_abs):
        assert tuple(hd.shape) == hr.shape
        r_h = max(r_h, (np.abs(_np(hd) - hr) / (LATENT_TOL["atol"] + LATENT_TOL["rtol"] * ha)).max())
    probs = _np(out["probs"])
    assert probs.shape == p_ref.shape
    r_p = (np.abs(probs - p_ref) / (PROBS_TOL["atol"] + PROBS_TOL["rtol"] * p_abs)).max()
    # ---- end to end against the reference's own weights: printed, not gated
    e_h = max(np.abs(_np(hd) - hr).max() for hd, hr in zip(out["h_mean"], ref["h_mean"]))
    e_p = np.abs(probs - ref["probs"]).max()
    print(f"{label}: ratios log_px {r_lpx:.3f} lw {r_lw:.3f} sum {r_sum:.3f} ess {r_ess:.3f} "
          f"h_mean {r_h:.3f} probs {r_p:.3f}; end-to-end max abs err h_mean {e_h:.2e} probs {e_p:.2e}; "
          f"ESS_ref/k {ref['ess'].min() / k:.3f}..{ref['ess'].max() / k:.3f}")
    ratios = dict(log_px=r_lpx, lw=r_lw, sum=r_sum, ess=r_ess, h_mean=r_h, probs=r_p)
    for name, r in ratios.items():
        assert r <= 1.0, (label, name, r)
    return ratios


# ------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("ai,N,k", GRID)
def test_parity_with_injected_noise(ai, N, k, path):
    O, spec, params, m = _setup(ai, path)
    x, eps, ref = _case(ai, N, k)
    fused = _expect_fused(ai, path, m, x)
    c0 = _counts(m)
    out = m.posterior(x, k, eps=eps, want=("h_mean", "probs", "weights", "ess", "log_px"))
    c1 = _counts(m)
    assert [c1[0] - c0[0], c1[1] - c0[1]] == ([1, 0] if fused else [0, 1]), (c0, c1, fused)
    if path == "auto" and ai in SMALL:
        assert fused                                           # these plans fit
    _check_parity(out, ref, k, f"arch {ai} N {N} k {k} {path}")
    np.testing.assert_array_equal(_np(m.reconstructed_x_probs_iw(x, k, eps=eps)), _np(out["probs"]))


def test_parity_at_k_5000():
    """k = 5000, two images, the configs[1] architecture: 79 to 313 partials per
    image, the weight-ring first pass.  Among 5000 samples of this model the
    smallest w~ is about 1e-11 on images with 30 % of their pixels on (oracle,
    80 seeds), below the floor every case asserts; on sparse images (3 % on) it
    is about 1e-9 (ESS 117 and 136 of 5000 here), so this case uses those."""
    O, spec, params, m = _setup(BIG, "auto")
    x, eps, ref = _case(BIG, 2, 5000, seed=117, density=0.03)
    c0 = _counts(m)
    out = m.posterior(x, 5000, eps=eps, want=("h_mean", "probs", "weights", "ess", "log_px"))
    c1 = _counts(m)
    assert [c1[0] - c0[0], c1[1] - c0[1]] == [1, 0]
    _check_parity(out, ref, 5000, "arch 5 N 2 k 5000 auto")


# --------------------------------------------------------------------- 2. SIR
def _pick_u(w, rng):
    """u per image at least 1e-4 from every boundary of the float64 cumulative
    sum of the returned weights (the device's f32 sum of k <= 130 terms is within
    k 2^-24 < 1e-5 of it)."""
    c = np.cumsum(w.astype(np.float64), axis=1)
    u = np.empty(w.shape[0])
    for b in range(w.shape[0]):
        for _ in range(1000):
            u[b] = rng.random()
            if np.abs(c[b] - u[b]).min() >= 1e-4 and u[b] <= 1 - 1e-4:
                break
        else:
            raise AssertionError("no u away from the boundaries")
    return u.astype(np.float32)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("ai,N,k", [(ai, 5, 17) for ai in range(len(ARCHS))] + [(ai, 3, 130) for ai in SMALL] +
                         [(1, 33, 130)])
def test_sir_draw_is_the_sample_the_cumulative_sum_selects(ai, N, k, path):
    O, spec, params, m = _setup(ai, path)
    x, eps, ref = _case(ai, N, k)
    w = _np(m.posterior(x, k, eps=eps, want=("weights",))["weights"])
    rng = np.random.default_rng(k + N)
    u = _pick_u(w, rng)
    out = m.posterior(x, k, eps=eps, u=u, want=("h_sir", "weights"))
    np.testing.assert_array_equal(_np(out["weights"]), w)          # deterministic
    idx = R.sir_index(w.astype(np.float64), u.astype(np.float64))
    assert len(set(idx.tolist())) > 1 or N == 1 or k == 1
    for hd, hr in zip(out["h_sir"], R.sir_latents(idx, ref["cache"])):
        assert tuple(hd.shape) == hr.shape
        np.testing.assert_allclose(_np(hd), hr, **LATENT_TOL)
    # the draw alone (no other output) is the same draw
    alone = m.posterior(x, k, eps=eps, u=u, want="h_sir")["h_sir"]
    for a, b in zip(alone, out["h_sir"]):
        np.testing.assert_array_equal(_np(a), _np(b))


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("ai", [0, 2, 3])
def test_one_sample_is_mean_and_draw_bit_for_bit(ai, path):
    O, spec, params, m = _setup(ai, path)
    x, eps, ref = _case(ai, 5, 1)
    out = m.posterior(x, 1, eps=eps, u=np.full(5, 0.5, np.float32))
    np.testing.assert_array_equal(_np(out["weights"]), np.ones((5, 1), np.float32))
    np.testing.assert_array_equal(_np(out["ess"]), np.ones(5, np.float32))
    for a, b, hr in zip(out["h_mean"], out["h_sir"], ref["cache"]["h"]):
        np.testing.assert_array_equal(_np(a), _np(b))
        np.testing.assert_allclose(_np(a), hr[0], **LATENT_TOL)
    np.testing.assert_allclose(_np(out["probs"]), ref["cache"]["p"][0], **PROBS_TOL)


# ------------------------------------------------------------------ 3. chunks
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("ai", [1, 3])
def test_three_chunks_the_last_ragged(ai, path):
    O, spec, params, m = _setup(ai, path)
    x, eps, ref = _case(ai, 5, 17)
    fused = _expect_fused(ai, path, m, x)
    want = ("h_mean", "probs", "weights", "ess", "log_px")
    whole = m.posterior(x, 17, eps=eps, want=want)
    c0 = _counts(m)
    parts = m.posterior(x, 17, eps=eps, chunk=2, want=want)
    c1 = _counts(m)
    assert [c1[0] - c0[0], c1[1] - c0[1]] == ([3, 0] if fused else [0, 3])
    _check_parity(parts, ref, 17, f"arch {ai} N 5 k 17 chunk 2 {path}")
    hm_abs, p_abs = R.combine_abs(ref["weights"], ref["cache"])
    for a, b, s in zip(parts["h_mean"], whole["h_mean"], hm_abs):
        assert (np.abs(_np(a) - _np(b)) <= LATENT_TOL["atol"] + LATENT_TOL["rtol"] * s).all()
    assert (np.abs(_np(parts["probs"]) - _np(whole["probs"])) <= PROBS_TOL["atol"] + PROBS_TOL["rtol"] * p_abs).all()
    # SIR across chunks: u is indexed by the image, not by its place in the chunk
    w = _np(parts["weights"])
    u = _pick_u(w, np.random.default_rng(5))
    idx = R.sir_index(w.astype(np.float64), u.astype(np.float64))
    hs = m.posterior(x, 17, eps=eps, u=u, chunk=2, want="h_sir")["h_sir"]
    for hd, hr in zip(hs, R.sir_latents(idx, ref["cache"])):
        np.testing.assert_allclose(_np(hd), hr, **LATENT_TOL)


def _fresh(ai, path):
    O, spec, params = _spec_params(ai)
    he, hd, le, ld = ARCHS[ai]
    m = make_model(he, hd, le, ld, x_dim=spec.x_dim, kernel_path=path)
    m.set_weights(weights_from_flat(m, O.flatten_params(spec, params)))
    return m


def _flatten(out):
    return [_np(t) for name in sorted(out) for t in (out[name] if isinstance(out[name], list) else [out[name]])]


def test_first_layer_groups_of_four_and_three_images():
    """Fused, the first encoder layer runs once per group of images
    (set_tuning("nll_group")): 7 images in chunks of 2 with groups of 4 give the
    groups [0, 4) and [4, 7), the third chunk starting a group in the middle of
    the call and the last chunk holding one image (group_cases.py).  On a model
    that has run nothing, so no earlier call's rows are in the workspace: four
    post_kernel launches, none layer-wise; parity as every other case; and bit
    for bit the same call with the default group size (one group: the chunks
    are the same, only the first layer's rows come from a launch over 4 or 3
    images instead of 7)."""
    ai, N, k = 1, GC.N, GC.K
    x, eps, ref = _case(ai, N, k)
    want = ("h_mean", "probs", "weights", "ess", "log_px")
    m = _fresh(ai, "auto")
    out, one_group, d = GC.groups_then_one_group(
        m, (17, 18), lambda: m.posterior(x, k, eps=eps, chunk=GC.CHUNK, want=want))
    assert d == [4, 0], d                                           # chunks [0,2) [2,4) | [4,6) [6,7)
    _check_parity(out, ref, k, f"arch {ai} N {N} k {k} chunk 2 group 4")
    for a, b in zip(_flatten(out), _flatten(one_group)):
        np.testing.assert_array_equal(a, b)


def test_log_px_of_a_few_images_then_their_posterior_on_a_fresh_model():
    """The first evaluation call of a model sizes the workspace for its own
    images (a first-layer group is at most the call's N images), and a later
    call grows it: log_px of 4 images, then their posterior, both within the
    bars, the posterior on post_kernel."""
    ai, N, k = 1, 4, 5
    x, eps, ref = _case(ai, N, k)
    m = _fresh(ai, "auto")
    lp = _np(m.log_px(x, k, eps=eps)).astype(np.float64)
    assert np.abs(lp - ref["log_px"]).max() <= NLL_TOL, (lp, ref["log_px"])
    c0 = _counts(m)
    out = m.posterior(x, k, eps=eps, want=("h_mean", "probs", "weights", "ess", "log_px"))
    c1 = _counts(m)
    assert [c1[0] - c0[0], c1[1] - c0[1]] == [1, 0], (c0, c1)
    _check_parity(out, ref, k, f"arch {ai} N {N} k {k} after log_px")


# ------------------------------------------------------------ 4. device noise

@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("ai,N,k", [(1, 5, 17), (2, 3, 130)])
def test_device_noise_is_reproducible_on_fresh_models(ai, N, k, path):
    x, _, _ = _case(ai, N, k)
    outs = []
    for _ in range(2):
        m = _fresh(ai, path)
        m.set_seed(4242)
        outs.append(_flatten(m.posterior(x, k)))
    for a, b in zip(*outs):
        assert np.isfinite(a).all()
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("ai,N,k", [(1, 5, 17), (2, 3, 17), (0, 5, 17)])
def test_both_passes_and_both_paths_draw_the_same_device_noise(ai, N, k):
    """Fused against layer-wise after the same set_seed, within twice the
    combination bars.  The layer-wise second pass reads the latents its first
    pass stored, so this fails if post_kernel's second pass draws other noise
    than the first.  The bars need sum_s w~_s |v_s| of rows nobody injected: the
    rows are read back through the SIR draw (u inside sample j's interval of
    the cumulative weights selects sample j), the probabilities' scale is the
    value itself.  softmax(get_log_weights) after the same set_seed matches the
    weights within the part-1 bar."""
    O, spec, params, mf = _setup(ai, "auto")
    _, _, _, ml = _setup(ai, "layerwise")
    x, _, _ = _case(ai, N, k)
    res = {}
    for name, m in (("fused", mf), ("layerwise", ml)):
        m.set_noise_stream(0)
        m.set_seed(99)
        res[name] = m.posterior(x, k)
        m.set_seed(99)
        lw = _np(m.get_log_weights(x, k)).astype(np.float64).T           # [N, k]
        w = _np(res[name]["weights"]).astype(np.float64)
        implied = np.log(w) + _np(res[name]["log_px"]).astype(np.float64)[:, None] + np.log(k)
        r = np.abs(implied - lw).max() / (REL * np.abs(lw).max())
        print(f"{name}: implied log weights against get_log_weights, ratio {r:.3f}")
        assert r <= 1.0
    assert _counts(mf)[0] > 0 and _counts(ml)[0] == 0
    # the layer-wise model's rows of h_i, one sample index at a time
    w = _np(res["layerwise"]["weights"]).astype(np.float64)
    c = np.cumsum(w, axis=1)
    lo = np.concatenate([np.zeros((N, 1)), c[:, :-1]], axis=1)
    rows = [np.empty((k, N, d)) for d in spec.n_latent_encoder]
    for j in range(k):
        ml.set_seed(99)
        hs = ml.posterior(x, k, u=(0.5 * (lo[:, j] + c[:, j])).astype(np.float32), want="h_sir")["h_sir"]
        for i, t in enumerate(hs):
            rows[i][j] = _np(t)
    worst = 0.0
    for i, (a, b) in enumerate(zip(res["fused"]["h_mean"], res["layerwise"]["h_mean"])):
        scale = np.einsum("bs,sbd->bd", w, np.abs(rows[i]))
        ratio = (np.abs(_np(a) - _np(b)) / (2 * (LATENT_TOL["atol"] + LATENT_TOL["rtol"] * scale))).max()
        worst = max(worst, ratio)
    pf, pl = _np(res["fused"]["probs"]), _np(res["layerwise"]["probs"])
    rp = (np.abs(pf - pl) / (2 * (PROBS_TOL["atol"] + PROBS_TOL["rtol"] * pl))).max()
    print(f"fused against layer-wise: ratios h_mean {worst:.3f} probs {rp:.3f}")
    assert worst <= 1.0 and rp <= 1.0
    # other noise would be far off: a second call (fresh noise) differs visibly
    again = mf.posterior(x, k, want="h_mean")["h_mean"]
    assert max(np.abs(_np(a) - _np(b)).max() for a, b in zip(again, res["fused"]["h_mean"])) > 1e-3


# ------------------------------------------------------------------- 5. state
def test_posterior_between_train_steps_changes_nothing():
    """Weights, optimizer state and captured graphs are as they were, and the
    next train_steps call is bit for bit that of a model that never called
    posterior (it calls log_px on the same images instead, which moves the
    noise position by the same one chunk)."""
    from iwae_replication_project_amd import Adam
    he, hd, le, ld = ARCHS[1]
    rng = np.random.default_rng(3)
    x = (rng.random((40, 784)) < 0.3).astype(np.float32)
    models = []
    for _ in range(2):
        m = make_model(he, hd, le, ld, seed=11)
        m.compile(optimizer=Adam(learning_rate=1e-3, epsilon=1e-4))
        models.append(m)
    a, b = models
    b.set_weights(a.get_weights())
    la, lb = a.train_steps(x, 20), b.train_steps(x, 20)
    np.testing.assert_array_equal(np.asarray(la), np.asarray(lb))
    w0, (m0, v0, t0), g0 = a.get_weights(), a.get_optimizer_state(), a.graph_captures()
    c0 = _counts(a)
    out = a.posterior(x[:5], 17)
    assert _counts(a)[0] == c0[0] + 1
    assert all(np.isfinite(v).all() for v in _flatten(out))
    b.log_px(x[:5], 17)
    w1, (m1, v1, t1) = a.get_weights(), a.get_optimizer_state()
    for p, q in zip(w0, w1):
        np.testing.assert_array_equal(p, q)
    np.testing.assert_array_equal(m0, m1)
    np.testing.assert_array_equal(v0, v1)
    assert t0 == t1 and a.graph_captures() == g0
    la, lb = a.train_steps(x, 20), b.train_steps(x, 20)
    assert a.graph_captures() == g0                        # replayed, not re-captured
    np.testing.assert_array_equal(np.asarray(la), np.asarray(lb))
    for p, q in zip(a.get_weights(), b.get_weights()):
        np.testing.assert_array_equal(p, q)
    a.check_kernel_status()


def test_padding_columns_and_rows_past_n_keep_their_sentinel():
    import torch
    from iwae_replication_project_amd import _lib
    for path in PATHS:
        O, spec, params, m = _setup(4, path)                # x_dim = 64
        x, eps, ref = _case(4, 5, 17)
        N, rows, xd, k = 5, 7, spec.x_dim, 17
        ld = xd + 8
        with torch.cuda.stream(m._stream):
            xt = torch.from_numpy(x).to(m.device)
            probs = torch.full((rows, ld), -7.0, device=m.device)
            hm = [torch.full((rows, d), -7.0, device=m.device) for d in spec.n_latent_encoder]
            wt = torch.full((rows, k), -7.0, device=m.device)
        marr, nm = _lib.fptr_array(hm)
        m._call(m._lib.iwae_posterior(m._h, _lib.fptr(xt), N, k, 0, None, 0, None, marr, nm, _lib.fptr(probs), ld,
                                      None, 0, _lib.fptr(wt), None, None))
        m._stream.synchronize()
        probs, wt = probs.cpu().numpy(), wt.cpu().numpy()
        assert (probs[:N, xd:] == -7.0).all() and (probs[N:] == -7.0).all() and (wt[N:] == -7.0).all()
        assert ((probs[:N, :xd] > 0) & (probs[:N, :xd] < 1)).all() and (wt[:N] > 0).all()
        for h in hm:
            h = h.cpu().numpy()
            assert (h[N:] == -7.0).all() and (h[:N] != -7.0).all()


# --------------------------------------------------------------- 6. arguments
def test_bad_arguments_raise_before_any_launch():
    import torch
    from iwae_replication_project_amd import _lib
    O, spec, params, m = _setup(1, "auto")
    x, eps, ref = _case(1, 5, 17)
    c0 = _counts(m)
    n0 = int(m._lib.iwae_debug_count(m._h, 0))
    with pytest.raises(ValueError):
        m.posterior(np.zeros((0, 784), np.float32), 17)           # N = 0
    with pytest.raises(ValueError):
        m.posterior(x, 0)                                         # k = 0
    with pytest.raises(ValueError):
        m.posterior(x, 17, want=())                               # all outputs off
    with pytest.raises(ValueError):
        m.posterior(x, 17, want=("h_mean", "nothing"))
    with pytest.raises(ValueError):
        m.posterior(x, 17, eps=eps[:1])                           # wrong eps count
    with pytest.raises(ValueError):
        m.posterior(x, 17, eps=[eps[0], eps[1][:, :, :-1]])       # wrong eps shape
    with pytest.raises(ValueError):
        m.posterior(x, 17, u=np.zeros(4, np.float32))             # wrong u shape
    with pytest.raises(ValueError):
        m.posterior(x, (1 << 20) + 1, want="log_px")              # k > 2^20
    with torch.cuda.stream(m._stream):
        xt = torch.from_numpy(x).to(m.device)
        buf = torch.zeros(5, 788, device=m.device)
        e = [torch.zeros(17, 5, d, device=m.device) for d in spec.n_latent_encoder]
    post = m._lib.iwae_posterior
    xp, p = _lib.fptr(xt), _lib.fptr(buf)
    arr3 = (_lib.FP * 3)(*[_lib.fptr(t) for t in e + e[:1]])
    arr2 = (_lib.FP * 2)(_lib.fptr(e[0]), None)
    for rc in (post(m._h, xp, 5, 17, 0, None, 0, None, None, 0, None, 0, None, 0, None, None, None),   # all NULL
               post(m._h, xp, 0, 17, 0, None, 0, None, None, 0, None, 0, None, 0, None, None, p),      # N = 0
               post(m._h, xp, 5, 0, 0, None, 0, None, None, 0, None, 0, None, 0, None, None, p),       # k = 0
               post(m._h, xp, 5, (1 << 20) + 1, 0, None, 0, None, None, 0, None, 0, None, 0, None, None, p),
               post(m._h, xp, 5, 17, 0, arr3, 3, None, None, 0, None, 0, None, 0, None, None, p),      # eps count
               post(m._h, xp, 5, 17, 0, arr2, 2, None, None, 0, None, 0, None, 0, None, None, p),      # NULL in eps
               post(m._h, xp, 5, 17, 0, None, 0, None, arr2, 1, None, 0, None, 0, None, None, p),      # n_mean
               post(m._h, xp, 5, 17, 0, None, 0, None, arr2, 2, None, 0, None, 0, None, None, p),      # NULL in h_mean
               post(m._h, xp, 5, 17, 0, None, 0, None, None, 0, None, 0, arr2, 2, None, None, p),      # NULL in h_sir
               post(m._h, xp, 5, 17, 0, None, 0, None, None, 0, p, 786, None, 0, None, None, None),    # ld % 4
               post(m._h, xp, 5, 17, 0, None, 0, None, None, 0, p, 780, None, 0, None, None, None),    # ld < x_dim
               post(m._h, xp, 5, 17, 0, None, 0, None, None, 0,
                    ctypes.cast(ctypes.c_void_p(buf.data_ptr() + 4), _lib.FP), 788, None, 0, None, None, None)):
        assert rc == -1
        with pytest.raises(ValueError):
            _lib.check(m._lib, m._h, rc)
    m._stream.synchronize()
    assert _counts(m) == c0 and int(m._lib.iwae_debug_count(m._h, 0)) == n0
    assert (buf == 0).all()
