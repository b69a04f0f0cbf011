"""Missing-pixel imputation (iwae_impute, Flexible_Model.impute /
log_px_observed): the masked mega_fwd_kernel first pass and the layer-wise
first pass against the float64 reference of tests/impute_ref.py.

Models: test_gpu_posterior's (the seven architectures of test_gpu_generate,
float32-rounded weights, every Dense kernel times 0.5) and one with x_dim off a
multiple of 4, ([16], [16], [4], [70]).  Masks: image 0 fully observed, image 1
fully missing, image 2 its first half observed, image 3 only its last three
pixels, the others Bernoulli(0.5); x is Bernoulli(0.3).

Every case asserts, from the reference alone, min w~_ref >= 1e-10, ESS_ref > 1
for every image (k > 1) and min_b ESS_ref / k < 0.99 (N >= 3 and k > 1: one
sample has ESS = k by definition): the weighting is neither one-hot nor flat.
The parity is test_gpu_posterior's two parts (the weights; the combination
under the DEVICE weights), the SIR latents, and the draw: x_draw at the missing
pixels equals (u_pix < p_ref(h_1 of the resampled sample)) except where |u_pix -
p_ref| is within the PROBS_TOL bar of that pixel -- at most max(1, 1 %) of a
case's missing pixels, asserted (the reference alone expects about 2 bar <= 4e-4
of them there).  The masked and the unmasked log p(x) of these cases are 19 to
297 nats apart (asserted above 1), so a kernel that ignored the mask fails the
first part outright.

Worst ratios measured on an MI355X (error / bar over the 80 injected-noise
cases, fused / layer-wise; DESIGN.md s9 has the table): log_px 0.004 / 0.003,
implied log weights 0.008 / 0.008, sum of weights 0.051 / 0.044, ess 0.067 /
0.064, h_mean 0.102 / 0.102, x_mean 0.064 / 0.065; at most 4 of a case's missing
pixels left out of the draw's comparison; fused against layer-wise on device
noise (twice the bars) h_mean 0.129, x_mean 0.004, the draws equal.  Chunked
against whole: every output the same bits layer-wise; on the fused path all but
the weights-dependent outputs of images whose rows change their 16-row tile in
mega_fwd_kernel's workgroup (test_three_chunks_the_last_ragged says why)."""
import ctypes
import functools

import numpy as np
import pytest

import group_cases as GC
import impute_ref as I
import posterior_ref as R
import test_gpu_posterior as TP
from test_gpu_generate import ARCHS, LATENT_TOL, PROBS_TOL
from test_gpu_parity import NLL_TOL, REL, make_model, weights_from_flat

pytestmark = pytest.mark.gpu

PATHS = ("auto", "layerwise")
KS = (1, 17, 130)          # degenerate; straddles a 16-row tile; several partials per image, k >= 128 (no ring here)
NS = (1, 5, 33)            # 33: past the 32-image few-row first layer
SMALL = (0, 1, 2)
ODD = len(ARCHS)           # the extra model: x_dim = 70, off a multiple of 4
MODELS = list(ARCHS) + [([16], [16], [4], [70])]
GRID = [(ai, N, k) for ai in SMALL for N in NS for k in KS] + \
       [(ai, N, k) for ai in range(len(MODELS)) if ai not in SMALL for N, k in ((5, 17), (3, 130))]
EPS23 = 2.0 ** -23
ALL = ("x_mean", "x_draw", "h_mean", "h_sir", "weights", "ess", "log_px")
SEEDS = {}                 # (ai, N, k) -> seed, where the default seed's reference misses a non-vacuity condition


def _spec_params(ai):
    from oracle import iwae_oracle as O
    he, hd, le, ld = MODELS[ai]
    x_dim = ld[-1]
    rng = np.random.default_rng(100 + ai)
    spec = O.ModelSpec(he, hd, le, ld, x_dim=x_dim)
    params = O.glorot_init(spec, rng, out_bias=O.output_bias_from_mean(rng.uniform(0.02, 0.4, x_dim)))
    params = {n: [(0.5 * w).astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64)]
              for n, (w, b) in params.items()}
    return O, spec, params


def _fresh(ai, path):
    O, spec, params = _spec_params(ai)
    he, hd, le, ld = MODELS[ai]
    m = make_model(he, hd, le, ld, x_dim=spec.x_dim, kernel_path=path)
    m.set_weights(weights_from_flat(m, O.flatten_params(spec, params)))
    return m


@functools.lru_cache(maxsize=None)
def _setup(ai, path):
    O, spec, params = _spec_params(ai)
    return O, spec, params, _fresh(ai, path)


def make_mask(rng, N, xd):
    mask = (rng.random((N, xd)) < 0.5).astype(np.float32)
    if N > 0:
        mask[0] = 1.0
    if N > 1:
        mask[1] = 0.0
    if N > 2:
        mask[2] = 0.0
        mask[2, :xd // 2] = 1.0
    if N > 3:
        mask[3] = 0.0
        mask[3, -3:] = 1.0
    return mask


def case_inputs(ai, N, k, seed=None, ones=False):
    O, spec, params = _spec_params(ai)
    if seed is None:
        seed = SEEDS.get((ai, N, k), 9000 + 100 * ai + 10 * N + k)
    rng = np.random.default_rng(seed)
    xd = spec.x_dim
    x = (rng.random((N, xd)) < 0.3).astype(np.float32)
    mask = make_mask(rng, N, xd)
    if ones:
        mask = np.ones_like(mask)
    eps = [rng.standard_normal((k, N, d)).astype(np.float32) for d in spec.n_latent_encoder]
    u_pix = rng.random((N, xd)).astype(np.float32)
    return x, mask, eps, u_pix


def check_non_vacuous(ref, N, k):
    """From the reference alone; returns (min w~, min ESS / k)."""
    assert ref["weights"].min() >= 1e-10, ref["weights"].min()
    if k > 1:
        assert (ref["ess"] > 1).all(), ref["ess"]
    if N >= 3 and k > 1:                       # (k = 1: ESS = k by definition)
        assert ref["ess"].min() / k < 0.99, ref["ess"] / k
    return ref["weights"].min(), ref["ess"].min() / k


@functools.lru_cache(maxsize=None)
def _case(ai, N, k, ones=False):
    """Inputs and the float64 reference of one case (computed once, shared, never changed)."""
    O, spec, params = _spec_params(ai)
    x, mask, eps, u_pix = case_inputs(ai, N, k, ones=ones)
    ref = I.impute(params, spec, x, mask, eps)
    if not ones:
        check_non_vacuous(ref, N, k)
    return x, mask, eps, u_pix, ref


def _counts(m):
    return [int(m._lib.iwae_debug_count(m._h, i)) for i in (19, 20, 0, 3)]


def _expect_fused(ai, path, m, x):
    """iwae_posterior's rule: the masked mega_fwd_kernel runs (id 19) when the
    path is not layer-wise, the fused NLL kernel applies to the model and
    post_plan fits; else the layer-wise first pass (id 20).  The extra model is
    test_gpu_generate's 16-16-4-64 with six more pixels: its plan (three buffers
    of at most 96 columns) fits."""
    if path != "auto":
        return False
    return TP._nll_is_fused(ai, m, x) and (ai == ODD or TP._post_plan_fits(ai))


def _np(t):
    return t.cpu().numpy()


def _bar(tol, scale):
    return tol["atol"] + tol["rtol"] * scale


def _check(out, x, mask, u, u_pix, ref, k, label):
    """Checks 1-4 on one call's outputs (all of ALL); returns the worst ratios."""
    obs = mask != 0
    w = _np(out["weights"]).astype(np.float64)
    lpx = _np(out["log_px"]).astype(np.float64)
    ess = _np(out["ess"]).astype(np.float64)
    N = w.shape[0]
    assert w.shape == (N, k) and lpx.shape == (N,) and ess.shape == (N,)
    lw_ref = ref["lw"].T
    c = ref["cache"]
    # ---- 1. the weights
    r_lpx = np.abs(lpx - ref["log_px"]).max() / NLL_TOL
    assert (w > 0).all()
    implied = np.log(w) + lpx[:, None] + np.log(k)
    r_lw = np.abs(implied - lw_ref).max() / (REL * np.abs(lw_ref).max())
    r_sum = np.abs(w.sum(1) - 1.0).max() / ((k + 8) * EPS23)
    r_ess = np.abs(ess * (w * w).sum(1) - 1.0).max() / ((k + 8) * EPS23)
    # ---- 2. the combination under the device's weights
    hm_ref, p_ref = R.combine(w, c)
    hm_abs, p_abs = R.combine_abs(w, c)
    r_h = 0.0
    for hd, hr, ha in zip(out["h_mean"], hm_ref, hm_abs):
        assert tuple(hd.shape) == hr.shape
        r_h = max(r_h, (np.abs(_np(hd) - hr) / _bar(LATENT_TOL, ha)).max())
    xm, xw = _np(out["x_mean"]), _np(out["x_draw"])
    assert xm.shape == x.shape and xw.shape == x.shape
    np.testing.assert_array_equal(xm[obs], x[obs])
    np.testing.assert_array_equal(xw[obs], x[obs])
    r_p = (np.abs(xm - p_ref) / _bar(PROBS_TOL, p_abs))[~obs].max() if (~obs).any() else 0.0
    # ---- 3. the resampled latents
    idx = R.sir_index(w, u.astype(np.float64))
    for hd, hr in zip(out["h_sir"], R.sir_latents(idx, c)):
        assert tuple(hd.shape) == hr.shape
        np.testing.assert_allclose(_np(hd), hr, **LATENT_TOL)
    # ---- 4. the draw
    p_sel = I.p_sir(idx, c)
    miss = ~obs
    near = miss & (np.abs(u_pix.astype(np.float64) - p_sel) <= _bar(PROBS_TOL, p_sel))
    cap = max(1, int(0.01 * miss.sum()))
    assert near.sum() <= cap, (label, int(near.sum()), cap)
    cmp = miss & ~near
    assert set(np.unique(xw[miss]).tolist()) <= {0.0, 1.0}
    np.testing.assert_array_equal(xw[cmp], (u_pix.astype(np.float64) < p_sel)[cmp].astype(np.float32))
    e_p = np.abs(xm - ref["x_mean"]).max()
    print(f"{label}: ratios log_px {r_lpx:.3f} lw {r_lw:.3f} sum {r_sum:.3f} ess {r_ess:.3f} h_mean {r_h:.3f} "
          f"x_mean {r_p:.3f}; draw: {int(miss.sum())} missing, {int(near.sum())} left out (cap {cap}); end-to-end "
          f"x_mean err {e_p:.2e}; ESS_ref/k {ref['ess'].min() / k:.3f}..{ref['ess'].max() / k:.3f}; "
          f"min w~_ref {ref['weights'].min():.1e}")
    ratios = dict(log_px=r_lpx, lw=r_lw, sum=r_sum, ess=r_ess, h_mean=r_h, x_mean=r_p)
    for name, r in ratios.items():
        assert r <= 1.0, (label, name, r)
    return ratios


def _run(m, x, mask, eps, u_pix, k, rng, chunk=0):
    """The weights first (they fix a u away from the cumulative sum's steps), then everything."""
    w = _np(m.impute(x, mask, k, eps=eps, chunk=chunk, want=("weights",))["weights"])
    u = TP._pick_u(w, rng)
    out = m.impute(x, mask, k, eps=eps, u=u, u_pix=u_pix, chunk=chunk, want=ALL)
    np.testing.assert_array_equal(_np(out["weights"]), w)           # deterministic
    return out, u


# ------------------------------------------------------------------ 1-4, 8
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("ai,N,k", GRID)
def test_parity_with_injected_noise(ai, N, k, path):
    O, spec, params, m = _setup(ai, path)
    x, mask, eps, u_pix, ref = _case(ai, N, k)
    fused = _expect_fused(ai, path, m, x)
    c0 = _counts(m)
    out, u = _run(m, x, mask, eps, u_pix, k, np.random.default_rng(k + N))
    c1 = _counts(m)
    d = [a - b for a, b in zip(c1, c0)]
    assert d == ([2, 0, 0, 0] if fused else [0, 2, 0, 0]), (c0, c1, fused)       # two calls of one chunk each
    if path == "auto" and (ai in SMALL or ai == ODD):
        assert fused                                           # these plans fit
    _check(out, x, mask, u, u_pix, ref, k, f"arch {ai} N {N} k {k} {path}")
    if N > 1:
        # the mask matters: the unmasked estimate is nats away
        full = _np(m.log_px(x, k, eps=eps)).astype(np.float64)
        assert np.abs(full - ref["log_px"])[1:].min() > 1.0
    np.testing.assert_array_equal(_np(m.log_px_observed(x, mask, k, eps=eps)), _np(out["log_px"]))


# ------------------------------------------------------------------------ 5
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("ai,N,k", [(1, 5, 17), (ODD, 5, 17), (2, 3, 130)])
def test_nan_at_missing_pixels_changes_no_bit(ai, N, k, path):
    O, spec, params, m = _setup(ai, path)
    x, mask, eps, u_pix, ref = _case(ai, N, k)
    u = np.random.default_rng(1).random(N).astype(np.float32)
    a = m.impute(x, mask, k, eps=eps, u=u, u_pix=u_pix)
    # the draw alone (no h_sir buffer of the caller's, no other output) is the same draw
    alone = m.impute(x, mask, k, eps=eps, u=u, u_pix=u_pix, want="x_draw")["x_draw"]
    np.testing.assert_array_equal(_np(alone), _np(a["x_draw"]))
    for junk in (np.nan, np.inf):
        xj = np.where(mask != 0, x, np.float32(junk)).astype(np.float32)
        b = m.impute(xj, mask, k, eps=eps, u=u, u_pix=u_pix)
        for p, q in zip(TP._flatten(a), TP._flatten(b)):
            assert np.isfinite(q).all()
            np.testing.assert_array_equal(p, q)


# ------------------------------------------------------------------------ 6
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("ai", [1, 3, ODD])
def test_three_chunks_the_last_ragged(ai, path):
    O, spec, params, m = _setup(ai, path)
    x, mask, eps, u_pix, ref = _case(ai, 5, 17)
    fused = _expect_fused(ai, path, m, x)
    rng = np.random.default_rng(5)
    c0 = _counts(m)
    parts, u = _run(m, x, mask, eps, u_pix, 17, rng, chunk=2)
    c1 = _counts(m)
    assert [a - b for a, b in zip(c1, c0)] == ([6, 0, 0, 0] if fused else [0, 6, 0, 0])
    # mask, u and u_pix rows follow the chunk's first image: every image against its own reference
    _check(parts, x, mask, u, u_pix, ref, 17, f"arch {ai} N 5 k 17 chunk 2 {path}")
    whole = m.impute(x, mask, 17, eps=eps, u=u, u_pix=u_pix)
    # What may depend on the chunking.  lse_kernel, post_weights_kernel and group_wsum_kernel work
    # image by image in sample order, post_kernel's tiles belong to one image, the layer-wise GEMMs
    # (the draw's output MLP on 2 or 5 rows among them) accumulate an output row over K alone, and
    # the first encoder layer runs on the same 5 images in both calls (one first-layer group when
    # fused).  Layer-wise, therefore, every output matches bit for bit.  On the fused path
    # mega_fwd_kernel's log weight of a row depends, in its last bits (1-2 ulp of log w), on WHICH
    # 16-row tile of its 64-row workgroup the row falls in: the first tile's rows round differently
    # from the other three's (measured on an MI355X with one image repeated at five places: the
    # same neighbours, other places, two values per row; the unmasked instantiations, which this
    # kernel must equal, do the same through iwae_posterior).  A chunk moves an image's rows to
    # other tiles unless it starts where the whole call's workgroups start, so:
    #   - h_sir and x_draw (no weight enters them beyond the index) match bit for bit everywhere;
    #   - images 0 and 1 (the first chunk: the same workgroup-local rows in both calls) match bit
    #     for bit in every output;
    #   - images 2-4 keep the bars of checks 1-2 on weights, ess, log_px, h_mean and x_mean.
    def pairs(name):
        return zip(parts[name], whole[name]) if isinstance(parts[name], list) else [(parts[name], whole[name])]
    same = {name: [all(np.array_equal(_np(p)[b], _np(q)[b]) for p, q in pairs(name)) for b in range(5)] for name in ALL}
    print(f"arch {ai} {path}: chunk 2 against one chunk, bit-identical per image: {same}")
    for name in ALL:
        exact = range(5) if (not fused or name in ("h_sir", "x_draw")) else (0, 1)
        for b in exact:
            assert same[name][b], (name, b, same)
    if fused:
        wp, ww = _np(parts["weights"]).astype(np.float64), _np(whole["weights"]).astype(np.float64)
        lp, lw_ = _np(parts["log_px"]).astype(np.float64), _np(whole["log_px"]).astype(np.float64)
        assert np.abs(lp - lw_).max() <= NLL_TOL
        assert np.abs(np.log(wp) + lp[:, None] - np.log(ww) - lw_[:, None]).max() <= REL * np.abs(ref["lw"]).max()
        ep, ew = _np(parts["ess"]).astype(np.float64), _np(whole["ess"]).astype(np.float64)
        # ess = (sum e)^2 / sum e^2: log weights within the bar d of check 1 move it by at most 4 d, relative
        assert (np.abs(ep / ew - 1.0) <= 4 * REL * np.abs(ref["lw"]).max() + (17 + 8) * EPS23).all()
        hm_abs, p_abs = R.combine_abs(ref["weights"], ref["cache"])
        for a, b, sc in zip(parts["h_mean"], whole["h_mean"], hm_abs):
            assert (np.abs(_np(a) - _np(b)) <= _bar(LATENT_TOL, sc)).all()
        assert (np.abs(_np(parts["x_mean"]) - _np(whole["x_mean"])) <= _bar(PROBS_TOL, p_abs)).all()


def test_first_layer_groups_of_four_and_three_images():
    """Fused, the first encoder layer runs once per group of images
    (set_tuning("nll_group")), and so does the staging of x and of the
    likelihood's -1 copy: 7 images in chunks of 2 with groups of 4 give the
    groups [0, 4) and [4, 7), the third chunk starting a group in the middle of
    the call and the last chunk holding one image (group_cases.py).  On a model
    that has run nothing, so no earlier call's rows are in the workspaces: two
    calls (_run) of four masked mega_fwd_kernel launches, none layer-wise;
    checks 1-4 as every other case; and bit for bit the same call with the
    default group size (one group: the chunks are the same, only the staged
    rows and the first layer's come from launches over 4 or 3 images)."""
    ai, N, k = 1, GC.N, GC.K
    x, mask, eps, u_pix, ref = _case(ai, N, k)
    m = _fresh(ai, "auto")
    m.set_tuning("nll_group", GC.GROUP)
    (out, u), d = GC.counter_deltas(m, (19, 20, 0, 3), lambda: _run(m, x, mask, eps, u_pix, k, np.random.default_rng(k + N),
                                                                   chunk=GC.CHUNK))
    assert d == [8, 0, 0, 0], d                                     # twice the chunks [0,2) [2,4) | [4,6) [6,7)
    _check(out, x, mask, u, u_pix, ref, k, f"arch {ai} N {N} k {k} chunk 2 group 4")
    m.set_tuning("nll_group", 16384)
    one_group = m.impute(x, mask, k, eps=eps, u=u, u_pix=u_pix, chunk=GC.CHUNK, want=ALL)
    for a, b in zip(TP._flatten(out), TP._flatten(one_group)):
        np.testing.assert_array_equal(a, b)


# ------------------------------------------------------------------------ 7
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("ai", [0, 1, 2, ODD])
def test_all_ones_mask_is_the_posterior(ai, path):
    O, spec, params, m = _setup(ai, path)
    N, k = 5, 17
    x, mask, eps, u_pix, ref = _case(ai, N, k, ones=True)
    want = ("weights", "log_px", "h_mean")
    a = m.impute(x, mask, k, eps=eps, want=want + ("x_mean",))
    b = m.posterior(x, k, eps=eps, want=want)
    np.testing.assert_array_equal(_np(a["x_mean"]), x)
    wa, wb = _np(a["weights"]).astype(np.float64), _np(b["weights"]).astype(np.float64)
    la, lb = _np(a["log_px"]).astype(np.float64), _np(b["log_px"]).astype(np.float64)
    assert np.abs(la - lb).max() <= NLL_TOL
    lw_a, lw_b = np.log(wa) + la[:, None], np.log(wb) + lb[:, None]
    assert np.abs(lw_a - lw_b).max() <= REL * np.abs(ref["lw"]).max()
    hm_abs, _ = R.combine_abs(ref["weights"], ref["cache"])
    for p, q, s in zip(a["h_mean"], b["h_mean"], hm_abs):
        assert (np.abs(_np(p) - _np(q)) <= _bar(LATENT_TOL, s)).all()
    same = all(np.array_equal(p, q) for p, q in zip(TP._flatten({n: a[n] for n in want}), TP._flatten(b)))
    print(f"arch {ai} {path}: all-ones impute against posterior bit-identical: {same}")


# ------------------------------------------------------------------------ 9
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("ai,N,k", [(1, 5, 17), (ODD, 5, 17)])
def test_device_noise_is_reproducible_on_fresh_models(ai, N, k, path):
    x, mask, _, _, _ = _case(ai, N, k)
    outs = []
    for _ in range(2):
        m = _fresh(ai, path)
        m.set_seed(4242)
        outs.append(TP._flatten(m.impute(x, mask, k)))
    for a, b in zip(*outs):
        assert np.isfinite(a).all()
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("ai,N,k", [(1, 5, 17), (0, 5, 17), (ODD, 5, 17)])
def test_both_paths_draw_the_same_device_noise(ai, N, k):
    """Fused against layer-wise after the same set_seed, within twice the
    combination bars (test_gpu_posterior's test of the same name: the rows'
    scale is read back through the SIR draw of the layer-wise model)."""
    O, spec, params, mf = _setup(ai, "auto")
    _, _, _, ml = _setup(ai, "layerwise")
    x, mask, _, _, _ = _case(ai, N, k)
    obs = mask != 0
    res = {}
    for name, m in (("fused", mf), ("layerwise", ml)):
        m.set_noise_stream(0)
        m.set_seed(99)
        res[name] = m.impute(x, mask, k)
    assert _counts(mf)[0] > 0 and _counts(ml)[0] == 0
    wf, w = _np(res["fused"]["weights"]).astype(np.float64), _np(res["layerwise"]["weights"]).astype(np.float64)
    lf, ll = _np(res["fused"]["log_px"]).astype(np.float64), _np(res["layerwise"]["log_px"]).astype(np.float64)
    assert np.abs(lf - ll).max() <= 2 * NLL_TOL
    lwl = np.log(w) + ll[:, None]
    assert np.abs(np.log(wf) + lf[:, None] - lwl).max() <= 2 * REL * np.abs(lwl + np.log(k)).max()
    c = np.cumsum(w, axis=1)
    lo = np.concatenate([np.zeros((N, 1)), c[:, :-1]], axis=1)
    rows = [np.empty((k, N, d)) for d in spec.n_latent_encoder]
    for j in range(k):
        ml.set_seed(99)
        hs = ml.impute(x, mask, k, u=(0.5 * (lo[:, j] + c[:, j])).astype(np.float32), want="h_sir")["h_sir"]
        for i, t in enumerate(hs):
            rows[i][j] = _np(t)
    worst = 0.0
    for i, (a, b) in enumerate(zip(res["fused"]["h_mean"], res["layerwise"]["h_mean"])):
        scale = np.einsum("bs,sbd->bd", w, np.abs(rows[i]))
        worst = max(worst, (np.abs(_np(a) - _np(b)) / (2 * _bar(LATENT_TOL, scale))).max())
    pf, pl = _np(res["fused"]["x_mean"]), _np(res["layerwise"]["x_mean"])
    rp = (np.abs(pf - pl) / (2 * _bar(PROBS_TOL, pl))).max()
    np.testing.assert_array_equal(pf[obs], x[obs])
    df, dl = _np(res["fused"]["x_draw"]), _np(res["layerwise"]["x_draw"])
    flips = int((df != dl).sum())
    print(f"fused against layer-wise: ratios h_mean {worst:.3f} x_mean {rp:.3f}; draws differ in {flips} pixels")
    assert worst <= 1.0 and rp <= 1.0
    assert flips <= max(1, int(0.01 * (~obs).sum()))
    # other noise would be far off: a second call (fresh noise) differs visibly
    again = mf.impute(x, mask, k, want="h_mean")["h_mean"]
    assert max(np.abs(_np(a) - _np(b)).max() for a, b in zip(again, res["fused"]["h_mean"])) > 1e-3


def test_impute_between_train_steps_changes_nothing():
    from iwae_replication_project_amd import Adam
    he, hd, le, ld = ARCHS[1]
    rng = np.random.default_rng(3)
    x = (rng.random((40, 784)) < 0.3).astype(np.float32)
    mask = make_mask(rng, 5, 784)
    m = make_model(he, hd, le, ld, seed=11)
    m.compile(optimizer=Adam(learning_rate=1e-3, epsilon=1e-4))
    m.train_steps(x, 20)
    w0, (m0, v0, t0), g0 = m.get_weights(), m.get_optimizer_state(), m.graph_captures()
    c0 = _counts(m)
    out = m.impute(x[:5], mask, 17)
    assert _counts(m)[0] == c0[0] + 1
    assert all(np.isfinite(v).all() for v in TP._flatten(out))
    w1, (m1, v1, t1) = m.get_weights(), m.get_optimizer_state()
    for p, q in zip(w0, w1):
        np.testing.assert_array_equal(p, q)
    np.testing.assert_array_equal(m0, m1)
    np.testing.assert_array_equal(v0, v1)
    assert t0 == t1 and m.graph_captures() == g0
    m.train_steps(x, 20)
    assert m.graph_captures() == g0                            # replayed, not re-captured
    m.check_kernel_status()


def test_padding_columns_and_rows_past_n_keep_their_sentinel():
    import torch
    from iwae_replication_project_amd import _lib
    for path in PATHS:
        O, spec, params, m = _setup(ODD, path)              # x_dim = 70
        x, mask, eps, u_pix, ref = _case(ODD, 5, 17)
        N, rows, xd, k = 5, 7, spec.x_dim, 17
        ld = 80
        with torch.cuda.stream(m._stream):
            xt, mt = torch.from_numpy(x).to(m.device), torch.from_numpy(mask).to(m.device)
            xm = torch.full((rows, ld), -7.0, device=m.device)
            xw = torch.full((rows, ld), -7.0, device=m.device)
        m._call(m._lib.iwae_impute(m._h, _lib.fptr(xt), _lib.fptr(mt), N, k, 0, None, 0, None, None, _lib.fptr(xm), ld,
                                   _lib.fptr(xw), ld, None, 0, None, 0, None, None, None))
        m._stream.synchronize()
        for t in (xm.cpu().numpy(), xw.cpu().numpy()):
            assert (t[:N, xd:] == -7.0).all() and (t[N:] == -7.0).all()
            assert ((t[:N, :xd] >= 0) & (t[:N, :xd] <= 1)).all()


# ----------------------------------------------------------------------- 10
def test_bad_arguments_raise_before_any_launch():
    import torch
    from iwae_replication_project_amd import _lib
    O, spec, params, m = _setup(1, "auto")
    x, mask, eps, u_pix, ref = _case(1, 5, 17)
    c0 = _counts(m)
    p0 = TP._counts(m)
    with pytest.raises(ValueError):
        m.impute(x, None, 17)                                     # no mask
    with pytest.raises(ValueError):
        m.impute(x, mask[:4], 17)                                 # wrong mask shape
    with pytest.raises(ValueError):
        m.impute(x, mask, 0)                                      # k = 0
    with pytest.raises(ValueError):
        m.impute(x, mask, 17, want=())                            # all outputs off
    with pytest.raises(ValueError):
        m.impute(x, mask, 17, want=("x_mean", "probs"))           # unknown name
    with pytest.raises(ValueError):
        m.impute(x, mask, 17, u=np.zeros(4, np.float32))          # wrong u shape
    with pytest.raises(ValueError):
        m.impute(x, mask, 17, u_pix=np.zeros((5, 783), np.float32))
    with pytest.raises(ValueError):
        m.impute(x, mask, (1 << 20) + 1, want="log_px")           # k > 2^20
    with torch.cuda.stream(m._stream):
        xt, mt = torch.from_numpy(x).to(m.device), torch.from_numpy(mask).to(m.device)
        buf = torch.zeros(5, 788, device=m.device)
        e = [torch.zeros(17, 5, d, device=m.device) for d in spec.n_latent_encoder]
    imp = m._lib.iwae_impute
    xp, mp, p = _lib.fptr(xt), _lib.fptr(mt), _lib.fptr(buf)
    arr2 = (_lib.FP * 2)(_lib.fptr(e[0]), None)
    off = ctypes.cast(ctypes.c_void_p(buf.data_ptr() + 4), _lib.FP)
    Z = (None, 0)
    for rc in (imp(m._h, xp, None, 5, 17, 0, None, 0, None, None, None, 0, None, 0, *Z, *Z, None, None, p),   # NULL mask
               imp(m._h, xp, mp, 5, 17, 0, None, 0, None, None, None, 0, None, 0, *Z, *Z, None, None, None),  # all NULL
               imp(m._h, xp, mp, 5, 17, 0, None, 0, None, None, p, 786, None, 0, *Z, *Z, None, None, None),   # ld % 4
               imp(m._h, xp, mp, 5, 17, 0, None, 0, None, None, p, 780, None, 0, *Z, *Z, None, None, None),   # ld < x_dim
               imp(m._h, xp, mp, 5, 17, 0, None, 0, None, None, None, 0, p, 786, *Z, *Z, None, None, None),   # x_draw ld
               imp(m._h, xp, mp, 5, 17, 0, None, 0, None, None, off, 788, None, 0, *Z, *Z, None, None, None), # alignment
               imp(m._h, xp, mp, 5, 17, 0, None, 0, None, None, None, 0, None, 0, arr2, 1, *Z, None, None, p),  # n_mean
               imp(m._h, xp, mp, 5, 17, 0, None, 0, None, None, None, 0, None, 0, *Z, arr2, 1, None, None, p),  # n_sir
               imp(m._h, xp, mp, 5, 17, 0, None, 0, None, None, None, 0, None, 0, *Z, arr2, 2, None, None, p),  # NULL in h_sir
               imp(m._h, xp, mp, 5, (1 << 20) + 1, 0, None, 0, None, None, None, 0, None, 0, *Z, *Z, None, None, p)):
        assert rc == -1
        with pytest.raises(ValueError):
            _lib.check(m._lib, m._h, rc)
    m._stream.synchronize()
    assert _counts(m) == c0 and TP._counts(m) == p0
    assert (buf == 0).all()
