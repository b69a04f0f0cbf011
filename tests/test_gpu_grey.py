"""Grey-level pixels on the GPU: every kernel's two-log Bernoulli branch
(x log p + (1 - x) log(1 - p): tc_bern of the train engine, mg_bern of the fused
NLL / score / impute kernels, nr_bern_frac of the weight-ring kernels, the
tiled GEMM's epilogue) against the float64 oracle on identical injected
weights and noise, on the cases of tests/grey_cases.py: all-grey batches,
batches that mix binarised and grey images (one launch takes both branches, a
deciding group's boundary lies inside an image and inside a 16-row tile), and
logits of -100, -88 and -87.5, where exp(-l) overflows float32 or its
reciprocal is a denormal.  The launch counters pin which kernels ran
(grey_cases.expected_kernels).

Bars, the project's own: loss and whole gradient 1e-4 relative, each parameter
tensor 5e-4 of its largest entry, Adam as test_gpu_configs._check; log-weights
1e-4 of max|ref|; log p(x) 1e-3 nats; posterior, score and impute by the checks
of their own GPU tests (test_gpu_posterior._check_parity, test_gpu_score.
_check_terms, test_gpu_impute._check).  tests/test_grey_cases.py shows the
reference run in float32 stays within a quarter of them on these very inputs.

Measured on an MI355X, the largest deviation over all cases, patterns, losses
and paths: loss 1.2e-6, whole gradient 4.3e-5, worst tensor 7.7e-5, post-Adam
weights 6.9e-5 (R2 deep, beside 10 x its largest gradient error); log-weights
8.9e-6 of max|lw|, L_k 1.4e-6, L_alpha 6.6e-7, E_q 3.5e-7, reconstruction loss
3.9e-7, log p(x) 6.2e-4 nats (R2 mixed, layer-wise; 784 pixels), log_px_masked
1.5e-4 nats; posterior / impute at most 0.28 of their bars (h_mean), score's
log p(x|h) 1.2e-6 of S_r; binarised images of a mixed batch against the
all-binarised batch 1.9e-7 of max|lw| and 3.1e-5 nats.  Deep logits: -100 with
x = 0.25, -88 with x = 0 and -87.5 with x = 1 each give log p(x) within 5.8e-4
nats and log p(x|h) within 3.9e-5 nats on every path.  Before the two-log
branch formed its sigmoids from exp(-|l|), the same inputs gave NaN at -100 on
the engine, the ring train forward, the fused and the ring NLL (exp(-l) = inf
times 1 / inf = 0), and at -88 with x = 0 an error of 13.9 nats in log p(x) on
the fused and the ring NLL (v_rcp_f32 returns 0 for the denormal
1 / (1 + e^88), so 1 - p became its offset 9.1e-7); -87.5 with x = 1 was within
the bars (0 x log(1 - p)).  The tiled GEMM epilogue was within them throughout."""
import functools

import numpy as np
import pytest

import grey_cases as G
import impute_ref
import pathgrad_ref as R
import posterior_ref
import score_ref
from oracle import iwae_oracle as O

pytestmark = pytest.mark.gpu

REL = 1e-4
TENSOR = 5e-4
ADAM_ATOL = 6e-5
LOGPX_ATOL = 1e-3
PATHS = ("auto", "fused", "layerwise")
COUNTERS = (0, 2, 3, 4, 5, 6, 13, 17, 18, 19, 20, 23, 24)

# (case, pattern, loss id, path, knob set)
TRAIN = [(n, pt, v[0], p, "") for n in ("G1", "G2", "G3") for pt in G.PATTERNS[n] for v in G.loss_variants(n, pt)
         for p in PATHS]
TRAIN += [("GW", pt, "IWAE", "auto", kn) for pt in G.PATTERNS["GW"] for kn in G.GW_KNOBS]
TRAIN += [(n, pt, "IWAE", "auto", kn) for n in G.RING for pt in G.PATTERNS[n] for kn in G.RING_KNOBS]
TRAIN += [("R2", "deep", "L_alpha", "auto", "ring-b3")]        # need_bce: declined by the ring forward, on the engine
FORWARD = [(n, pt, p, "") for n in ("G1", "G2") for pt in G.PATTERNS[n] for p in ("fused", "layerwise")]
FORWARD += [(n, pt, p, kn) for n in G.RING for pt in G.PATTERNS[n]
            for p, kn in (("fused", "nring1"), ("fused", "nring0"), ("layerwise", ""))]
FWD_KNOBS = {"": {}, "nring1": dict(nring=1), "nring0": dict(nring=0)}
ALL_KNOBS = dict(G.GW_KNOBS, **G.RING_KNOBS, **FWD_KNOBS)


def _ids(rows):
    return ["-".join(str(c) for c in r if c != "") for r in rows]


def _flat(ws):
    return np.concatenate([np.asarray(w, np.float64).ravel() for w in ws])


def _np(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _reference(name, pattern, vid):
    out = G.reference_step(name, pattern, vid)
    for a in out[1:]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _forward_reference(name, pattern):
    out = G.forward_reference(name, pattern)
    out[0].setflags(write=False)
    out[3].setflags(write=False)
    return out


def _variant(name, pattern, vid):
    """The loss of a pattern; "binary" and the single-column "deep<j>" run their parent's."""
    return G.variant(name, "deep" if pattern.startswith("deep") else "grey" if pattern == "binary" else pattern, vid)


def _model(name, pattern, vid="IWAE", **kw):
    from iwae_replication_project_amd import Adam, Flexible_Model
    from iwae_replication_project_amd.flexible_iwae import _split, weight_shapes
    he, hd, le, ld, x_dim, B, k, seed = G.CASES[name]
    _, loss, lkw = _variant(name, pattern, vid)
    spec, params, mean, x, eps = G.make(name, pattern)
    m = Flexible_Model(he, hd, le, ld, dataset_bias=mean, loss_function=loss, k=k, seed=1, x_dim=x_dim, **lkw, **kw)
    m.set_weights(_split(O.flatten_params(spec, params).astype(np.float32), weight_shapes(m.dense)))
    m.compile(Adam(learning_rate=1e-3, epsilon=1e-4))
    draws = eps + (G.second_draw(name) if loss == "CIWAE" else [])
    return m, x.astype(np.float32), [e.astype(np.float32) for e in draws]


def _counts(m):
    return {i: int(m._lib.iwae_debug_count(m._h, i)) for i in COUNTERS}


def _advance(m, before):
    return {i: v - before[i] for i, v in _counts(m).items()}


def _assert_counters(adv, exp, ids):
    for i in ids:
        if exp[i] is not None:
            assert (adv[i] > 0) == bool(exp[i]), (i, adv, exp)


def _train_step(name, pattern, vid, path, knobs):
    """One injected-noise train step against float64: loss, gradient (whole and
    per tensor), post-Adam weights.  Returns (model, gradient, reference gradient, counters)."""
    _, loss, lkw = _variant(name, pattern, vid)
    m, x, eps = _model(name, pattern, vid, kernel_path=path, tuning=dict(knobs))
    spec, params = G.make(name, pattern)[:2]
    c0 = _counts(m)
    loss_gpu = m.train_step(x, eps=eps)[loss]
    m.check_kernel_status()
    adv = _advance(m, c0)
    ref_loss, ref_g, ref_w = _reference(name, pattern, vid) if pattern in G.PATTERNS[name] else \
        G.reference_step(name, pattern, vid)
    g, w = _flat(m.get_gradients()), _flat(m.get_weights())
    whole = R.rel_l2(g, ref_g)
    per = [np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)
           for a, b in zip(R.split_tensors(spec, g), R.split_tensors(spec, ref_g))]
    print(f"{name} {pattern} {vid} {path} {knobs}: loss rel {abs(loss_gpu - ref_loss) / abs(ref_loss):.2e}, "
          f"gradient rel-L2 {whole:.2e}, worst tensor {np.max(per):.2e}, post-Adam weights {np.abs(w - ref_w).max():.2e}, "
          f"counters {adv}")
    assert np.isfinite(loss_gpu) and np.isfinite(g).all() and np.isfinite(w).all()
    assert abs(loss_gpu - ref_loss) <= REL * abs(ref_loss), (loss_gpu, ref_loss)
    assert whole <= REL, whole
    assert max(per) <= TENSOR, per
    # Adam as test_gpu_configs._check
    w_from_g = O.Adam(1e-3, 0.9, 0.999, 1e-4).apply(O.flatten_params(spec, params), g)
    np.testing.assert_allclose(w, w_from_g, atol=2e-6)
    np.testing.assert_allclose(w, ref_w, atol=max(ADAM_ATOL, 10 * np.abs(g - ref_g).max()))
    return m, g, ref_g, adv


# ------------------------------------------------------------- a. train step
@pytest.mark.parametrize("name,pattern,vid,path,kn", TRAIN, ids=_ids(TRAIN))
def test_train_step_matches_float64_and_runs_the_expected_kernels(name, pattern, vid, path, kn):
    """Grey, mixed and deep-logit batches through the train step of every path:
    the engine's tc_bern (16-, 32- and 64-row deciding groups on GW; its Keras-BCE
    two-log branch under L_alpha), the row-block and layer-wise paths' tiled GEMM
    epilogue, and on the ring shapes nring_kernel's train forward with the g it
    stores for nrb_kernel (counters 4 / 5 / 6) beside the engine's launches."""
    _, loss, lkw = G.variant(name, pattern, vid)
    knobs = ALL_KNOBS[kn]
    _, g, ref_g, adv = _train_step(name, pattern, vid, path, knobs)
    exp = G.expected_kernels(name, loss, path, knobs, p=lkw.get("p", 1.0))
    _assert_counters(adv, exp, (2, 13, 4, 5, 6))
    if pattern == "deep":
        # the constructed columns' entries of the output Dense's kernel and bias
        spec = G.make(name, pattern)[0]
        gt, rt = R.split_tensors(spec, g)[-2:], R.split_tensors(spec, ref_g)[-2:]
        cols = list(G.deep_columns(G.CASES[name][4]))
        gW, rW = gt[0].reshape(-1, spec.x_dim), rt[0].reshape(-1, spec.x_dim)
        assert np.isfinite(gW[:, cols]).all() and np.isfinite(gt[1][cols]).all()
        assert np.abs(gW[:, cols] - rW[:, cols]).max() <= TENSOR * np.abs(rW).max()
        assert np.abs(gt[1][cols] - rt[1][cols]).max() <= TENSOR * np.abs(rt[1]).max()


# ------------------------------------------------------ b. forward quantities
def _check_forward(m, x, eps, name, pattern, label):
    k = G.CASES[name][6]
    lw_ref, lk_ref, eq_ref, lp_ref, la_ref = _forward_reference(name, pattern) if pattern in G.PATTERNS[name] else \
        G.forward_reference(name, pattern)
    lw = _np(m.get_log_weights(x, k, eps=eps))
    lk = m.get_L_k(x, k, eps=eps)
    la = m.get_L_alpha(x, k, 0.3, eps=eps)
    eq = m.get_E_qhIx_log_pxIh(x, k, eps=eps)
    c0 = _counts(m)
    lp = _np(m.log_px(x, k, eps=eps))
    adv = _advance(m, c0)
    m.check_kernel_status()
    e_lw = np.abs(lw - lw_ref).max() / np.abs(lw_ref).max()
    print(f"{label}: log-weights {e_lw:.2e} of max|lw|, L_k rel {abs(lk - lk_ref) / abs(lk_ref):.2e}, "
          f"L_alpha rel {abs(la - la_ref) / abs(la_ref):.2e}, E_q rel {abs(eq - eq_ref) / abs(eq_ref):.2e}, "
          f"log p(x) {np.abs(lp - lp_ref).max():.2e} nats, counters {adv}")
    assert lw.shape == lw_ref.shape
    assert np.isfinite(lw).all() and np.isfinite(lp).all()
    assert e_lw <= REL, e_lw
    assert abs(lk - lk_ref) <= REL * abs(lk_ref), (lk, lk_ref)
    assert abs(la - la_ref) <= REL * abs(la_ref), (la, la_ref)
    assert abs(eq - eq_ref) <= REL * abs(eq_ref), (eq, eq_ref)
    assert np.abs(lp - lp_ref).max() <= LOGPX_ATOL
    return adv


@pytest.mark.parametrize("name,pattern,path,kn", FORWARD, ids=_ids(FORWARD))
def test_forward_quantities_match_float64(name, pattern, path, kn):
    """get_log_weights, the IWAE and L_alpha bounds, E_q log p(x|h) (the need_bce
    two-log terms) and log_px on injected noise: the fused NLL kernel's mg_bern
    (counter 0), on the ring shapes nr_bern_frac of nring_kernel (counter 3;
    k = 192 >= 128) or mg_bern with the ring off, and the layer-wise GEMM."""
    knobs = FWD_KNOBS[kn]
    m, x, eps = _model(name, pattern, kernel_path=path, tuning=dict(knobs))
    adv = _check_forward(m, x, eps, name, pattern, f"{name} {pattern} {path} {kn}")
    _assert_counters(adv, G.expected_kernels(name, "IWAE", path, knobs), (0, 3))


@pytest.mark.parametrize("path", ["auto", "layerwise"])
@pytest.mark.parametrize("name,pattern", [(n, pt) for n in ("G1", "G2") for pt in G.PATTERNS[n]])
def test_reconstruction_loss_matches_float64(name, pattern, path):
    """get_reconstruction_loss: the Keras BCE of grey pixels against the
    reconstructed probabilities (tests/test_gpu_statistics.py's comparison)."""
    m, x, _ = _model(name, pattern, kernel_path=path)
    spec, params, _, x64, _ = G.make(name, pattern)
    le, L, B = spec.n_latent_encoder, spec.L, x.shape[0]
    rng = np.random.default_rng(G.CASES[name][7] + 1)
    e_enc = [rng.standard_normal((1, B, d)).astype(np.float32) for d in le]
    e_pri = [rng.standard_normal((1, B, le[L - 2 - j])).astype(np.float32) for j in range(L - 1)]
    loss = m.get_reconstruction_loss(x, eps=e_enc + e_pri)
    _, rl = O.reconstruct(params, spec, x64, [e.astype(np.float64) for e in e_enc], [e.astype(np.float64) for e in e_pri])
    print(f"{name} {pattern} {path}: reconstruction loss rel {abs(loss - rl) / abs(rl):.2e}")
    assert abs(loss - rl) <= REL * abs(rl), (loss, rl)


@pytest.mark.parametrize("path", ["fused", "layerwise"])
@pytest.mark.parametrize("pattern", G.PATTERNS["G2"])
def test_log_px_masked_matches_float64(pattern, path):
    """log_px_masked (latent units zeroed, F:466-F:494) on grey pixels."""
    m, x, eps = _model("G2", pattern, kernel_path=path)
    spec, params, _, x64, e64 = G.make("G2", pattern)
    masks = [np.array([1, 0, 1, 1, 0, 1, 1], np.float64), np.array([1, 1, 0], np.float64)]
    k = G.CASES["G2"][6]
    ref = O.log_px_per_image(params, spec, x64, k, eps=e64, masks=masks)
    lp = _np(m.log_px_masked(x, masks, k, eps=eps))
    print(f"G2 {pattern} {path}: masked log p(x) {np.abs(lp - ref).max():.2e} nats")
    assert np.abs(lp - ref).max() <= LOGPX_ATOL


# ------------------------------------------- c. posterior, score and impute
@pytest.mark.parametrize("path", ["auto", "layerwise"])
@pytest.mark.parametrize("pattern", ["grey", "mixed"])
def test_posterior_score_and_impute_match_float64(pattern, path):
    """G2 through iwae_posterior, iwae_score (log p(x|h) of the oracle's own
    latents: score_kernel's mg_bern, counter 23) and iwae_impute with 30 % of the
    pixels missing (the MASK instantiation of mg_bern, where x <= 0 || x == 1
    counts as binarised; counter 19), by the checks and bars of their own tests."""
    import test_gpu_impute as TI
    import test_gpu_posterior as TP
    import test_gpu_score as TS
    m, x, eps = _model("G2", pattern, kernel_path=path)
    spec, params, _, x64, e64 = G.make("G2", pattern)
    k = G.CASES["G2"][6]
    fused = path == "auto"
    # posterior
    ref = posterior_ref.posterior(params, spec, x64, e64)
    c0 = _counts(m)
    out = m.posterior(x, k, eps=eps, want=("h_mean", "probs", "weights", "ess", "log_px"))
    adv = _advance(m, c0)
    assert (adv[17] > 0, adv[18] > 0) == (fused, not fused), adv
    TP._check_parity(out, ref, k, f"posterior G2 {pattern} {path}")
    # against the reference's own weights and ess: log-weights good to e = 1e-4 max|lw| move
    # log w~ = lw - logsumexp(lw) by at most 2 e, so w~ by a factor exp(+-2 e) and
    # ess = 1 / sum w~^2 by a factor exp(+-4 e)
    e = REL * np.abs(ref["lw"]).max()
    w, ess = _np(out["weights"]).astype(np.float64), _np(out["ess"]).astype(np.float64)
    assert (np.abs(w - ref["weights"]) <= np.expm1(2 * e) * ref["weights"]).all()
    assert (np.abs(ess - ref["ess"]) <= np.expm1(4 * e) * ref["ess"]).all()
    # score, on the reference's latents rounded to float32
    h = [score_ref.f32r(v) for v in ref["cache"]["h"]]
    sref = score_ref.score(params, spec, x64, h)
    c0 = _counts(m)
    sout = m.score(x, [np.asarray(v, np.float32) for v in h], want=("log_px",))
    adv = _advance(m, c0)
    assert (adv[23] > 0, adv[24] > 0) == (fused, not fused), adv
    TS._check_terms(sout, sref, f"score G2 {pattern} {path}")
    # impute
    mask = G.impute_mask("G2")
    rng = np.random.default_rng(G.CASES["G2"][7] + 300)
    u_pix = rng.random(x.shape).astype(np.float32)
    iref = impute_ref.impute(params, spec, x64, mask, e64)
    c0 = _counts(m)
    iout, u = TI._run(m, x, mask, eps, u_pix, k, rng)
    adv = _advance(m, c0)
    assert (adv[19] > 0, adv[20] > 0) == (fused, not fused), adv
    TI._check(iout, x, mask, u, u_pix, iref, k, f"impute G2 {pattern} {path}")
    m.check_kernel_status()


# ------------------------------------------------- d. the mixed-batch property
MIXED = [("G1", "auto", ""), ("G2", "auto", ""), ("G2", "layerwise", ""), ("GW", "auto", "wide2"), ("GW", "auto", "rt2"),
         ("R1", "auto", "nring1"), ("R2", "auto", "nring1"), ("R2", "auto", "nring0")]


@pytest.mark.parametrize("name,path,kn", MIXED, ids=_ids(MIXED))
def test_binarised_images_do_not_depend_on_their_neighbours(name, path, kn):
    """The binarised images of a mixed batch against the same images (same noise)
    in an all-binarised batch: their log-weight rows and log p(x) agree within
    the bars -- not bit for bit: a grey neighbour may switch their tile or
    workgroup to the two-log form, which is the same function."""
    knobs = ALL_KNOBS[kn]
    k = G.CASES[name][6]
    out = {}
    for pattern in ("mixed", "binary"):
        m, x, eps = _model(name, pattern, kernel_path=path, tuning=dict(knobs))
        out[pattern] = (_np(m.get_log_weights(x, k, eps=eps)).astype(np.float64), _np(m.log_px(x, k, eps=eps)).astype(np.float64))
        m.check_kernel_status()
    b = G.binarised_images(name)
    lw_ref = G.forward_reference(name, "binary")[0]
    d_lw = np.abs(out["mixed"][0][:, b] - out["binary"][0][:, b]).max() / np.abs(lw_ref[:, b]).max()
    d_lp = np.abs(out["mixed"][1][b] - out["binary"][1][b]).max()
    print(f"{name} {path} {kn}: binarised images, mixed against all-binarised batch: log-weights {d_lw:.2e} of max|lw|, "
          f"log p(x) {d_lp:.2e} nats")
    assert np.isfinite(out["mixed"][0]).all() and np.isfinite(out["binary"][0]).all()
    assert d_lw <= REL, d_lw
    assert d_lp <= LOGPX_ATOL, d_lp
    # and the all-binarised batch is the reference's
    assert np.abs(out["binary"][0] - lw_ref).max() <= REL * np.abs(lw_ref).max()


# ------------------------------------------------------------ e. deep logits
DEEP_ONE = [(n, j) for n in G.DEEP_CASES for j in range(3)]


@pytest.mark.parametrize("name,j", DEEP_ONE, ids=[f"{n}-deep{j}" for n, j in DEEP_ONE])
def test_deep_logit_columns_one_at_a_time(name, j):
    """One constructed column alone (logit -100, -88 or -87.5 in every row), so
    the record shows what each pixel gives: forward quantities on the fused and
    layer-wise paths, the engine's train step, and on the ring shape the ring
    NLL and the ring train forward.  Everything finite and within the bars."""
    pattern = f"deep{j}"
    ring = name in G.RING
    for path, knobs in (("fused", dict(nring=1)), ("layerwise", {})):
        m, x, eps = _model(name, pattern, kernel_path=path, tuning=dict(knobs))
        _check_forward(m, x, eps, name, pattern, f"{name} logit {G.DEEP_BIASES[j]} x {G.DEEP_PIXELS[j]} {path}")
    _train_step(name, pattern, "IWAE", "auto", G.RING_KNOBS["ring-b0"] if ring else {})
    if not ring:
        _train_step(name, pattern, "L_alpha", "auto", {})
    if name == "G2":
        spec, params, _, x64, e64 = G.make(name, pattern)
        m, x, eps = _model(name, pattern)
        h = [score_ref.f32r(v) for v in O.forward(params, spec, x64, e64)["h"]]
        sref = score_ref.score(params, spec, x64, h)
        got = _np(m.score(x, [np.asarray(v, np.float32) for v in h], want=("log_px",))["log_px"])
        err = np.abs(got - sref["logpx"]).max()
        print(f"{name} logit {G.DEEP_BIASES[j]} x {G.DEEP_PIXELS[j]} score: log p(x|h) max abs err {err:.2e} nats")
        assert np.isfinite(got).all() and err <= REL * np.abs(sref["logpx"]).max()
