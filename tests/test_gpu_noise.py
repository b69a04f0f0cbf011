"""Device noise on the GPU: every kernel that draws Philox noise against the
host restatement of tests/noise_ref.py (Philox4x32-10 in integers, the kernel's
float32 uniforms, Box-Muller in float64).

a. The normals themselves: with every lmu / lstd kernel and bias zeroed each
   latent is eps (1 + 1e-6), so iwae_generate's h_out (gen_kernel and the
   layer-wise gen_top_kernel / gauss_fwd_kernel), iwae_encode's lat_out and
   iwae_posterior's k = 1 h_mean / h_sir (post_kernel from rng[1], and the
   layer-wise pass) show the draws directly, at noise positions 0 and 1.
b. Every drawing home with general (Glorot) weights against the float64 oracle
   fed with the reference noise, under the project's own bars (module docstring
   of tests/test_gpu_shapes.py; reconstruction, encoder means, generation,
   posterior and imputation as tests/test_gpu_statistics.py,
   tests/test_gpu_generate.py, tests/test_gpu_posterior.py and
   tests/test_gpu_impute.py state them).  tests/test_noise_ref.py shows the
   oracle in float32 on the same noise stays within a quarter of them.
c. Position and key bookkeeping: a sequence of calls leaves the position
   noise_ref.ADVANCE predicts; noise streams keep their own positions and keys.

The launch counters (iwae_debug_count) pin which kernel ran in every test.

NORMAL_BAR is 4 x the largest |device - reference| over all draws of (a) as
measured on an MI355X, rounded up to one digit (the draws are deterministic;
the margin is for another instruction sequence of a later compiler).  A single
element beyond it beside agreeing neighbours is an addressing error.

Measured on an MI355X (test_zz_print_the_worst_measured_values prints them):
a. normals: max |device - reference| 4.965e-07 over all draws (numpy's own
   float32 Box-Muller on the same uniforms: 1.1e-06, tests/test_noise_ref.py),
   so NORMAL_BAR = 2e-6.
b. worst value per bar: train step loss 3.9e-6, whole gradient 5.8e-5, worst
   tensor 1.6e-4, post-Adam weights 9.8e-6; three steps loss 8.6e-7, final
   weights 8.0e-7; log-weights 7.1e-6 of max|lw|; bounds 4.4e-6; log p(x) 7.2e-4
   nats (the 784-pixel weight-ring model; 2.0e-4 on the 20-pixel ones); as
   error / bar: reconstruction probs 0.08, encoder means 0.33, generation probs
   0.11 and latents 0.30, encode latents 0.81, posterior lw 0.25, sum 0.03, ess
   0.06, h_mean 0.24, h_sir 0.35, probs 0.08, imputation lw 0.12, sum 0.05, ess
   0.07, h_mean 0.14, x_mean 0.07; every pixel draw and resampled index equal.
No kernel or host code had to change: every drawing site addresses Philox as
include/iwae.h says."""
import numpy as np
import pytest

import noise_ref as N
import pathgrad_ref as R
import posterior_ref as P
from oracle import iwae_oracle as O
from test_gpu_generate import LATENT_TOL, PROBS_TOL

pytestmark = pytest.mark.gpu

KEY = N.key(N.SEED)
REL = 1e-4
TENSOR = 5e-4
ADAM_ATOL = 6e-5
LOGPX_ATOL = 1e-3
STEPS_W_ATOL = 1e-5                  # test_five_adam_steps_track_oracle's
NORMAL_BAR = 2e-6                    # 4 x 4.965e-07 = 1.986e-06, rounded up to one digit
SC = np.float64(np.float32(1.0) + np.float32(1e-6))      # exp(0) + 1e-6 in float32
COUNTERS = (0, 1, 2, 3, 4, 5, 6, 7, 10, 11, 12, 13, 14, 17, 18, 19, 20, 22, 23, 24)
WORST = {}


def _note(name, value):
    WORST[name] = max(WORST.get(name, 0.0), float(value))


def _flat(ws):
    return np.concatenate([np.asarray(w, np.float64).ravel() for w in ws])


def _np(t):
    return t.cpu().numpy()


def _counts(m):
    return {i: int(m._lib.iwae_debug_count(m._h, i)) for i in COUNTERS}


def _advance(m, before):
    return {i: v - before[i] for i, v in _counts(m).items()}


def _model(model, B=3, vid="IWAE", k=17, zero_heads=False, **kw):
    """The model of a case on the GPU with the oracle's float32-rounded weights,
    seeded with noise_ref.SEED; (model, x float32)."""
    from iwae_replication_project_amd import Adam, Flexible_Model
    from iwae_replication_project_amd.flexible_iwae import _split, weight_shapes
    (he, hd, le, ld), x_dim = N.arch(model)
    _, spec, params, _, x = N.case(model, B)
    if zero_heads:
        params = {n: ([np.zeros_like(w), np.zeros_like(b)] if n.endswith((".lmu", ".lstd")) else [w, b])
                  for n, (w, b) in params.items()}
    m = Flexible_Model(he, hd, le, ld, dataset_bias=None, loss_function=vid, k=k, seed=N.SEED, x_dim=x_dim,
                       **N.loss_kw(vid, k), **kw)
    m.set_weights(_split(O.flatten_params(spec, params).astype(np.float32), weight_shapes(m.dense)))
    m.compile(Adam(learning_rate=1e-3, epsilon=1e-4))
    return m, x.astype(np.float32)


def _bar(tol, ref):
    return tol["atol"] + tol["rtol"] * np.abs(ref)


def _within(a, ref, tol, name):
    r = (np.abs(np.asarray(a, np.float64) - ref) / _bar(tol, ref)).max()
    _note(name + " (error / bar)", r)
    assert r <= 1.0, (name, r)


# =================================================== a. the normals themselves
def _normal_err(dev, ref, what):
    dev = np.asarray(dev, np.float64)
    assert dev.shape == ref.shape, (what, dev.shape, ref.shape)
    err = np.abs(dev - ref)
    worst = float(err.max())
    _note("a. normals max |device - reference|", worst)
    print(f"{what}: max |device - reference| {worst:.3e} over {err.size} draws")
    assert worst <= NORMAL_BAR, (what, worst, np.argwhere(err > NORMAL_BAR)[:8])
    return worst


@pytest.mark.parametrize("path", ["auto", "layerwise"])
@pytest.mark.parametrize("model", list(N.MODELS))
def test_generated_latents_are_the_reference_normals(model, path):
    """iwae_generate without h_top: h_L is the top draw itself (layer id
    MAX_LAYERS + L - 1), prior layer j's latent its draw (MAX_LAYERS + j) times
    1 + 1e-6; 19 rows straddle a 16-row tile; the second call draws at position 1."""
    m, _ = _model(model, zero_heads=True, kernel_path=path)
    dims, n = m.n_latent_encoder, 19
    L = len(dims)
    c0 = _counts(m)
    for pos in (0, 1):
        hs = m.sample(n, return_latents=True)["h"]
        _normal_err(_np(hs[L - 1]), N.eps_top(KEY, pos, n, dims)[0], f"{model} {path} position {pos} h_{L}")
        for j, e in enumerate(N.eps_prior(KEY, pos, n, dims)):
            _normal_err(_np(hs[L - 2 - j]), e[0] * SC, f"{model} {path} position {pos} h_{L - 1 - j}")
    adv = _advance(m, c0)
    assert adv[10] == (2 if path == "auto" else 0), adv


@pytest.mark.parametrize("B,k,chunk", [(3, 17, 0), (5, 1, 0), (5, 17, 2)])
@pytest.mark.parametrize("model", list(N.MODELS))
def test_encoded_latents_are_the_reference_normals(model, B, k, chunk):
    """iwae_encode's lat_out (gauss_fwd_kernel): row = b k + s within the chunk,
    layer id i; every chunk of every call at the next position."""
    m, x = _model(model, B, zero_heads=True)
    dims = m.n_latent_encoder
    c0 = _counts(m)
    pos = 0
    for call in range(2):
        hs, _, _ = m.encoder(x, k, chunk=chunk)
        ref, chunks = N.eps_chunked(KEY, pos, B, k, dims, chunk or B)
        for i, (h, e) in enumerate(zip(hs, ref)):
            _normal_err(_np(h), e * SC, f"{model} B={B} k={k} chunk={chunk} call {call} h_{i + 1}")
        assert chunks == N.advance("encode", N=B, k=k, chunk=chunk)
        pos += chunks
    adv = _advance(m, c0)
    assert adv[0] == 0 and adv[13] == 0 and adv[2] == 0, adv      # layer-wise kernels whatever the path


@pytest.mark.parametrize("path", ["auto", "layerwise"])
@pytest.mark.parametrize("chunk", [0, 2])
@pytest.mark.parametrize("model", list(N.MODELS))
def test_posterior_latents_at_one_sample_are_the_reference_normals(model, chunk, path):
    """iwae_posterior at k = 1: h_mean and h_sir are the single sample's latents.
    The fused second pass (post_kernel) recomputes them from the base the first
    pass left in rng[1]; the layer-wise one reads the first pass's rows."""
    NN = N.NLL_N
    m, x = _model(model, NN, zero_heads=True, kernel_path=path)
    dims = m.n_latent_encoder
    c0 = _counts(m)
    pos = 0
    for call in range(2):
        out = m.posterior(x, 1, chunk=chunk, want=("h_mean", "h_sir", "weights"))
        ref, chunks = N.eps_chunked(KEY, pos, NN, 1, dims, chunk or NN)
        np.testing.assert_array_equal(_np(out["weights"]), 1.0)
        for i, e in enumerate(ref):
            _normal_err(_np(out["h_mean"][i]), e[0] * SC, f"{model} {path} chunk={chunk} call {call} h_mean_{i + 1}")
            _normal_err(_np(out["h_sir"][i]), e[0] * SC, f"{model} {path} chunk={chunk} call {call} h_sir_{i + 1}")
        pos += chunks
    adv = _advance(m, c0)
    assert (adv[17], adv[18]) == ((pos, 0) if path == "auto" else (0, pos)), adv


# ================================================ b. every home, oracle on the reference noise
TRAIN = [c + (p,) for c in N.TRAIN for p in N.TRAIN_PATHS]


def _check_step(m, spec, params, vid, loss_gpu, ref, label):
    ref_loss, ref_g, ref_w = ref
    g, w = _flat(m.get_gradients()), _flat(m.get_weights())
    whole = R.rel_l2(g, ref_g)
    per = [np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)
           for a, b in zip(R.split_tensors(spec, g), R.split_tensors(spec, ref_g))]
    e_loss = abs(loss_gpu - ref_loss) / abs(ref_loss)
    print(f"{label}: loss rel {e_loss:.2e}, gradient rel-L2 {whole:.2e}, worst tensor {max(per):.2e}, "
          f"post-Adam weights {np.abs(w - ref_w).max():.2e}")
    _note("b. train loss rel", e_loss)
    _note("b. train gradient rel-L2", whole)
    _note("b. train worst tensor", max(per))
    _note("b. train post-Adam weights", np.abs(w - ref_w).max())
    assert np.isfinite(loss_gpu) and np.isfinite(g).all()
    assert e_loss <= REL, (loss_gpu, ref_loss)
    assert whole <= REL, whole
    assert max(per) <= TENSOR, per
    w_from_g = O.Adam(1e-3, 0.9, 0.999, 1e-4).apply(O.flatten_params(spec, params), g)
    np.testing.assert_allclose(w, w_from_g, atol=2e-6)
    np.testing.assert_allclose(w, ref_w, atol=max(ADAM_ATOL, 10 * np.abs(g - ref_g).max()))


@pytest.mark.parametrize("model,B,k,vid,path", TRAIN, ids=["-".join(map(str, c)) for c in TRAIN])
def test_train_step_on_device_noise_matches_float64(model, B, k, vid, path):
    """One train step that draws its own noise, against the oracle's step on
    the reference noise of position 0 (CIWAE: the second draw from rows
    (B + b) k + s): layer-wise, row-block and engine; IWAE_DREG's path-gradient
    jobs re-read the stored eps."""
    m, x = _model(model, B, vid, k, kernel_path=path)
    _, spec, params, _, _ = N.case(model, B)
    c0 = _counts(m)
    loss_gpu = m.train_step(x)[vid]
    m.check_kernel_status()
    adv = _advance(m, c0)
    _check_step(m, spec, params, vid, loss_gpu, N.train_reference(model, B, k, vid), f"{model} {B}x{k} {vid} {path} {adv}")
    engine = path == "auto" and vid not in R.LOSSES
    row_block = path == "fused" or (path == "auto" and vid in R.LOSSES)
    assert (adv[2] > 0) == engine and (adv[13] > 0) == row_block, adv
    if vid in R.LOSSES:
        assert (adv[11] > 0) == row_block and (adv[12] > 0) == (not row_block), adv


@pytest.mark.parametrize("tc_bound", [1, 0])
def test_train_step_at_4097_rows_on_the_wide_engine_and_the_weight_ring(tc_bound):
    """B = 17, k = 241: the wide engine launches and the weight-ring train
    forward (counter 4) draw the noise.  With 17 images of 241 samples the
    bound runs inside the engine's backward launch (use_tc_bound: up to 64
    images of up to 256 samples), which then runs the whole backward; with that
    knob off the bound is a launch of its own and the weight-ring backwards
    (counters 5 and 6) re-read the stored eps."""
    model, B, k, vid = N.RING_POINT
    m, x = _model(model, B, vid, k, tuning={"tc_bound": tc_bound})
    _, spec, params, _, _ = N.case(model, B)
    c0 = _counts(m)
    loss_gpu = m.train_step(x)[vid]
    m.check_kernel_status()
    adv = _advance(m, c0)
    assert adv[2] > 0 and adv[4] > 0, adv
    assert (adv[5] > 0, adv[6] > 0) == ((True, True) if tc_bound == 0 else (False, False)), adv
    _check_step(m, spec, params, vid, loss_gpu, N.train_reference(model, B, k, vid), f"RING {B}x{k} tc_bound={tc_bound} {adv}")


@pytest.mark.parametrize("graphs", [True, False])
def test_three_steps_track_the_oracle_on_the_noise_of_each_position(graphs):
    """train_steps: step i draws at position i (captured graphs or eager
    launches); the oracle is stepped through Adam on the same three draws."""
    model, B, k, n = N.STEPS
    m, _ = _model(model, B, "IWAE", k, use_graphs=graphs)
    c0 = _counts(m)
    losses = np.asarray(m.train_steps(N.steps_images().astype(np.float32), B), np.float64)
    m.check_kernel_status()
    adv = _advance(m, c0)
    ref_l, ref_w = N.steps_reference()
    w = _flat(m.get_weights())
    print(f"graphs {graphs}: loss rel {np.abs(losses / ref_l - 1).max():.2e}, final weights {np.abs(w - ref_w).max():.2e}, {adv}")
    _note("b. three steps loss rel", np.abs(losses / ref_l - 1).max())
    _note("b. three steps final weights", np.abs(w - ref_w).max())
    assert adv[2] > 0 and (adv[7] > 0) == graphs, adv
    assert (np.abs(losses - ref_l) <= REL * np.abs(ref_l)).all(), (losses, ref_l)
    np.testing.assert_allclose(w, ref_w, atol=STEPS_W_ATOL)
    assert m.get_optimizer_state()[2] == n


FORWARD = [c + (p,) for c in N.FORWARD for p in N.TRAIN_PATHS]


@pytest.mark.parametrize("model,B,k,path", FORWARD, ids=["-".join(map(str, c)) for c in FORWARD])
def test_log_weights_and_bound_on_device_noise_match_float64(model, B, k, path):
    """get_log_weights at position 0, then the forward-only IWAE bound at 1 and
    E_q log p(x|h) at 2."""
    m, x = _model(model, B, k=k, kernel_path=path)
    c0 = _counts(m)
    lw = _np(m.get_log_weights(x, k)).astype(np.float64)
    lk = m.get_L_k(x, k)
    eq = m.get_E_qhIx_log_pxIh(x, k)
    m.check_kernel_status()
    adv = _advance(m, c0)
    refs = [N.forward_reference(model, B, k, pos) for pos in range(3)]
    lk_ref, eq_ref = float(O.L_k_from_weights(refs[1]["lw"])), float(np.mean(refs[2]["bce_row"]))
    e_lw = np.abs(lw - refs[0]["lw"]).max() / np.abs(refs[0]["lw"]).max()
    print(f"{model} {B}x{k} {path}: log-weights {e_lw:.2e} of max|lw|, L_k rel {abs(lk - lk_ref) / abs(lk_ref):.2e}, "
          f"E_q rel {abs(eq - eq_ref) / abs(eq_ref):.2e}, {adv}")
    _note("b. log-weights / max|lw|", e_lw)
    _note("b. bound rel", max(abs(lk - lk_ref) / abs(lk_ref), abs(eq - eq_ref) / abs(eq_ref)))
    assert lw.shape == refs[0]["lw"].shape and e_lw <= REL, e_lw
    assert abs(lk - lk_ref) <= REL * abs(lk_ref), (lk, lk_ref)
    assert abs(eq - eq_ref) <= REL * abs(eq_ref), (eq, eq_ref)
    assert adv[2] == 0 and (adv[13] > 0) == (path != "layerwise"), adv


NLL = [c + (p,) for c in N.NLL for p in ("auto", "layerwise")]


@pytest.mark.parametrize("model,NN,k,chunk,rows,path", NLL, ids=["-".join(map(str, c)) for c in NLL])
def test_log_px_chunks_draw_at_consecutive_positions_with_local_rows(model, NN, k, chunk, rows, path):
    """log_px, then log_px_partials from where it stopped: every (image chunk,
    sample chunk) draws at the next position with rows local to it --
    mega_fwd_kernel, the weight ring where a sample chunk has 128 rows per
    image or more (counter 3), the layer-wise fallback."""
    m, x = _model(model, NN, kernel_path=path, tuning={} if rows is None else {"nll_rows": rows})
    c0 = _counts(m)
    lp = _np(m.log_px(x, k, chunk=chunk)).astype(np.float64)
    adv = _advance(m, c0)
    ref, chunks = N.nll_reference(model, NN, k, chunk, rows)
    mm, ss = m.log_px_partials(x, k, chunk=chunk)
    lp2 = _np(mm).astype(np.float64) + np.log(_np(ss).astype(np.float64)) - np.log(k)
    ref2, _ = N.nll_reference(model, NN, k, chunk, rows, base=chunks)
    m.check_kernel_status()
    print(f"{model} N={NN} k={k} chunk={chunk} nll_rows={rows} {path}: log p(x) {np.abs(lp - ref).max():.2e} nats, partials "
          f"{np.abs(lp2 - ref2).max():.2e} nats, {chunks} chunks, {adv}")
    _note("b. log p(x) nats", max(np.abs(lp - ref).max(), np.abs(lp2 - ref2).max()))
    assert np.abs(lp - ref).max() <= LOGPX_ATOL and np.abs(lp2 - ref2).max() <= LOGPX_ATOL
    imgs, ks = N.nll_chunks(NN, k, chunk, **({} if rows is None else dict(nll_rows=rows)))
    ring = sum(1 for _ in range(0, NN, imgs) for s0 in range(0, k, ks) if min(ks, k - s0) >= 128) if model == "RING" else 0
    assert adv[0] == (chunks if path == "auto" else 0) and adv[3] == (ring if path == "auto" else 0), (adv, chunks, ring)


def test_log_px_masked_draws_the_reference_noise():
    model, NN, k, rows = N.NLL_MASKED
    masks = N.latent_masks(model)
    m, x = _model(model, NN, tuning={"nll_rows": rows})
    c0 = _counts(m)
    lp = _np(m.log_px_masked(x, masks, k)).astype(np.float64)
    adv = _advance(m, c0)
    ref, chunks = N.nll_reference(model, NN, k, 0, rows, masks=masks)
    print(f"log_px_masked: {np.abs(lp - ref).max():.2e} nats over {chunks} chunks, {adv}")
    _note("b. log p(x) nats", np.abs(lp - ref).max())
    assert chunks > 1 and adv[0] == 0, (chunks, adv)
    assert np.abs(lp - ref).max() <= LOGPX_ATOL


@pytest.mark.parametrize("path", ["auto", "layerwise"])
@pytest.mark.parametrize("model", N.STAT_MODELS)
def test_reconstruction_and_encoder_means_draw_the_reference_noise(model, path):
    """reconstructed_x_probs: encoder ids at row b, then the prior ids, position
    0; the loss at position 1; encoder_means (row = b n + s) at position 2."""
    B = N.SHAPES[0][0]
    m, x = _model(model, B, kernel_path=path)
    probs = _np(m.reconstructed_x_probs(x))
    loss = m.get_reconstruction_loss(x)
    rp, _ = N.reconstruct_reference(model, B, 0)
    _, rl = N.reconstruct_reference(model, B, 1)
    assert probs.shape == (1, B, N.X_DIM)
    _within(probs, rp, PROBS_TOL, "b. reconstruction probs")
    _note("b. bound rel", abs(loss - rl) / abs(rl))
    assert abs(loss - rl) <= REL * abs(rl), (loss, rl)
    m2, x5 = _model(model, N.NLL_N, kernel_path=path)
    means = m2.encoder_means(x5, N.MEANS_N)
    for a, r in zip(means, N.encoder_means_reference(model, N.NLL_N, N.MEANS_N, 0)):
        assert tuple(a.shape) == r.shape
        _within(_np(a), r, LATENT_TOL, "b. encoder means")
    again = m2.encoder_means(x5, N.MEANS_N)
    for a, r in zip(again, N.encoder_means_reference(model, N.NLL_N, N.MEANS_N, 1)):
        _within(_np(a), r, LATENT_TOL, "b. encoder means")
    m.check_kernel_status()


@pytest.mark.parametrize("path", ["auto", "layerwise"])
@pytest.mark.parametrize("model", N.STAT_MODELS)
def test_sample_draws_the_reference_latents_and_pixels(model, path):
    """sample: latents, probabilities and the pixel draws (layer id
    2 MAX_LAYERS, row = the generated row), at positions 0 and 1."""
    m, _ = _model(model, kernel_path=path)
    n = 19
    c0 = _counts(m)
    for pos in (0, 1):
        out = m.sample(n, return_latents=True)
        rp, rh, u = N.generate_reference(model, n, pos)
        _within(_np(out["probs"]), rp, PROBS_TOL, "b. generation probs")
        for hd, hr in zip(out["h"], rh):
            assert tuple(hd.shape) == hr.shape
            _within(_np(hd), hr, LATENT_TOL, "b. generation latents")
        px = _np(out["x"])
        sure = np.abs(u.astype(np.float64) - rp) > 1e-3          # no near tie (probs within 2.02e-4 of rp)
        assert sure.mean() > 0.98 and np.isin(px, (0.0, 1.0)).all()
        np.testing.assert_array_equal(px[sure], (u < rp).astype(np.float32)[sure])
    assert _advance(m, c0)[10] == (2 if path == "auto" else 0)


def _check_weights(out, ref, k, label):
    """log p(x) under this module's 1e-3 nats (the posterior tests' own bar on it
    is 0.05); returns the device weights."""
    w = _np(out["weights"]).astype(np.float64)
    lpx = _np(out["log_px"]).astype(np.float64)
    _note("b. log p(x) nats", np.abs(lpx - ref["log_px"]).max())
    assert np.abs(lpx - ref["log_px"]).max() <= LOGPX_ATOL
    return w


@pytest.mark.parametrize("path", ["auto", "layerwise"])
@pytest.mark.parametrize("chunk", [0, 2])
@pytest.mark.parametrize("model", N.POSTERIOR_MODELS)
def test_posterior_draws_the_reference_noise_and_resampling_uniform(model, chunk, path):
    """iwae_posterior at k = 17: weights, ess, log p(x), h_mean, probs by
    test_gpu_posterior's bars; the SIR index from the reference uniform (layer
    id 2 MAX_LAYERS + 1, row = image in chunk, the chunk's base in rng[1]) and
    the device's weights; h_sir = that sample's latents."""
    from test_gpu_posterior import _check_parity
    NN, k = N.NLL_N, N.POSTERIOR_K
    m, x = _model(model, NN, kernel_path=path)
    c0 = _counts(m)
    out = m.posterior(x, k, chunk=chunk)
    adv = _advance(m, c0)
    ref = N.posterior_reference(model, NN, k, chunk or NN)
    w = _check_weights(out, ref, k, model)
    ratios = _check_parity(out, ref, k, f"{model} chunk={chunk} {path}")
    for name, r in ratios.items():
        _note(f"b. posterior {name} (error / bar)", r)
    cum = np.cumsum(w, axis=1)
    assert np.abs(cum - ref["u"][:, None].astype(np.float64)).min() >= 1e-5        # no near tie in the device's own sum
    idx = P.sir_index(w, ref["u"].astype(np.float64))
    np.testing.assert_array_equal(idx, ref["sir_index"])
    assert len(set(idx.tolist())) > 1
    for hd, hr in zip(out["h_sir"], P.sir_latents(idx, ref["cache"])):
        _within(_np(hd), hr, LATENT_TOL, "b. posterior h_sir")
    n = ref["chunks"]
    assert (adv[17], adv[18]) == ((n, 0) if path == "auto" else (0, n)), adv
    assert adv[0] == (n if path == "auto" else 0), adv


@pytest.mark.parametrize("path", ["auto", "layerwise"])
@pytest.mark.parametrize("chunk", [0, 2])
@pytest.mark.parametrize("model", N.POSTERIOR_MODELS)
def test_impute_draws_the_reference_noise_and_pixel_uniforms(model, chunk, path):
    """iwae_impute: the masked first pass, x_mean, the SIR latents and x_draw
    from the reference u_pix stream (layer id 2 MAX_LAYERS + 2), by
    tests/test_gpu_impute.py's checks."""
    from test_gpu_impute import _check
    NN, k = N.NLL_N, N.POSTERIOR_K
    m, x = _model(model, NN, kernel_path=path)
    mask = N.pixel_mask(NN, N.X_DIM)
    c0 = _counts(m)
    out = m.impute(x, mask, k, chunk=chunk)
    adv = _advance(m, c0)
    ref = N.posterior_reference(model, NN, k, chunk or NN, mask=mask)
    _check_weights(out, ref, k, model)
    u_pix = N.impute_uniforms(KEY, 0, NN, N.X_DIM, chunk or NN)
    ratios = _check(out, x, mask, ref["u"], u_pix, ref, k, f"{model} chunk={chunk} {path}")
    for name, r in ratios.items():
        _note(f"b. impute {name} (error / bar)", r)
    idx = P.sir_index(_np(out["weights"]).astype(np.float64), ref["u"].astype(np.float64))
    np.testing.assert_array_equal(idx, ref["sir_index"])
    n = ref["chunks"]
    assert (adv[19], adv[20]) == ((n, 0) if path == "auto" else (0, n)), adv


@pytest.mark.parametrize("model", N.STAT_MODELS)
def test_encode_latents_are_what_layerwise_log_weights_weigh(model):
    """iwae_encode's latents against the oracle's on the reference noise; a
    layer-wise get_log_weights of the same seed, N and k equals both the oracle
    on that noise and iwae_score of the encoded latents."""
    B, k = N.SHAPES[0]
    m, x = _model(model, B, k=k, kernel_path="layerwise")
    hs, lq, _ = m.encoder(x, k)
    ref = N.forward_reference(model, B, k, 0)
    for hd, hr in zip(hs, ref["h"]):
        _within(_np(hd), hr, LATENT_TOL, "b. encode latents")
    scale = np.abs(ref["lw"]).max()
    assert np.abs(_np(lq) - ref["logq"]).max() <= REL * scale
    m.set_seed(N.SEED)
    lw = _np(m.get_log_weights(x, k)).astype(np.float64)
    sc = _np(m.score(x, hs)["log_w"]).astype(np.float64)
    _note("b. log-weights / max|lw|", np.abs(lw - ref["lw"]).max() / scale)
    assert np.abs(lw - ref["lw"]).max() <= REL * scale
    assert np.abs(sc - lw).max() <= REL * scale, np.abs(sc - lw).max()


# ===================================================== c. position and key bookkeeping
def _lw_err(m, x, k, key_, pos, model, B):
    lw = _np(m.get_log_weights(x, k)).astype(np.float64)
    ref = N.forward_reference(model, B, k, pos, key_=key_)["lw"]
    return np.abs(lw - ref).max() / np.abs(ref).max()


def test_a_sequence_of_calls_leaves_the_predicted_position():
    model, (B, k) = "S2", N.SHAPES[0]
    m, x = _model(model, B, "IWAE", k)
    m.set_seed(N.SEED)
    grey = np.random.default_rng(1604).random((7, N.X_DIM)).astype(np.float32)
    pos = 0
    m.train_step(x)
    pos += N.advance("train_step")
    m.log_px(x, k, chunk=2)
    pos += N.advance("nll", N=B, k=k, chunk=2)
    m.sample(4)
    pos += N.advance("generate", n=4)
    assert m.binarize(grey[:0]).shape[0] == 0
    pos += N.advance("binarize", n=0)
    m.binarize(grey)
    pos += N.advance("binarize", n=7)
    m.reconstructed_x_probs(x)
    pos += N.advance("reconstruct")
    hs = [np.zeros((2, B, d), np.float32) for d in m.n_latent_encoder]
    m.score(x, hs)
    pos += N.advance("score")
    assert pos == 1 + 2 + 1 + 0 + 1 + 1 + 0
    # the train step moved the weights: the oracle runs on the device's
    _, spec, _, _, x64 = N.case(model, B)
    params = O.unflatten_params(spec, _flat(m.get_weights()))
    lw = _np(m.get_log_weights(x, k)).astype(np.float64)
    errs = {}
    for p in range(pos - 2, pos + 3):
        ref = O.forward(params, spec, x64, N.eps_forward(KEY, p, B, k, spec.n_latent_encoder))["lw"]
        errs[p] = np.abs(lw - ref).max() / np.abs(ref).max()
    print(f"log-weights against the oracle at positions around {pos}: " + ", ".join(f"{p}: {e:.1e}" for p, e in errs.items()))
    assert errs[pos] <= REL, errs
    assert all(e > 100 * REL for p, e in errs.items() if p != pos), errs
    m.check_kernel_status()


def test_noise_streams_keep_their_keys_and_positions():
    model, (B, k) = "S2", N.SHAPES[0]
    m, x = _model(model, B, k=k, kernel_path="layerwise")
    k0, k3 = N.key(N.SEED, 0), N.key(N.SEED, 3)
    assert _lw_err(m, x, k, k0, 0, model, B) <= REL
    assert _lw_err(m, x, k, k0, 1, model, B) <= REL
    m.set_noise_stream(3)
    assert _lw_err(m, x, k, k3, 0, model, B) <= REL
    m.set_noise_stream(0)
    assert _lw_err(m, x, k, k0, 2, model, B) <= REL          # stream 0 goes on where it stopped
    m.set_noise_stream(3)
    assert _lw_err(m, x, k, k3, 1, model, B) <= REL
    m.set_seed(N.SEED)                                       # restarts both; the current stream stays 3
    assert _lw_err(m, x, k, k3, 0, model, B) <= REL
    m.set_noise_stream(0)
    assert _lw_err(m, x, k, k0, 0, model, B) <= REL
    # another seed: another key for both streams
    m.set_seed(N.SEED + 1)
    assert _lw_err(m, x, k, N.key(N.SEED + 1), 0, model, B) <= REL
    assert _lw_err(m, x, k, k0, 1, model, B) > 100 * REL


def test_a_data_parallel_rank_draws_under_its_stream_key():
    """iwae_dp_init(rank 1 of 2) without a communicator: noise stream 1."""
    model, (B, k) = "S2", N.SHAPES[0]
    m, x = _model(model, B, k=k)
    m._call(m._lib.iwae_dp_init(m._h, 1, 2, None))
    assert _lw_err(m, x, k, N.key(N.SEED, 1), 0, model, B) <= REL
    assert _lw_err(m, x, k, N.key(N.SEED, 1), 1, model, B) <= REL
    m._call(m._lib.iwae_dp_init(m._h, 0, 1, None))
    assert _lw_err(m, x, k, N.key(N.SEED, 0), 0, model, B) <= REL


def test_zz_print_the_worst_measured_values():
    """Runs last in the module: the worst value per bar over the tests above."""
    for name in sorted(WORST):
        print(f"{name}: {WORST[name]:.3e}")
