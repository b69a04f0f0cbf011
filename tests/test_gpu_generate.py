"""Generation from the prior (iwae_generate, Flexible_Model.generate_x /
sample): the fused gen_kernel and the layer-wise path against a float64
restatement of Decoder.generate_x (F:107-F:119)."""
import ctypes
import functools

import numpy as np
import pytest

from test_gpu_parity import make_model, weights_from_flat
from test_gpu_statistics import ARCHS as STAT_ARCHS

pytestmark = pytest.mark.gpu

# the 1-, 2- and 3-layer models of test_gpu_statistics, one whose latent width
# is no multiple of 4, one with x_dim = 64; then two wider ones the fused plan
# runs on 32-row and on 16-row workgroups (the five above fit 64 rows), the
# last with K > 256 (several weight fetches per column tile)
ARCHS = list(STAT_ARCHS) + [([40, 24], [24, 40], [20, 10], [20, 784]), ([16], [16], [4], [64]),
                            ([200, 100], [100, 200], [100, 50], [100, 784]), ([600], [600], [50], [784])]
ROWS = (1, 9, 70)          # 70 straddles a 16-row tile and every workgroup size (16, 32, 64 rows)
PATHS = ("auto", "layerwise")
PROBS_TOL = dict(rtol=2e-4, atol=2e-6)      # test_reconstruction_matches_oracle's, the same quantity
LATENT_TOL = dict(rtol=1e-4, atol=2e-5)     # test_unit_activity_matches_oracle's (latent means)


@functools.lru_cache(maxsize=None)
def _setup(ai, path):
    """Model ai on kernel path `path` with float32-rounded weights, and the same
    weights as float64 for the reference (as test_gpu_statistics._setup)."""
    from oracle import iwae_oracle as O
    he, hd, le, ld = ARCHS[ai]
    x_dim = ld[-1]
    rng = np.random.default_rng(100 + ai)
    spec = O.ModelSpec(he, hd, le, ld, x_dim=x_dim)
    params = O.glorot_init(spec, rng, out_bias=O.output_bias_from_mean(rng.uniform(0.02, 0.4, x_dim)))
    params = {n: [w.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64)]
              for n, (w, b) in params.items()}
    m = make_model(he, hd, le, ld, x_dim=x_dim, kernel_path=path)
    m.set_weights(weights_from_flat(m, O.flatten_params(spec, params)))
    return O, spec, params, m


def _ref(O, spec, params, h_top, e_pri):
    """Decoder.generate_x (F:107-F:119) in float64: (probs [n, x_dim], latents
    in encoder order h_1..h_L); e_pri[j] is [1, n, d_{L-2-j}]."""
    hs = [np.asarray(h_top, np.float64)]
    for j in range(spec.L - 1):
        dj = O._stoch_forward(params, f"dec{j}", hs[-1])                       # F:113
        hs.append(np.asarray(e_pri[j][0], np.float64) * dj["scale"] + dj["mu"])   # F:114 sample()
    (W1, b1), (W2, b2), (W3, b3) = params["out.l1"], params["out.l2"], params["out.l3"]
    logit = np.tanh(np.tanh(hs[-1] @ W1 + b1) @ W2 + b2) @ W3 + b3
    p = (1.0 / (1.0 + np.exp(-logit))) * O.PROB_SCALE + O.PROB_SHIFT           # F:101-F:102
    return p, hs[::-1]


def _noise(spec, n, seed):
    rng = np.random.default_rng(seed)
    le, L = spec.n_latent_encoder, spec.L
    e_top = rng.standard_normal((1, n, le[L - 1])).astype(np.float32)
    e_pri = [rng.standard_normal((1, n, le[L - 2 - j])).astype(np.float32) for j in range(L - 1)]
    return rng, e_top, e_pri


def _count(m):
    return int(m._lib.iwae_debug_count(m._h, 10))


# ------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("ai", range(len(ARCHS)))
def test_generation_matches_float64_with_injected_noise(ai, n, path):
    """Both entry forms (h_top given; h_L drawn from eps) against float64; the
    launch counter pins which path ran."""
    O, spec, params, m = _setup(ai, path)
    rng, e_top, e_pri = _noise(spec, n, 1000 * ai + n)
    rp, rh = _ref(O, spec, params, e_top[0], e_pri)
    c0 = _count(m)
    probs = m.generate_x(e_top[0], eps=e_pri).cpu().numpy()
    out = m.sample(n, eps=[e_top] + e_pri, u=rng.random((n, spec.x_dim)).astype(np.float32), return_latents=True)
    c1 = _count(m)
    assert c1 - c0 == (2 if path == "auto" else 0), (c0, c1)
    assert probs.shape == (n, spec.x_dim)
    err = np.abs(probs - rp)
    print(f"probs: max abs err {err.max():.3e}, max rel err {(err / rp).max():.3e}")
    np.testing.assert_allclose(probs, rp, **PROBS_TOL)
    np.testing.assert_allclose(out["probs"].cpu().numpy(), rp, **PROBS_TOL)
    assert len(out["h"]) == spec.L
    for i, (hd, hr) in enumerate(zip(out["h"], rh)):
        assert tuple(hd.shape) == (n, spec.n_latent_encoder[i])
        np.testing.assert_allclose(hd.cpu().numpy(), hr, **LATENT_TOL)
    np.testing.assert_array_equal(out["h"][-1].cpu().numpy(), e_top[0])         # h_L = eps * 1 + 0
    # the reference's call forms: [S, B, d_L] through model.decoder
    if n == 9:
        p3 = m.decoder.generate_x(e_top[0].reshape(3, 3, -1), eps=e_pri).cpu().numpy()
        assert p3.shape == (3, 3, spec.x_dim)
        np.testing.assert_array_equal(p3.reshape(9, -1), probs)


# ------------------------------------------------------------- 2. pixel draws
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("ai", [1, 4, 6])
def test_pixel_draws_follow_the_injected_uniforms(ai, path):
    """u within 1e-3 of the float64 probability is moved to exactly 1e-3 away on
    its own side; the device probability is within 2.02e-4 of it (PROBS_TOL), so
    no pixel is a near tie and every pixel equals (u < p_ref)."""
    O, spec, params, m = _setup(ai, path)
    n = 70
    rng, e_top, e_pri = _noise(spec, n, 77 + ai)
    rp, _ = _ref(O, spec, params, e_top[0], e_pri)
    u = rng.random((n, spec.x_dim))
    near = np.abs(u - rp) < 1e-3
    u = np.where(near, np.where(u < rp, rp - 1e-3, rp + 1e-3), u).astype(np.float32)
    x = m.sample(n, eps=[e_top] + e_pri, u=u, return_probs=False)["x"].cpu().numpy()
    assert x.shape == (n, spec.x_dim)
    assert np.isin(x, (0.0, 1.0)).all()
    np.testing.assert_array_equal(x, (u.astype(np.float64) < rp).astype(np.float32))


# -------------------------------------------------------------- 3. cross-path
@pytest.mark.parametrize("ai", [1, 2])
def test_generate_x_of_the_encoders_top_latent_equals_reconstruction(ai):
    """generate_x(h_L of one q(h|x) draw) is what reconstructed_x_probs computes
    on its own path; both sides carry device rounding: twice the parity tolerance."""
    O, spec, params, m = _setup(ai, "auto")
    B = 9
    rng, _, e_pri = _noise(spec, B, 31 + ai)
    e_enc = [rng.standard_normal((1, B, d)).astype(np.float32) for d in spec.n_latent_encoder]
    x = (rng.random((B, spec.x_dim)) < 0.3).astype(np.float32)
    h_top = m.encoder_means(x, 1, eps=e_enc)[-1]          # the mean of one draw is the draw
    c0 = _count(m)
    gen = m.generate_x(h_top, eps=e_pri).cpu().numpy()
    assert _count(m) == c0 + 1
    rec = m.reconstructed_x_probs(x, eps=e_enc + e_pri).cpu().numpy()[0]
    np.testing.assert_allclose(gen, rec, rtol=4e-4, atol=4e-6)


# ------------------------------------------------------------ 4. device noise
@pytest.mark.parametrize("ai", [0, 2])
def test_device_noise_is_reproducible_fresh_and_the_same_on_both_paths(ai):
    O, spec, params, m = _setup(ai, "auto")
    _, _, _, lw = _setup(ai, "layerwise")
    n = 70

    def draw(model):
        o = model.sample(n, return_latents=True)
        return [o["x"].cpu().numpy(), o["probs"].cpu().numpy()] + [h.cpu().numpy() for h in o["h"]]

    m.set_noise_stream(0)
    m.set_seed(2024)
    c0 = _count(m)
    a, b = draw(m), draw(m)
    assert _count(m) == c0 + 2
    m.set_seed(2024)
    c = draw(m)
    for p, q in zip(a, c):
        np.testing.assert_array_equal(p, q)                # same seed: bitwise equal
    assert np.abs(a[1] - b[1]).max() > 1e-4                # a second call draws fresh noise
    assert np.abs(a[-1] - b[-1]).max() > 1e-2
    m.set_seed(2024)
    m.set_noise_stream(3)
    d = draw(m)
    m.set_noise_stream(0)
    assert np.abs(a[-1] - d[-1]).max() > 1e-2              # another noise stream
    for v in a + b + d:
        assert np.isfinite(v).all()
    assert np.isin(a[0], (0.0, 1.0)).all()
    lw.set_noise_stream(0)
    lw.set_seed(2024)
    c0 = _count(lw)
    e = draw(lw)
    assert _count(lw) == c0
    np.testing.assert_allclose(e[1], a[1], **PROBS_TOL)    # the identical Philox stream
    for p, q in zip(e[2:], a[2:]):
        np.testing.assert_allclose(p, q, **LATENT_TOL)


# ------------------------------------------------------------ 5. distribution
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("ai", [0, 1])
def test_samples_have_the_priors_moments(ai, path):
    """n = 4096, 5 standard errors: mean of h_L within 5 / sqrt(n) = 0.08,
    its variance within 5 sqrt(2 / n) = 0.11 of 1, and per pixel the mean of x
    within 5 sqrt(0.25 / n) = 0.04 of the mean of probs."""
    O, spec, params, m = _setup(ai, path)
    n = 4096
    m.set_noise_stream(0)
    m.set_seed(99)
    o = m.sample(n, return_latents=True)
    hL = o["h"][-1].double().cpu().numpy()
    assert np.abs(hL.mean(0)).max() <= 0.08
    assert np.abs(hL.var(0) - 1.0).max() <= 0.11
    x, p = o["x"].double().cpu().numpy(), o["probs"].double().cpu().numpy()
    assert np.isin(x, (0.0, 1.0)).all()
    assert np.abs(x.mean(0) - p.mean(0)).max() <= 0.04


# ------------------------------------------------- 6. leaves the model alone
def test_sampling_between_train_steps_changes_nothing():
    from iwae_replication_project_amd import Adam
    he, hd, le, ld = ARCHS[1]
    m = make_model(he, hd, le, ld)
    m.compile(optimizer=Adam(learning_rate=1e-3, epsilon=1e-4))
    rng = np.random.default_rng(3)
    x = (rng.random((6, 784)) < 0.3).astype(np.float32)
    m.train_step(x)
    m.train_step(x)
    w0, (m0, v0, t0), g0 = m.get_weights(), m.get_optimizer_state(), m.graph_captures()
    c0 = _count(m)
    out = m.sample(16)
    assert _count(m) == c0 + 1 and np.isfinite(out["probs"].cpu().numpy()).all()
    w1, (m1, v1, t1) = m.get_weights(), m.get_optimizer_state()
    for a, b in zip(w0, w1):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(m0, m1)
    np.testing.assert_array_equal(v0, v1)
    assert t0 == t1 and m.graph_captures() == g0
    m.train_step(x)
    assert m.graph_captures() == g0                        # the captured step is replayed, not re-captured
    m.check_kernel_status()


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("ai", [1, 4])
def test_padding_columns_and_rows_past_n_keep_their_sentinel(ai, path):
    import torch
    from iwae_replication_project_amd import _lib
    O, spec, params, m = _setup(ai, path)
    n, rows, xd = 21, 24, spec.x_dim
    ld = xd + 8
    with torch.cuda.stream(m._stream):
        probs = torch.full((rows, ld), -7.0, device=m.device)
        pixels = torch.full((rows, ld), -7.0, device=m.device)
        hs = [torch.full((rows, d), -7.0, device=m.device) for d in spec.n_latent_encoder]
    harr, nh = _lib.fptr_array(hs)
    m._call(m._lib.iwae_generate(m._h, n, None, None, 0, None, _lib.fptr(probs), ld, _lib.fptr(pixels), ld, harr, nh))
    m._stream.synchronize()
    probs, pixels = probs.cpu().numpy(), pixels.cpu().numpy()
    for t in (probs, pixels):
        assert (t[:n, xd:] == -7.0).all() and (t[n:] == -7.0).all()
    assert ((probs[:n, :xd] > 0) & (probs[:n, :xd] < 1)).all()
    assert np.isin(pixels[:n, :xd], (0.0, 1.0)).all()
    for h in hs:
        h = h.cpu().numpy()
        assert (h[n:] == -7.0).all() and (h[:n] != -7.0).all()


# ---------------------------------------------------------------- 7. arguments
def test_zero_rows_return_empty_tensors():
    O, spec, params, m = _setup(1, "auto")
    c0 = _count(m)
    o = m.sample(0, return_latents=True)
    assert tuple(o["x"].shape) == (0, 784) and tuple(o["probs"].shape) == (0, 784)
    assert [tuple(h.shape) for h in o["h"]] == [(0, d) for d in spec.n_latent_encoder]
    assert tuple(m.generate_x(np.zeros((0, spec.n_latent_encoder[-1]), np.float32)).shape) == (0, 784)
    assert m._lib.iwae_generate(m._h, 0, None, None, 0, None, None, 784, None, 784, None, 0) == -1   # both NULL
    assert _count(m) == c0


def test_bad_arguments_raise_before_any_launch():
    import torch
    from iwae_replication_project_amd import _lib
    O, spec, params, m = _setup(1, "auto")
    n = 5
    _, e_top, e_pri = _noise(spec, n, 8)
    c0 = _count(m)
    with pytest.raises(ValueError):
        m.sample(n, eps=e_pri)                              # h_L's draw is missing
    with pytest.raises(ValueError):
        m.generate_x(e_top[0], eps=[e_top] + e_pri)         # one array too many
    with pytest.raises(ValueError):
        m.generate_x(np.zeros((n, spec.n_latent_encoder[-1] + 1), np.float32))
    with pytest.raises(ValueError):
        m.sample(n, u=np.zeros((n, 783), np.float32))
    with torch.cuda.stream(m._stream):
        buf = torch.zeros(n, 788, device=m.device)
        eps = [torch.zeros(1, n, d, device=m.device) for d in (16, 32)]
    gen = m._lib.iwae_generate
    p = _lib.fptr(buf)
    arr3 = (_lib.FP * 3)(*[_lib.fptr(t) for t in eps + eps[:1]])
    arr2 = (_lib.FP * 2)(_lib.fptr(eps[0]), None)
    for rc in (gen(m._h, n, None, None, 0, None, None, 0, None, 0, None, 0),          # both outputs NULL
               gen(m._h, n, None, None, 0, None, p, 786, None, 0, None, 0),           # ld no multiple of 4
               gen(m._h, n, None, None, 0, None, None, 0, p, 780, None, 0),           # ld below x_dim
               gen(m._h, n, None, arr3, 3, None, p, 788, None, 0, None, 0),           # wrong eps count
               gen(m._h, n, None, arr2, 2, None, p, 788, None, 0, None, 0),           # NULL inside eps
               gen(m._h, n, None, None, 0, None, p, 788, None, 0, arr2, 1),           # wrong h_out count
               gen(m._h, n, None, None, 0, None, p, 788, None, 0, arr2, 2),           # NULL inside h_out
               gen(m._h, -1, None, None, 0, None, p, 788, None, 0, None, 0)):
        assert rc == -1
        with pytest.raises(ValueError):
            _lib.check(m._lib, m._h, rc)
    m._stream.synchronize()
    assert _count(m) == c0
    assert (buf == 0).all()
