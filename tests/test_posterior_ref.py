"""The float64 reference of the importance-weighted posterior
(tests/posterior_ref.py) against what its definitions imply (no GPU needed)."""
import numpy as np
import pytest

import posterior_ref as R


def _model(k, B, seed, scale=0.5):
    from oracle import iwae_oracle as O
    rng = np.random.default_rng(seed)
    spec = O.ModelSpec([24, 16], [16, 24], [10, 6], [10, 40], x_dim=40)
    params = O.glorot_init(spec, rng, out_bias=O.output_bias_from_mean(rng.uniform(0.1, 0.4, 40)))
    params = {n: [w * scale, b] for n, (w, b) in params.items()}
    x = (rng.random((B, 40)) < 0.3).astype(np.float64)
    eps = O.draw_eps(spec, k, B, rng)
    return O, spec, params, x, eps, rng


def test_one_sample_is_the_sample_itself():
    O, spec, params, x, eps, rng = _model(1, 4, 0)
    r = R.posterior(params, spec, x, eps, u=rng.random(4))
    c = r["cache"]
    np.testing.assert_array_equal(r["weights"], np.ones((4, 1)))
    np.testing.assert_array_equal(r["ess"], np.ones(4))
    for hm, hs, h in zip(r["h_mean"], r["h_sir"], c["h"]):
        np.testing.assert_array_equal(hm, h[0])
        np.testing.assert_array_equal(hs, h[0])
    np.testing.assert_array_equal(r["probs"], c["p"][0])
    np.testing.assert_allclose(r["log_px"], c["lw"][0], rtol=0, atol=1e-12)


def test_equal_log_weights_give_the_plain_mean():
    O, spec, params, x, eps, rng = _model(7, 3, 1)
    c = O.forward(params, spec, x, eps)
    w, logpx, ess = R.weights(np.full((7, 3), -123.25))
    np.testing.assert_allclose(w, 1.0 / 7, rtol=1e-15)
    np.testing.assert_allclose(ess, 7.0, rtol=1e-14)
    np.testing.assert_allclose(logpx, -123.25, rtol=1e-14)
    h_mean, probs = R.combine(w, c)
    for hm, h in zip(h_mean, c["h"]):
        np.testing.assert_allclose(hm, h.mean(0), rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(probs, c["p"].mean(0), rtol=1e-13)


def test_permuting_the_samples_leaves_the_means_unchanged():
    O, spec, params, x, eps, rng = _model(13, 3, 2)
    perm = rng.permutation(13)
    a = R.posterior(params, spec, x, eps)
    b = R.posterior(params, spec, x, [e[perm] for e in eps])
    np.testing.assert_allclose(b["weights"], a["weights"][:, perm], rtol=1e-12)
    for p, q in zip(a["h_mean"], b["h_mean"]):
        np.testing.assert_allclose(p, q, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(a["probs"], b["probs"], rtol=1e-12)
    np.testing.assert_allclose(a["ess"], b["ess"], rtol=1e-12)
    np.testing.assert_allclose(a["log_px"], b["log_px"], rtol=1e-13)


@pytest.mark.parametrize("k", [1, 5, 64])
def test_sir_index_is_the_inverse_cdf_and_ess_is_in_range(k):
    O, spec, params, x, eps, rng = _model(k, 6, 3 + k)
    u = rng.random(6)
    u[0], u[1] = 0.0, np.nextafter(1.0, 0.0)          # the ends of [0, 1)
    r = R.posterior(params, spec, x, eps, u=u)
    w = r["weights"]
    np.testing.assert_allclose(w.sum(1), 1.0, rtol=1e-14)
    want = [min(int(np.searchsorted(np.cumsum(w[b]), u[b], side="right")), k - 1) for b in range(6)]
    np.testing.assert_array_equal(r["sir_index"], want)
    assert r["sir_index"][0] == int(np.argmax(w[0] > 0)) and (r["sir_index"] <= k - 1).all()
    for hs, h in zip(r["h_sir"], r["cache"]["h"]):
        for b in range(6):
            np.testing.assert_array_equal(hs[b], h[want[b], b])
    assert (r["ess"] >= 1 - 1e-12).all() and (r["ess"] <= k + 1e-9).all()
    np.testing.assert_allclose(r["ess"], 1.0 / (w * w).sum(1), rtol=1e-12)
    np.testing.assert_allclose(r["log_px"], O.L_k_per_image(r["lw"]), rtol=1e-13)


def test_combine_takes_any_weights():
    O, spec, params, x, eps, rng = _model(9, 2, 11)
    c = O.forward(params, spec, x, eps)
    w = np.zeros((2, 9))
    w[0, 4] = w[1, 8] = 1.0                            # one-hot: the sample itself
    h_mean, probs = R.combine(w, c)
    for hm, h in zip(h_mean, c["h"]):
        np.testing.assert_array_equal(hm[0], h[4, 0])
        np.testing.assert_array_equal(hm[1], h[8, 1])
    np.testing.assert_array_equal(probs[1], c["p"][8, 1])
    ha, pa = R.combine_abs(w, c)
    np.testing.assert_array_equal(ha[0][0], np.abs(c["h"][0][4, 0]))
    np.testing.assert_array_equal(pa[0], c["p"][4, 0])
