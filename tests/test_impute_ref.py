"""The float64 reference of missing-pixel imputation (tests/impute_ref.py)
against what its definitions imply (no GPU needed)."""
import numpy as np

import impute_ref as I
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


def test_an_all_ones_mask_is_the_posterior():
    O, spec, params, x, eps, rng = _model(9, 4, 0)
    u = rng.random(4)
    a = I.impute(params, spec, x, np.ones_like(x), eps, u=u, u_pix=rng.random(x.shape))
    b = R.posterior(params, spec, x, eps, u=u)
    for name in ("lw", "weights", "log_px", "ess", "probs", "sir_index"):
        np.testing.assert_array_equal(a[name], b[name])
    for p, q in zip(a["h_mean"] + a["h_sir"], b["h_mean"] + b["h_sir"]):
        np.testing.assert_array_equal(p, q)
    np.testing.assert_array_equal(a["x_mean"], x)
    np.testing.assert_array_equal(a["x_draw"], x)


def test_values_of_x_at_missing_pixels_do_not_matter():
    O, spec, params, x, eps, rng = _model(7, 5, 1)
    mask = (rng.random(x.shape) < 0.5).astype(np.float64)
    u, up = rng.random(5), rng.random(x.shape)
    a = I.impute(params, spec, x, mask, eps, u=u, u_pix=up)
    for junk in (np.nan, np.inf, 1.0 - x, 7.5):
        xj = np.where(mask != 0, x, junk)
        b = I.impute(params, spec, xj, mask, eps, u=u, u_pix=up)
        for name in ("lw", "weights", "log_px", "ess", "x_mean", "x_draw"):
            np.testing.assert_array_equal(a[name], b[name])
        for p, q in zip(a["h_mean"] + a["h_sir"], b["h_mean"] + b["h_sir"]):
            np.testing.assert_array_equal(p, q)
    # and the mask matters: the unmasked log weights are far away
    full = R.posterior(params, spec, x, eps)
    assert np.abs(full["log_px"] - a["log_px"]).min() > 1.0


def test_a_fully_missing_image_has_prior_over_proposal_weights():
    O, spec, params, x, eps, rng = _model(6, 3, 2)
    mask = np.ones_like(x)
    mask[1] = 0.0
    a = I.impute(params, spec, x, mask, eps)
    z = O.forward(params, spec, np.zeros_like(x), eps)
    np.testing.assert_array_equal(a["lw"][:, 1], (z["logp"] - z["logq"])[:, 1])
    np.testing.assert_array_equal(a["cache"]["logpx"][:, 1], np.zeros(6))
    # its x_mean is the weighted probabilities everywhere
    np.testing.assert_array_equal(a["x_mean"][1], a["probs"][1])


def test_observed_pixels_are_returned_as_they_are():
    O, spec, params, x, eps, rng = _model(8, 6, 3)
    x = rng.random(x.shape)                              # fractional pixels
    mask = (rng.random(x.shape) < 0.4).astype(np.float64) * 3.0     # any non-zero value = observed
    u, up = rng.random(6), rng.random(x.shape)
    a = I.impute(params, spec, x, mask, eps, u=u, u_pix=up)
    obs = mask != 0
    np.testing.assert_array_equal(a["x_mean"][obs], x[obs])
    np.testing.assert_array_equal(a["x_draw"][obs], x[obs])
    np.testing.assert_array_equal(a["x_mean"][~obs], a["probs"][~obs])
    p_sel = I.p_sir(a["sir_index"], a["cache"])
    np.testing.assert_array_equal(a["x_draw"][~obs], (up < p_sel)[~obs].astype(np.float64))
    assert set(np.unique(a["x_draw"][~obs])) <= {0.0, 1.0}
    for b in range(6):
        np.testing.assert_array_equal(p_sel[b], a["cache"]["p"][a["sir_index"][b], b])
