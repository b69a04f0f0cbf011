"""The float64 reference of the pixel-masked scoring family
(tests/observed_ref.py) checked on the CPU (no GPU needed):

1. with an all-ones mask every masked reference is its unmasked original, exactly;
2. on the encoder's own samples the masked log weights are impute_ref's and
   missing_ref.forward's;
3. float32 and the float32 + emulated-bf16x3 run stay within a quarter of each
   bar tests/test_gpu_observed.py applies (1e-4 of max|ref| and of S_r for the
   values, 1e-4 relative L2 per layer for the gradients, 1e-4 of max|ref| for
   the AIS weights and latents and refine's parameters, bound and weights;
   equal decisions);
4. the searched AIS and HMC cases meet, under the float64 reference alone, the
   conditions they were searched under (ais_ref's: |dH| < 5, each decision 0.4
   nats clear of its margin in log u, some chains accept and some reject), and
   a fresh search returns the committed constants.  Refinement takes no
   decision: its cases run in refine_ref's fixed setting (T, LR, ranges, SEED)."""
import numpy as np
import pytest

import ais_ref as A
import impute_ref as I
import missing_ref as M
import observed_ref as OB
import refine_ref as RF
import score_ref as R
import scoregrad_ref as G

BAR = 1e-4
QUARTER = BAR / 4
CASES = list(OB.CASES)
VALUES = (("logq", "Sq"), ("logp", "Sp"), ("logpx", "Spx"))


def test_cases_are_the_stated_ones():
    assert CASES == ["OS1", "OS2", "OS3", "OK130", "OC784", "O50", "OG"]
    for name in CASES:
        spec, _, x, mask, _, x_full = OB.case(name)
        assert not mask[0].any() and mask[1].all() and 0.3 < mask[2:].mean() < 0.7
        assert np.isnan(x[mask == 0]).all() and np.isfinite(x[mask != 0]).all() and np.isfinite(x_full).all()
    assert OB.case("O50")[0].x_dim == 50 and OB.case("O50")[0].x_dim % 4
    xg, mg = OB.case("OG")[5], OB.case("OG")[3]
    grey = (xg > 0) & (xg < 1)
    assert grey[1::2].all() and not grey[0::2].any() and (grey & (mg != 0)).any()
    assert OB.case("OC784")[0].x_dim == 784 and OB.CASES["OK130"][2:4] == (3, 130)


# ------------------------------------------------- 1. all-ones mask: the originals
@pytest.mark.parametrize("kw", [{}, {"dtype": np.float32}, {"dtype": np.float32, "dense": R.dense_bf16x3}],
                         ids=["f64", "f32", "bf16x3"])
@pytest.mark.parametrize("name", ["OS2", "OS3", "OG"])
def test_all_ones_mask_gives_score_and_grads_exactly(name, kw):
    spec, params, _, mask, _, x_full = OB.case(name)
    ones = np.ones_like(mask)
    h = OB.latents(name, "off")
    a, b = OB.score(params, spec, x_full, ones, h, **kw), R.score(params, spec, x_full, h, **kw)
    assert set(a) == set(b)
    for n in b:
        np.testing.assert_array_equal(a[n], b[n], err_msg=n)
    ga, gb = OB.grads(params, spec, x_full, ones, h, **kw), G.grads(params, spec, x_full, h, **kw)
    for t in G.TERMS:
        for u, v in zip(ga[t], gb[t]):
            np.testing.assert_array_equal(u, v, err_msg=t)


def test_all_ones_mask_gives_hmc_ais_and_refine_exactly():
    name = "OS2"
    spec, params, _, mask, _, x_full = OB.case(name)
    ones = np.ones_like(mask)
    h = OB.latents(name, "on")
    r = OB.momenta_of(name, 11, 1)[0]
    for u, v in zip(OB.hmc_step(params, spec, x_full, ones, h, r, 0.2, 3), G.hmc_step(params, spec, x_full, h, r, 0.2, 3)):
        for a, b in zip(u if isinstance(u, list) else [u], v if isinstance(v, list) else [v]):
            np.testing.assert_array_equal(a, b)
    mom = OB.momenta_of(name, 12, len(A.BETAS) - 1)
    for init in A.INITS:
        a = OB.ais_run(params, spec, x_full, ones, h, A.BETAS, init, 0.2, A.N_LEAPFROG, A.ADAPT, mom, A.log_u_rule)
        b = A.run(params, spec, x_full, h, A.BETAS, init, 0.2, A.N_LEAPFROG, A.ADAPT, mom, A.log_u_rule)
        assert set(a) == set(b)
        for n in b:
            for u, v in zip(a[n] if isinstance(a[n], list) else [a[n]], b[n] if isinstance(b[n], list) else [b[n]]):
                np.testing.assert_array_equal(u, v, err_msg=n)
    m0, s0, eps = OB.refine_setting(name)
    for objective in RF.OBJECTIVES:
        a = OB.refine_run(params, spec, x_full, ones, m0, s0, eps, objective, 2)
        b = RF.run(params, spec, x_full, m0, s0, eps, objective, 2)
        for n in ("mean", "logstd", "adam", "h"):
            for u, v in zip(a[n], b[n]):
                np.testing.assert_array_equal(u, v, err_msg=n)
        for n in ("bound", "log_w", "logpx", "ess"):
            np.testing.assert_array_equal(a[n], b[n], err_msg=n)


# --------------------------------- 2. the log weights of the features already built
@pytest.mark.parametrize("name", CASES)
def test_masked_log_weights_are_imputes_and_the_masked_bounds(name):
    spec, params, x, mask, eps, _ = OB.case(name)
    h = OB.latents(name, "on", rounded=False)
    sc = OB.score(params, spec, x, mask, h)
    lw = (sc["logp"] + sc["logpx"]) - sc["logq"]
    for other in (I.forward(params, spec, x, mask, eps), M.forward(params, spec, np.asarray(x), mask, eps)):
        np.testing.assert_allclose(lw, other["lw"], rtol=1e-12, atol=1e-10)
        np.testing.assert_allclose(sc["logpx"], other["logpx"], rtol=1e-12, atol=1e-10)
    assert (sc["logpx"][:, 0] == 0.0).all() and (sc["Spx"][:, 0] == 0.0).all()     # the all-missing image
    g = OB.grads(params, spec, x, mask, h)
    assert not g["px"][0][:, 0].any() and g["px"][0][:, 1].any()
    assert all(np.isfinite(v).all() for t in g.values() for v in t)


def test_gradient_reference_is_the_derivative_of_the_masked_densities():
    name = "OS2"
    spec, params, x, mask, _, _ = OB.case(name)
    h = OB.latents(name, "off")
    rng = np.random.default_rng(17)
    v = [rng.standard_normal(a.shape) for a in h]
    e = 3e-5
    up = OB.score(params, spec, x, mask, [a + e * b for a, b in zip(h, v)])
    dn = OB.score(params, spec, x, mask, [a - e * b for a, b in zip(h, v)])
    g = OB.grad_reference(name, "off")
    for t, key in zip(G.TERMS, ("logq", "logp", "logpx")):
        fd = (up[key] - dn[key]) / (2 * e)
        an = sum((a * b).sum(-1) for a, b in zip(g[t], v))
        assert np.abs(fd - an).max() <= 1e-7 * np.abs(an).max(), t


# ------------------------------------------------------------ 3. the emulation
@pytest.mark.parametrize("which", OB.LATENTS)
@pytest.mark.parametrize("name", CASES)
def test_score_emulation_stays_within_a_quarter_of_both_bars(name, which):
    spec, params, x, mask, _, _ = OB.case(name)
    h, ref = OB.latents(name, which), OB.reference(name, which)
    for label, kw in (("float32", dict(dtype=np.float32)), ("bf16x3", dict(dtype=np.float32, dense=R.dense_bf16x3))):
        got = OB.score(params, spec, x, mask, h, **kw)
        for key, sk in VALUES:
            err = np.abs(np.asarray(got[key], np.float64) - ref[key])
            of_max = err.max() / np.abs(ref[key]).max()
            live = ref[sk] > 0                       # (the all-missing image's log_px: no addend, exactly 0)
            assert (np.asarray(got[key])[~live] == 0).all()
            of_row = (err[live] / ref[sk][live]).max()
            print(f"[{name} {which} {label}] {key}: {of_max:.2e} of max|ref|, {of_row:.2e} of S_r")
            assert of_max <= QUARTER and of_row <= QUARTER, (label, key, of_max, of_row)
        assert np.abs(got["probs"] - ref["probs"]).max() <= 1e-5


@pytest.mark.parametrize("which", OB.LATENTS)
@pytest.mark.parametrize("name", CASES)
def test_gradient_emulation_stays_within_a_quarter_of_the_bar(name, which):
    spec, params, x, mask, _, _ = OB.case(name)
    ref = OB.grad_reference(name, which)
    f32 = OB.grads(params, spec, x, mask, OB.latents(name, which), dtype=np.float32)
    for label, got in (("float32", f32), ("bf16x3", OB.grad_emulated(name, which))):
        for t in G.TERMS:
            r = [G.rel_l2(a, b) for a, b in zip(got[t], ref[t])]
            for a, v in zip(got[t], r):
                if v is None:                        # a layer the term does not reach: exactly zero
                    assert not np.asarray(a).any()
            worst = max(v for v in r if v is not None)
            print(f"[{name} {which} {label}] {t}: {worst:.2e}")
            assert worst <= QUARTER, (label, t, worst)
        tot, scale = G.combine(ref, (0.0, 1.0, 1.0))
        etot, _ = G.combine(got, (0.0, 1.0, 1.0))
        assert max(G.rel_l2(a, b, s) for a, b, s in zip(etot, tot, scale)) <= QUARTER


@pytest.mark.parametrize("name,init", list(OB.AIS_CASES))
def test_ais_emulation_decides_as_float64_and_stays_within_a_quarter_of_the_bars(name, init):
    ref, emu = OB.ais_case(name, init), OB.ais_emulated(name, init)
    np.testing.assert_array_equal(emu["accept"], ref["accept"])
    np.testing.assert_array_equal(emu["step"], ref["step"])
    ew = np.abs(emu["log_w"] - ref["log_w"]).max() / np.abs(ref["log_w"]).max()
    eh = [np.abs(a - b).max() / np.abs(b).max() for a, b in zip(emu["h"], ref["h"])]
    print(f"[{name} {init}] emulation: log_w {ew:.2e} of max|ref|, latents {max(eh):.2e} of max|ref|")
    assert ew <= QUARTER and max(eh) <= QUARTER, (ew, eh)


@pytest.mark.parametrize("name,objective", [("OS2", "ELBO"), ("OS2", "IWAE"), ("OC784", "ELBO")])
def test_refine_emulation_stays_within_a_quarter_of_the_bars(name, objective):
    ref, emu = OB.refine_case(name, objective), OB.refine_emulated(name, objective)
    of_max = lambda got, r: float(np.abs(np.asarray(got, np.float64) - r).max() / np.abs(r).max())
    fig = {n: max(of_max(a, b) for a, b in zip(emu[n], ref[n])) for n in ("mean", "logstd")}
    fig["bound"] = of_max(emu["bound"], ref["bound"])
    fig["log_w"] = of_max(emu["log_w"], ref["log_w"])
    print(f"[{name} {objective}] " + ", ".join(f"{n} {v:.2e}" for n, v in fig.items()))
    for n, v in fig.items():
        assert v <= QUARTER, (n, v)


def test_hmc_emulation_decides_as_float64():
    name = "OS2"
    spec, params, x, mask, _, _ = OB.case(name)
    step, nl, _ = OB.HMC_CASES[name]
    r, q, H0, H1, lu, acc = OB.hmc_case(name)
    qe, E0, E1 = OB.hmc_step(params, spec, x, mask, OB.latents(name, "on"), r, step, nl, dtype=np.float32,
                             dense=R.dense_bf16x3)
    assert np.abs((E1 - E0) - (H1 - H0)).max() <= 0.1          # (the margin is 0.4)
    assert max(np.abs(a - b).max() / np.abs(b).max() for a, b in zip(qe, q)) <= QUARTER


# ------------------------------------------------------- 4. the searched cases
@pytest.mark.parametrize("name,init", list(OB.AIS_CASES))
def test_ais_case_conditions(name, init):
    out = OB.ais_case(name, init)
    big, nrej = A.conditions(out)
    print(f"[{name} {init}] max|dH| {big:.2f}, transitions with a rejection {nrej}, accept rate {out['accept'].mean():.2f}")
    assert big < 5.0 and nrej >= 2
    assert np.abs(out["log_u"] + out["dH"]).min() >= 0.4 - 1e-9
    assert (out["log_u"] <= -1e-3).all()
    u = np.exp(out["log_u"]).astype(np.float32)
    assert ((u > 0) & (u < 1)).all()
    assert out["accept"].any() and not out["accept"].all()
    np.testing.assert_array_equal(out["accepts"], out["accept"].sum(0))
    assert OB.ais_search(name, init) == OB.AIS_CASES[name, init]
    # the all-missing image moves under the prior alone from "prior": Delta = log p(x_obs|h) = 0
    if init == "prior":
        assert (out["log_w"][:, 0] == 0.0).all()


def test_hmc_case_conditions():
    name = "OS2"
    out = OB.hmc_case(name)
    big, n_acc, n_rej, margin = OB.hmc_conditions(out)
    print(f"[{name}] max|dH| {big:.2f}, accepted {n_acc}, rejected {n_rej}, margin {margin:.2f}")
    assert big < 5.0 and n_acc >= 1 and n_rej >= 2 and margin >= 0.4 - 1e-9
    assert np.isfinite(np.exp(out[4]).astype(np.float32)).all() and (out[4][~out[5]] < 0).all()   # a rejecting u is below 1
    assert OB.hmc_search(name) == OB.HMC_CASES[name]
