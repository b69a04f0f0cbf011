"""The float64 reference of tests/scoregrad_ref.py is the derivative of
score_ref.score, float32 and the emulated bf16x3 path stay well inside the bars
the GPU test applies, and the HMC reference conserves H as a leapfrog should
(no GPU needed).

Bars pinned here for tests/test_gpu_scoregrad.py: relative L2 error per layer
and per term.  Every case but SH: the emulation within 2.5e-5, a quarter of the
GPU's 1e-4 (found: float32 at most 6e-7, emulation at most 1.5e-5).  SH (scales
of about e^-3 amplify the products' rounding): the figures found are recorded
in SH_FOUND and held to 1.5 times themselves; the GPU test allows the kernels
twice the emulation's figure."""
import numpy as np
import pytest

import score_ref as R
import scoregrad_ref as G

BAR = 1e-4
# SH, bf16x3 emulation, worst layer: (latent set, term) -> relative L2 error found
SH_FOUND = {("on", "q"): 7.2e-5, ("prior", "ph"): 1.9e-4}


def _directional(name, which, seed):
    spec, params, x, _ = R.case(name)
    h = R.latents(name, which)
    rng = np.random.default_rng(seed)
    v = [rng.standard_normal(a.shape) for a in h]
    e = 3e-5                                  # near (3 u |f| / |f'''|)^(1/3) for |f| of a few hundred
    up = R.score(params, spec, x, [a + e * b for a, b in zip(h, v)])
    dn = R.score(params, spec, x, [a - e * b for a, b in zip(h, v)])
    g = G.reference(name, which)
    out = {}
    for t, key in zip(G.TERMS, ("logq", "logp", "logpx")):
        fd = (up[key] - dn[key]) / (2 * e)
        an = sum((a * b).sum(-1) for a, b in zip(g[t], v))
        out[t] = float(np.abs(fd - an).max() / np.abs(an).max())
    return out


@pytest.mark.parametrize("which", R.LATENTS)
@pytest.mark.parametrize("name", ["S1", "S2", "S3"])
def test_reference_is_the_derivative_of_the_scored_densities(name, which):
    r = _directional(name, which, 17)
    print(name, which, {k: f"{v:.2e}" for k, v in r.items()})
    for t, v in r.items():
        assert v <= 1e-7, (t, v)


def _figures(name, which, **kw):
    spec, params, x, _ = R.case(name)
    ref = G.reference(name, which)
    got = G.grads(params, spec, x, R.latents(name, which), **kw)
    out = {}
    for t in G.TERMS:
        r = [G.rel_l2(a, b) for a, b in zip(got[t], ref[t])]
        for a, b, v in zip(got[t], ref[t], r):
            if v is None:                       # a layer the term does not reach: exactly zero
                assert not np.asarray(a).any()
        out[t] = max(v for v in r if v is not None)
    return out


@pytest.mark.parametrize("which", R.LATENTS)
@pytest.mark.parametrize("name", [n for n in R.CASES if n != "SH"])
def test_float32_and_bf16x3_emulation_stay_within_a_quarter_of_the_bar(name, which):
    f32 = _figures(name, which, dtype=np.float32)
    emu = G.emulation_figures(name, which)
    print(name, which, "float32", {k: f"{v:.2e}" for k, v in f32.items()}, "bf16x3", {k: f"{v:.2e}" for k, v in emu.items()})
    for t in G.TERMS:
        assert f32[t] <= 0.25 * BAR, (t, f32[t])
        assert emu[t] <= 0.25 * BAR, (t, emu[t])


@pytest.mark.parametrize("which", R.LATENTS)
def test_sharp_case_figures_are_pinned(which):
    f32 = _figures("SH", which, dtype=np.float32)
    emu = G.emulation_figures("SH", which)
    print("SH", which, "float32", {k: f"{v:.2e}" for k, v in f32.items()}, "bf16x3", {k: f"{v:.2e}" for k, v in emu.items()})
    for t in G.TERMS:
        assert f32[t] <= 0.25 * BAR, (t, f32[t])            # the f32 path keeps the project's bar on SH too
        found = SH_FOUND.get((which, t))
        if found is None:
            assert emu[t] <= 0.25 * BAR, (t, emu[t])
        else:
            assert emu[t] <= 1.5 * found, (t, emu[t])


def test_combined_coefficients_are_measured_against_the_terms_norms():
    g = G.reference("S2", "on")
    tot, scale = G.combine(g, (-1.0, 1.0, 1.0))
    for i, (a, s) in enumerate(zip(tot, scale)):
        np.testing.assert_allclose(a, -g["q"][i] + g["ph"][i] + g["px"][i], rtol=0, atol=1e-12)
        assert np.linalg.norm(a) <= s * (1 + 1e-12)


@pytest.mark.parametrize("name", list(G.HMC_CASES))
def test_hmc_reference_conserves_the_hamiltonian(name):
    spec, params, x, _ = R.case(name)
    step, nl, _ = G.HMC_CASES[name]
    r, q, H0, H1, lu, acc = G.hmc_case(name)
    h = R.latents(name, "on")
    dH = H1 - H0
    assert np.abs(dH).max() < 5, np.abs(dH).max()
    assert acc.any() and (~acc).any()
    assert (np.abs(lu - -dH) >= 0.4 - 1e-12).all()
    # well below the test's step the energy error falls as step^2: the same trajectory at step / 4 and step / 8
    _, A0, A1 = G.hmc_step(params, spec, x, h, r, step / 4, 4 * nl)
    _, B0, B1 = G.hmc_step(params, spec, x, h, r, step / 8, 8 * nl)
    ratio = np.abs(B1 - B0).mean() / np.abs(A1 - A0).mean()
    print(name, "mean |dH|", np.abs(dH).mean(), "at step / 4", np.abs(A1 - A0).mean(), "at step / 8",
          np.abs(B1 - B0).mean(), "ratio", ratio)
    assert 0.2 <= ratio <= 0.3, ratio
    # the emulated bf16x3 trajectory decides as the reference: dH within 0.1 nats (the margin is 0.4)
    _, E0, E1 = G.hmc_step(params, spec, x, h, r, step, nl, dtype=np.float32, dense=R.dense_bf16x3)
    d = np.abs((E1 - E0) - dH).max()
    print(name, "emulated dH off by", d)
    assert d <= 0.1, d
