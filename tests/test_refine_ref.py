"""The float64 reference of per-image variational refinement (tests/refine_ref.py)
checked on the CPU: the bound is the objective of the scored densities, the
gradients are those of the float64 objective, the float32 + bf16x3 emulation
stays within a quarter of the GPU test's bars, and refinement improves the
bound of every image."""
import numpy as np
import pytest

from oracle import iwae_oracle as O
import ais_ref as A
import refine_ref as F
import score_ref as R

BAR = 1e-4          # tests/test_gpu_refine.py's


def _of_max(got, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("objective", F.OBJECTIVES)
@pytest.mark.parametrize("name", ["S1", "S3"])
def test_one_iteration_bound_is_the_objective_of_the_scored_densities(name, objective):
    spec, params, x, B, k = F.case(name)
    m0, s0, eps = F.setting(name)
    out = F.run(params, spec, x, m0, s0, eps, objective, 1, evaluate=False)
    h = F.sample(m0, s0, eps[0])
    sc = R.score(params, spec, x, h)
    # log q* as the normal density of the unrounded sample under N(m, exp(ls)^2)
    exact = F.sample(m0, s0, eps[0], rounded=False)
    lq = sum(O.normal_log_prob(v, m[None], np.exp(s)[None])[0].sum(-1) for v, m, s in zip(exact, m0, s0))
    lw = sc["logp"] + sc["logpx"] - lq
    want = lw.mean(0) if objective == "ELBO" else np.log(np.exp(lw).mean(0))
    assert out["bound"].shape == (1, B)
    np.testing.assert_allclose(out["bound"][0], want, rtol=1e-10, atol=1e-10)


@pytest.mark.parametrize("objective", F.OBJECTIVES)
def test_gradients_agree_with_central_differences_of_the_float64_objective(objective):
    spec, params, x, B, k = F.case("S1")
    m0, s0, eps = F.setting("S1")
    _, Gm, Gl = F.objective_and_grads(params, spec, x, m0, s0, eps[0], objective, rounded=False)

    def J(mean, logstd):
        return F.value(F.weights(params, spec, x, mean, logstd, eps[0], rounded=False)[1], objective)
    step = 1e-5
    for i in range(len(m0)):
        for j in range(m0[i].shape[1]):          # column j of every image at once (images are independent)
            for which, got in (("m", Gm[i][:, j]), ("ls", Gl[i][:, j])):
                hi = [[np.array(v) for v in m0], [np.array(v) for v in s0]]
                lo = [[np.array(v) for v in m0], [np.array(v) for v in s0]]
                p = 0 if which == "m" else 1
                hi[p][i][:, j] += step
                lo[p][i][:, j] -= step
                fd = (J(*hi) - J(*lo)) / (2 * step)
                np.testing.assert_allclose(got, fd, rtol=1e-6, atol=1e-7, err_msg=f"{which}_{i}[:, {j}]")


@pytest.mark.parametrize("objective", F.OBJECTIVES)
@pytest.mark.parametrize("name", F.SHAPES + F.EXTRA)
def test_emulation_stays_within_a_quarter_of_the_gpu_bars(name, objective):
    ref, emu = F.refine_case(name, objective), F.emulated_case(name, objective)
    fig = {}
    for n in ("mean", "logstd"):
        fig[n] = max(_of_max(a, b) for a, b in zip(emu[n], ref[n]))
    fig["bound"] = _of_max(emu["bound"], ref["bound"])
    fig["log_w"] = _of_max(emu["log_w"], ref["log_w"])
    fig["grad"] = F.grad_errors(*emu["grads"][0], ref)
    print(f"[{name} {objective}] " + ", ".join(f"{n} {v:.2e}" for n, v in fig.items()))
    for n, v in fig.items():
        assert v <= BAR / 4, (n, v)
    assert all(a.dtype == np.float32 for a in emu["mean"] + emu["logstd"] + emu["adam"])


def test_refinement_improves_every_images_bound():
    spec, params, x, B, k = F.case("S1")
    m0, s0, _ = F.setting("S1")
    n = 200
    rng = np.random.default_rng(F.SEED + 1)
    dims = spec.n_latent_encoder
    eps = [[R.f32r(rng.standard_normal((k, B, d))) for d in dims] for _ in range(n)]
    out = F.run(params, spec, x, m0, s0, eps, "ELBO", n, evaluate=False)
    fresh = [R.f32r(rng.standard_normal((2000, B, d))) for d in dims]
    before = F.weights(params, spec, x, m0, s0, fresh)[1].mean(0)
    after = F.weights(params, spec, x, out["mean"], out["logstd"], fresh)[1].mean(0)
    print("ELBO at k = 2000 before", before, "after", after)
    assert (after > before).all()


def test_two_runs_continue_as_one():
    spec, params, x, B, k = F.case("S2")
    m0, s0, eps = F.setting("S2")
    whole = F.run(params, spec, x, m0, s0, eps, "IWAE", 4)
    a = F.run(params, spec, x, m0, s0, eps[:2], "IWAE", 2, evaluate=False)
    b = F.run(params, spec, x, a["mean"], a["logstd"], eps[2:], "IWAE", 2, step0=2, adam0=a["adam"])
    for n in ("mean", "logstd", "adam", "h"):
        for u, v in zip(b[n], whole[n]):
            np.testing.assert_array_equal(u, v)
    np.testing.assert_array_equal(np.concatenate([a["bound"], b["bound"]]), whole["bound"])
    np.testing.assert_array_equal(b["log_w"], whole["log_w"])


def test_device_noise_addressing():
    spec, _, _, B, k = F.case("S2")
    eps = F.device_noise("S2", 77, 2, base0=5)
    assert F.NOISE_LAYER == 29 and [e.shape for e in eps[1]] == [(k, B, d) for d in spec.n_latent_encoder]
    import noise_ref as NR
    row = 3 * k + 4                                     # image 3, sample 4
    want = NR.normals(NR.key(77), 6, [row], spec.n_latent_encoder[1], 30)[0]
    np.testing.assert_array_equal(eps[1][1][4, 3], want)
