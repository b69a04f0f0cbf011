"""The aggregate posterior on the GPU (iwae_aggregate; Flexible_Model.log_q_aggregate,
aggregate_posterior, information_statistics) against the float64 reference of
tests/aggregate_ref.py.

Bars (test_gpu_score.py's): each output within 1e-4 max|ref| and, per row, within
1e-4 S_r, S_r the sum of the absolute addends of the row's dominant reference
term.  tests/test_aggregate_ref.py shows the same lines in float32 within a
quarter of both on every case.  The kernel cases inject loc, scale and h1, so
they depend on the model only through d1."""
import functools

import numpy as np
import pytest

import aggregate_ref as AR
import latent_shape_cases as LS
import pathgrad_ref as PR
from test_gpu_parity import make_model, weights_from_flat

pytestmark = pytest.mark.gpu

WANT = AR.OUTPUTS
N_MODEL, K_MODEL = 33, 3
# L = 1 with x_dim % 4 == 2 and L = 2 with every width beside 64, x_dim = 66 (tests/latent_shape_cases.py)
MODEL_CASES = {"L1": ("LO1", 7301), "L2": ("LO2w", 7302)}


@functools.lru_cache(maxsize=None)
def _handle(d1):
    """A model whose only use is its handle: d1 units in the first stochastic layer."""
    return make_model([8], [8], [d1], [16], x_dim=16)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _counts(m, ids=(39, 40, 41)):
    return [int(m._lib.iwae_debug_count(m._h, i)) for i in ids]


def _np(out):
    return {n: v.cpu().numpy() for n, v in out.items()}


def _run(name, want=WANT):
    h, mu, s, P = AR.inputs(name)
    m = _handle(h.shape[1])
    return _np(m.log_q_aggregate(_f32(h), loc=_f32(mu), scale=_f32(s), own_period=P, want=want)), m


def _check(got, ref, label):
    worst = AR.errors(got, ref)
    for n, (e_max, e_row) in worst.items():
        print(f"{label} {n}: {e_max * AR.REL:.2e} of max|ref|, {e_row * AR.REL:.2e} of S_r")
    for n, (e_max, e_row) in worst.items():
        assert e_max <= 1.0 and e_row <= 1.0, (label, n, e_max, e_row)
    return worst


# ------------------------------------------------------------- kernel cases
@pytest.mark.parametrize("name", sorted(AR.SHAPES))
def test_kernel_case(name):
    ref = AR.reference(name)
    got, m = _run(name)
    assert set(got) == set(WANT)
    for n in WANT:
        assert got[n].shape == ref[n].shape
    _check(got, ref, f"[{name}]")
    m.check_kernel_status()


def test_one_row_against_many_references_takes_the_split_path():
    from iwae_replication_project_amd.flexible_iwae import aggregate_split
    name = "d64_M1000_R1"
    d, M, R = AR.SHAPES[name]
    assert aggregate_split(R, M, d) == (16, 16)            # 16 segments of one tile on both kernels
    c0 = _counts(_handle(d))
    got, m = _run(name)
    assert [b - a for a, b in zip(c0, _counts(m))] == [1, 1, 1]
    _check(got, AR.reference(name), "[split]")
    # an unsplit call over the same references (enough rows), row 0 the same latent: the same value to the bars
    h, mu, s, P = AR.inputs(name)
    many = np.repeat(h, 1024 * 64, axis=0)
    assert aggregate_split(len(many), M, d)[0] == 1
    one = _np(m.log_q_aggregate(_f32(many), loc=_f32(mu), scale=_f32(s), want=("log_q_agg",)))["log_q_agg"]
    assert (one == one[0]).all()
    assert abs(float(one[0]) - AR.reference(name)["log_q_agg"][0]) <= AR.REL * AR.reference(name)["S"][0]


def test_outputs_are_optional_and_counted():
    name = "d50_M63_R1"
    full, m = _run(name)
    for want, delta in ((("log_q_agg",), [1, 1, 0]), (("log_q_dim",), [1, 0, 1]), (("log_q_own", "log_q_own_dim"), [1, 0, 0])):
        c0 = _counts(m)
        got, _ = _run(name, want)
        assert [b - a for a, b in zip(c0, _counts(m))] == delta
        assert set(got) == set(want)
        for n in want:
            np.testing.assert_array_equal(got[n], full[n])


@pytest.mark.parametrize("name", ["d64_M65_R257", "d200_M1000_R257"])
def test_scalar_path_gives_the_float4_paths_bits(name):
    import torch
    h, mu, s, P = AR.inputs(name)
    m = _handle(h.shape[1])
    a = m.log_q_aggregate(_f32(h), loc=_f32(mu), scale=_f32(s), own_period=P, want=WANT)
    pad = torch.zeros(h.size + 1, device=m.device)
    pad[1:] = torch.as_tensor(_f32(h)).to(m.device).reshape(-1)
    off = pad[1:].view(*h.shape)                           # the same latents, 4 bytes off 16-byte alignment
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    b = m.log_q_aggregate(off, loc=_f32(mu), scale=_f32(s), own_period=P, want=WANT)
    for n in WANT:
        np.testing.assert_array_equal(a[n].cpu().numpy(), b[n].cpu().numpy(), err_msg=n)


# --------------------------------------------------------------- edge inputs
def test_small_scales():
    got, _ = _run("small")
    ref = AR.reference("small")
    _check(got, ref, "[small]")
    logM = np.log(AR.EDGES["small"][1])
    # off-image terms underflow: the aggregate is the own term over M, the information log M
    np.testing.assert_allclose(got["log_q_agg"], got["log_q_own"] - logM, rtol=0, atol=AR.REL * ref["S"].max())
    mi = (got["log_q_own"].astype(np.float64) - got["log_q_agg"]).mean()
    assert abs(mi - logM) <= 1e-4 * logM


def test_wide_scales():
    got, _ = _run("wide")
    _check(got, AR.reference("wide"), "[wide]")


@pytest.mark.parametrize("name", ["d260", "d260s"])
def test_units_beyond_one_chunk(name):
    from iwae_replication_project_amd.flexible_iwae import aggregate_split
    d, M, R, _ = AR.EDGES[name]
    assert d > 256 and (aggregate_split(R, M, d)[1] > 1) == (name == "d260s")
    got, m = _run(name)
    _check(got, AR.reference(name), f"[{name}]")
    m.check_kernel_status()


def test_poisoned_row_stays_alone():
    got, _ = _run("poison")
    ref = AR.reference("poison")
    for n in WANT:
        bad = ~np.isfinite(got[n].reshape(len(ref["S"]), -1))
        assert bad[5].all() and not np.delete(bad, 5, axis=0).any(), n
    _check(got, ref, "[poison]")                           # the finite rows, to the bars


@pytest.mark.parametrize("name", ["m1", "d1_M1_R1", "d200_M1_R15"])
def test_one_component_is_the_own_term(name):
    got, _ = _run(name)
    ref = AR.reference(name)
    _check(got, ref, f"[{name}]")
    S = ref["S"]
    assert (np.abs(got["log_q_agg"].astype(np.float64) - got["log_q_own"]) <= AR.REL * S).all()
    assert (np.abs(got["log_q_dim"].astype(np.float64) - got["log_q_own_dim"]) <= AR.REL * S[:, None]).all()


def test_own_period_of_sample_major_latents():
    h, mu, s, P = AR.inputs("own")
    k, N, d = 3, 5, 3
    assert P == N and h.shape == (k * N, d)
    m = _handle(d)
    got = _np(m.log_q_aggregate(_f32(h).reshape(k, N, d), loc=_f32(mu), scale=_f32(s), own_period=N, want=WANT))
    assert got["log_q_own"].shape == (k, N) and got["log_q_own_dim"].shape == (k, N, d)
    # explicit indices: sample j of image i against component i
    for j in range(k):
        for i in range(N):
            t = -0.5 * ((h[j * N + i] - mu[i]) / s[i]) ** 2 - np.log(s[i]) - AR.HALF_LOG_2PI
            S = AR.reference("own")["S"][j * N + i]
            assert np.abs(got["log_q_own_dim"][j, i] - t).max() <= AR.REL * S
            assert abs(got["log_q_own"][j, i] - t.sum()) <= AR.REL * S
    flat = {n: v.reshape((k * N,) + v.shape[2:]) for n, v in got.items()}
    _check(flat, AR.reference("own"), "[own]")
    # another period picks other components
    other = _np(m.log_q_aggregate(_f32(h), loc=_f32(mu), scale=_f32(s), own_period=2, want=("log_q_own",)))["log_q_own"]
    ref2 = AR.aggregate(h, mu, s, 2)["log_q_own"]
    assert (np.abs(other - ref2) <= AR.REL * np.maximum(AR.reference("own")["S"], np.abs(ref2))).all()


def test_library_rejects_bad_arguments_and_launches_nothing():
    import torch
    from iwae_replication_project_amd import _lib
    m = _handle(3)
    M, R, d = 4, 6, 3
    dev = m.device
    h1, loc, sc = torch.zeros(R, d, device=dev), torch.zeros(M, d, device=dev), torch.ones(M, d, device=dev)
    out, outd = torch.zeros(R, device=dev), torch.zeros(R, d, device=dev)
    x = torch.zeros(M, m.x_dim, device=dev)
    f, fn = _lib.fptr, m._lib.iwae_aggregate
    c0 = _counts(m)
    calls = [
        (None, M, 0, f(loc), f(sc), f(h1), R, 0, None, None, None, None),          # every output NULL
        (None, M, 0, f(loc), f(sc), None, R, 0, f(out), None, None, None),         # lat1 NULL
        (None, M, 0, f(loc), f(sc), f(h1), 0, 0, f(out), None, None, None),        # R < 1
        (None, M, 0, f(loc), f(sc), f(h1), (1 << 30) + 1, 0, f(out), None, None, None),
        (None, 0, 0, f(loc), f(sc), f(h1), R, 0, f(out), None, None, None),        # M < 1
        (f(x), (1 << 24) + 1, 0, None, None, f(h1), R, 0, f(out), None, None, None),
        (None, M, 0, None, f(sc), f(h1), R, 0, f(out), None, None, None),          # no x_ref and no loc
        (None, M, 0, f(loc), None, f(h1), R, 0, f(out), None, None, None),
        (None, M, 0, f(loc), f(sc), f(h1), R, -1, f(out), None, None, None),       # P < 0
        (None, M, 0, f(loc), f(sc), f(h1), R, M + 1, f(out), None, None, None),    # P > M
        (None, M, 0, f(loc), f(sc), f(h1), R, 0, f(out), None, f(out), None),      # own outputs with P = 0
        (None, M, 0, f(loc), f(sc), f(h1), R, 0, f(out), None, None, f(outd)),
    ]
    for a in calls:
        assert fn(m._h, *a) == -1, a
    assert _counts(m) == c0
    assert fn(m._h, None, M, 0, f(loc), f(sc), f(h1), R, M, f(out), f(outd), f(out), f(outd)) == 0
    m._stream.synchronize()


# --------------------------------------------------------------- model cases
@functools.lru_cache(maxsize=None)
def _case(tag):
    """(arch, spec, params, x, eps) of a model case: the named shape with N = 33 images."""
    name, seed = MODEL_CASES[tag]
    he, hd, le, ld, x_dim = LS.CASES[name][:5]
    spec, params, _, x, eps = PR.make_case((he, hd, le, ld), N_MODEL, K_MODEL, seed, x_dim=x_dim)
    return (he, hd, le, ld), spec, params, x, eps


@functools.lru_cache(maxsize=None)
def _model(tag, path="auto", precision="bf16x3", seed=0):
    from oracle import iwae_oracle as O
    (he, hd, le, ld), spec, params, _, _ = _case(tag)
    m = make_model(he, hd, le, ld, x_dim=spec.x_dim, kernel_path=path, precision=precision, seed=seed)
    m.set_weights(weights_from_flat(m, O.flatten_params(spec, params)))
    m.compile()
    return m


@functools.lru_cache(maxsize=None)
def _oracle(tag):
    """The float64 forward of the case: first-layer parameters and latents."""
    from oracle import iwae_oracle as O
    _, spec, params, x, eps = _case(tag)
    c = O.forward(params, spec, x, eps)
    return c["enc"][0]["mu"], c["enc"][0]["scale"], AR.f32r(c["h"][0])


def test_components_are_the_encoders_bits_for_one_layer():
    _, _, _, x, _ = _case("L1")
    m = _model("L1")
    _, _, top = m.encoder(_f32(x), 1)
    h1 = np.zeros((4, m.n_latent_encoder[0]), np.float32)
    out = m.log_q_aggregate(h1, x_ref=_f32(x), want=("log_q_agg", "loc", "scale"))
    np.testing.assert_array_equal(out["loc"].cpu().numpy(), top.loc.cpu().numpy())
    np.testing.assert_array_equal(out["scale"].cpu().numpy(), top.scale.cpu().numpy())


def test_components_match_the_oracles_first_layer_for_two_layers():
    _, _, _, x, _ = _case("L2")
    mu, s, h = _oracle("L2")
    out = _model("L2").log_q_aggregate(_f32(h), x_ref=_f32(x), want=("log_q_agg", "loc", "scale"))
    assert np.abs(out["loc"].cpu().numpy() - mu).max() <= 1e-4 * np.abs(mu).max()
    assert np.abs(out["scale"].cpu().numpy() - s).max() <= 1e-4 * np.abs(s).max()


@pytest.mark.parametrize("tag", list(MODEL_CASES))
def test_chunk_independence_and_determinism(tag):
    _, _, _, x, _ = _case(tag)
    _, _, h = _oracle(tag)
    m = _model(tag)
    want = WANT + ("loc", "scale")
    base = _np(m.log_q_aggregate(_f32(h), x_ref=_f32(x), own_period=N_MODEL, want=want, chunk=0))
    for chunk in (0, 1, 7, 33):
        got = _np(m.log_q_aggregate(_f32(h), x_ref=_f32(x), own_period=N_MODEL, want=want, chunk=chunk))
        for n in want:
            np.testing.assert_array_equal(got[n], base[n], err_msg=f"chunk {chunk} {n}")


@pytest.mark.parametrize("path,precision", [("auto", "bf16x3"), ("layerwise", "bf16x3"), ("auto", "f32")])
@pytest.mark.parametrize("tag", list(MODEL_CASES))
def test_model_parity(tag, path, precision):
    _, _, _, x, _ = _case(tag)
    mu, s, h = _oracle(tag)
    ref = AR.aggregate(h.reshape(-1, h.shape[-1]), mu, s, N_MODEL)
    got = _np(_model(tag, path, precision).log_q_aggregate(_f32(h), x_ref=_f32(x), own_period=N_MODEL, want=WANT))
    assert got["log_q_agg"].shape == h.shape[:2] and got["log_q_dim"].shape == h.shape
    flat = {n: v.reshape((-1,) + v.shape[2:]) for n, v in got.items()}
    _check(flat, ref, f"[{tag} {path} {precision}]")


@pytest.mark.parametrize("tag", list(MODEL_CASES))
def test_information_statistics(tag):
    _, _, _, x, eps = _case(tag)
    mu, s, _ = _oracle(tag)
    m = _model(tag)
    e32 = [_f32(e) for e in eps]
    a = m.aggregate_posterior(_f32(x), K_MODEL, eps=e32, per_unit=True)
    d1 = m.n_latent_encoder[0]
    assert tuple(a["log_q_agg"].shape) == (N_MODEL, K_MODEL) and tuple(a["log_q_dim"].shape) == (N_MODEL, K_MODEL, d1)
    assert tuple(a["h"][0].shape) == (K_MODEL, N_MODEL, d1)
    # the reference formed from the same samples: the device's latents against the oracle's components
    h = a["h"][0].cpu().numpy().astype(np.float64).reshape(-1, d1)                   # rows s N + i
    ref = AR.aggregate(h, mu, s, N_MODEL)
    lq, lp = (a[n].cpu().numpy().astype(np.float64).T.reshape(-1) for n in ("log_q", "log_ph"))
    kl, mi, mkl = AR.information(lq, lp, ref["log_q_own"], ref["log_q_agg"])
    tc = (ref["log_q_agg"] - ref["log_q_dim"].sum(-1)).mean()
    mi_unit = (ref["log_q_own_dim"] - ref["log_q_dim"]).mean(0)
    st = m.information_statistics(_f32(x), K_MODEL, eps=e32)
    bar = AR.REL * ref["S"].mean()                         # the row bar, averaged as the statistics are
    print(f"[{tag}] kl {st['kl']:.5f} mi {st['mi']:.5f} ({mi:.5f}) marginal {st['marginal_kl']:.5f} ({mkl:.5f}) "
          f"tc {st['total_correlation']:.5f} ({tc:.5f}); bar {bar:.2e}")
    assert st["kl"] == pytest.approx(kl, abs=1e-12 + 1e-9 * abs(kl))
    assert abs(st["mi"] - mi) <= bar and abs(st["marginal_kl"] - mkl) <= bar
    assert abs(st["total_correlation"] - tc) <= 2 * bar   # two outputs' errors
    assert st["mi_per_unit"].shape == (d1,) and np.abs(st["mi_per_unit"] - mi_unit).max() <= bar
    assert 0.0 <= st["mi"] <= np.log(N_MODEL) + bar
    # mi + marginal_kl == kl by construction: float64 means of the same float32 rows
    assert abs(st["mi"] + st["marginal_kl"] - st["kl"]) <= 1e-6 * max(1.0, abs(st["kl"]))
    # without injected noise the call draws, as model.encoder does; with another x_ref there are no own terms
    b = m.aggregate_posterior(_f32(x), 2, x_ref=_f32(x[:7]))
    assert "log_q_own" not in b and tuple(b["log_q_agg"].shape) == (N_MODEL, 2)


@pytest.mark.parametrize("tag", list(MODEL_CASES))
def test_state_is_untouched(tag):
    """A train step before and after gives the bits of a run without the call: weights, Adam
    state, noise position and captured graphs stay."""
    _, _, _, x, _ = _case(tag)
    _, _, h = _oracle(tag)
    a, b = (_model(tag, seed=41 + i) for i in range(2))
    xb = _f32(x[:6])
    for m in (a, b):
        m.set_weights(_model(tag).get_weights())
        m.set_seed(123)
    la = [a.train_step(xb)]
    lb = [b.train_step(xb)]
    g0 = a.graph_captures()
    a.log_q_aggregate(_f32(h), x_ref=_f32(x), own_period=N_MODEL, want=WANT)
    a.log_q_aggregate(_f32(h), loc=np.zeros((5, h.shape[-1]), np.float32), scale=np.ones((5, h.shape[-1]), np.float32))
    assert a.graph_captures() == g0
    la.append(a.train_step(xb))
    lb.append(b.train_step(xb))
    assert la == lb
    for wa, wb in zip(a.get_weights(), b.get_weights()):
        np.testing.assert_array_equal(np.asarray(wa), np.asarray(wb))
    a.check_kernel_status()
