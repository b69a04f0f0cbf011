"""Gradients of the scored densities with respect to the latents
(iwae_score_grad; Flexible_Model.score_grad, Flexible_Model.hmc) against the
float64 reference of tests/scoregrad_ref.py, on the fused sg_kernel (the
automatic path of these cases) and on the layer-wise path.

Bars.  Gradients: relative L2 error per layer <= 1e-4 (the project's gradient
bar); for a combined coefficient vector relative to sum_t |c_t| ||g_t||, so
cancellation between the terms does not tighten it.  Values: test_gpu_score's
two bars.  tests/test_scoregrad_ref.py shows float32 and the emulated bf16x3
path within a quarter of the gradient bar on every case but SH.

SH (scales of about e^-3): the 1e-4 bar under precision="f32"; under bf16x3 at
most twice the CPU emulation's figure of the same term and latent set (the
factor allows for the kernels' summation order; it is measured against the
emulation, never against the kernels).  test_parity prints every ratio
(DESIGN.md s9 has the table)."""
import ctypes

import numpy as np
import pytest

import group_cases as GC
import score_ref as R
import scoregrad_ref as G
from test_gpu_parity import make_model
from test_gpu_score import _check_terms, _f32, _model, fresh_group_model

pytestmark = pytest.mark.gpu

BAR = 1e-4
PATHS = ("auto", "layerwise")
UNITS = {"q": (1.0, 0.0, 0.0), "ph": (0.0, 1.0, 0.0), "px": (0.0, 0.0, 1.0)}
VALUE = {"q": "log_q", "ph": "log_ph", "px": "log_px"}
POST = (0.0, 1.0, 1.0)


def _counts(m, ids=(25, 26, 23, 24, 3)):
    return [int(m._lib.iwae_debug_count(m._h, i)) for i in ids]


def _np(ts):
    return [t.cpu().numpy() for t in ts]


def _layer_errors(got, ref, scale=None):
    """Relative L2 error per layer; a layer the reference does not reach must be exactly zero."""
    out = []
    for i, (a, b) in enumerate(zip(got, ref)):
        assert a.shape == b.shape
        r = G.rel_l2(a, b, None if scale is None else scale[i])
        if r is None:
            assert not a.any(), i
        else:
            out.append(r)
    return out


# ------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("which", R.LATENTS)
@pytest.mark.parametrize("name", list(R.CASES))
def test_parity(name, which, path):
    _, _, x, _ = R.case(name)
    h, ref, vref = R.latents(name, which), G.reference(name, which), R.reference(name, which)
    sharp = name == "SH"
    for precision in (("bf16x3", "f32") if sharp else ("bf16x3",)):
        m = _model(name, path, precision)
        emulated = sharp and precision == "bf16x3"
        label = f"[{name} {which} {path} {precision}]"
        for t, coef in UNITS.items():
            out = m.score_grad(_f32(x), _f32(h), coef=coef, want=("grad", VALUE[t]))
            errs = _layer_errors(_np(out["grad"]), ref[t])
            bar = 2 * G.emulation_figures(name, which)[t] if emulated else BAR
            print(f"{label} d{VALUE[t]}/dh: {max(errs):.2e} (bar {bar:.2e})")
            assert max(errs) <= bar, (label, t, errs)
            _check_terms(out, vref, label, row_bar=not emulated)
        out = m.score_grad(_f32(x), _f32(h), coef=POST)
        tot, scale = G.combine(ref, POST)
        errs = _layer_errors(_np(out["grad"]), tot, scale)
        bar = BAR
        if emulated:
            etot, _ = G.combine(G.emulated(name, which), POST)
            bar = 2 * max(G.rel_l2(a, b, s) for a, b, s in zip(etot, tot, scale))
        print(f"{label} (0, 1, 1): {max(errs):.2e} of sum |c_t| ||g_t|| (bar {bar:.2e})")
        assert max(errs) <= bar, (label, errs)
        m.check_kernel_status()


# -------------------------------------------------------------- 2. path taken
@pytest.mark.parametrize("name", list(R.CASES))
def test_path_taken(name):
    _, _, x, _ = R.case(name)
    h = _f32(R.latents(name, "off"))
    want = ("grad", "log_q", "log_ph", "log_px")
    m = _model(name, "auto")
    c0 = _counts(m)
    m.score_grad(_f32(x), h, coef=(-1.0, 1.0, 1.0), want=want)
    c1 = _counts(m)
    m.score(_f32(x), h)
    c2 = _counts(m)
    d = [b - a for a, b in zip(c0, c1)]
    assert sorted(d[:2]) == [0, 1], d                     # exactly one of 25 / 26, one chunk
    assert (d[0] == 1) == (c2[2] > c1[2]), (d, c1, c2)    # fused exactly when score on the same model is
    if name in ("C784", "K130"):
        assert d[0] == 1, d
    assert d[2:] == [0, 0, 0], d                          # not counted as iwae_score's; never the ring
    lw = _model(name, "layerwise")
    c0 = _counts(lw)
    lw.score_grad(_f32(x), h, coef=(-1.0, 1.0, 1.0), want=want)
    d = [b - a for a, b in zip(c0, _counts(lw))]
    assert d == [0, 1, 0, 0, 0], d


# ---------------------------------------------------------- 3. term selection
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", ["S1", "S2", "S3"])
def test_term_selection(name, path):
    _, _, x, _ = R.case(name)
    h = _f32(R.latents(name, "off"))
    ref, vref = G.reference(name, "off"), R.reference(name, "off")
    m = _model(name, path)
    # log p(h) alone needs no images
    a = m.score_grad(None, h, coef=UNITS["ph"], want=("grad", "log_ph"))
    b = m.score_grad(_f32(x), h, coef=UNITS["ph"], want=("grad", "log_ph"))
    for u, v in zip(_np(a["grad"]) + [a["log_ph"].cpu().numpy()], _np(b["grad"]) + [b["log_ph"].cpu().numpy()]):
        np.testing.assert_array_equal(u, v)
    with pytest.raises(ValueError):
        m.score_grad(None, h, coef=POST)
    # a zero coefficient with its value asked for: the value within the bars, the gradient without the term
    out = m.score_grad(_f32(x), h, coef=POST, want=("grad", "log_q", "log_ph", "log_px"))
    _check_terms(out, vref, f"[{name} {path} zero c_q]")
    plain = m.score_grad(_f32(x), h, coef=POST)
    for u, v in zip(_np(out["grad"]), _np(plain["grad"])):
        np.testing.assert_array_equal(u, v)
    tot, scale = G.combine(ref, POST)
    assert max(_layer_errors(_np(out["grad"]), tot, scale)) <= BAR
    # n_grad 0: a scoring call
    vals = m.score_grad(_f32(x), h, want=("log_q", "log_ph", "log_px"))
    assert "grad" not in vals and "log_w" in vals
    _check_terms(vals, vref, f"[{name} {path} values only]")


@pytest.mark.parametrize("path", PATHS)
def test_grad_is_overwritten_not_accumulated(path):
    import torch
    from iwae_replication_project_amd import _lib
    _, _, x, _ = R.case("S2")
    _, B, k = R.CASES["S2"][:3]
    m = _model("S2", path)
    dev = m.device
    xt = torch.as_tensor(_f32(x), device=dev)
    hs = [torch.as_tensor(v, device=dev).contiguous() for v in _f32(R.latents("S2", "off"))]
    lat, n = _lib.fptr_array(hs)
    coef = (ctypes.c_float * 3)(-1.0, 1.0, 1.0)
    res = []
    for fill in (0.0, 7.5, float("nan")):
        gs = [torch.full_like(t, fill) for t in hs]
        garr, ng = _lib.fptr_array(gs)
        assert m._lib.iwae_score_grad(m._h, _lib.fptr(xt), B, k, 0, lat, n, coef, garr, ng, None, None, None) == 0
        m._stream.synchronize()
        res.append(_np(gs))
    for other in res[1:]:
        for u, v in zip(res[0], other):
            np.testing.assert_array_equal(u, v)


# ------------------------------------------------------------------- 4. chunks
@pytest.mark.parametrize("path", PATHS)
def test_chunks_do_not_change_a_bit(path):
    _, _, x, _ = R.case("S2")
    h = _f32(R.latents("S2", "off"))
    m = _model("S2", path)
    want = ("grad", "log_q", "log_ph", "log_px")
    coef = (-1.0, 1.0, 1.0)
    c0 = _counts(m)
    whole = m.score_grad(_f32(x), h, coef=coef, want=want, chunk=0)
    assert sum(_counts(m)[:2]) == sum(c0[:2]) + 1
    for chunk, launches in ((1, 5), (2, 3)):
        c0 = _counts(m)
        out = m.score_grad(_f32(x), h, coef=coef, want=want, chunk=chunk)
        assert sum(_counts(m)[:2]) == sum(c0[:2]) + launches
        for u, v in zip(_np(out["grad"]), _np(whole["grad"])):
            np.testing.assert_array_equal(u, v, err_msg=f"chunk {chunk} grad")
        for n in want[1:]:
            np.testing.assert_array_equal(out[n].cpu().numpy(), whole[n].cpu().numpy(), err_msg=f"chunk {chunk} {n}")


def test_first_layer_groups_of_four_and_three_images():
    """7 images in chunks of 2 under first-layer groups of 4 (group_cases.py), on
    a model that has run nothing: four sg_kernel launches, none layer-wise, none
    of iwae_score's; the gradient of log w and the three values within the bars;
    bit for bit the same call with the default group size."""
    name = GC.GROUP_CASE
    _, _, x, _ = R.case(name)
    h = _f32(R.latents(name, "off"))
    ref, vref = G.reference(name, "off"), R.reference(name, "off")
    m = fresh_group_model()
    want, coef = ("grad", "log_q", "log_ph", "log_px"), (-1.0, 1.0, 1.0)
    out, one_group, d = GC.groups_then_one_group(
        m, (25, 26, 23, 24, 3), lambda: m.score_grad(_f32(x), h, coef=coef, want=want, chunk=GC.CHUNK))
    assert d == [4, 0, 0, 0, 0], d                        # chunks [0,2) [2,4) | [4,6) [6,7)
    tot, scale = G.combine(ref, coef)
    errs = _layer_errors(_np(out["grad"]), tot, scale)
    print(f"[G7 off auto group 4] (-1, 1, 1): {max(errs):.2e} of sum |c_t| ||g_t||")
    assert max(errs) <= BAR, errs
    _check_terms(out, vref, "[G7 off auto group 4]")
    for u, v in zip(_np(out["grad"]), _np(one_group["grad"])):
        np.testing.assert_array_equal(u, v, err_msg="grad")
    for n in want[1:]:
        np.testing.assert_array_equal(out[n].cpu().numpy(), one_group[n].cpu().numpy(), err_msg=n)


# --------------------------------------------------------- 5. row independence
@pytest.mark.parametrize("bad", [1e30, float("nan")])
@pytest.mark.parametrize("path", PATHS)
def test_rows_are_independent(path, bad):
    _, _, x, _ = R.case("S2")
    _, B, k = R.CASES["S2"][:3]
    h = _f32(R.latents("S2", "off"))
    m = _model("S2", path)
    want = ("grad", "log_q", "log_ph", "log_px")
    coef = (-1.0, 1.0, 1.0)
    base = m.score_grad(_f32(x), h, coef=coef, want=want)
    b, s = 1, 3
    hb = [v.copy() for v in h]
    for v in hb:
        v[s, b, :] = bad
    out = m.score_grad(_f32(x), hb, coef=coef, want=want)
    keep = np.ones((k, B), bool)
    keep[s, b] = False
    for u, v in zip(_np(out["grad"]), _np(base["grad"])):
        np.testing.assert_array_equal(u[keep], v[keep])
    for n in want[1:]:
        np.testing.assert_array_equal(out[n].cpu().numpy()[keep], base[n].cpu().numpy()[keep], err_msg=n)
    m.check_kernel_status()


# ---------------------------------------------------------------- 6. determinism
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", ["S3", "C784"])
def test_two_calls_are_bit_identical(name, path):
    _, _, x, _ = R.case(name)
    h = _f32(R.latents(name, "prior"))
    m = _model(name, path)
    want = ("grad", "log_q", "log_ph", "log_px")
    a = m.score_grad(_f32(x), h, coef=(-1.0, 1.0, 1.0), want=want)
    b = m.score_grad(_f32(x), h, coef=(-1.0, 1.0, 1.0), want=want)
    for u, v in zip(_np(a["grad"]), _np(b["grad"])):
        np.testing.assert_array_equal(u, v)
    for n in want[1:]:
        np.testing.assert_array_equal(a[n].cpu().numpy(), b[n].cpu().numpy())


# -------------------------------------------------------------------- 7. state
def test_score_grad_and_hmc_leave_the_training_state_alone():
    from iwae_replication_project_amd import Adam
    he, hd, le, ld = R.CASES["C784"][0]
    rng = np.random.default_rng(5)
    x = (rng.random((40, 784)) < 0.3).astype(np.float32)
    k = 17
    eps = [rng.standard_normal((k, 5, d)).astype(np.float32) for d in le]
    models = []
    for _ in range(2):
        m = make_model(he, hd, le, ld, seed=11)
        m.compile(optimizer=Adam(learning_rate=1e-3, epsilon=1e-4))
        models.append(m)
    a, b = models
    b.set_weights(a.get_weights())
    la, lb = a.train_steps(x, 20), b.train_steps(x, 20)
    np.testing.assert_array_equal(np.asarray(la), np.asarray(lb))
    w0, (m0, v0, t0), g0 = a.get_weights(), a.get_optimizer_state(), a.graph_captures()
    h, _, _ = a.encoder(x[:5], k, eps=eps)
    b.encoder(x[:5], k, eps=eps)
    out = a.score_grad(x[:5], h, coef=(-1.0, 1.0, 1.0), want=("grad", "log_q", "log_ph", "log_px"))
    assert all(np.isfinite(v).all() for v in _np(out["grad"]))
    hn, acc, rate, lp = a.hmc(x[:5], h, 0.05, 3, n_iter=2)                  # device-drawn momenta and u
    assert np.isfinite(lp.cpu().numpy()).all() and 0.0 <= rate <= 1.0 and tuple(acc.shape) == (k, 5)
    w1, (m1, v1, t1) = a.get_weights(), a.get_optimizer_state()
    for p, q in zip(w0, w1):
        np.testing.assert_array_equal(p, q)
    np.testing.assert_array_equal(m0, m1)
    np.testing.assert_array_equal(v0, v1)
    assert t0 == t1 and a.graph_captures() == g0
    # the noise position stayed: the next device-noise log weights and train steps are the other model's
    np.testing.assert_array_equal(a.get_log_weights(x[:5], k).cpu().numpy(), b.get_log_weights(x[:5], k).cpu().numpy())
    la, lb = a.train_steps(x, 20), b.train_steps(x, 20)
    assert a.graph_captures() == g0                        # replayed, not re-captured
    np.testing.assert_array_equal(np.asarray(la), np.asarray(lb))
    for p, q in zip(a.get_weights(), b.get_weights()):
        np.testing.assert_array_equal(p, q)
    a.check_kernel_status()


# ------------------------------------------------------------------- 8. errors
@pytest.mark.parametrize("path", PATHS)
def test_invalid_arguments_return_einval_and_launch_nothing(path):
    import torch
    from iwae_replication_project_amd import _lib
    name = "S2"
    _, _, x, _ = R.case(name)
    _, B, k = R.CASES[name][:3]
    m = _model(name, path)
    dev = m.device
    xt = torch.as_tensor(_f32(x), device=dev)
    hs = [torch.as_tensor(v, device=dev).contiguous() for v in _f32(R.latents(name, "off"))]
    gs = [torch.empty_like(t) for t in hs]
    o = [torch.empty(B, k, device=dev) for _ in range(3)]
    lat, n = _lib.fptr_array(hs)
    grad, ng = _lib.fptr_array(gs)
    one = (_lib.FP * 2)(_lib.fptr(hs[0]), None)
    gone = (_lib.FP * 2)(_lib.fptr(gs[0]), None)
    P, N0 = _lib.fptr, None
    C = lambda *c: (ctypes.c_float * 3)(*c)

    def call(x=P(xt), N=B, k=k, chunk=0, lat=lat, n=n, coef=C(-1, 1, 1), grad=grad, ng=ng, q=P(o[0]), ph=P(o[1]),
             px=P(o[2])):
        return m._lib.iwae_score_grad(m._h, x, N, k, chunk, lat, n, coef, grad, ng, q, ph, px)
    bad = dict(
        nothing_asked_for=dict(grad=N0, ng=0, q=N0, ph=N0, px=N0),
        coef_null=dict(coef=N0),
        coef_nan=dict(coef=C(0, float("nan"), 1)),
        coef_inf=dict(coef=C(float("inf"), 1, 1)),
        n_lat_not_L=dict(n=1),
        lat_null=dict(lat=N0),
        a_null_latent=dict(lat=one),
        n_grad_not_0_or_L=dict(ng=1),
        grad_null=dict(grad=N0),
        a_null_gradient=dict(grad=gone),
        x_null_with_c_q=dict(x=N0, coef=C(1, 1, 0), q=N0, px=N0),
        x_null_with_c_px=dict(x=N0, coef=C(0, 1, 1), q=N0, px=N0),
        x_null_with_log_q=dict(x=N0, coef=C(0, 1, 0), px=N0),
        x_null_with_log_px=dict(x=N0, coef=C(0, 1, 0), q=N0),
        N_zero=dict(N=0), N_negative=dict(N=-3), k_zero=dict(k=0), k_negative=dict(k=-1),
        k_above_limit=dict(k=(1 << 20) + 1),
        chunk_above_limit=dict(N=4096, k=1 << 20, chunk=2048),
    )
    c0 = _counts(m)
    for what, kw in bad.items():
        assert call(**kw) == -1, what
        assert m._lib.iwae_last_error(m._h), what
    assert _counts(m) == c0                                   # nothing was launched
    assert call() == 0
    assert call(x=N0, coef=C(0, 1, 0), q=N0, px=N0) == 0
    m.check_kernel_status()
    out = m.score_grad(_f32(x), _f32(R.latents(name, "off")), coef=POST)
    tot, scale = G.combine(G.reference(name, "off"), POST)
    assert max(_layer_errors(_np(out["grad"]), tot, scale)) <= BAR


# ---------------------------------------------------------------------- 9. HMC
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", list(G.HMC_CASES))
def test_hmc_follows_the_float64_leapfrog_and_decides_as_it_does(name, path):
    _, _, x, _ = R.case(name)
    step, nl, _ = G.hmc_entry(name)
    r, q, H0, H1, lu, acc = G.hmc_case(name)
    h = _f32(R.latents(name, "on"))
    m = _model(name, path)
    c0 = _counts(m)
    hn, got, rate, lp = m.hmc(_f32(x), h, step, nl, momentum=[_f32(r)], u=np.exp(lu)[None])
    d = [b - a for a, b in zip(c0, _counts(m))]
    assert d[0] + d[1] == nl + 1 and d[4] == 0, d             # one gradient call per leapfrog and the start's
    info = m.hmc_info
    for i, (a, b) in enumerate(zip(_np(info["proposal"]), q)):
        err = np.abs(a - b).max() / np.abs(b).max()
        print(f"[{name} {path}] proposal h_{i + 1}: {err:.2e} of max|ref|")
        assert err <= 1e-4, (i, err)
    g0, g1 = info["h_old"].cpu().numpy().astype(np.float64), info["h_new"].cpu().numpy().astype(np.float64)
    e = np.abs((g1 - g0) - (H1 - H0)) / (np.abs(H0) + np.abs(H1))
    print(f"[{name} {path}] dH: {e.max():.2e} of |H_old| + |H_new|")
    assert e.max() <= 1e-4, e.max()
    got = got.cpu().numpy()
    np.testing.assert_array_equal(got, acc)
    assert got.any() and (~got).any()
    assert rate == pytest.approx(acc.mean(), abs=1e-6)
    for a, p, src in zip(_np(hn), _np(info["proposal"]), h):
        np.testing.assert_array_equal(a[~got], src[~got])     # rejected chains return their input bits
        np.testing.assert_array_equal(a[got], p[got])
    ref_lp = -np.where(acc, H1, H0)                           # log p(x, h) of the returned state: H minus the kinetic term
    kin = 0.5 * sum((v.astype(np.float64) ** 2).sum(-1) for v in _f32(r))
    assert np.abs(lp.cpu().numpy()[~got] - (ref_lp + kin)[~got]).max() <= 1e-4 * np.abs(H0).max()
    m.check_kernel_status()
