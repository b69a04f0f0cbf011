"""The latent-space entry points (iwae_score, iwae_score_grad and the facade's
hmc, iwae_ais, iwae_refine, and the _masked siblings) on the shapes of
tests/latent_shape_cases.py, at the edges of mega_plan and sgrad_plan: odd and
minimal widths, x_dim off 4 and a second pixel slab of 3 pixels, 4 dY2 column
tiles per wave, both sides of the 32-tile limit, all three row tiles, the
deepest fused plan and the layer-wise fall-back to IWAE_MAX_LAYERS, d = 1, d >
256, both sides of the chain-group switch.  Automatic and layer-wise paths,
bf16x3 products.

Bars: the existing files' own, by import (test_gpu_score._check_terms and
PROBS_TOL, test_gpu_scoregrad._layer_errors at 1e-4, test_gpu_ais._compare,
test_gpu_refine._compare, test_gpu_observed._check_terms); no case needs SH's
emulation rule (tests/test_latent_shape_cases.py shows float32 and the bf16x3
emulation within a quarter of each).  Every counter assertion is
latent_shape_cases.expected()'s, never observed behaviour.  DESIGN.md s9 has
the measured ratios and the mutations these tests were checked against."""
import numpy as np
import pytest

import ais_ref as A
import latent_shape_cases as LS
import observed_ref as OB
import refine_ref as RF
import score_ref as R
import scoregrad_ref as G
import test_gpu_ais as TA
import test_gpu_observed as TO
import test_gpu_refine as TR
import test_gpu_scoregrad as TG
from test_gpu_generate import PROBS_TOL
from test_gpu_score import ALL, _check_terms, _f32, _model
from test_gpu_scoregrad import POST, UNITS, VALUE, _layer_errors, _np

pytestmark = pytest.mark.gpu

BAR = 1e-4
PATHS = ("auto", "layerwise")
GALL = ("grad", "log_q", "log_ph", "log_px")
IDS = (23, 24, 25, 26, 31, 32, 33, 34, 3)      # score fused / layer-wise, score_grad, their masked siblings; the ring


def _counts(m):
    return [int(m._lib.iwae_debug_count(m._h, i)) for i in IDS]


def _delta(m, c0):
    return [b - a for a, b in zip(c0, _counts(m))]


def _pair(fused, n=1):
    return [n, 0] if fused else [0, n]


# ------------------------------------------------------------------- 1. score
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("which", R.LATENTS)
@pytest.mark.parametrize("name", LS.SCORE_CASES)
def test_score(name, which, path):
    _, _, x, _ = R.case(name)
    h, ref = R.latents(name, which), R.reference(name, which)
    m = _model(name, path)
    c0 = _counts(m)
    out = m.score(_f32(x), _f32(h), want=ALL)
    d = _delta(m, c0)
    assert d[:2] == _pair(LS.expected(name, path=path)["score_fused"]) and not any(d[2:]), d
    _check_terms(out, ref, f"[{name} {which} {path}]")
    np.testing.assert_array_equal(out["log_w"].cpu().numpy(), ((out["log_ph"] + out["log_px"]) - out["log_q"]).cpu().numpy())
    probs = out["probs"].cpu().numpy()
    assert probs.shape == ref["probs"].shape
    np.testing.assert_allclose(probs, ref["probs"], **PROBS_TOL)
    m.check_kernel_status()


# -------------------------------------------------------------- 2. score_grad
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("which", R.LATENTS)
@pytest.mark.parametrize("name", LS.SCORE_CASES)
def test_score_grad(name, which, path):
    _, _, x, _ = R.case(name)
    h, ref, vref = R.latents(name, which), G.reference(name, which), R.reference(name, which)
    m = _model(name, path)
    label = f"[{name} {which} {path}]"
    for t, coef in UNITS.items():
        c0 = _counts(m)
        out = m.score_grad(_f32(x), _f32(h), coef=coef, want=("grad", VALUE[t]))
        d = _delta(m, c0)
        assert d[2:4] == _pair(LS.expected(name, coef=coef, path=path, values=(t,))["sgrad_fused"]), (t, d)
        assert not any(d[:2]) and not any(d[4:]), d
        errs = _layer_errors(_np(out["grad"]), ref[t])
        if errs:                                              # (one layer: log p(h) alone reaches h_1 by -h_1 only)
            print(f"{label} d{VALUE[t]}/dh: {max(errs):.2e} (bar {BAR:.2e})")
            assert max(errs) <= BAR, (label, t, errs)
        _check_terms(out, vref, label)
    c0 = _counts(m)
    out = m.score_grad(_f32(x), _f32(h), coef=POST)
    assert _delta(m, c0)[2:4] == _pair(LS.expected(name, coef=POST, path=path)["sgrad_fused"])
    tot, scale = G.combine(ref, POST)
    errs = _layer_errors(_np(out["grad"]), tot, scale)
    print(f"{label} (0, 1, 1): {max(errs):.2e} of sum |c_t| ||g_t|| (bar {BAR:.2e})")
    assert max(errs) <= BAR, (label, errs)
    m.check_kernel_status()


# -------------------------------------------------------------- 3. path taken
@pytest.mark.parametrize("name", LS.SCORE_CASES)
def test_path_taken(name):
    _, _, x, _ = R.case(name)
    h = _f32(R.latents(name, "off"))
    for path in PATHS:
        m = _model(name, path)
        # every output of score_grad with every gradient term: the longest stage list
        e = LS.expected(name, coef=(-1.0, 1.0, 1.0), path=path, values=G.TERMS)
        c0 = _counts(m)
        m.score_grad(_f32(x), h, coef=(-1.0, 1.0, 1.0), want=GALL)
        d = _delta(m, c0)
        assert d[2:4] == _pair(e["sgrad_fused"]) and not any(d[:2]) and not any(d[4:]), (path, d, e)
        # values alone (no gradient buffer): the forward stages only
        e = LS.expected(name, grads=False, path=path, values=G.TERMS)
        c0 = _counts(m)
        m.score_grad(_f32(x), h, want=GALL[1:])
        d = _delta(m, c0)
        assert d[2:4] == _pair(e["sgrad_fused"]), (path, d, e)
        # a zero coefficient whose value is asked for runs forward only
        e = LS.expected(name, coef=(0.0, 1.0, 0.0), path=path, values=("px",))
        c0 = _counts(m)
        m.score_grad(_f32(x), h, coef=(0.0, 1.0, 0.0), want=("grad", "log_px"))
        assert _delta(m, c0)[2:4] == _pair(e["sgrad_fused"]), (path, e)


# --------------------------------------------------------- 4. masked siblings
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("which", R.LATENTS)
@pytest.mark.parametrize("name", LS.MASKED)
def test_masked(name, which, path):
    oname = "O" + name
    x, mask = TO._xm(oname)
    h = _f32(OB.latents(oname, which))
    ref, gref = OB.reference(oname, which), OB.grad_reference(oname, which)
    m = _model(name, path)
    label = f"[{oname} {which} {path}]"
    c0 = _counts(m)
    out = m.score_observed(x, mask, h, want=ALL)
    d = _delta(m, c0)
    assert d[4:6] == _pair(LS.expected(name, path=path)["score_fused"]) and not any(d[:4]) and not any(d[6:]), d
    TO._check_terms(out, ref, label)                          # a row without an observed pixel: exactly 0
    np.testing.assert_allclose(out["probs"].cpu().numpy(), ref["probs"], **PROBS_TOL)
    for t, coef in UNITS.items():
        c0 = _counts(m)
        out = m.score_grad_observed(x, mask, h, coef=coef, want=("grad", VALUE[t]))
        d = _delta(m, c0)
        assert d[6:8] == _pair(LS.expected(name, coef=coef, path=path, values=(t,))["sgrad_fused"]), (t, d)
        assert not any(d[:6]) and not d[8], d
        errs = TO._layer_errors(_np(out["grad"]), gref[t])
        if errs:
            print(f"{label} d{VALUE[t]}/dh: {max(errs):.2e}")
            assert max(errs) <= BAR, (label, t, errs)
        TO._check_terms(out, ref, label)
        if t == "px":                                         # image 0 has no observed pixel
            assert all(not a[:, 0].any() for a in _np(out["grad"]))
            assert (out["log_px"].cpu().numpy()[:, 0] == 0.0).all()
    out = m.score_grad_observed(x, mask, h, coef=POST)
    tot, scale = G.combine(gref, POST)
    errs = TO._layer_errors(_np(out["grad"]), tot, scale)
    print(f"{label} (0, 1, 1): {max(errs):.2e} of sum |c_t| ||g_t||")
    assert max(errs) <= BAR, (label, errs)
    m.check_kernel_status()


# --------------------------------------------------------------------- 5. HMC
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", list(LS.HMC_CASES))
def test_hmc(name, path):
    m = _model(name, path)
    c0 = _counts(m)
    TG.test_hmc_follows_the_float64_leapfrog_and_decides_as_it_does(name, path)
    nl = LS.HMC_CASES[name][1]
    assert _delta(m, c0)[2:4] == _pair(LS.expected(name, coef=POST, path=path, values=("ph", "px"))["sgrad_fused"], nl + 1)


# --------------------------------------------------------------------- 6. AIS
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name,init", list(LS.AIS_CASES))
def test_ais(name, init, path):
    m = _model(name, path)
    c0 = _counts(m)
    TA.test_parity(name, init, path)
    values = G.TERMS if init == "q" else ("ph", "px")
    fused = [LS.expected(name, coef=A.coefs(init, b), path=path, values=values)["sgrad_fused"] for b in A.BETAS[1:]]
    n = A.N_LEAPFROG + 1
    assert _delta(m, c0)[2:4] == [n * sum(fused), n * (len(fused) - sum(fused))]


# ------------------------------------------------------------------ 7. refine
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("objective", RF.OBJECTIVES)
@pytest.mark.parametrize("name", LS.REFINE_CASES)
def test_refine(name, objective, path):
    m = _model(name, path)
    c0 = _counts(m)
    TR.test_parity(name, objective, path)
    d = _delta(m, c0)
    # (T + 1 passes of the full run, one of the one-iteration run; gradient passes and the evaluation fuse alike)
    e = [LS.expected(name, coef=POST, grads=g, path=path, values=("ph", "px"))["sgrad_fused"] for g in (True, False)]
    assert d[2:4] == [(RF.T + 1) * e[0] + e[1], (RF.T + 1) * (not e[0]) + (not e[1])], d
    if max(R.case(name)[0].n_latent_encoder) <= LS.kCols:
        return
    # the second round of kCols columns: moved, and at the reference
    ref = RF.refine_case(name, objective)
    m0, s0, _ = RF.setting(name)
    out = TR._run(m, name, objective)
    for n, start in (("mean", m0), ("logstd", s0)):
        got, want = out[n][0].cpu().numpy()[:, LS.kCols:], ref[n][0][:, LS.kCols:]
        assert got.shape[1] > 0 and (np.abs(got - _f32(start[0])[:, LS.kCols:]) > 1e-2).all(), n
        err = np.abs(got - want).max() / np.abs(want).max()
        print(f"[{name} {objective} {path}] {n} columns >= {LS.kCols}: {err:.2e} of max|ref|")
        assert err <= BAR, (n, err)


# ---------------------------------------------------------------- 8. chunking
@pytest.mark.parametrize("path", PATHS)
def test_chunks_do_not_change_a_bit(path):
    name, chunk = LS.CHUNK_CASE, LS.CHUNK
    _, _, x, _ = R.case(name)
    B = R.entry(name)[1]
    chunks = -(-B // chunk)
    assert B % chunk                                          # a ragged last chunk
    h = _f32(R.latents(name, "off"))
    m = _model(name, path)
    coef = (-1.0, 1.0, 1.0)
    whole = m.score(_f32(x), h, want=ALL, chunk=B)
    gwhole = m.score_grad(_f32(x), h, coef=coef, want=GALL, chunk=B)
    c0 = _counts(m)
    out = m.score(_f32(x), h, want=ALL, chunk=chunk)
    d = _delta(m, c0)
    assert d[:2] == _pair(LS.expected(name, path=path)["score_fused"], chunks), d
    c0 = _counts(m)
    gout = m.score_grad(_f32(x), h, coef=coef, want=GALL, chunk=chunk)
    d = _delta(m, c0)
    assert d[2:4] == _pair(LS.expected(name, coef=coef, path=path, values=G.TERMS)["sgrad_fused"], chunks), d
    for n in whole:
        np.testing.assert_array_equal(out[n].cpu().numpy(), whole[n].cpu().numpy(), err_msg=f"score {n}")
    for u, v in zip(_np(gout["grad"]), _np(gwhole["grad"])):
        np.testing.assert_array_equal(u, v, err_msg="grad")
    for n in GALL[1:]:
        np.testing.assert_array_equal(gout[n].cpu().numpy(), gwhole[n].cpu().numpy(), err_msg=f"score_grad {n}")
    m.check_kernel_status()
