"""Pixel masks for scoring, latent gradients, HMC, AIS and refinement
(iwae_score_masked, iwae_score_grad_masked, iwae_ais_masked, iwae_refine_masked;
Flexible_Model.score_observed, score_grad_observed, hmc_observed, ais_observed,
refine_observed) against the float64 reference of tests/observed_ref.py, on the
automatic path (the masked score_kernel / sg_kernel where the unmasked call is
fused) and on the layer-wise path, bf16x3 products.

Bars (the unmasked tests' own).  Values: max|err| <= 1e-4 max|ref| and per row
|err_r| <= 1e-4 S_r, S_r the sum of the absolute values of the term's addends
over the observed pixels (a row with none: exactly 0); probs: PROBS_TOL on every
pixel.  Gradients: relative L2 per layer <= 1e-4, a combined vector relative to
sum_t |c_t| ||g_t||; a layer the reference does not reach exactly zero.  AIS:
test_gpu_ais._compare.  Refinement: test_gpu_refine._compare.  HMC: equal
decisions, states within 1e-4 of max|ref|.  tests/test_observed_ref.py shows the
float32 + bf16x3 emulation within a quarter of each.  The cases' x holds NaN at
the missing pixels throughout."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import iwae_oracle as O
import ais_ref as A
import group_cases as GC
import missing_ref as M
import observed_ref as OB
import refine_ref as RF
import scoregrad_ref as G
from test_gpu_ais import _compare as _compare_ais
from test_gpu_generate import PROBS_TOL
from test_gpu_parity import make_model, weights_from_flat
from test_gpu_refine import ADAM, _compare as _compare_refine, _same as _same_refine
from test_gpu_score import _f32, _model, fresh_group_model

pytestmark = pytest.mark.gpu

BAR = 1e-4
PATHS = ("auto", "layerwise")
CASES = list(OB.CASES)
TERMS = (("log_q", "logq", "Sq"), ("log_ph", "logp", "Sp"), ("log_px", "logpx", "Spx"))
ALL = ("log_q", "log_ph", "log_px", "probs")
GALL = ("grad", "log_q", "log_ph", "log_px")
UNITS = {"q": (1.0, 0.0, 0.0), "ph": (0.0, 1.0, 0.0), "px": (0.0, 0.0, 1.0)}
VALUE = {"q": "log_q", "ph": "log_ph", "px": "log_px"}
POST = (0.0, 1.0, 1.0)
T = len(A.BETAS) - 1
RALL = ("bound", "log_w", "logpx", "ess", "h")
IDS = (31, 32, 33, 34, 23, 24, 25, 26, 0, 3, 27, 28, 29, 30)


@functools.lru_cache(maxsize=None)
def _own(name, path):
    spec, params = OB.case(name)[:2]
    he, hd, le, ld = OB.arch(name)
    m = make_model(he, hd, le, ld, x_dim=spec.x_dim, kernel_path=path, precision="bf16x3", seed=0)
    m.set_weights(weights_from_flat(m, O.flatten_params(spec, params)))
    return m


def _m(name, path):
    """The case's model, built as test_gpu_score._model builds its own (a case on a base of score_ref: that model)."""
    base = OB.CASES[name][0]
    return _model(base, path) if base is not None else _own(name, path)


def _xm(name, fill=np.nan):
    _, _, x, mask, _, x_full = OB.case(name)
    return _f32(x if np.isnan(fill) else M.with_holes(x_full, mask, fill)), _f32(mask)


def _bk(name):
    return OB.CASES[name][2], OB.CASES[name][3]


def _counts(m, ids=IDS):
    return [int(m._lib.iwae_debug_count(m._h, i)) for i in ids]


def _np(ts):
    return [t.cpu().numpy() for t in ts]


def _check_terms(out, ref, label):
    for name, key, sk in TERMS:
        if name not in out:
            continue
        got = out[name].cpu().numpy()
        assert got.shape == ref[key].shape
        err = np.abs(got.astype(np.float64) - ref[key])
        of_max = float(err.max() / np.abs(ref[key]).max())
        live = ref[sk] > 0
        assert (got[~live] == 0.0).all(), (label, name)          # no observed addend: exactly 0
        of_row = float((err[live] / ref[sk][live]).max())
        print(f"{label} {name}: {of_max:.2e} of max|ref|, {of_row:.2e} of S_r")
        assert of_max <= BAR and of_row <= BAR, (label, name, of_max, of_row)


def _layer_errors(got, ref, scale=None):
    out = []
    for i, (a, b) in enumerate(zip(got, ref)):
        assert a.shape == b.shape
        r = G.rel_l2(a, b, None if scale is None else scale[i])
        if r is None:
            assert not a.any(), i                                # a layer the reference does not reach
        else:
            out.append(r)
    return out


def _equal(a, b, what):
    """Two facade results, bit for bit (tensors, lists of tensors, nested state dicts)."""
    assert set(a) == set(b), what
    for n in a:
        u, v = a[n], b[n]
        if isinstance(u, dict):
            _equal(u, v, f"{what} {n}")
        elif isinstance(u, (list, tuple)):
            for p, q in zip(u, v):
                np.testing.assert_array_equal(p.cpu().numpy(), q.cpu().numpy(), err_msg=f"{what} {n}")
        elif hasattr(u, "cpu"):
            np.testing.assert_array_equal(u.cpu().numpy(), v.cpu().numpy(), err_msg=f"{what} {n}")
        else:
            assert u == v, (what, n)


# ----------------------------------------------------------- 1. score parity
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("which", OB.LATENTS)
@pytest.mark.parametrize("name", CASES)
def test_score_parity(name, which, path):
    x, mask = _xm(name)
    h, ref = OB.latents(name, which), OB.reference(name, which)
    m = _m(name, path)
    out = m.score_observed(x, mask, _f32(h), want=ALL)
    _check_terms(out, ref, f"[{name} {which} {path}]")
    lw = out["log_w"].cpu().numpy()
    np.testing.assert_array_equal(lw, ((out["log_ph"] + out["log_px"]) - out["log_q"]).cpu().numpy())
    probs = out["probs"].cpu().numpy()
    assert probs.shape == ref["probs"].shape
    np.testing.assert_allclose(probs, ref["probs"], **PROBS_TOL)          # every pixel, observed or not
    m.check_kernel_status()


# -------------------------------------------------------- 2. gradient parity
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("which", OB.LATENTS)
@pytest.mark.parametrize("name", CASES)
def test_gradient_parity(name, which, path):
    x, mask = _xm(name)
    h = _f32(OB.latents(name, which))
    ref, vref = OB.grad_reference(name, which), OB.reference(name, which)
    m = _m(name, path)
    label = f"[{name} {which} {path}]"
    for t, coef in UNITS.items():
        out = m.score_grad_observed(x, mask, h, coef=coef, want=("grad", VALUE[t]))
        errs = _layer_errors(_np(out["grad"]), ref[t])
        print(f"{label} d{VALUE[t]}/dh: {max(errs):.2e}")
        assert max(errs) <= BAR, (label, t, errs)
        _check_terms(out, vref, label)
    out = m.score_grad_observed(x, mask, h, coef=POST)
    tot, scale = G.combine(ref, POST)
    errs = _layer_errors(_np(out["grad"]), tot, scale)
    print(f"{label} (0, 1, 1): {max(errs):.2e} of sum |c_t| ||g_t||")
    assert max(errs) <= BAR, (label, errs)
    m.check_kernel_status()


# ------------------------------------------------------ 3. all-missing image
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", CASES)
def test_all_missing_image(name, path):
    x, mask = _xm(name)
    assert not mask[0].any() and mask[1].all()
    h = _f32(OB.latents(name, "off"))
    ref, vref = OB.grad_reference(name, "off"), OB.reference(name, "off")
    m = _m(name, path)
    sc = m.score_observed(x, mask, h, want=("log_px",))["log_px"].cpu().numpy()
    out = m.score_grad_observed(x, mask, h, coef=UNITS["px"], want=("grad", "log_px"))
    lpx, g = out["log_px"].cpu().numpy(), _np(out["grad"])
    for v in (sc, lpx):
        assert (v[:, 0] == 0.0).all()
    for a in g:
        assert not a[:, 0].any()                                  # d log p(x|h) / dh of image 0: exactly zero
    # its neighbours within the bars
    assert max(_layer_errors([a[:, 1:] for a in g], [b[:, 1:] for b in ref["px"]])) <= BAR
    _check_terms(out, vref, f"[{name} {path} all-missing]")
    assert np.abs(lpx[:, 1:]).min() > 0


# -------------------------------------------------------- 4. holes never leak
def _ais_run(m, name, init, x, mask, ref, betas=A.BETAS, **kw):
    B, k = _bk(name)
    step, _ = OB.AIS_CASES[name, init]
    n = len(betas) - 1
    kw.setdefault("momentum", [_f32(r) for r in ref["momenta"][:n]])
    kw.setdefault("u", np.exp(ref["log_u"]).astype(np.float32)[:n])
    return m.ais_observed(x, mask, k, betas=betas, init=init, h0=_f32(OB.latents(name, A.START[init])), step_size=step,
                          n_leapfrog=A.N_LEAPFROG, adapt=A.ADAPT, **kw)


def _refine_run(m, name, objective, x, mask, n_iters=RF.T, eps="setting", init=None, **kw):
    _, k = _bk(name)
    m0, s0, e = OB.refine_setting(name)
    want = kw.setdefault("want", RALL)
    if eps == "setting":
        evaluate = any(w != "bound" for w in want)
        eps = [_f32(p) for p in e[:n_iters] + (e[RF.T:] if evaluate else [])]
    return m.refine_observed(x, mask, k, n_iters=n_iters, objective=objective, init=init or (_f32(m0), _f32(s0)), eps=eps,
                             **ADAM, **kw)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", ["OS2", "O50"])
def test_holes_never_leak(name, path):
    m = _m(name, path)
    h = _f32(OB.latents(name, "off"))
    res = []
    for fill in (np.nan, np.inf, 7.0):
        x, mask = _xm(name, fill)
        assert (x[mask == 0] == fill).all() if np.isfinite(fill) else not np.isfinite(x[mask == 0]).any()
        out = {"score": m.score_observed(x, mask, h, want=ALL),
               "grad": m.score_grad_observed(x, mask, h, coef=(-1.0, 1.0, 1.0), want=GALL)}
        if name == "OS2":
            out["ais"] = _ais_run(m, name, "q", x, mask, OB.ais_case(name, "q"))
            out["refine"] = _refine_run(m, name, "IWAE", x, mask)
        res.append(out)
    for other, fill in zip(res[1:], ("+Inf", "7.0")):
        _equal(res[0], other, f"NaN against {fill} at the holes")
    for out in res[0].values():
        for v in out.values():
            for t in (v if isinstance(v, list) else [v]):
                if hasattr(t, "cpu"):
                    assert np.isfinite(t.cpu().numpy()).all()
    m.check_kernel_status()


# ------------------------------------- 5. an all-ones mask is the unmasked entry
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", ["OS2", "OC784"])
def test_all_ones_mask_is_the_unmasked_entry_bit_for_bit(name, path):
    _, _, _, mask, _, x_full = OB.case(name)
    B, k = _bk(name)
    x, ones = _f32(x_full), np.ones_like(_f32(mask))
    m = _m(name, path)
    for which in ("off", "on"):
        h = _f32(OB.latents(name, which))
        _equal(m.score_observed(x, ones, h, want=ALL), m.score(x, h, want=ALL), f"score {which}")
        for coef in ((-1.0, 1.0, 1.0), POST, UNITS["px"]):
            _equal(m.score_grad_observed(x, ones, h, coef=coef, want=GALL), m.score_grad(x, h, coef=coef, want=GALL),
                   f"score_grad {which} {coef}")
    # hmc: injected momenta and u
    h = _f32(OB.latents(name, "on"))
    rng = np.random.default_rng(31)
    r = [[rng.standard_normal(v.shape).astype(np.float32) for v in h] for _ in range(2)]
    u = rng.uniform(0.05, 0.95, (2, k, B)).astype(np.float32)
    a = m.hmc_observed(x, ones, h, 0.2, 3, n_iter=2, momentum=r, u=u)
    b = m.hmc(x, h, 0.2, 3, n_iter=2, momentum=r, u=u)
    for p, q in zip(a[0], b[0]):
        np.testing.assert_array_equal(p.cpu().numpy(), q.cpu().numpy())
    np.testing.assert_array_equal(a[1].cpu().numpy(), b[1].cpu().numpy())
    assert a[2] == b[2]
    np.testing.assert_array_equal(a[3].cpu().numpy(), b[3].cpu().numpy())
    # ais and refine: injected noise
    init = {"OS2": "q", "OC784": "prior"}[name]
    ref = OB.ais_case(name, init)
    step, _ = OB.AIS_CASES[name, init]
    kw = dict(betas=A.BETAS, init=init, h0=_f32(OB.latents(name, A.START[init])), step_size=step, n_leapfrog=A.N_LEAPFROG,
              adapt=A.ADAPT, momentum=[_f32(p) for p in ref["momenta"]], u=np.exp(ref["log_u"]).astype(np.float32))
    _equal(m.ais_observed(x, ones, k, **kw), m.ais(x, k, **kw), "ais")
    m0, s0, e = OB.refine_setting(name)
    kw = dict(n_iters=RF.T, objective="IWAE", init=(_f32(m0), _f32(s0)), eps=[_f32(p) for p in e], want=RALL, **ADAM)
    _equal(m.refine_observed(x, ones, k, **kw), m.refine(x, k, **kw), "refine")
    m.check_kernel_status()


# ------------------------------------------------------ 6. chunk independence
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", ["OK130", "OS3"])
def test_chunks_do_not_change_a_bit(name, path):
    x, mask = _xm(name)
    B, _ = _bk(name)
    h = _f32(OB.latents(name, "off"))
    m = _m(name, path)
    whole = m.score_observed(x, mask, h, want=ALL, chunk=0)
    gwhole = m.score_grad_observed(x, mask, h, coef=(-1.0, 1.0, 1.0), want=GALL, chunk=0)
    for chunk in (1, 2):
        chunks = (B + chunk - 1) // chunk
        c0 = _counts(m)
        out = m.score_observed(x, mask, h, want=ALL, chunk=chunk)
        c1 = _counts(m)
        gout = m.score_grad_observed(x, mask, h, coef=(-1.0, 1.0, 1.0), want=GALL, chunk=chunk)
        c2 = _counts(m)
        assert (c1[0] - c0[0]) + (c1[1] - c0[1]) == chunks and c1[2:] == c0[2:]
        assert (c2[2] - c1[2]) + (c2[3] - c1[3]) == chunks and c2[:2] == c1[:2] and c2[4:] == c1[4:]
        _equal(out, whole, f"score chunk {chunk}")
        _equal(gout, gwhole, f"score_grad chunk {chunk}")


def test_first_layer_groups_of_four_and_three_images():
    """The masked entries under first-layer groups of 4 images, 7 images in
    chunks of 2 (group_cases.py), each on a model that has run nothing: both
    staged copies of x and the first layer's rows come from launches over 4 and
    3 images.  Four masked score_kernel / sg_kernel launches and nothing else;
    within the bars of the parity tests; bit for bit the calls with the default
    group size."""
    name = "O" + GC.GROUP_CASE
    x, mask = _xm(name)
    h = _f32(OB.latents(name, "off"))
    ref, gref = OB.reference(name, "off"), OB.grad_reference(name, "off")
    coef = (-1.0, 1.0, 1.0)
    m = fresh_group_model()
    out, one_group, d = GC.groups_then_one_group(m, IDS, lambda: m.score_observed(x, mask, h, want=ALL, chunk=GC.CHUNK))
    assert d == [4] + [0] * (len(IDS) - 1), d             # chunks [0,2) [2,4) | [4,6) [6,7)
    _check_terms(out, ref, f"[{name} off auto group 4]")
    np.testing.assert_allclose(out["probs"].cpu().numpy(), ref["probs"], **PROBS_TOL)
    _equal(out, one_group, "score, groups of 4")
    m = fresh_group_model()
    gout, gone_group, d = GC.groups_then_one_group(
        m, IDS, lambda: m.score_grad_observed(x, mask, h, coef=coef, want=GALL, chunk=GC.CHUNK))
    assert d == [0, 0, 4] + [0] * (len(IDS) - 3), d
    tot, scale = G.combine(gref, coef)
    errs = _layer_errors(_np(gout["grad"]), tot, scale)
    print(f"[{name} off auto group 4] (-1, 1, 1): {max(errs):.2e} of sum |c_t| ||g_t||")
    assert max(errs) <= BAR, errs
    _check_terms(gout, ref, f"[{name} off auto group 4]")
    _equal(gout, gone_group, "score_grad, groups of 4")


# -------------------------------------------------------------- 7. path taken
@pytest.mark.parametrize("name", CASES)
def test_path_taken(name):
    x, mask = _xm(name)
    x_full = _f32(OB.case(name)[5])
    h = _f32(OB.latents(name, "off"))
    m = _m(name, "auto")
    c0 = _counts(m)
    m.score_observed(x, mask, h)
    c1 = _counts(m)
    m.score_grad_observed(x, mask, h, coef=(-1.0, 1.0, 1.0), want=GALL)
    c2 = _counts(m)
    m.score(x_full, h)
    m.score_grad(x_full, h, coef=(-1.0, 1.0, 1.0), want=GALL)
    c3 = _counts(m)
    d1 = [b - a for a, b in zip(c0, c1)]
    d2 = [b - a for a, b in zip(c1, c2)]
    d3 = [b - a for a, b in zip(c2, c3)]
    assert sorted(d1[:2]) == [0, 1] and not any(d1[2:]), d1       # exactly one of 31 / 32; nothing else moves
    assert sorted(d2[2:4]) == [0, 1] and not any(d2[:2]) and not any(d2[4:]), d2
    assert not any(d3[:4]) and sorted(d3[4:6]) == [0, 1] and sorted(d3[6:8]) == [0, 1], d3
    assert (d1[0] == 1) == (d3[4] == 1), (d1, d3)                 # fused exactly when the unmasked call is
    assert (d2[2] == 1) == (d3[6] == 1), (d2, d3)
    if name in ("OC784", "OK130"):
        assert d1[0] == 1 and d2[2] == 1, (d1, d2)
    lw = _m(name, "layerwise")
    c0 = _counts(lw)
    lw.score_observed(x, mask, h)
    c1 = _counts(lw)
    lw.score_grad_observed(x, mask, h, coef=(-1.0, 1.0, 1.0), want=GALL)
    c2 = _counts(lw)
    assert [b - a for a, b in zip(c0, c1)] == [0, 1] + [0] * (len(IDS) - 2)
    assert [b - a for a, b in zip(c1, c2)] == [0, 0, 0, 1] + [0] * (len(IDS) - 4)


# --------------------------------------------------------------------- 8. AIS
def _dev(m, arrays):
    import torch
    return [torch.as_tensor(np.ascontiguousarray(a, np.float32), device=m.device) for a in arrays]


def _raw_ais(m, x, mask, hs, betas, init, nl, step, adapt, accumulate=0, mom=None, u=None, step_io=None, log_w=None,
             accepts=None, logpx=None, ess=None, chunk=0, **over):
    """iwae_ais_masked through ctypes on device tensors (hs [k, B, d_i] updated in place); returns the code.
    over: x_null, mask_null, betas_null, cfg_null, N, k, lat, n_lat, n_mom, n_temps."""
    import torch
    from iwae_replication_project_amd import _lib
    kk, BB = hs[0].shape[:2]
    bt = np.ascontiguousarray(betas, np.float32)
    c = _lib.IwaeAisConfig(init=init, n_temps=over.get("n_temps", bt.size - 1), n_leapfrog=nl, accumulate=accumulate,
                           step=step, adapt_inc=adapt[0], adapt_dec=adapt[1], step_min=adapt[2], step_max=adapt[3])
    harr, nh = _lib.fptr_array(hs)
    marr, nm = _lib.fptr_array(mom) if mom is not None else (None, 0)
    P = _lib.fptr
    with torch.cuda.stream(m._stream):
        rc = m._lib.iwae_ais_masked(m._h, None if over.get("x_null") else P(x), None if over.get("mask_null") else P(mask),
                                    over.get("N", BB), over.get("k", kk), chunk, over.get("lat", harr),
                                    over.get("n_lat", nh), None if over.get("cfg_null") else ctypes.byref(c),
                                    None if over.get("betas_null") else bt.ctypes.data_as(_lib.FP), marr,
                                    over.get("n_mom", nm), P(u), P(step_io), P(log_w), P(accepts), P(logpx), P(ess))
    m._stream.synchronize()
    return rc


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name,init", list(OB.AIS_CASES))
def test_ais(name, init, path):
    import torch
    x, mask = _xm(name)
    B, k = _bk(name)
    ref = OB.ais_case(name, init)
    m = _m(name, path)
    c0 = _counts(m)
    whole = _ais_run(m, name, init, x, mask, ref)
    d = [b - a for a, b in zip(c0, _counts(m))]
    passes = T * (A.N_LEAPFROG + 1)
    assert d[10] == T and d[11] == passes and d[2] + d[3] == passes and not any(d[4:8]), d     # 27 / 28 as the sibling's
    assert tuple(whole["log_w"].shape) == (k, B) and tuple(whole["logpx"].shape) == (B,)
    h0 = OB.latents(name, A.START[init])
    _compare_ais(whole, ref, h0, T, f"[{name} {init} {path}]")
    assert (ref["accepts"] < T).any() and (ref["accepts"] > 0).any()
    # two calls over a split schedule against one, on the first call's state: injected and device noise
    step, _ = OB.AIS_CASES[name, init]
    xt, mt = _dev(m, [x, mask])                                    # (x with its NaN holes)
    mom_all = [_dev(m, r) for r in ref["momenta"]]
    u_all = torch.as_tensor(np.ascontiguousarray(np.exp(ref["log_u"]).astype(np.float32).transpose(0, 2, 1)),
                            device=m.device)                                                    # [T][B][k]
    for noise in ("injected", "device"):
        res = []
        for split in (False, True):
            m.set_seed(4242)
            hs = _dev(m, h0)
            st = torch.full((B, k), step, device=m.device)
            lw, ac = torch.full((B, k), 9.0, device=m.device), torch.full((B, k), 9.0, device=m.device)
            lp, es = torch.empty(B, device=m.device), torch.empty(B, device=m.device)
            for j, (t0, t1) in enumerate(((0, 2), (2, T)) if split else ((0, T),)):
                kw = {}
                if noise == "injected":
                    kw = dict(mom=[t for r in mom_all[t0:t1] for t in r], u=u_all[t0:t1].contiguous())
                assert _raw_ais(m, xt, mt, hs, A.BETAS[t0:t1 + 1], 0 if init == "prior" else 1, A.N_LEAPFROG, step, A.ADAPT,
                                accumulate=int(j > 0), step_io=st, log_w=lw, accepts=ac, logpx=lp, ess=es, **kw) == 0
            res.append(_np(hs) + _np([st, lw, ac, lp, es]))
        for a, b in zip(*res):
            np.testing.assert_array_equal(a, b, err_msg=f"two calls against one, {noise} noise")
        if noise == "injected":                                      # and both are the facade's result
            for a, b in zip(res[0], _np(whole["h"]) + [whole["step"].t().cpu().numpy(), whole["log_w"].t().cpu().numpy()]):
                np.testing.assert_array_equal(a, b)
    m.check_kernel_status()


# ------------------------------------------------------------------ 9. refine
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name,objective", [("OS2", "ELBO"), ("OS2", "IWAE"), ("OC784", "ELBO")])
def test_refine(name, objective, path):
    import torch
    x, mask = _xm(name)
    B, k = _bk(name)
    ref = OB.refine_case(name, objective)
    m = _m(name, path)
    c0 = _counts(m)
    whole = _refine_run(m, name, objective, x, mask)
    d = [b - a for a, b in zip(c0, _counts(m))]
    assert d[12] == RF.T and d[13] == RF.T + 1 and d[2] + d[3] == RF.T + 1 and not any(d[4:8]), d   # 29 / 30 as the sibling's
    assert tuple(whole["bound"].shape) == (RF.T, B) and tuple(whole["log_w"].shape) == (k, B)
    _compare_refine(whole, ref, f"[{name} {objective} {path}]")
    for a, b in zip(_np(whole["h"]), ref["h"]):
        assert np.abs(a - b).max() <= BAR * np.abs(b).max()
    # continuation with step0: two calls against one, bit for bit
    e = OB.refine_setting(name)[2]
    first = _refine_run(m, name, objective, x, mask, n_iters=2, want=("bound",), eps=[_f32(p) for p in e[:2]])
    assert first["state"]["step"] == 2
    second = _refine_run(m, name, objective, x, mask, n_iters=2, init=(first["mean"], first["logstd"]),
                         state=first["state"], eps=[_f32(p) for p in e[2:]])
    assert second["state"]["step"] == RF.T
    _same_refine(second, whole, "two calls against one")
    both = torch.cat([first["bound"], second["bound"]]).cpu().numpy()
    np.testing.assert_array_equal(both, whole["bound"].cpu().numpy())
    m.check_kernel_status()


# -------------------------------------------------------------------- 10. HMC
@pytest.mark.parametrize("path", PATHS)
def test_hmc(path):
    name = "OS2"
    x, mask = _xm(name)
    step, nl, _ = OB.HMC_CASES[name]
    r, q, H0, H1, lu, acc = OB.hmc_case(name)
    h = _f32(OB.latents(name, "on"))
    m = _m(name, path)
    c0 = _counts(m)
    hn, got, rate, lp = m.hmc_observed(x, mask, h, step, nl, momentum=[_f32(r)], u=np.exp(lu)[None])
    d = [b - a for a, b in zip(c0, _counts(m))]
    assert d[2] + d[3] == nl + 1 and not any(d[4:8]), d           # masked gradient passes only
    got = got.cpu().numpy()
    np.testing.assert_array_equal(got, acc)
    assert got.any() and (~got).any()
    assert rate == pytest.approx(acc.mean(), abs=1e-6)
    for i, (a, b) in enumerate(zip(_np(m.hmc_info["proposal"]), q)):
        err = np.abs(a - b).max() / np.abs(b).max()
        print(f"[{name} {path}] proposal h_{i + 1}: {err:.2e} of max|ref|")
        assert err <= BAR, (i, err)
    for a, p, src in zip(_np(hn), q, h):
        want = np.where(acc[..., None], p, src)
        assert np.abs(a - want).max() <= BAR * np.abs(want).max()
        np.testing.assert_array_equal(a[~got], src[~got])         # rejected chains return their input bits
    m.check_kernel_status()


# ------------------------------------------- 11. the features already built
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", ["OS2", "OS3", "OC784", "O50"])
def test_consistent_with_log_px_observed(name, path):
    x, mask = _xm(name)
    _, k = _bk(name)
    eps = _f32(OB.case(name)[4])
    m = _m(name, path)
    xz = np.where(mask != 0, x, np.float32(0))
    h, _, _ = m.encoder(xz, k, eps=eps)
    lw = m.score_observed(x, mask, h)["log_w"].cpu().numpy().astype(np.float64)
    got = A.finish(lw)[0]
    ref = m.log_px_observed(x, mask, k, eps=eps).cpu().numpy().astype(np.float64)
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"[{name} {path}] logsumexp of the scored weights against log_px_observed: {err:.2e} of max|ref|")
    assert err <= BAR, err


# ----------------------------------------------------------------- 12. errors
@pytest.mark.parametrize("path", PATHS)
def test_invalid_arguments_return_einval_and_launch_nothing(path):
    import torch
    from iwae_replication_project_amd import _lib
    name = "OS2"
    x, mask = _xm(name)
    B, k = _bk(name)
    spec = OB.case(name)[0]
    L = spec.L
    m = _m(name, path)
    dev, xd = m.device, m.x_dim
    xt, mt = _dev(m, [np.nan_to_num(x, nan=0.5)])[0], _dev(m, [mask])[0]
    h0 = OB.latents(name, "on")
    hs = _dev(m, h0)
    gs = [torch.empty_like(t) for t in hs]
    o = [torch.empty(B, k, device=dev) for _ in range(3)]
    pr = torch.empty(B * k * xd + 8, device=dev)
    lat, n = _lib.fptr_array(hs)
    grad, ng = _lib.fptr_array(gs)
    one = (_lib.FP * L)(_lib.fptr(hs[0]), *([None] * (L - 1)))
    gone = (_lib.FP * L)(_lib.fptr(gs[0]), *([None] * (L - 1)))
    nullpp = ctypes.cast(None, _lib.FPP)
    P, N0 = _lib.fptr, None
    C = lambda *c: (ctypes.c_float * 3)(*c)
    nan, inf = float("nan"), float("inf")
    off = ctypes.cast(ctypes.c_void_p(pr.data_ptr() + 4), _lib.FP)
    limits = dict(N_zero=dict(N=0), N_negative=dict(N=-3), k_zero=dict(k=0), k_negative=dict(k=-1),
                  k_above_limit=dict(k=(1 << 20) + 1), chunk_above_limit=dict(N=4096, k=1 << 20, chunk=2048))
    c0 = _counts(m)

    def check(call, bad):
        for what, kw in bad.items():
            assert call(**kw) == -1, what
            assert m._lib.iwae_last_error(m._h), what
            m._stream.synchronize()
        assert _counts(m) == c0, "something was launched"

    # ---- iwae_score_masked
    def score(x=P(xt), mask=P(mt), N=B, k=k, chunk=0, lat=lat, n=n, q=P(o[0]), ph=P(o[1]), px=P(o[2]), probs=N0, ld=0):
        return m._lib.iwae_score_masked(m._h, x, mask, N, k, chunk, lat, n, q, ph, px, probs, ld)
    check(score, dict(
        mask_null=dict(mask=N0), x_null=dict(x=N0), x_null_for_log_ph_alone=dict(x=N0, q=N0, px=N0),
        every_output_null=dict(q=N0, ph=N0, px=N0), n_lat_not_L=dict(n=1), lat_null=dict(lat=N0), a_null_latent=dict(lat=one),
        ld_below_x_dim=dict(probs=P(pr), ld=xd - 4), ld_not_multiple_of_4=dict(probs=P(pr), ld=xd + 2),
        ld_above_limit=dict(probs=P(pr), ld=(1 << 22) + 4), probs_misaligned=dict(probs=off, ld=xd), **limits))

    # ---- iwae_score_grad_masked
    def sgrad(x=P(xt), mask=P(mt), N=B, k=k, chunk=0, lat=lat, n=n, coef=C(-1, 1, 1), grad=grad, ng=ng, q=P(o[0]),
              ph=P(o[1]), px=P(o[2])):
        return m._lib.iwae_score_grad_masked(m._h, x, mask, N, k, chunk, lat, n, coef, grad, ng, q, ph, px)
    check(sgrad, dict(
        mask_null=dict(mask=N0), x_null=dict(x=N0), x_null_where_the_sibling_needs_none=dict(x=N0, coef=C(0, 1, 0), q=N0, px=N0),
        nothing_asked_for=dict(grad=N0, ng=0, q=N0, ph=N0, px=N0), coef_null=dict(coef=N0),
        coef_nan=dict(coef=C(0, nan, 1)), coef_inf=dict(coef=C(inf, 1, 1)), n_lat_not_L=dict(n=1), lat_null=dict(lat=N0),
        a_null_latent=dict(lat=one), n_grad_not_0_or_L=dict(ng=1), grad_null=dict(grad=N0), a_null_gradient=dict(grad=gone),
        **limits))

    # ---- iwae_ais_masked
    ref = OB.ais_case(name, "q")
    mom = [t for r in ref["momenta"] for t in _dev(m, r)]
    mnull = list(mom)
    mnull[3] = None
    ok = dict(betas=A.BETAS, init=1, nl=2, step=0.1, adapt=A.ADAPT)
    check(lambda **kw: _raw_ais(m, xt, mt, hs, **{**ok, **kw}), dict(
        mask_null=dict(mask_null=True), x_null=dict(x_null=True), cfg_null=dict(cfg_null=True),
        betas_null=dict(betas_null=True), lat_null=dict(lat=nullpp), a_null_latent=dict(lat=one), n_lat_not_L=dict(n_lat=L - 1),
        n_mom_not_0_or_TL=dict(mom=mom[:-1]), n_mom_without_buffers=dict(n_mom=T * L), a_null_momentum=dict(mom=mnull),
        init_2=dict(init=2), init_negative=dict(init=-1), no_transition=dict(n_temps=0), T_negative=dict(n_temps=-1),
        T_above_limit=dict(n_temps=(1 << 24) + 1), no_leapfrog=dict(nl=0), beta_nan=dict(betas=(0.0, nan, 1.0)),
        beta_inf=dict(betas=(0.0, inf)), beta_above_1=dict(betas=(0.0, 1.5)), beta_negative=dict(betas=(-0.1, 1.0)),
        step_zero=dict(step=0.0), step_negative=dict(step=-0.1), step_nan=dict(step=nan), step_inf=dict(step=inf),
        inc_zero=dict(adapt=(0.0, 0.5, 0.01, 2.0)), dec_negative=dict(adapt=(1.25, -0.5, 0.01, 2.0)),
        inc_nan=dict(adapt=(nan, 0.5, 0.01, 2.0)), min_above_max=dict(adapt=(1.25, 0.5, 2.0, 0.01)),
        chains_above_limit=dict(N=2048, k=1 << 20, chunk=1), **limits))
    for a, b in zip(_np(hs), h0):
        np.testing.assert_array_equal(a, _f32(b))                  # state untouched

    # ---- iwae_refine_masked
    m0, s0, e = OB.refine_setting(name)
    mean, logstd = _dev(m, m0), _dev(m, s0)
    eps2 = [t for p in e[:2] for t in _dev(m, p)]
    adam = [torch.zeros(B, d, device=dev) for d in spec.n_latent_encoder for _ in range(4)]
    lo = [torch.empty(k, B, d, device=dev) for d in spec.n_latent_encoder]
    lp = torch.empty(B, device=dev)
    mone = (_lib.FP * L)(_lib.fptr(mean[0]), *([None] * (L - 1)))

    def refine(x=P(xt), mask=P(mt), N=B, k=k, chunk=0, mean_arr=None, logstd_arr=None, n_par=L, cfg=True, objective=0,
               n_iters=2, step0=0, lr=0.05, beta1=0.9, beta2=0.999, epsilon=1e-3, ls_min=-12.0, ls_max=4.0, eps=None,
               n_eps=None, adam=None, n_adam=None, lat_out=None, n_lat=None, logpx=None):
        c = _lib.IwaeRefineConfig(objective=objective, n_iters=n_iters, step0=step0, lr=lr, beta1=beta1, beta2=beta2,
                                  epsilon=epsilon, logstd_min=ls_min, logstd_max=ls_max)
        marr, _ = _lib.fptr_array(mean)
        sarr, _ = _lib.fptr_array(logstd)
        earr, ne = _lib.fptr_array(eps) if eps is not None else (None, 0)
        aarr, na = _lib.fptr_array(adam) if adam is not None else (None, 0)
        harr, nh = _lib.fptr_array(lat_out) if lat_out is not None else (None, 0)
        with torch.cuda.stream(m._stream):
            return m._lib.iwae_refine_masked(m._h, x, mask, N, k, chunk, marr if mean_arr is None else mean_arr,
                                             sarr if logstd_arr is None else logstd_arr, n_par,
                                             ctypes.byref(c) if cfg else None, earr, ne if n_eps is None else n_eps, aarr,
                                             na if n_adam is None else n_adam, None, harr, nh if n_lat is None else n_lat,
                                             None, P(logpx), None)
    check(refine, dict(
        mask_null=dict(mask=N0), x_null=dict(x=N0), cfg_null=dict(cfg=False), mean_null=dict(mean_arr=nullpp),
        logstd_null=dict(logstd_arr=nullpp), a_null_mean=dict(mean_arr=mone), a_null_logstd=dict(logstd_arr=mone),
        n_par_not_L=dict(n_par=L - 1), n_eps_not_0_or_PL=dict(eps=eps2[:-1]), n_eps_without_buffers=dict(n_eps=2 * L),
        n_eps_misses_the_evaluation=dict(eps=eps2, logpx=lp), a_null_eps=dict(eps=eps2[:1] + [None] + eps2[2:]),
        n_adam_not_0_or_4L=dict(adam=adam[:-1]), n_adam_without_buffers=dict(n_adam=4 * L),
        a_null_adam=dict(adam=adam[:2] + [None] + adam[3:]), n_lat_not_0_or_L=dict(lat_out=lo[:-1]),
        n_lat_without_buffers=dict(n_lat=L), a_null_sample_buffer=dict(lat_out=[None] + lo[1:]),
        objective_2=dict(objective=2), objective_negative=dict(objective=-1), n_iters_negative=dict(n_iters=-1),
        n_iters_above_limit=dict(n_iters=(1 << 24) + 1), step0_negative=dict(step0=-1, adam=adam),
        step0_without_adam=dict(step0=3), nothing_to_do=dict(n_iters=0), lr_zero=dict(lr=0.0), lr_negative=dict(lr=-0.1),
        lr_nan=dict(lr=nan), lr_inf=dict(lr=inf), epsilon_zero=dict(epsilon=0.0), epsilon_nan=dict(epsilon=nan),
        epsilon_inf=dict(epsilon=inf), beta1_one=dict(beta1=1.0), beta1_negative=dict(beta1=-0.1), beta2_one=dict(beta2=1.0),
        beta2_nan=dict(beta2=nan), min_above_max=dict(ls_min=1.0, ls_max=0.0), min_nan=dict(ls_min=nan),
        max_inf=dict(ls_max=inf), rows_above_limit=dict(N=2048, k=1 << 20, chunk=1), **limits))
    for a, b in zip(_np(mean) + _np(logstd), list(m0) + list(s0)):
        np.testing.assert_array_equal(a, _f32(b))                  # parameters untouched

    # ---- the handle stays usable: each entry runs
    assert score() == 0 and sgrad() == 0 and _raw_ais(m, xt, mt, hs, **ok) == 0 and refine(eps=eps2) == 0
    m._stream.synchronize()
    m.check_kernel_status()


def test_facade_raises_value_error():
    name = "OS2"
    x, mask = _xm(name)
    B, k = _bk(name)
    h = _f32(OB.latents(name, "off"))
    m = _m(name, "auto")
    c0 = _counts(m)
    calls = {
        "score_observed": lambda x, mask: m.score_observed(x, mask, h),
        "score_grad_observed": lambda x, mask: m.score_grad_observed(x, mask, h),
        "hmc_observed": lambda x, mask: m.hmc_observed(x, mask, h, 0.1, 2),
        "ais_observed": lambda x, mask: m.ais_observed(x, mask, k, betas=(0.0, 1.0), h0=h),
        "refine_observed": lambda x, mask: m.refine_observed(x, mask, k, n_iters=1),
    }
    for what, f in calls.items():
        for bad in (None, mask[:-1], mask[:, :-1], np.ones(B, np.float32)):
            with pytest.raises(ValueError):
                f(x, bad)
        with pytest.raises(ValueError):
            f(x[:, :-1], mask)
    for f in (calls["score_observed"], calls["score_grad_observed"]):
        with pytest.raises(ValueError):
            f(None, mask)
    with pytest.raises(ValueError):
        m.score_observed(x, mask, h, want=("weights",))
    with pytest.raises(ValueError):
        m.score_grad_observed(x, mask, h, coef=(1.0, 1.0))
    assert _counts(m) == c0
