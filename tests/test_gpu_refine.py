"""Per-image variational refinement on the device (iwae_refine;
Flexible_Model.refine) against the float64 reference of tests/refine_ref.py, on
the automatic path of these cases (the fused sg_kernel) and on the layer-wise
path.

Bars.  mean and logstd per layer, the bound trace and the evaluation's log_w
each within 1e-4 of max|ref|: the project's bar, as test_gpu_ais.py uses it;
tests/test_refine_ref.py shows the float32 + bf16x3 emulation within a quarter
of it.  logpx and ess against float64 formulas on the device's own log_w at 1e-5
relative, so the reduction is tested apart from the run.  After a one-iteration
call adam[..] / (1 - beta1) is the gradient itself: relative L2 error against
test_gpu_scoregrad's combined-gradient scale carried through the sum over
samples (refine_ref.objective_and_grads) at 1e-4.  test_parity prints the worst
figures (DESIGN.md s9 has the table)."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import iwae_oracle as O
import ais_ref as A
import refine_ref as F
import score_ref as R
from test_gpu_parity import make_model, weights_from_flat
from test_gpu_score import _f32, _model

pytestmark = pytest.mark.gpu

BAR = 1e-4
PATHS = ("auto", "layerwise")
T = F.T
ADAM = dict(lr=F.LR, betas=F.BETAS, epsilon=F.EPS_HAT, logstd_range=F.LS_RANGE)
ALL = ("bound", "log_w", "logpx", "ess", "h")


@functools.lru_cache(maxsize=None)
def _own(name, path):
    spec, params = F.case(name)[:2]
    he, hd, le, ld = F.arch(name)
    m = make_model(he, hd, le, ld, x_dim=spec.x_dim, kernel_path=path, precision="bf16x3", seed=0)
    m.set_weights(weights_from_flat(m, O.flatten_params(spec, params)))
    return m


def _m(name, path):
    return _own(name, path) if name in F.OWN else _model(name, path)


def _counts(m, ids=(29, 30, 25, 26)):
    return [int(m._lib.iwae_debug_count(m._h, i)) for i in ids]


def _np(ts):
    return [t.cpu().numpy() for t in ts]


def _run(m, name, objective, n_iters=T, eps="setting", init=None, **kw):
    """The facade on the fixed setting: injected noise of passes 0 .. n_iters - 1 and, evaluating, pass T's."""
    _, _, x, _, k = F.case(name)
    m0, s0, e = F.setting(name)
    want = kw.setdefault("want", ALL)
    if eps == "setting":
        evaluate = any(w != "bound" for w in want)
        eps = [_f32(p) for p in e[:n_iters] + (e[T:] if evaluate else [])]
    return m.refine(_f32(x), k, n_iters=n_iters, objective=objective, init=init or (_f32(m0), _f32(s0)), eps=eps,
                    **ADAM, **kw)


def _of_max(got, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max())


def _compare(out, ref, label):
    """The device's run against the reference's: parameters, bound trace, weights, the reduction."""
    fig = {"mean": max(_of_max(a, b) for a, b in zip(_np(out["mean"]), ref["mean"])),
           "logstd": max(_of_max(a, b) for a, b in zip(_np(out["logstd"]), ref["logstd"])),
           "bound": _of_max(out["bound"].cpu().numpy(), ref["bound"]),
           "log_w": _of_max(out["log_w"].cpu().numpy(), ref["log_w"])}
    lw = out["log_w"].cpu().numpy().astype(np.float64)
    lp, ess = A.finish(lw)
    ep = np.abs(out["logpx"].cpu().numpy() - lp).max() / np.abs(lp).max()
    ee = (np.abs(out["ess"].cpu().numpy() - ess) / ess).max()
    print(f"{label} " + ", ".join(f"{n} {v:.2e}" for n, v in fig.items()) + f" of max|ref|; logpx {ep:.2e}, ess {ee:.2e} relative")
    for n, v in fig.items():
        assert v <= BAR, (label, n, v)
    assert ep <= 1e-5 and ee <= 1e-5, (label, ep, ee)
    return fig


# ------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("objective", F.OBJECTIVES)
@pytest.mark.parametrize("name", F.SHAPES + F.EXTRA)
def test_parity(name, objective, path):
    ref = F.refine_case(name, objective)
    spec, _, _, B, k = F.case(name)
    m = _m(name, path)
    out = _run(m, name, objective)
    assert tuple(out["bound"].shape) == (T, B) and tuple(out["log_w"].shape) == (k, B)
    assert tuple(out["logpx"].shape) == (B,) and tuple(out["ess"].shape) == (B,)
    assert [tuple(t.shape) for t in out["h"]] == [(k, B, d) for d in spec.n_latent_encoder]
    assert out["state"]["step"] == T
    label = f"[{name} {objective} {path}]"
    _compare(out, ref, label)
    for a, b in zip(_np(out["h"]), ref["h"]):                  # the evaluation's samples
        assert _of_max(a, b) <= BAR
    # one iteration: the first moments are (1 - beta1) G
    one = _run(m, name, objective, n_iters=1, want=("bound",))
    omb1 = float(np.float32(1) - np.float32(F.BETAS[0]))
    ad = _np(one["state"]["adam"])
    Gm = [ad[4 * i].astype(np.float64) / omb1 for i in range(spec.L)]
    Gl = [ad[4 * i + 2].astype(np.float64) / omb1 for i in range(spec.L)]
    eg = F.grad_errors(Gm, Gl, ref)
    print(f"{label} first-step gradients {eg:.2e} of the carried combined-gradient scale")
    assert eg <= BAR, (label, eg)
    np.testing.assert_array_equal(one["bound"].cpu().numpy()[0], out["bound"].cpu().numpy()[0])
    m.check_kernel_status()


# ---------------------------------------------------------------- 2. counters
@pytest.mark.parametrize("path", PATHS)
def test_counters(path):
    name = "S2"
    B = F.case(name)[3]
    m = _m(name, path)
    for chunk, chunks in ((0, 1), (2, (B + 1) // 2)):
        for want, P in ((ALL, T + 1), (("bound",), T)):
            c0 = _counts(m)
            _run(m, name, "ELBO", chunk=chunk, want=want)
            d = [b - a for a, b in zip(c0, _counts(m))]
            assert d[0] == T and d[1] == T + 1, d
            assert d[2] + d[3] == P * chunks, d
            assert (d[3] == 0) if path == "auto" else (d[2] == 0), d
    c0 = _counts(m)
    _run(m, name, "ELBO", n_iters=0)                          # evaluation only: the begin launch, one scoring pass
    assert [b - a for a, b in zip(c0, _counts(m))][:2] == [0, 1]


# ------------------------------------------------------------ 3. continuation
def _same(a, b, what, keys=("log_w", "logpx", "ess")):
    for n in ("mean", "logstd", "h"):
        for u, v in zip(_np(a[n]), _np(b[n])):
            np.testing.assert_array_equal(u, v, err_msg=f"{what} {n}")
    for u, v in zip(_np(a["state"]["adam"]), _np(b["state"]["adam"])):
        np.testing.assert_array_equal(u, v, err_msg=f"{what} adam")
    for n in keys:
        np.testing.assert_array_equal(a[n].cpu().numpy(), b[n].cpu().numpy(), err_msg=f"{what} {n}")


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name,objective", [("S2", "IWAE"), ("S4", "ELBO")])
def test_two_calls_continue_as_one(name, objective, path):
    import torch
    m = _m(name, path)
    e = F.setting(name)[2]
    for noise in ("injected", "device"):
        m.set_seed(4242)
        whole = _run(m, name, objective, **({} if noise == "injected" else dict(eps=None)))
        m.set_seed(4242)
        first = _run(m, name, objective, n_iters=2, want=("bound",),
                     eps=[_f32(p) for p in e[:2]] if noise == "injected" else None)
        assert first["state"]["step"] == 2
        second = _run(m, name, objective, n_iters=2, init=(first["mean"], first["logstd"]), state=first["state"],
                      eps=[_f32(p) for p in e[2:]] if noise == "injected" else None)
        assert second["state"]["step"] == T
        _same(second, whole, f"two calls against one, {noise} noise")
        both = torch.cat([first["bound"], second["bound"]]).cpu().numpy()
        np.testing.assert_array_equal(both, whole["bound"].cpu().numpy())
    m.check_kernel_status()


# ------------------------------------------------------------ 4. bit-exactness
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name,objective", [("S2", "ELBO"), ("C784", "IWAE"), ("K300", "IWAE"), ("K1100", "IWAE")])
def test_bit_exactness(name, objective, path):
    m = _m(name, path)
    whole = _run(m, name, objective)
    _same(whole, _run(m, name, objective), "the same call twice", keys=("bound", "log_w", "logpx", "ess"))
    _same(whole, _run(m, name, objective, chunk=1), "chunk 1", keys=("bound", "log_w", "logpx", "ess"))
    m.check_kernel_status()


# ------------------------------------------------------------- 5. device noise
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name,objective", [("S2", "ELBO"), ("S4", "IWAE")])
def test_device_noise(name, objective, path):
    seed, n = 6101, 2
    m = _m(name, path)
    m.set_seed(seed)
    for call in range(2):                                      # the second call draws at bases P ..
        ref = F.noise_case(name, objective, seed, call * (n + 1), n)
        out = _run(m, name, objective, n_iters=n, eps=None)
        _compare(out, ref, f"[{name} {objective} {path} device noise, call {call}]")
        for a, b in zip(_np(out["h"]), ref["h"]):
            assert _of_max(a, b) <= BAR
    m.check_kernel_status()


# ------------------------------------------------- 6. meets the existing code
@pytest.mark.parametrize("path", PATHS)
def test_encoder_init_without_iterations_is_the_nll_estimate(path):
    name = "S1"
    _, _, x, B, k = F.case(name)
    e = F.setting(name)[2][T]
    m = _m(name, path)
    out = m.refine(_f32(x), k, n_iters=0, init="encoder", eps=[_f32(e)], want=("logpx", "log_w"))
    want = m.log_px(_f32(x), k, eps=_f32(e)).cpu().numpy()
    got = out["logpx"].cpu().numpy()
    assert np.abs(got - want).max() <= BAR * np.abs(want).max(), (got, want)
    assert out["state"]["step"] == 0
    m.check_kernel_status()


@pytest.mark.parametrize("name", ["S1", "S3"])
def test_encoder_init_is_the_encoders_mean_chain(name):
    spec, params, x, B, k = F.case(name)
    m = _m(name, "auto")
    out = m.refine(_f32(x), k, n_iters=0, init="encoder", want=("logpx",))
    X = x
    for i, (mu, ls) in enumerate(zip(_np(out["mean"]), _np(out["logstd"]))):
        q = O._stoch_forward(params, f"enc{i}", X)
        assert _of_max(mu, q["mu"]) <= BAR and _of_max(np.exp(ls.astype(np.float64)), q["scale"]) <= BAR, i
        X = q["mu"]


# -------------------------------------------------------------------- 7. state
def test_refine_leaves_the_training_state_alone():
    from iwae_replication_project_amd import Adam
    he, hd, le, ld = R.CASES["C784"][0]
    rng = np.random.default_rng(5)
    x = (rng.random((40, 784)) < 0.3).astype(np.float32)
    k, n = 17, 3
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
    init = ([np.zeros((5, le[0]), np.float32)], [np.full((5, le[0]), -1.0, np.float32)])
    out = a.refine(x[:5], k, n_iters=n, init=init)            # device noise; n + 1 passes
    assert np.isfinite(out["logpx"].cpu().numpy()).all() and tuple(out["log_w"].shape) == (k, 5)
    w1, (m1, v1, t1) = a.get_weights(), a.get_optimizer_state()
    for p, q in zip(w0, w1):
        np.testing.assert_array_equal(p, q)
    np.testing.assert_array_equal(m0, m1)
    np.testing.assert_array_equal(v0, v1)
    assert t0 == t1 and a.graph_captures() == g0
    for _ in range(n + 1):                                 # the position moved by n + 1: the other model draws as often
        b.get_log_weights(x[:5], k)
    np.testing.assert_array_equal(a.get_log_weights(x[:5], k).cpu().numpy(), b.get_log_weights(x[:5], k).cpu().numpy())
    la, lb = a.train_steps(x, 20), b.train_steps(x, 20)
    assert a.graph_captures() == g0                        # replayed, not re-captured
    np.testing.assert_array_equal(np.asarray(la), np.asarray(lb))
    for p, q in zip(a.get_weights(), b.get_weights()):
        np.testing.assert_array_equal(p, q)
    a.check_kernel_status()


# ------------------------------------------------------- 8. rows are independent
@pytest.mark.parametrize("path", PATHS)
def test_a_nan_image_stays_alone(path):
    name, objective = "S2", "IWAE"
    _, _, _, B, k = F.case(name)
    m = _m(name, path)
    base = _run(m, name, objective)
    m0, s0, _ = F.setting(name)
    bad = 1
    mn = [np.array(v) for v in _f32(m0)]
    mn[0][bad, 2] = np.nan
    out = _run(m, name, objective, init=(mn, _f32(s0)))
    others = [i for i in range(B) if i != bad]
    for n in ("mean", "logstd", "h"):
        for u, v in zip(_np(out[n]), _np(base[n])):
            np.testing.assert_array_equal(u[..., others, :], v[..., others, :], err_msg=n)
    for n in ("bound", "log_w", "logpx", "ess"):
        u, v = out[n].cpu().numpy(), base[n].cpu().numpy()
        np.testing.assert_array_equal(u[..., others], v[..., others], err_msg=n)
        assert not np.isfinite(u[..., bad]).any(), n
    assert np.isnan(out["mean"][0].cpu().numpy()[bad]).any()
    m.check_kernel_status()


# ---------------------------------------------------------------- 9. arguments
def _dev(m, arrays):
    import torch
    return [torch.as_tensor(np.ascontiguousarray(a, np.float32), device=m.device) for a in arrays]


def _raw(m, x, mean, logstd, k, objective=0, n_iters=2, step0=0, lr=0.05, beta1=0.9, beta2=0.999, epsilon=1e-3, ls_min=-12.0,
         ls_max=4.0, eps=None, adam=None, bound=None, lat_out=None, log_w=None, logpx=None, ess=None, chunk=0, cfg=True,
         x_null=False, N=None, n_par=None, mean_arr=None, logstd_arr=None, n_eps=None, n_adam=None, n_lat=None):
    """iwae_refine through ctypes on device tensors; returns the code."""
    import torch
    from iwae_replication_project_amd import _lib
    c = _lib.IwaeRefineConfig(objective=objective, n_iters=n_iters, step0=step0, lr=lr, beta1=beta1, beta2=beta2,
                              epsilon=epsilon, logstd_min=ls_min, logstd_max=ls_max)
    marr, nm = _lib.fptr_array(mean)
    sarr, _ = _lib.fptr_array(logstd)
    earr, ne = _lib.fptr_array(eps) if eps is not None else (None, 0)
    aarr, na = _lib.fptr_array(adam) if adam is not None else (None, 0)
    harr, nh = _lib.fptr_array(lat_out) if lat_out is not None else (None, 0)
    P = _lib.fptr
    with torch.cuda.stream(m._stream):
        rc = m._lib.iwae_refine(m._h, None if x_null else P(x), mean[0].shape[0] if N is None else N, k, chunk,
                                marr if mean_arr is None else mean_arr, sarr if logstd_arr is None else logstd_arr,
                                nm if n_par is None else n_par, ctypes.byref(c) if cfg else None,
                                earr, ne if n_eps is None else n_eps, aarr, na if n_adam is None else n_adam,
                                P(bound), harr, nh if n_lat is None else n_lat, P(log_w), P(logpx), P(ess))
    m._stream.synchronize()
    return rc


@pytest.mark.parametrize("path", PATHS)
def test_invalid_arguments_return_einval_and_launch_nothing(path):
    import torch
    from iwae_replication_project_amd import _lib
    name = "S2"
    spec, _, x, B, k = F.case(name)
    L = spec.L
    m0, s0, e = F.setting(name)
    m = _m(name, path)
    xt = _dev(m, [x])[0]
    mean, logstd = _dev(m, m0), _dev(m, s0)
    eps2 = [t for p in e[:2] for t in _dev(m, p)]              # two passes: n_iters = 2, no evaluation
    adam = [torch.zeros(B, d, device=m.device) for d in spec.n_latent_encoder for _ in range(4)]
    lat = [torch.empty(k, B, d, device=m.device) for d in spec.n_latent_encoder]
    lp = torch.empty(B, device=m.device)
    one = (_lib.FP * L)(_lib.fptr(mean[0]), *([None] * (L - 1)))
    nullp = ctypes.cast(None, _lib.FPP)
    nan, inf = float("nan"), float("inf")
    bad = dict(
        cfg_null=dict(cfg=False), x_null=dict(x_null=True), mean_null=dict(mean_arr=nullp), logstd_null=dict(logstd_arr=nullp),
        a_null_mean=dict(mean_arr=one), a_null_logstd=dict(logstd_arr=one), n_par_not_L=dict(n_par=L - 1),
        n_eps_not_0_or_PL=dict(eps=eps2[:-1]), n_eps_without_buffers=dict(n_eps=2 * L),
        n_eps_misses_the_evaluation=dict(eps=eps2, logpx=lp), a_null_eps=dict(eps=eps2[:1] + [None] + eps2[2:]),
        n_adam_not_0_or_4L=dict(adam=adam[:-1]), n_adam_without_buffers=dict(n_adam=4 * L),
        a_null_adam=dict(adam=adam[:2] + [None] + adam[3:]), n_lat_not_0_or_L=dict(lat_out=lat[:-1]),
        n_lat_without_buffers=dict(n_lat=L), a_null_sample_buffer=dict(lat_out=[None] + lat[1:]),
        objective_2=dict(objective=2), objective_negative=dict(objective=-1),
        n_iters_negative=dict(n_iters=-1), n_iters_above_limit=dict(n_iters=(1 << 24) + 1),
        step0_negative=dict(step0=-1, adam=adam), step0_without_adam=dict(step0=3),
        nothing_to_do=dict(n_iters=0),
        lr_zero=dict(lr=0.0), lr_negative=dict(lr=-0.1), lr_nan=dict(lr=nan), lr_inf=dict(lr=inf),
        epsilon_zero=dict(epsilon=0.0), epsilon_nan=dict(epsilon=nan), epsilon_inf=dict(epsilon=inf),
        beta1_one=dict(beta1=1.0), beta1_negative=dict(beta1=-0.1), beta2_one=dict(beta2=1.0), beta2_nan=dict(beta2=nan),
        min_above_max=dict(ls_min=1.0, ls_max=0.0), min_nan=dict(ls_min=nan), max_inf=dict(ls_max=inf),
        N_zero=dict(N=0), N_negative=dict(N=-3), k_zero=dict(k=0), k_negative=dict(k=-1),
        k_above_limit=dict(k=(1 << 20) + 1), chunk_above_limit=dict(N=4096, k=1 << 20, chunk=2048),
        rows_above_limit=dict(N=2048, k=1 << 20, chunk=1),
    )
    c0 = _counts(m)
    for what, kw in bad.items():
        args = dict(k=k)
        args.update(kw)
        assert _raw(m, xt, mean, logstd, **args) == -1, what
        assert m._lib.iwae_last_error(m._h), what
    assert _counts(m) == c0                                   # nothing was launched
    for a, b in zip(_np(mean) + _np(logstd), list(m0) + list(s0)):
        np.testing.assert_array_equal(a, _f32(b))
    assert _raw(m, xt, mean, logstd, k=k, eps=eps2) == 0       # every output absent: the parameters alone move
    assert np.abs(mean[0].cpu().numpy() - _f32(m0[0])).max() > 0
    m.check_kernel_status()


def test_facade_rejects_bad_arguments():
    name = "S2"
    _, _, x, B, k = F.case(name)
    m = _m(name, "auto")
    with pytest.raises(ValueError):
        m.refine(_f32(x), k, n_iters=1, objective="VAE")
    with pytest.raises(ValueError):
        m.refine(_f32(x), k, n_iters=1, init="prior")
    with pytest.raises(ValueError):
        m.refine(_f32(x), k, n_iters=1, want=("weights",))
    with pytest.raises(ValueError):
        m.refine(_f32(x), k, n_iters=0, want=("bound",))
    with pytest.raises(ValueError):
        m.refine(_f32(x), k, n_iters=1, lr=-1.0)
