"""The float64 reference of the reweighted wake-sleep step
(tests/wakesleep_ref.py) without a GPU: against finite differences of the plain
functions L_wake(phi) and L_sleep(phi), against the oracle's IWAE step and the
path-gradient reference, and the fairness of the inputs the GPU tests
(tests/test_gpu_wakesleep.py) run on."""
import numpy as np
import pytest

import pathgrad_ref as PR
import wakesleep_ref as W
from oracle import iwae_oracle as O

# the GPU tests' bars (tests/test_gpu_pathgrad.py)
GPU_REL, GPU_TENSOR = 1e-4, 5e-4

FD_ARCHS = [([8], [8], [4], [12]),
            ([10, 8], [8, 10], [5, 3], [5, 12]),
            ([10, 8, 6], [6, 8, 10], [5, 4, 3], [4, 5, 12])]


def _fd_case(arch):
    return W.make_case(arch, 3, 4, 5, 177 + len(arch[0]), x_dim=12)


@pytest.mark.parametrize("arch", FD_ARCHS, ids=["1L", "2L", "3L"])
@pytest.mark.parametrize("phase", ["wake", "sleep"])
def test_reference_matches_finite_differences(arch, phase):
    """The analytic gradients of L_wake and L_sleep equal central finite
    differences (step 1e-6) of those plain functions of the encoder's
    parameters at fixed constants (samples, weights, dreams), at
    test_pathgrad_ref.py's bar: 1e-7 relative."""
    spec, params, _, x, eps, dreams = _fd_case(arch)
    c = O.forward(params, spec, x, eps)
    h, a = c["h"], W.wake_weights(c["lw"])

    def value(p, grads=None):
        if phase == "wake":
            return W.wake_value_and_grads(p, spec, x, h, a, grads)
        return W.sleep_value_and_grads(p, spec, dreams, grads)

    g = W.zeros_like_params(params, spec)
    value(params, g)
    ne = PR.enc_size(spec)
    flat = O.flatten_params(spec, params)
    fd = np.zeros(ne)
    step = 1e-6
    for j in range(ne):
        vals = []
        for sgn in (1.0, -1.0):
            f = flat.copy()
            f[j] += sgn * step
            vals.append(value(O.unflatten_params(spec, f)))
        fd[j] = (vals[0] - vals[1]) / (2 * step)
    ana = O.flatten_params(spec, g)[:ne]
    err = np.abs(ana - fd).max() / np.abs(fd).max()
    print(f"{phase} {len(arch[0])}L: FD max rel {err:.2e}, rel-L2 {PR.rel_l2(ana, fd):.2e}")
    assert err <= 1e-7, err
    assert PR.rel_l2(ana, fd) <= 1e-7
    assert not np.any(O.flatten_params(spec, g)[ne:])       # nothing outside the encoder


@pytest.mark.parametrize("arch", FD_ARCHS, ids=["1L", "2L", "3L"])
@pytest.mark.parametrize("coef", W.COEFS)
def test_decoder_gradient_and_value_are_the_iwae_steps(arch, coef):
    spec, params, _, x, eps, dreams = _fd_case(arch)
    vals, _, g = W.train_step(params, spec, x, eps, dreams, coef[0], coef[1], O.Adam(1e-3, 0.9, 0.999, 1e-4))
    loss, _, go = O.train_step(params, spec, x, eps, "IWAE", 4, O.Adam(1e-3, 0.9, 0.999, 1e-4))
    ne = PR.enc_size(spec)
    assert vals[0] == loss
    assert np.array_equal(g[ne:], go[ne:])
    assert (vals[1] == 0) == (coef[0] == 0) and (vals[2] == 0) == (coef[1] == 0)


def test_one_layer_wake_gradient_is_iwae_minus_stl():
    """One stochastic layer, (1, 0): the total reparameterised IWAE gradient is
    its path part (STL) plus the density part; the wake-phi gradient is minus
    that density part."""
    spec, params, _, x, eps, dreams = _fd_case(FD_ARCHS[0])
    _, _, g = W.train_step(params, spec, x, eps, dreams, 1.0, 0.0, O.Adam())
    _, _, g_iwae = O.train_step(params, spec, x, eps, "IWAE", 4, O.Adam())
    _, _, g_stl = PR.train_step(params, spec, x, eps, "IWAE_STL", O.Adam())
    ne = PR.enc_size(spec)
    want = -(g_iwae[:ne] - g_stl[:ne])
    assert np.abs(g[:ne] - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("arch", FD_ARCHS[:2], ids=["1L", "2L"])
def test_zero_coefficient_removes_its_phase(arch):
    spec, params, _, x, eps, (xd, hd) = _fd_case(arch)
    ne = PR.enc_size(spec)
    # c_sleep = 0: dreams full of NaN change nothing
    nan_dreams = (np.full_like(xd, np.nan), [np.full_like(v, np.nan) for v in hd])
    v0, _, g0 = W.train_step(params, spec, x, eps, (xd, hd), 1.0, 0.0, O.Adam())
    v1, _, g1 = W.train_step(params, spec, x, eps, nan_dreams, 1.0, 0.0, O.Adam())
    assert v0 == v1 and v1[2] == 0 and np.array_equal(g0, g1)
    # c_wake = 0: a NaN image poisons L_theta and the decoder, never the encoder
    xn = x.copy()
    xn[0, 0] = np.nan
    v2, _, g2 = W.train_step(params, spec, x, eps, (xd, hd), 0.0, 1.0, O.Adam())
    with np.errstate(invalid="ignore"):
        v3, _, g3 = W.train_step(params, spec, xn, eps, (xd, hd), 0.0, 1.0, O.Adam())
    assert v3[1] == 0 and v3[2] == v2[2] and np.isnan(v3[0])
    assert np.array_equal(g2[:ne], g3[:ne]) and np.isfinite(g3[:ne]).all()


@pytest.mark.parametrize("name", list(W.CASES))
@pytest.mark.parametrize("coef", W.COEFS)
def test_gpu_inputs_are_fair(name, coef):
    """A condition on the GPU tests' inputs (not a measurement of the GPU
    code): the reference itself run in float32 stays within a quarter of the
    GPU bars against float64, and both phases carry weight in the encoder's
    gradient."""
    _, B, k, n, c64 = W.case(name)
    spec, params, _, x, eps, dreams = c64
    _, p32, _, x32, e32, d32 = W.cast_case(c64, np.float32)
    opt = lambda: O.Adam(1e-3, 0.9, 0.999, 1e-4)
    v64, _, g64 = W.train_step(params, spec, x, eps, dreams, coef[0], coef[1], opt())
    v32, _, g32 = W.train_step(p32, spec, x32, e32, d32, coef[0], coef[1], opt())
    whole = PR.rel_l2(g32.astype(np.float64), g64)
    per = max(np.abs(a.astype(np.float64) - b).max() / np.abs(b).max()
              for a, b in zip(PR.split_tensors(spec, g32), PR.split_tensors(spec, g64)))
    vrel = max(abs(float(a) - b) / abs(b) for a, b in zip(v32, v64) if b != 0)
    print(f"{name} {coef}: float32 reference values rel {vrel:.2e}, whole rel-L2 {whole:.2e}, per tensor {per:.2e}")
    assert vrel <= GPU_REL / 4, vrel
    assert whole <= GPU_REL / 4, whole
    assert per <= GPU_TENSOR / 4, per
    for a, b in zip(v32, v64):
        assert (a == 0) == (b == 0)
    ne = PR.enc_size(spec)
    assert np.linalg.norm(g64[:ne]) > 1e-3 * np.linalg.norm(g64[ne:])
