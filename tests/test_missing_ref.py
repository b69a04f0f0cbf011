"""Training with missing pixels without a GPU: the float64 reference
(tests/missing_ref.py) against finite differences of the masked objective, its
reduction to the oracle under an all-ones mask, its blindness to what x holds
at a missing pixel, and the fairness of the inputs the GPU tests
(tests/test_gpu_missing.py) run on."""
import numpy as np
import pytest

import missing_ref as M
import pathgrad_ref as R
from oracle import iwae_oracle as O

# the GPU tests' bars (tests/test_gpu_pathgrad.py)
GPU_REL, GPU_TENSOR = 1e-4, 5e-4

FD_ARCHS = [([8], [8], [4], [12]),
            ([10, 8], [8, 10], [5, 3], [5, 12]),
            ([10, 8, 6], [6, 8, 10], [5, 4, 3], [4, 5, 12])]
FD_LOSSES = ["IWAE", "VAE", "L_alpha", "VAE_V1", "CIWAE", "PIWAE", "IWAE_DREG"]


def _fd_case(arch):
    B, k = 4, 4
    spec, params, _, x, eps = R.make_case(arch, B, k, 177 + len(arch[0]), x_dim=12)
    eps2 = O.draw_eps(spec, k, B, np.random.default_rng(5))
    mask = M.make_mask(B, 12, 9, p_obs=0.6)
    return spec, params, M.with_holes(x, mask), eps, eps2, mask, k


def _fd(f, flat, idx, step=1e-6):
    out = np.zeros(len(idx))
    for n, j in enumerate(idx):
        v = []
        for sgn in (1.0, -1.0):
            w = flat.copy()
            w[j] += sgn * step
            v.append(f(w))
        out[n] = (v[0] - v[1]) / (2 * step)
    return out


@pytest.mark.parametrize("arch", FD_ARCHS, ids=["1L", "2L", "3L"])
@pytest.mark.parametrize("loss", FD_LOSSES)
def test_reference_matches_finite_differences(arch, loss):
    """The masked gradient equals central differences (step 1e-6) of the masked
    objective at 40 random parameters, to 1e-7 of the largest gradient entry.
    NaN sits at the missing entries of x, image 0 is entirely missing, image 1
    entirely observed.  PIWAE: the decoder's entries against IWAE's objective,
    the encoder's against MIWAE's.  IWAE_DREG: the encoder's against the
    surrogate of pathgrad_ref (sampling on one parameter copy, densities on
    another), the decoder's against IWAE's objective."""
    spec, params, x, eps, eps2, mask, k = _fd_case(arch)
    kw = M.loss_kwargs(loss, k, eps2)
    if loss == "PIWAE":
        kw = {"k1": 2, "k2": 2}
    J, g = M.objective_and_grads(params, spec, x, mask, eps, loss, **kw)
    assert np.isfinite(J)
    flat, ana = O.flatten_params(spec, params), O.flatten_params(spec, g)
    assert np.isfinite(ana).all()
    ne = R.enc_size(spec)
    rng = np.random.default_rng(3)

    def obj(name, **k2):
        return lambda w: M.objective_and_grads(O.unflatten_params(spec, w), spec, x, mask, eps, name, with_grads=False,
                                               **k2)[0]
    if loss == "PIWAE":
        groups = [(np.arange(ne), obj("MIWAE", **kw)), (np.arange(ne, flat.size), obj("IWAE"))]
    elif loss == "IWAE_DREG":
        a = R.enc_weights(M.forward(params, spec, x, mask, eps)["lw"], loss)
        groups = [(np.arange(ne), lambda w: M.surrogate(O.unflatten_params(spec, w), params, spec, x, mask, eps, a)),
                  (np.arange(ne, flat.size), obj("IWAE"))]
    else:
        groups = [(np.arange(flat.size), obj(loss, **kw))]
    worst = 0.0
    for members, f in groups:
        idx = rng.choice(members, min(40 // len(groups), members.size), replace=False)
        worst = max(worst, np.abs(_fd(f, flat, idx) - ana[idx]).max() / np.abs(ana).max())
    print(f"{loss} {len(arch[0])}L: worst FD error / max|g| {worst:.2e}")
    assert worst <= 1e-7, worst


@pytest.mark.parametrize("loss", FD_LOSSES + ["L_power_p", "L_median", "MIWAE", "IWAE_STL"])
def test_all_ones_mask_is_the_oracle(loss):
    spec, params, x, eps, eps2, mask, k = _fd_case(FD_ARCHS[1])
    x = np.where(mask != 0, x, 0.0)
    ones = np.ones_like(mask)
    kw = M.loss_kwargs(loss, k, eps2)
    if loss in ("PIWAE", "MIWAE"):
        kw = {"k1": 2, "k2": 2}
    if loss == "L_power_p":
        kw = {"p": 0.5}
    J, g = M.objective_and_grads(params, spec, x, ones, eps, loss, **kw)
    if loss in R.LOSSES:
        Jo, go = R.objective_and_grads(params, spec, x, eps, loss)
    else:
        Jo, go = O.objective_and_grads(params, spec, x, eps, loss, k, **kw)
    assert J == Jo
    assert np.array_equal(O.flatten_params(spec, g), O.flatten_params(spec, go))


@pytest.mark.parametrize("loss", ["IWAE", "L_alpha", "IWAE_DREG"])
def test_missing_entries_never_leak(loss):
    spec, params, x, eps, eps2, mask, k = _fd_case(FD_ARCHS[1])
    outs = []
    for fill in (np.nan, np.inf, 0.0, 1.0):
        J, g = M.objective_and_grads(params, spec, M.with_holes(x, mask, fill), mask, eps, loss)
        outs.append(np.concatenate([[J], O.flatten_params(spec, g)]))
    assert np.isfinite(outs[0]).all()
    for o in outs[1:]:
        assert np.array_equal(o, outs[0])
    # and the mask matters: the complete image gives another objective
    J1, _ = M.objective_and_grads(params, spec, M.with_holes(x, mask, 0.0), np.ones_like(mask), eps, loss)
    assert abs(J1 - outs[0][0]) > 1e-3 * abs(J1)


GPU_LOSSES = {"M1": ["IWAE"], "M2w": ["IWAE"], "M784": ["IWAE"], "M784k": ["IWAE"],
              "M2": ["IWAE", "VAE", "L_alpha", "VAE_V1", "CIWAE", "PIWAE", "IWAE_DREG"],
              "M50": ["IWAE", "VAE", "L_alpha", "VAE_V1", "CIWAE", "PIWAE", "IWAE_DREG"]}


@pytest.mark.parametrize("name", list(GPU_LOSSES))
def test_gpu_inputs_are_fair(name):
    """A condition on the GPU tests' inputs, not a measurement of the GPU code:
    the reference itself run in float32 stays within a quarter of the GPU bars
    against float64 on those very inputs, and the mask moves the gradient by far
    more than the bars."""
    _, B, k, _, (spec, params, _, x, eps, eps2, mask) = M.shape_case(name)
    opt = lambda: O.Adam(1e-3, 0.9, 0.999, 1e-4)
    p32 = O.cast_params(params, np.float32)
    x32, e32, f32 = x.astype(np.float32), [e.astype(np.float32) for e in eps], [e.astype(np.float32) for e in eps2]
    for loss in GPU_LOSSES[name]:
        l64, _, g64 = M.train_step(params, spec, x, mask, eps, loss, opt(), **M.loss_kwargs(loss, k, eps2))
        l32, _, g32 = M.train_step(p32, spec, x32, mask, e32, loss, opt(), **M.loss_kwargs(loss, k, f32))
        whole = R.rel_l2(g32.astype(np.float64), g64)
        per = M.worst_tensor(spec, g32.astype(np.float64), g64)
        lrel = abs(float(l32) - l64) / abs(l64)
        print(f"{name} {loss}: float32 reference loss rel {lrel:.2e}, whole rel-L2 {whole:.2e}, per tensor {per:.2e}")
        assert lrel <= GPU_REL / 4, lrel
        assert whole <= GPU_REL / 4, whole
        assert per <= GPU_TENSOR / 4, per
    _, _, g_m = M.train_step(params, spec, x, mask, eps, "IWAE", opt())
    _, _, g_1 = M.train_step(params, spec, np.where(mask != 0, x, 0.0), np.ones_like(mask), eps, "IWAE", opt())
    assert R.rel_l2(g_m, g_1) >= 0.05
