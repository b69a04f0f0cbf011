"""IWAE_STL / IWAE_DREG without a GPU: the ABI ids and the binding, the float64
reference of the two estimators (tests/pathgrad_ref.py) against finite
differences, and the fairness of the inputs the GPU tests
(tests/test_gpu_pathgrad.py) run on."""
import os
import re

import numpy as np
import pytest

import pathgrad_ref as R
from oracle import iwae_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "iwae.h")

# the GPU tests' bars (tests/test_gpu_parity.py, tests/test_gpu_configs.py)
GPU_REL, GPU_TENSOR = 1e-4, 5e-4


def test_abi_ids_and_binding():
    from iwae_replication_project_amd import _lib
    from iwae_replication_project_amd.flexible_iwae import LOSSES, loss_config
    src = open(HEADER).read()
    ids = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"IWAE_LOSS_([A-Z_0-9]+) = (\d+)", src))
    assert ids["IWAE_STL"] == 9 and ids["IWAE_DREG"] == 10
    assert _lib.LOSS_IDS["IWAE_STL"] == 9 and _lib.LOSS_IDS["IWAE_DREG"] == 10
    assert "IWAE_STL" in LOSSES and "IWAE_DREG" in LOSSES
    lc = loss_config("IWAE_DREG", 8)
    assert (lc.loss, lc.k) == (10, 8)
    assert loss_config("IWAE_STL", 3).loss == 9
    # ids stay dense and unique
    assert sorted(_lib.LOSS_IDS.values()) == list(range(11))


FD_ARCHS = [([8], [8], [4], [12]),
            ([10, 8], [8, 10], [5, 3], [5, 12]),
            ([10, 8, 6], [6, 8, 10], [5, 4, 3], [4, 5, 12])]


@pytest.mark.parametrize("arch", FD_ARCHS, ids=["1L", "2L", "3L"])
@pytest.mark.parametrize("loss", R.LOSSES)
def test_reference_matches_finite_differences(arch, loss):
    """The analytic path gradient equals central finite differences (step 1e-6)
    of the surrogate whose encoder sampling runs on one parameter copy and
    whose densities and decoder on another, to 1e-7 relative (measured: 2e-9);
    the decoder group equals the oracle's IWAE gradient exactly."""
    spec, params, _, x, eps = R.make_case(arch, 3, 4, 77 + len(arch[0]), x_dim=12)
    J, g = R.objective_and_grads(params, spec, x, eps, loss)
    Jo, go = O.objective_and_grads(params, spec, x, eps, "IWAE", 4)
    assert J == Jo
    for n, _, _ in spec.dense:
        if not n.startswith("enc"):
            assert np.array_equal(g[n][0], go[n][0]) and np.array_equal(g[n][1], go[n][1]), n
    a = R.enc_weights(O.forward(params, spec, x, eps)["lw"], loss)
    ne = R.enc_size(spec)
    flat = O.flatten_params(spec, params)
    fd = np.zeros(ne)
    step = 1e-6
    for j in range(ne):
        vals = []
        for sgn in (1.0, -1.0):
            f = flat.copy()
            f[j] += sgn * step
            vals.append(R.surrogate(O.unflatten_params(spec, f), params, spec, x, eps, a))
        fd[j] = (vals[0] - vals[1]) / (2 * step)
    ana = O.flatten_params(spec, g)[:ne]
    err = np.abs(ana - fd).max() / np.abs(fd).max()
    print(f"{loss} {len(arch[0])}L: FD max rel {err:.2e}, rel-L2 {R.rel_l2(ana, fd):.2e}")
    assert err <= 1e-7, err
    assert R.rel_l2(ana, fd) <= 1e-7


def _enc(spec, flat):
    return flat[:R.enc_size(spec)]


def _cases():
    for name in R.SHAPES:
        arch, B, k, case = R.shape_case(name)
        yield name, len(arch[0]), case
    # BASELINE configs[0] at its own size, the auto-path test's second case (seeds of test_gpu_configs.py)
    for loss in R.LOSSES:
        arch = ([200], [200], [50], [784])
        yield "C0-" + loss, 1, R.make_case(arch, 20, 5, 300 + len(loss), x_dim=784)


@pytest.mark.parametrize("name,L,case", list(_cases()), ids=[c[0] for c in _cases()])
def test_gpu_inputs_are_fair_and_discriminating(name, L, case):
    """Conditions on the GPU tests' inputs (not measurements of the GPU code):
    the reference itself run in float32 stays within a quarter of the GPU bars
    against float64, and the inputs tell the estimators -- and the density
    chain -- apart by far more than those bars."""
    spec, params, _, x, eps = case
    opt = lambda: O.Adam(1e-3, 0.9, 0.999, 1e-4)
    p32 = O.cast_params(params, np.float32)
    x32, e32 = x.astype(np.float32), [e.astype(np.float32) for e in eps]
    g = {}
    for loss in R.LOSSES:
        _, _, g64 = R.train_step(params, spec, x, eps, loss, opt())
        _, _, g32 = R.train_step(p32, spec, x32, e32, loss, opt())
        g[loss] = g64
        whole = R.rel_l2(g32.astype(np.float64), g64)
        per = max(np.abs(a.astype(np.float64) - b).max() / np.abs(b).max()
                  for a, b in zip(R.split_tensors(spec, g32), R.split_tensors(spec, g64)))
        print(f"{name} {loss}: float32 reference whole rel-L2 {whole:.2e}, per tensor {per:.2e}")
        assert whole <= GPU_REL / 4, whole
        assert per <= GPU_TENSOR / 4, per
    _, _, g_iwae = O.train_step(params, spec, x, eps, "IWAE", eps[0].shape[0], opt())
    d_stl = R.rel_l2(_enc(spec, g["IWAE_STL"]), _enc(spec, g_iwae))
    d_dreg = R.rel_l2(_enc(spec, g["IWAE_DREG"]), _enc(spec, g["IWAE_STL"]))
    print(f"{name}: encoder STL<->IWAE {d_stl:.3f}, DReG<->STL {d_dreg:.4f}")
    assert d_stl >= 0.05, d_stl
    assert d_dreg >= 5e-3, d_dreg
    if L >= 2:
        def enc0_kernels(flat):       # the four Dense kernels of enc0 (tensors 0, 2, 4, 6)
            return np.concatenate(R.split_tensors(spec, flat)[0:8:2])
        assert [n for n, _, _ in spec.dense[:4]] == ["enc0.l1", "enc0.l2", "enc0.lmu", "enc0.lstd"]
        for loss in R.LOSSES:
            _, _, g_nod = R.train_step(params, spec, x, eps, loss, opt(), density=False)
            d = R.rel_l2(enc0_kernels(g_nod), enc0_kernels(g[loss]))
            print(f"{name} {loss}: enc0 without the density chain {d:.3f}")
            assert d >= 0.05, d
