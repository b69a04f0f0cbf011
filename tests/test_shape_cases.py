"""The shape-sweep cases (tests/shape_cases.py) without a GPU: the constants
expected_paths() restates against the library's sources, the branches the table
covers, and the fairness of the float64 reference the GPU tests
(tests/test_gpu_shapes.py) compare with -- its gradient against finite
differences, and the same train step in float32 arithmetic within a quarter of
every GPU bar."""
import os
import re

import numpy as np
import pytest

import pathgrad_ref as R
import shape_cases as S
from oracle import iwae_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "iwae_replication_project_amd", "csrc")

# the GPU tests' bars (tests/test_gpu_shapes.py; test_gpu_parity.py / test_gpu_configs.py)
GPU_REL, GPU_TENSOR, GPU_ADAM_ATOL, GPU_LW = 1e-4, 5e-4, 6e-5, 1e-4

CASE_LOSS = [(n, v[0]) for n in S.CASES for v in S.loss_variants(n)]


_variant = S.variant
train_step = S.reference_step


# ------------------------------------------------------------ the rules' constants
def test_constants_match_the_sources():
    src = open(os.path.join(CSRC, "iwae_model.hip")).read() + open(os.path.join(CSRC, "iwae_kernels.h")).read()

    def const(name):
        return int(re.search(r"constexpr \w+ (?:\w+ = \d+, )?%s = (\d+)" % name, src).group(1))
    for name in ("kTcMaxLayers", "kRbMaxJobs", "kRbMaxWidth", "kUpdMaxJobs", "kUpdMaxTiles", "kMgMaxBufs",
                 "kMgMaxStages"):
        assert const(name) == getattr(S, name), name
    assert "constexpr size_t kTcLdsBytes = 160 * 1024;" in src
    assert re.search(r"long long upd_rows = (\d+);", src).group(1) == str(S.UPD_ROWS)
    assert re.search(r"int smallm_rows = (\d+);", src).group(1) == str(S.SMALLM_ROWS)
    assert "fin + 1 > %d || h->dense[di].fout > %d" % (S.SMALLM_WIDTH, S.SMALLM_WIDTH) in src
    assert "P.Bimg * P.kS >= %d;" % S.TCU_ROWS in src
    assert "P.Bimg * P.kS <= %d;" % S.RB_ROWS in src
    hdr = open(os.path.join(ROOT, "include", "iwae.h")).read()
    assert int(re.search(r"#define IWAE_MAX_LAYERS (\d+)", hdr).group(1)) == len(S.CASES["D8"][0])


def test_wx_is_the_first_width_whose_engine_plan_does_not_fit():
    assert S.WX_H == 1216
    assert S.engine_lds_bytes_1layer(S.WX_H - 64, 8, 16) <= S.kTcLdsBytes < S.engine_lds_bytes_1layer(S.WX_H, 8, 16)
    assert S.CASES["WX"][0] == [S.WX_H]
    assert not S.expected_paths("WX")["engine"] and S.expected_paths("W1024")["engine"]


def test_cases_are_small_and_mirrored():
    for name, (he, hd, le, ld, x_dim, B, k, seed) in S.CASES.items():
        assert B * k <= 300, name
        assert hd == he[::-1] and ld == le[::-1][1:] + [x_dim], name
        spec = S.make(name)[0]
        assert [(fin, fout) for fin, fout in S.dense_layers(name)] == _library_dense(spec), name
    for name in S.LOSS_CASES:
        assert name in S.CASES
    k1, k2 = S.split_k(S.CASES["E3"][6])
    assert k1 > 1 and k2 > 1                     # a composite k: MIWAE / PIWAE with a real split
    k1, k2 = S.split_k(S.CASES["D4"][6])
    assert k1 > 1 and k2 > 1 and k1 != k2


def _library_dense(spec):
    """The oracle's Dense list with each lmu / lstd pair merged into the library's head."""
    out = []
    for n, fin, fout in spec.dense:
        if n.endswith(".lstd"):
            out[-1] = (fin, out[-1][1] + fout)
        else:
            out.append((fin, fout))
    return out


# -------------------------------------------------------------- branch coverage
def test_every_branch_is_covered_in_both_directions():
    seen = {}
    for name, vid in CASE_LOSS:
        _, loss, kw = _variant(name, vid)
        for path in ("auto", "fused", "layerwise"):
            for key, val in S.expected_paths(name, loss, path, p=kw.get("p", 1.0)).items():
                seen.setdefault((path, key), set()).add(bool(val))
    for key in ("engine", "row_block", "update", "combined", "few_row", "x_direct", "nll_fused"):
        assert seen[("auto", key)] == {True, False}, key
    assert seen[("fused", "row_block")] == {True, False}      # the forced path and its fallback
    assert seen[("fused", "engine")] == {False} and seen[("layerwise", "row_block")] == {False}
    assert {S.CASES[n][4] % 4 for n in S.CASES} == {0, 1, 2}
    auto = {n: S.expected_paths(n) for n in S.CASES}
    # x_dim % 4 != 0: read directly by the few-row launch (O1), staged beyond 32 images (O2w)
    assert S.CASES["O1"][4] % 4 and auto["O1"]["x_direct"] and auto["O1"]["few_row"]
    assert S.CASES["O2w"][4] % 4 and auto["O2w"]["engine"] and not auto["O2w"]["x_direct"]
    # depth: 3 engine, 4 row-block, 5 and 8 layer-wise; the NLL kernel to 4
    assert auto["E3"]["engine"] and not auto["D4"]["engine"] and auto["D4"]["row_block"]
    assert not auto["D5"]["row_block"] and not auto["D8"]["row_block"]
    assert auto["D4"]["nll_fused"] and not auto["D5"]["nll_fused"] and not auto["D8"]["nll_fused"]
    assert len(S.dense_layers("D4")) == 24 > S.kUpdMaxJobs and not auto["D4"]["update"]
    # width: kRbMaxWidth on the forced row-block path, the update's tiles, the few-row width, the LDS fit
    assert S.expected_paths("W511", "IWAE", "fused")["row_block"]
    assert not S.expected_paths("W512", "IWAE", "fused")["row_block"]
    assert auto["W1024"]["engine"] and not auto["W1024"]["update"] and not auto["W1024"]["few_row"]
    assert not auto["WX"]["engine"] and not auto["WX"]["row_block"] and auto["WX"]["nll_fused"]
    assert auto["E2t"]["combined"] and not auto["E3"]["combined"]
    for loss in S.NO_ENGINE_LOSSES:
        assert S.expected_paths("O2", loss)["row_block"]
    # L_power_p: on the engine for p > 0, on the f32 row-block kernels for p < 0
    assert S.expected_paths("E3", "L_power_p", p=2.5)["engine"]
    assert S.expected_paths("E3", "L_power_p", p=-1.5)["row_block"]


# --------------------------------------------------------- reference fairness
def _objective(name, loss, kw, params, part):
    """The scalar whose gradient the reference's `part` ("enc" / "dec") entries are."""
    spec, _, _, x, eps = S.make(name)
    k = S.CASES[name][6]
    kw = dict(kw)
    if loss == "CIWAE":
        kw["eps2"] = S.second_draw(name)
    if loss == "PIWAE":                          # decoder: IWAE_{k1 k2}; encoder: MIWAE(k1, k2)
        loss = "IWAE" if part == "dec" else "MIWAE"
        kw = {} if part == "dec" else kw
    return O.objective_and_grads(params, spec, x, eps, loss, k, with_grads=False, **kw)[0]


@pytest.mark.parametrize("name,vid", CASE_LOSS, ids=["-".join(c) for c in CASE_LOSS])
def test_reference_gradient_matches_finite_differences(name, vid):
    """Central differences (step 1e-6, float64) of the objective on a handful of
    coordinates: the largest gradient entry of the first and of the last kernel,
    and four drawn ones.  Rounding of the differences: 2^-52 |J| / step < 1e-7 for
    |J| < 400; truncation ~ step^2."""
    _, loss, kw = _variant(name, vid)
    spec, params, _, x, eps = S.make(name)
    _, g, _ = train_step(name, vid)
    g = -g                                                     # gradient of J = -loss
    flat = O.flatten_params(spec, params)
    ne = R.enc_size(spec)
    tensors = np.cumsum([0] + [int(np.prod(s)) for s in spec.param_shapes()])
    rng = np.random.default_rng(S.CASES[name][7])
    coords = [int(np.abs(g[:tensors[1]]).argmax()), int(tensors[-3] + np.abs(g[tensors[-3]:tensors[-2]]).argmax())]
    coords += [int(c) for c in rng.integers(0, flat.size, 4)]
    if loss in R.LOSSES:
        a = R.enc_weights(O.forward(params, spec, x, eps)["lw"], loss)
    step, worst = 1e-6, 0.0
    for j in coords:
        vals = []
        for sgn in (1.0, -1.0):
            f = flat.copy()
            f[j] += sgn * step
            pj = O.unflatten_params(spec, f)
            if loss in R.LOSSES and j < ne:                    # the path gradient: sampling on pj, densities on params
                vals.append(R.surrogate(pj, params, spec, x, eps, a))
            elif loss in R.LOSSES:
                vals.append(_objective(name, "IWAE", {}, pj, "dec"))
            else:
                vals.append(_objective(name, loss, kw, pj, "enc" if j < ne else "dec"))
        fd = (vals[0] - vals[1]) / (2 * step)
        worst = max(worst, abs(fd - g[j]))
    scale = np.abs(g[coords]).max()
    print(f"{name} {vid}: FD max abs err {worst:.2e}, largest of the entries {scale:.2e}")
    assert worst <= 1e-6 * scale + 1e-7, (worst, scale)


@pytest.mark.parametrize("name,vid", CASE_LOSS, ids=["-".join(c) for c in CASE_LOSS])
def test_float32_reference_within_a_quarter_of_the_gpu_bars(name, vid):
    """A condition on the GPU tests' inputs, not a measurement of the GPU code:
    the reference's own train step in float32 arithmetic against float64."""
    spec = S.make(name)[0]
    l64, g64, w64 = train_step(name, vid)
    l32, g32, w32 = train_step(name, vid, np.float32)
    whole = R.rel_l2(g32, g64)
    # (VAE_V1 gives the decoder's prior layers an exactly zero gradient: 0 / tiny = 0)
    per = max(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)
              for a, b in zip(R.split_tensors(spec, g32), R.split_tensors(spec, g64)))
    adam = np.abs(w32 - w64).max()
    print(f"{name} {vid}: float32 loss rel {abs(l32 - l64) / abs(l64):.2e}, gradient rel-L2 {whole:.2e}, "
          f"per tensor {per:.2e}, post-Adam weights {adam:.2e}")
    assert abs(l32 - l64) <= GPU_REL / 4 * abs(l64)
    assert whole <= GPU_REL / 4, whole
    assert per <= GPU_TENSOR / 4, per
    assert adam <= max(GPU_ADAM_ATOL, 10 * np.abs(g32 - g64).max()) / 4, adam


@pytest.mark.parametrize("name", list(S.CASES))
def test_float32_log_weights_within_a_quarter_of_the_gpu_bar(name):
    spec, params, _, x, eps = S.make(name)
    lw64 = O.forward(params, spec, x, eps)["lw"]
    lw32 = O.forward(O.cast_params(params, np.float32), spec, x.astype(np.float32),
                     [e.astype(np.float32) for e in eps])["lw"]
    err = np.abs(lw32 - lw64).max() / np.abs(lw64).max()
    print(f"{name}: float32 log-weights {err:.2e} of max|lw|")
    assert err <= GPU_LW / 4, err
