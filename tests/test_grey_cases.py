"""The grey-pixel cases (tests/grey_cases.py) without a GPU: the patterns are
what the table says, the limits expected_kernels() restates are the sources',
and the float64 reference the GPU tests (tests/test_gpu_grey.py) compare with is
fair on these very inputs -- the same quantities in float32 arithmetic stay
within a quarter of every GPU bar (exp(100) overflows float32 there by design:
the float32 runs ignore the overflow warning)."""
import os
import re

import numpy as np
import pytest

import grey_cases as G
import impute_ref
import pathgrad_ref as R
import posterior_ref
import score_ref
from oracle import iwae_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "iwae_replication_project_amd", "csrc")

# the GPU tests' bars (tests/test_gpu_grey.py)
GPU_REL, GPU_TENSOR, GPU_ADAM_ATOL, GPU_LW, GPU_LOGPX = 1e-4, 5e-4, 6e-5, 1e-4, 1e-3

TRAIN = [(n, pt, v[0]) for n in G.CASES for pt in G.PATTERNS[n] for v in G.loss_variants(n, pt)]
FORWARD = [(n, pt) for n in ("G1", "G2", "R1", "R2") for pt in G.PATTERNS[n]]


# ------------------------------------------------------------------ the table
def test_cases_are_the_table():
    for name in G.SMALL:
        he, hd, le, ld, x_dim, B, k, seed = G.CASES[name]
        assert hd == he[::-1] and ld == le[::-1][1:] + [x_dim], name
        assert B * k <= 72
    assert G.CASES["GW"][:5] == G.CASES["G2"][:5] and G.CASES["GW"][5] * G.CASES["GW"][6] == 72
    assert G.CASES["G1"][5] * G.CASES["G1"][6] == 35           # 16-row tiles straddle images
    assert G.CASES["G2"][4] % 16 and G.CASES["G2"][4] % 4 == 1  # a ragged last tile and a last quad of one pixel
    for name in G.RING:
        B, k = G.CASES[name][5:7]
        assert B * k == 576 and k >= G.RING_MIN_K and k >= G.RING_NLL_MIN_K
        # workgroup 0 one image; workgroup 1 half and half; the last one ragged
        assert G.RING_WG_ROWS <= k and (k - G.RING_WG_ROWS) * 2 == G.RING_WG_ROWS and (B * k) % G.RING_WG_ROWS
    assert tuple(G.CASES["R1"][:4]) == G.ARCH1 and tuple(G.CASES["R2"][:4]) == G.ARCH2
    ids = lambda n, pt: [v[0] for v in G.loss_variants(n, pt)]
    full = ["IWAE", "VAE", "CIWAE", "L_alpha", "L_power_neg", "VAE_V1", "MIWAE", "PIWAE"]
    assert ids("G1", "grey") == ids("G1", "mixed") == full
    assert ids("G2", "grey") == full + ["IWAE_DREG"]
    for name in ("G3", "GW", "R1", "R2"):
        assert ids(name, "grey") == ids(name, "mixed") == ["IWAE"]
    for name in G.DEEP_CASES:
        assert ids(name, "deep") == ["IWAE", "L_alpha"]
    assert G.variant("G1", "grey", "L_power_neg")[2] == dict(p=-1.5)


@pytest.mark.parametrize("name", list(G.CASES))
def test_grey_pattern(name):
    x = G.make(name, "grey")[3]
    x_dim = G.CASES[name][4]
    assert np.array_equal(x, x.astype(np.float32).astype(np.float64))
    for i, row in enumerate(x):
        cols = list(G.special_columns(x_dim, i))
        assert tuple(row[cols]) == (0.0, 1.0, 2.0 ** -24, 1.0 - 2.0 ** -24)
        rest = np.delete(row, cols)
        assert (rest > 0).all() and (rest < 1).all()
    # the model and the noise are make_case's
    he, hd, le, ld, _, B, k, seed = G.CASES[name]
    spec, params, _, _, eps = R.make_case((he, hd, le, ld), B, k, seed, x_dim=x_dim)
    got = G.make(name, "grey")
    assert all(np.array_equal(a, b) for a, b in zip(eps, got[4]))
    np.testing.assert_array_equal(O.flatten_params(spec, params), O.flatten_params(got[0], got[1]))


@pytest.mark.parametrize("name", list(G.CASES))
def test_mixed_pattern_has_exactly_the_grey_pixels_listed(name):
    x_dim, B = G.CASES[name][4:6]
    grey = G.grey_pixels(name, "mixed")
    want = np.zeros((B, x_dim), bool)
    for i in range(B):
        kind = i if name in G.RING else i % 5
        if kind == 1:
            want[i] = True
            want[i, list(G.special_columns(x_dim, i))[:2]] = False        # its exact 0 and 1
        elif kind == 2:
            want[i, x_dim - 1 if name in G.RING else 0] = True
        elif kind == 3:
            want[i, x_dim - 1] = True
    np.testing.assert_array_equal(grey, want)
    assert not G.grey_pixels(name, "binary").any()
    # the binarised images are the all-binarised batch's
    b = G.binarised_images(name)
    assert b and 0 in b
    np.testing.assert_array_equal(G.make(name, "mixed")[3][b], G.make(name, "binary")[3][b])
    if name in G.RING:
        k = G.CASES[name][6]
        assert G.RING_WG_ROWS <= k                      # workgroup 0 lies inside image 0: binarised
        assert grey[1].any() and grey[2].sum() == 1


@pytest.mark.parametrize("name", G.DEEP_CASES)
def test_deep_logits_equal_the_biases_exactly(name):
    x_dim = G.CASES[name][4]
    cols = G.deep_columns(x_dim)
    assert len(set(cols)) == 3
    for dtype in (np.float64, np.float32):
        spec, params, _, x, eps = G.make(name, "deep")
        p = O.cast_params(params, dtype)
        with np.errstate(over="ignore"):
            c = O.forward(p, spec, x.astype(dtype), [e.astype(dtype) for e in eps])
        logit = c["o2"] @ p["out.l3"][0] + p["out.l3"][1]
        for col, b in zip(cols, G.DEEP_BIASES):
            assert (logit[..., col] == b).all()
        assert np.isfinite(c["lw"]).all()
    grey = G.grey_pixels(name, "deep")
    a, b, c3 = cols
    assert (x[:, a] == 0.25).all() and (x[:, b] == 0.0).all() and (x[:, c3] == 1.0).all()
    quad = [q for q in range(b // 4 * 4, min(b // 4 * 4 + 4, x_dim)) if q != b]
    assert grey[:, quad].any(1).all()                                  # the 0 shares its quad with a grey pixel
    tile = [q for q in range(c3 // 16 * 16, min(c3 // 16 * 16 + 16, x_dim)) if q != c3]
    assert grey[:, tile].any(1).all()                                  # the 1 shares its tile with a grey pixel
    assert all(v < 0 for v in G.DEEP_BIASES)
    # only these columns differ from the grey case's model, one alone in "deep<j>"
    base = G.make(name, "grey")[1]
    for j in range(3):
        W, bias = G.make(name, f"deep{j}")[1]["out.l3"]
        diff = np.flatnonzero((W != base["out.l3"][0]).any(0) | (bias != base["out.l3"][1]))
        assert diff.tolist() == [cols[j]]


# ------------------------------------------------------------- the constants
def test_limits_match_the_sources():
    model = open(os.path.join(CSRC, "iwae_model.hip")).read()
    ring = open(os.path.join(CSRC, "iwae_nring.hip")).read()
    assert "P.kS < %d" % G.RING_MIN_K in model and "L.kS < %d" % G.RING_MIN_K in ring
    nr_w = int(re.search(r"constexpr int NR_W = (\d+);", ring).group(1))
    assert "constexpr int NR_ROWS = 16 * NR_W;" in ring and 16 * nr_w == G.RING_WG_ROWS
    assert re.search(r"long long wide_rows = (\d+);", model).group(1) == str(G.WIDE_ROWS)
    assert re.search(r"long long nr_train_rows = (\d+);", model).group(1) == str(G.NRING_TRAIN_ROWS)
    assert "ring && P.kS >= %d" % G.RING_NLL_MIN_K in model
    assert "P.kS > %d || P.Bimg > %d" % (G.TC_BOUND_MAX_K, G.TC_BOUND_MAX_IMAGES) in model
    assert re.search(r"int tc_rt = 1;", model) and re.search(r"int nring_bwd = 3;", model)
    for knobs in list(G.GW_KNOBS.values()) + list(G.RING_KNOBS.values()):
        from iwae_replication_project_amd._lib import KNOBS
        assert set(knobs) <= set(KNOBS)


def test_expected_kernels_cover_the_paths():
    e = G.expected_kernels
    assert e("G1")[2] and not e("G1")[13] and e("G1", path="fused")[13] and not e("G1", path="layerwise")[13]
    assert e("G1", "L_power_p", p=-1.5)[13] and e("G1", "VAE_V1")[13] and e("G2", "IWAE_DREG")[13]
    assert e("G1", "L_alpha")[2]                                   # the engine's bce && !allbin branch
    assert e("G3")[2] and len(G.CASES["G3"][0]) == 3
    assert e("GW", knobs=G.GW_KNOBS["rt2"])["fwd_rows"] == 32
    assert e("GW", knobs=G.GW_KNOBS["wide2"])["fwd_rows"] == e("GW", knobs=G.GW_KNOBS["wide4"])["fwd_rows"] == 64
    assert e("G1")["fwd_rows"] == 16 and not e("G1")[4] and not e("G1")[3]
    for name in G.RING:
        L2 = name == "R2"
        assert not e(name)[4]                                      # 576 rows: below the default nring_train_rows
        r = e(name, knobs=G.RING_KNOBS["ring-b3"])
        assert r[4] and r[5] and r[6] == L2
        r = e(name, knobs=G.RING_KNOBS["ring-b0"])
        assert r[4] and r[5] is False and r[6] is False
        r = e(name, knobs=G.RING_KNOBS["ring-b3-tcb"])
        assert r[4] and r[5] is None
        r = e(name, knobs=G.RING_KNOBS["engine"])
        assert r[2] and not r[4] and not r[5] and not r[6]
        assert e(name)[3] and e(name)[0] and not e(name, knobs=dict(nring=0))[3]
        assert not e(name, path="layerwise")[0]
    assert not e("R2", "L_alpha", knobs=G.RING_KNOBS["ring-b3"])[4]  # the ring forward has no Keras-BCE epilogue


# --------------------------------------------------------- reference fairness
@pytest.mark.parametrize("name,pattern,vid", TRAIN, ids=["-".join(c) for c in TRAIN])
def test_float32_reference_within_a_quarter_of_the_gpu_bars(name, pattern, vid):
    """A condition on the GPU tests' inputs, not a measurement of the GPU code:
    the reference's own train step in float32 arithmetic against float64."""
    spec = G.make(name, pattern)[0]
    l64, g64, w64 = G.reference_step(name, pattern, vid)
    with np.errstate(over="ignore"):
        l32, g32, w32 = G.reference_step(name, pattern, vid, np.float32)
    assert np.isfinite(l64) and np.isfinite(g64).all() and np.isfinite(g32).all()
    whole = R.rel_l2(g32, g64)
    per = max(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)
              for a, b in zip(R.split_tensors(spec, g32), R.split_tensors(spec, g64)))
    adam = np.abs(w32 - w64).max()
    print(f"{name} {pattern} {vid}: float32 loss rel {abs(l32 - l64) / abs(l64):.2e}, gradient rel-L2 {whole:.2e}, "
          f"per tensor {per:.2e}, post-Adam weights {adam:.2e}")
    assert abs(l32 - l64) <= GPU_REL / 4 * abs(l64)
    assert whole <= GPU_REL / 4, whole
    assert per <= GPU_TENSOR / 4, per
    assert adam <= max(GPU_ADAM_ATOL, 10 * np.abs(g32 - g64).max()) / 4, adam


@pytest.mark.parametrize("name,pattern", FORWARD, ids=["-".join(c) for c in FORWARD])
def test_float32_forward_quantities_within_a_quarter_of_the_gpu_bars(name, pattern):
    lw64, lk64, eq64, lp64, la64 = G.forward_reference(name, pattern)
    with np.errstate(over="ignore"):
        lw32, lk32, eq32, lp32, la32 = G.forward_reference(name, pattern, np.float32)
    e_lw = np.abs(lw32 - lw64).max() / np.abs(lw64).max()
    e_lp = np.abs(lp32 - lp64).max()
    print(f"{name} {pattern}: float32 log-weights {e_lw:.2e} of max|lw|, log p(x) {e_lp:.2e} nats, "
          f"L_k rel {abs(lk32 - lk64) / abs(lk64):.2e}, E_q rel {abs(eq32 - eq64) / abs(eq64):.2e}, "
          f"L_alpha rel {abs(la32 - la64) / abs(la64):.2e}")
    assert e_lw <= GPU_LW / 4, e_lw
    assert e_lp <= GPU_LOGPX / 4, e_lp
    assert abs(lk32 - lk64) <= GPU_REL / 4 * abs(lk64)
    assert abs(eq32 - eq64) <= GPU_REL / 4 * abs(eq64)
    assert abs(la32 - la64) <= GPU_REL / 4 * abs(la64)


@pytest.mark.parametrize("pattern", ["grey", "mixed"])
def test_float32_posterior_score_and_impute_within_a_quarter(pattern):
    """G2: the log-weight and log p(x) parts of posterior_ref / impute_ref (30 %
    of the pixels missing) and score_ref's log p(x|h) in float32 arithmetic."""
    spec, params, _, x, eps = G.make("G2", pattern)
    mask = G.impute_mask("G2")
    assert 0.2 < (mask == 0).mean() < 0.4
    p32 = O.cast_params(params, np.float32)
    e32 = [e.astype(np.float32) for e in eps]
    post = posterior_ref.posterior(params, spec, x, eps)
    imp = impute_ref.impute(params, spec, x, mask, eps)
    lw32 = O.forward(p32, spec, x.astype(np.float32), e32)["lw"]
    assert np.abs(lw32 - post["lw"]).max() <= GPU_LW / 4 * np.abs(post["lw"]).max()
    c32 = O.forward(p32, spec, np.where(mask != 0, x, 0.0).astype(np.float32), e32)
    xb, pr = c32["x"][None], c32["p"]
    lpx32 = ((np.log1p(-pr) * (1 - xb) + np.log(pr) * xb) * (mask != 0)[None]).sum(-1)
    lwm32 = (c32["logp"] + lpx32) - c32["logq"]
    assert np.abs(lwm32 - imp["lw"]).max() <= GPU_LW / 4 * np.abs(imp["lw"]).max()
    assert np.abs(posterior_ref.weights(lwm32.astype(np.float64))[1] - imp["log_px"]).max() <= GPU_LOGPX / 4
    h = post["cache"]["h"]
    s64 = score_ref.score(params, spec, x, h)
    s32 = score_ref.score(params, spec, x, h, dtype=np.float32)
    assert np.abs(s32["logpx"] - s64["logpx"]).max() <= GPU_REL / 4 * np.abs(s64["logpx"]).max()
    assert (np.abs(s32["logpx"] - s64["logpx"]) / s64["Spx"]).max() <= GPU_REL / 4
