"""The sample-axis cases (tests/sample_cases.py) without a GPU.  Conditions on
the inputs of tests/test_gpu_samples.py, not measurements of the GPU code: the
reference's own train step in float32 arithmetic stays within a quarter of
every GPU bar; the order statistics beside each image's median are two
log-weight bars away from it; WIDE's log-weights spread as far as it says, TIE's
tied rows are exactly equal; and expected_bound()'s constants are the sources',
with both outcomes of each limit covered by some case."""
import os
import re

import numpy as np
import pytest

import pathgrad_ref as R
import sample_cases as C
from oracle import iwae_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "iwae_replication_project_amd", "csrc")

# the GPU tests' bars (tests/test_gpu_samples.py, as tests/test_gpu_shapes.py)
GPU_REL, GPU_TENSOR, GPU_ADAM_ATOL, GPU_LW = 1e-4, 5e-4, 6e-5, 1e-4

MEDIAN_CASES = [n for n in C.CASES if any(v[0] == "L_median" for v in C.loss_variants(n))]


# ------------------------------------------------------------------ the table
def test_the_table_is_the_one_asked_for():
    assert C.MODELS["S1"] == ([24], [6]) and C.MODELS["S2"] == ([20, 12], [6, 4]) and C.X_DIM == 20
    bk = {pt: v[:2] for pt, v in C.POINTS.items()}
    assert bk == {"K17": (3, 17), "K63": (2, 63), "K64": (2, 64), "K65": (2, 65), "K128": (2, 128), "K130": (2, 130),
                  "K256": (2, 256), "K257": (2, 257), "K1024": (3, 1024), "K1025": (2, 1025), "B64": (64, 4),
                  "B65": (65, 4), "M65": (65, 127), "C33": (33, 125), "M1025": (65, 1025)}
    for pt in C.POINTS:
        assert f"{pt}-S1" in C.CASES
        assert (f"{pt}-S2" in C.CASES) == (pt in ("K65", "K130", "K257", "K1025", "M65"))
    for name, (he, hd, le, ld, x_dim, B, k, seed) in C.CASES.items():
        assert hd == he[::-1] and ld == le[::-1][1:] + [x_dim], name
        assert seed == C.SEEDS[name]
    ids = lambda n: [v[0] for v in C.loss_variants(n)]
    for pt in ("K63", "K64", "K65", "K128", "K130", "K256", "K257", "B64", "B65", "M65", "K1024"):
        assert ids(f"{pt}-S1")[:10] == list(C.ALL_LOSSES)
    assert ids("K65-S2")[10:] == ids("K257-S2")[10:] == ["IWAE_STL", "IWAE_DREG"] and len(ids("K65-S1")) == 10
    assert ids("K17-S1") == ["IWAE", "L_median", "MIWAE"] and C.variant("K17-S1", "MIWAE")[2] == dict(k1=17, k2=1)
    assert ids("K1025-S2") == ["VAE", "IWAE", "CIWAE", "L_alpha", "L_power_p", "L_power_neg", "VAE_V1"]
    assert ids("C33-S1") == ["CIWAE"] and ids("M1025-S1") == ["IWAE"]
    assert C.variant("K128-S1", "PIWAE")[2] == dict(k1=64, k2=2)
    assert C.variant("K130-S2", "MIWAE")[2] == dict(k1=65, k2=2)
    assert C.variant("K257-S1", "MIWAE")[2] == dict(k1=257, k2=1)
    assert C.variant("K63-S1", "L_power_neg")[1:] == ("L_power_p", dict(p=-1.5))
    assert C.CASES["WIDE"][:3] == C.CASES["TIE64"][:3] == C.CASES["K65-S2"][:3]          # on S2
    assert C.CASES["WIDE"][5:7] == (3, 96) and C.CASES["TIE64"][5:7] == (3, 64) and C.CASES["TIE65"][5:7] == (3, 65)
    assert ids("WIDE") == ["IWAE", "L_power_p", "L_power_neg", "MIWAE", "CIWAE", "IWAE_DREG"]
    assert C.variant("WIDE", "MIWAE")[2] == dict(k1=48, k2=2)
    assert ids("TIE64") == ids("TIE65") == ["L_median"]
    # no loss make_plan rejects is in the table
    for name, vid in C.CASE_LOSS:
        assert not C.rejected(C.variant(name, vid)[1], C.CASES[name][6]), (name, vid)


# ------------------------------------------------------------ the rule's constants
def test_constants_match_the_sources():
    model = open(os.path.join(CSRC, "iwae_model.hip")).read()
    elem = open(os.path.join(CSRC, "iwae_elem.hip")).read()
    bound = open(os.path.join(CSRC, "iwae_bound.h")).read()
    m = re.search(r"static bool use_tc_bound\(.*?\n}", model, re.S).group(0)
    assert re.search(r"P\.kS > (\d+) \|\| P\.Bimg > (\d+) \|\| P\.need_bce \|\| P\.kl", m).groups() == \
        (str(C.TC_BOUND_K), str(C.TC_BOUND_IMAGES))
    assert "acc_off >= 64 + 8LL * r4(P.kS)" in m                     # the LDS condition (not restated)
    assert int(re.search(r"constexpr int kBoundWaves = (\d+);", elem).group(1)) == C.BOUND_WAVES
    assert 4 * C.BOUND_WAVES == C.TC_BOUND_IMAGES
    g = re.search(r"int bound_grid\(.*?\n}", elem, re.S).group(0)
    assert re.search(r"a\.Bimg <= 4 \* kBoundWaves \|\| rows <= (\d+)\) \? 1 : \(a\.Bimg \+ kBoundWaves - 1\) / kBoundWaves",
                     g).group(1) == str(C.BOUND_ROWS)
    assert "const bool staged = a.kS <= %d;" % C.STAGED_K in bound
    assert "&& a.kS > %d)" % C.STAGED_K in elem                       # launch_bound's refusal
    assert model.count("if (lc->k > %d) return fail(h, IWAE_EINVAL" % C.STAGED_K) == 2
    assert "if (rows > (1LL << 18)) return false;" in model and C.ENGINE_ROWS == 1 << 18
    assert "if (P.mode_a == BM_POWER && P.p < 0.f) return false;" in model


def test_bound_counters_are_in_the_header_and_the_library():
    hdr = " ".join(open(os.path.join(ROOT, "include", "iwae.h")).read().split()).replace(" * ", " ")
    assert "15 bound_kernel launches" in hdr
    assert "16 those of them with more than one workgroup" in hdr
    model = open(os.path.join(CSRC, "iwae_model.hip")).read()
    assert "case 15: return h->count.bound;" in model and "case 16: return h->count.bound_multi;" in model
    assert model.count("h->count.bound++;") == 1 and model.count("launch_bound(h->stream, b)") == 1


def test_both_outcomes_of_each_limit_are_covered():
    auto = {(n, v): C.expected_bound(n, v) for n, v in C.CASE_LOSS}
    home = lambda n, v="IWAE": auto[(n, v)]
    # k: 256 in, 257 out; images: 64 in, 65 out, CIWAE's 2 B counted
    assert home("K256-S1") == home("K256-S3") == ("in-launch", 0) and home("K257-S1") == ("standalone", 1)
    assert home("B64-S1") == ("in-launch", 0) and home("B65-S1") == ("standalone", 1)
    assert home("B64-S1", "CIWAE") == ("standalone", 1)              # 128 images, 512 rows
    # need_bce / kl; the losses off the engine
    for v in ("L_alpha", "VAE_V1", "L_power_neg"):
        assert home("K64-S1", v) == ("standalone", 1)
    assert home("K65-S2", "IWAE_STL") == home("K65-S2", "IWAE_DREG") == ("standalone", 1)
    assert home("K64-S1", "PIWAE") == home("K130-S2", "MIWAE") == home("K17-S1", "L_median") == ("in-launch", 0)
    # the grid rule: more than 64 images AND more than 8192 rows
    assert home("M65-S1") == home("M65-S2") == home("M1025-S1") == ("standalone", 5)
    assert home("C33-S1", "CIWAE") == ("standalone", 5)
    assert home("M65-S1", "CIWAE") == ("standalone", 9)
    assert home("K1024-S1") == ("standalone", 1) and 3 * 1024 <= C.BOUND_ROWS < 65 * 127
    assert home("K1025-S1", "CIWAE") == ("standalone", 1)             # 4 images, 4100 rows
    # off the engine, or with the knob at 0, never in the launch
    for (n, v) in C.CASE_LOSS:
        for path in ("fused", "layerwise"):
            assert C.expected_bound(n, v, path)[0] == "standalone"
        assert C.expected_bound(n, v, "auto", tc_bound=False)[0] == "standalone"
        assert C.expected_bound(n, v, "fused")[1] == C.expected_bound(n, v, "auto", tc_bound=False)[1]
    assert {h[0] for h in auto.values()} == {"in-launch", "standalone"}
    assert {h[1] > 1 for h in auto.values() if h[0] == "standalone"} == {True, False}
    several = {n for (n, v), h in auto.items() if h[1] > 1}
    assert several == {"M65-S1", "M65-S2", "C33-S1", "M1025-S1"}
    # the staged limit and the rejection beside it
    assert C.CASES["K1024-S1"][6] == C.STAGED_K and C.CASES["K1025-S1"][6] == C.STAGED_K + 1
    for loss in ("L_median", "MIWAE", "PIWAE"):
        assert C.rejected(loss, 1025) and not C.rejected(loss, 1024)
    assert not C.rejected("IWAE", 1025)
    for name in C.LDS_FALLBACK:
        assert home(name)[0] == "in-launch"


# --------------------------------------------------------------- the inputs
@pytest.mark.parametrize("name", MEDIAN_CASES)
def test_median_neighbours_are_two_log_weight_bars_away(name):
    """Every image of every L_median case (none left out): the gaps between the
    order statistics lo - 1, lo and hi, hi + 1 (a swap of lo and hi changes
    nothing) are at least 2 * 1e-4 max|lw|."""
    gaps, bar = C.median_gaps(name)
    B, k = C.CASES[name][5:7]
    assert gaps.shape == (2, B)
    print(f"{name}: smallest gap {gaps.min():.3e}, bar {bar:.3e}")
    assert bar == 2 * GPU_LW * np.abs(C.log_weights(name)).max()
    assert (gaps >= bar).all(), (gaps.min(), bar)


def test_median_cases_are_all_there():
    assert set(MEDIAN_CASES) == {n for n in C.CASES if n not in C.CONSTRUCTED and C.POINT_OF[n] not in
                                 ("K1025", "C33", "M1025")} | set(C.TIES)
    assert C.CASES["K1024-S1"][5] == 3 and C.CASES["M65-S2"][5] == 65


@pytest.mark.parametrize("name", C.TIES)
def test_tie_construction_gives_exactly_equal_rows(name):
    """The copy of the rank-(k-1)//2 sample's noise holds the next rank with a
    bit-identical float64 log-weight: for even k the two middle order statistics."""
    lw = C.log_weights(name)
    k, B = lw.shape
    lo, hi = O.median_indices(k)
    srt = np.sort(lw, axis=0)
    assert (srt[lo] == srt[lo + 1]).all()
    if k % 2 == 0:
        assert hi == lo + 1 and (srt[lo] == srt[hi]).all()
    assert (srt[lo - 1] < srt[lo]).all() and (srt[lo + 1] < srt[lo + 2]).all()      # one pair, not more
    order = np.argsort(lw, axis=0, kind="stable")
    eps = C.make(name)[4]
    for b in range(B):
        for e in eps:
            np.testing.assert_array_equal(e[order[lo, b], b], e[order[lo + 1, b], b])
    # the draw before the overwrite: its largest sample is gone from the top
    he, hd, le, ld, x_dim, _, _, seed = C.CASES[name]
    spec, params, _, x, eps0 = R.make_case((he, hd, le, ld), B, k, seed, x_dim=x_dim)
    lw0 = O.forward(params, spec, x, eps0)["lw"]
    assert ((lw != lw0).sum(axis=0) == 1).all() and (lw.max(axis=0) < lw0.max(axis=0)).all()


def test_the_last_index_carries_the_largest_or_the_median_log_weight():
    """k > 64: sample k - 1, which only the last pass of a loop q = lane; q < k;
    q += 64 reaches, is the image's largest log-weight (even images) or its median
    (odd images), in the first draw and in CIWAE's second."""
    seen = 0
    for name in C.CASES:
        spec, params, _, x, eps = C.make(name)
        k = C.CASES[name][6]
        if k <= 64 or name in C.TIES:
            continue
        draws = [eps] + ([C.second_draw(name)] if any(v[0] == "CIWAE" for v in C.loss_variants(name)) else [])
        for d in draws:
            rank = np.argsort(np.argsort(O.forward(params, spec, x, d)["lw"], axis=0, kind="stable"), axis=0)[k - 1]
            assert (rank[0::2] == k - 1).all() and (rank[1::2] == (k - 1) // 2).all(), name
            seen += 1
    assert seen >= 20


def test_wide_spread():
    lw = C.log_weights("WIDE")
    spread = lw.max(axis=0) - lw.min(axis=0)
    sm = np.exp(lw - lw.max(axis=0))
    ess = sm.sum(axis=0) ** 2 / (sm * sm).sum(axis=0)
    under = (np.exp((lw - lw.max(axis=0)).astype(np.float32)) == 0).sum(axis=0)
    print(f"WIDE: spreads {np.round(spread, 1)} nats, effective sample sizes {np.round(ess, 2)}, "
          f"samples whose float32 exp(lw - max) is 0: {under}")
    assert spread.min() >= 60.0 and spread.max() >= 90.0
    assert under.max() > 0
    he, hd, le, ld, x_dim, B, k, seed = C.CASES["WIDE"]
    plain = R.make_case((he, hd, le, ld), B, k, seed, x_dim=x_dim)[1]
    w, w0 = C.make("WIDE")[1]["out.l3"][0], plain["out.l3"][0]
    np.testing.assert_array_equal(w, (w0 * 8).astype(np.float32).astype(np.float64))


# --------------------------------------------------------- reference fairness
@pytest.mark.parametrize("name,vid", C.CASE_LOSS, ids=["-".join(c) for c in C.CASE_LOSS])
def test_float32_reference_within_a_quarter_of_the_gpu_bars(name, vid):
    """As tests/test_shape_cases.py: the reference's own train step in float32
    arithmetic against float64."""
    spec = C.make(name)[0]
    l64, g64, w64 = C.reference_step(name, vid)
    l32, g32, w32 = C.reference_step(name, vid, np.float32)
    whole = R.rel_l2(g32, g64)
    # (VAE_V1 gives the decoder's prior layers an exactly zero gradient: 0 / tiny = 0)
    per = max(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)
              for a, b in zip(R.split_tensors(spec, g32), R.split_tensors(spec, g64)))
    adam = np.abs(w32 - w64).max()
    print(f"{name} {vid}: float32 loss rel {abs(l32 - l64) / abs(l64):.2e}, gradient rel-L2 {whole:.2e}, "
          f"per tensor {per:.2e}, post-Adam weights {adam:.2e}")
    assert np.isfinite(g32).all()
    assert abs(l32 - l64) <= GPU_REL / 4 * abs(l64)
    assert whole <= GPU_REL / 4, whole
    assert per <= GPU_TENSOR / 4, per
    assert adam <= max(GPU_ADAM_ATOL, 10 * np.abs(g32 - g64).max()) / 4, adam


@pytest.mark.parametrize("name", list(C.CASES))
def test_float32_log_weights_within_a_quarter_of_the_gpu_bar(name):
    spec, params, _, x, eps = C.make(name)
    lw64 = C.log_weights(name)
    lw32 = O.forward(O.cast_params(params, np.float32), spec, x.astype(np.float32),
                     [e.astype(np.float32) for e in eps])["lw"]
    err = np.abs(lw32 - lw64).max() / np.abs(lw64).max()
    print(f"{name}: float32 log-weights {err:.2e} of max|lw|")
    assert err <= GPU_LW / 4, err


@pytest.mark.parametrize("model", ["S1", "S2"])
def test_float32_log_px_within_a_quarter_of_the_gpu_bar(model):
    """The log p(x) cases (k beside the NLL reductions' edges): 1e-3 nats on the GPU."""
    assert C.NLL_KS == (1, 63, 65, 127, 128, 2047, 2049) and C.NLL_B == 3
    for k in C.NLL_KS:
        err = np.abs(C.nll_reference(model, k, np.float32) - C.nll_reference(model, k)).max()
        print(f"{model} k = {k}: float32 log p(x) {err:.2e} nats")
        assert err <= 1e-3 / 4, (k, err)
