"""The latent-space shape sweep (tests/latent_shape_cases.py) without a GPU: the
constants expected() restates against the library's sources, the edges the
table reaches, and the fairness of the references the GPU tests
(tests/test_gpu_latent_shapes.py) compare with: the float32 run and the bf16x3
emulation within a quarter of every GPU bar, the HMC / AIS cases under the
existing searches and conditions, the refinement runs under
refine_ref.emulated_case.

Seeds passed over (worst figure over the latent sets, quantities and both
arithmetics, of the quarter 2.5e-5; the order is seed + 1000 j, j = 0 .. 7, and
a seed is taken at 0.9 of the quarter or less):
  LT1  j = 0: 4.08e-5 (the bf16x3 px gradient, a single number), j = 1: 7.62e-5, j = 2: 1.72e-5 taken
  LD5  j = 0: 2.490e-5 (the bf16x3 q gradient), j = 1: 2.523e-5, j = 2: 2.445e-5, j = 3: 1.68e-5 taken
Every other case keeps j = 0; the largest of them are LD8 2.08e-5 (ph gradient)
and LD4 2.01e-5 (q gradient).  No case needs SH's rule (a bar of twice the
emulation's figure)."""
import os
import re

import numpy as np
import pytest

import ais_ref as A
import latent_shape_cases as LS
import observed_ref as OB
import pathgrad_ref as PR
import refine_ref as RF
import score_ref as R
import scoregrad_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "iwae_replication_project_amd", "csrc")
BAR = 1e-4
QUARTER = BAR / 4
T = len(A.BETAS) - 1


def _src(name):
    return open(os.path.join(CSRC, name)).read()


# ------------------------------------------------------------ the rules' constants
def test_constants_match_the_sources():
    hdr, model, refine, dev = _src("iwae_kernels.h"), _src("iwae_model.hip"), _src("iwae_refine.hip"), _src("iwae_mega_dev.h")

    def const(src, name):
        return int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))
    for name in ("kSgMaxStages", "kSgOutTiles", "kSgWaves", "kMgMaxStages", "kMgMaxBufs"):
        assert const(hdr, name) == getattr(LS, name), name
    assert const(refine, "kCols") == LS.kCols
    assert const(dev, "MG_KS") == LS.MG_KS
    assert LS.kLdsBytes == 160 * 1024
    assert "if (bytes <= 160 * 1024) {" in model                              # sgrad_plan
    assert "if (bytes <= (waves == 4 ? 80 : 160) * 1024) {" in model          # mega_plan
    assert model.count("a.group = dmax <= %d ? 16 : 64;" % LS.kGroupSwitch) == 2      # ais_core, refine_core
    assert "if (nb > kMgMaxBufs || L > %d) return false;" % LS.kSgMaxLayers in model
    assert "if ((d3.fin + 15) / 16 > kSgOutTiles * kSgWaves) return false;" in model
    assert "W.widen(bP, %d);" % LS.kOutSlab in model
    assert "W.widen(bP, std::max(gk, 2 * C.d));" in model
    assert "while (fallback ? sdw % 8 != 4 : sdw % 16 != 8) ++sdw;" in model
    assert model.count("for (int c : {4, 2, 1}) {") >= 2                      # 64 / 32 / 16 rows, both plans
    assert "foff = std::max(foff, 3 * kSgWaves * R);" in model
    assert "S.g_ld[i] = h->enc[i].d | 1;" in model
    assert "d.ldF = (fin + 1 + 31) & ~31;" in model and "d.ldG = (fout + 31) & ~31;" in model
    assert "d.gx_steps = d.ldG / 32;" in model
    sg = _src("iwae_scoregrad.hip")
    assert "const int ns = min(MG_KS, (L.out_gx_ldk - %d * c) >> 5);" % LS.kOutSlab in sg
    assert "const int t2 = wave + q * NW;" in sg
    pub = open(os.path.join(ROOT, "include", "iwae.h")).read()
    assert int(re.search(r"#define IWAE_MAX_LAYERS (\d+)", pub).group(1)) == len(LS.CASES["LD8"][0]) == LS.kSgMaxLayers


def test_cases_are_small_mirrored_and_registered_beside_the_existing_ones():
    assert list(R.CASES) == list(PR.SHAPES) + ["K130", "C784", "SH"]
    assert A.SHAPES == ("S1", "S2", "S3", "S4", "K130", "C784")
    assert RF.SHAPES == ("S1", "S2", "S3", "S4", "C784", "K300")
    assert not set(LS.CASES) & set(R.CASES) and not {"O" + n for n in LS.MASKED} & set(OB.CASES)
    assert not set(LS.AIS_CASES) & set(A.AIS_CASES) and not set(LS.HMC_CASES) & set(G.HMC_CASES)
    seeds = set()
    for name, (he, hd, le, ld, x_dim, B, k, seed) in LS.CASES.items():
        assert B * k <= 66, name
        assert hd == he[::-1] and ld == le[::-1][1:] + [x_dim], name
        spec, params, x, eps = R.case(name)
        assert spec.x_dim == x_dim and list(spec.n_latent_encoder) == le and x.shape == (B, x_dim)
        assert [e.shape for e in eps] == [(k, B, d) for d in le]
        assert R.entry(name)[:3] == ((he, hd, le, ld), B, k)
        seeds |= {seed, seed + 1, seed + 2}
    assert len(seeds) == 3 * len(LS.CASES)                        # no two cases share a generator seed
    for name in LS.MASKED:
        spec, params, x, mask, _, x_full = OB.case("O" + name)
        assert mask.shape == x.shape and not mask[0].any() and mask[1].all()
        assert np.isnan(x[mask == 0]).all() and np.array_equal(x_full, R.case(name)[2])


# ----------------------------------------------------------------- reachability
def test_every_edge_is_reached():
    full = {n: LS.expected(n, coef=(1.0, 1.0, 1.0)) for n in LS.CASES}
    px = {n: LS.expected(n, coef=(0.0, 0.0, 1.0)) for n in LS.CASES}
    q = {n: LS.expected(n, coef=(1.0, 0.0, 0.0)) for n in LS.CASES}
    post = {n: LS.expected(n) for n in LS.CASES}
    # row tiles: all three instantiations of sg_kernel, and of its MASK variant on the masked cases
    assert {e["sgrad_rows"] for e in px.values()} == {0, 64, 32, 16}
    assert [px[n]["sgrad_rows"] for n in LS.MASKED] == [64, 32, 16]
    assert px["LW400"]["sgrad_rows"] == 32 and px["LW512"]["sgrad_rows"] == 16 and px["LZ260"]["sgrad_rows"] == 32
    assert {e["score_rows"] for e in px.values()} >= {64, 32}
    # SG_OUT's dY2 column tiles: q up to 3, and both sides of kSgOutTiles * kSgWaves
    assert px["LW400"]["out_tiles_per_wave"] == LS.kSgOutTiles and px["LW400"]["out_tiles"] == 25
    assert px["LW512"]["out_tiles"] == LS.kSgOutTiles * LS.kSgWaves and px["LW512"]["sgrad_fused"]
    assert px["LW528"]["out_tiles"] == LS.kSgOutTiles * LS.kSgWaves + 1
    assert not px["LW528"]["sgrad_fused"] and px["LW528"]["sgrad_reason"] == "out_tiles" and px["LW528"]["score_fused"]
    assert q["LW528"]["sgrad_fused"] and not post["LW528"]["sgrad_fused"] and not full["LW528"]["sgrad_fused"]
    # (a value alone does not need the backward half: log_px asked for with c_px = 0 stays fused)
    assert LS.expected("LW528", coef=(0.0, 1.0, 0.0), values=("px",))["sgrad_fused"]
    # depth: both sides of each stage limit
    assert full["LD4"]["stages"] == LS.full_stages(4) == 41 <= LS.kSgMaxStages < LS.full_stages(5) == 53
    assert full["LD4"]["mega_stages"] == 21 <= LS.kMgMaxStages < full["LD5"]["mega_stages"] == 27
    assert full["LD4"]["sgrad_fused"] and full["LD4"]["score_fused"]
    for n in ("LD5", "LD8"):
        assert not full[n]["score_fused"] and not full[n]["sgrad_fused"] and full[n]["sgrad_reason"] == "mega_stages"
        # ... and sgrad_plan alone refuses them too
        assert LS.sgrad_plan(n, (True, True, True), (1.0, 1.0, 1.0))["reason"] == "stages"
    assert len(LS.CASES["LD8"][0]) == LS.kSgMaxLayers
    # pixels: x_dim off 4 and off 16, a second slab, a last slab shorter than 16 pixels
    assert {LS.CASES[n][4] % 4 for n in LS.CASES} == {0, 1, 2, 3}
    assert any(LS.CASES[n][4] % 16 for n in LS.SCORE_CASES)
    assert px["LW400"]["pixel_slabs"] == 2 and 0 < px["LW400"]["last_slab_pixels"] < 16 and px["LW400"]["last_slab_ns"] == 1
    assert all(px[n]["pixel_slabs"] == 1 for n in LS.CASES if n != "LW400")
    # widths: odd hidden widths; every residue of d mod 4, d = 1, d < 4, d > kCols, either side of the group switch
    assert any(w % 2 for n in LS.SCORE_CASES for w in LS.CASES[n][0])
    ds = {d for n in LS.CASES for d in LS.CASES[n][2]}
    assert {d % 4 for d in ds} == {0, 1, 2, 3} and 1 in ds and 3 in ds
    assert max(LS.CASES["LZ260"][2]) > LS.kCols and "LZ260" in LS.REFINE_CASES
    assert max(LS.CASES["LZ64"][2]) == LS.kGroupSwitch and max(LS.CASES["LZ65"][2]) == LS.kGroupSwitch + 1
    assert ("LZ64", "prior") in LS.AIS_CASES and ("LZ65", "prior") in LS.AIS_CASES
    # an upper layer with 2 d > 256: buffer P wider than the output chain's slab
    assert q["LZ2"]["p_width"] == 288 > LS.kOutSlab == px["LZ2"]["p_width"] and q["LZ2"]["sgrad_fused"]
    # paths: layerwise is never fused; f32 products never are
    for n in LS.CASES:
        e = LS.expected(n, path="layerwise")
        assert not e["score_fused"] and not e["sgrad_fused"] and e["sgrad_reason"] == "path"
        assert not LS.expected(n, precision="f32")["score_fused"]
    assert LS.CASES[LS.CHUNK_CASE][5] % LS.CHUNK and LS.CASES[LS.CHUNK_CASE][5] > 32


# ------------------------------------------------------------------------ bars
@pytest.mark.parametrize("name", list(LS.CASES))
def test_float32_and_bf16x3_emulation_stay_within_a_quarter_of_the_gpu_bars(name):
    """A condition on the GPU tests' inputs, not a measurement of the GPU code: score_ref.score and
    scoregrad_ref.grads in float32 and with the emulated products, every latent set."""
    fig = LS.figures(name)
    print(name, {a: {k: f"{v:.2e}" for k, v in d.items()} for a, d in fig.items()})
    for arith, d in fig.items():
        for key, v in d.items():
            assert v <= QUARTER, (arith, key, v)


@pytest.mark.parametrize("name", list(LS.CASES))
def test_seed_is_the_first_of_the_fixed_order_the_emulation_accepts(name):
    taken = [t[6] for t in LS._TABLE if t[0] == name][0]
    assert taken < LS.SEED_TRIES
    for j in range(taken + 1):
        fig = LS.figures(LS.candidate(name, j))
        worst = max(max(d.values()) for d in fig.values())
        print(f"{name} j = {j}: {worst:.3e}")
        assert (worst <= LS.SELECT) == (j == taken), (j, worst)
    pos = [t[0] for t in LS._TABLE].index(name)
    assert LS.CASES[name][7] == LS.SEED0 + 10 * pos + 1000 * taken


@pytest.mark.parametrize("which", R.LATENTS)
@pytest.mark.parametrize("name", LS.MASKED)
def test_masked_references_stay_within_a_quarter(name, which):
    oname = "O" + name
    spec, params, x, mask, _, _ = OB.case(oname)
    h, ref, gref = OB.latents(oname, which), OB.reference(oname, which), OB.grad_reference(oname, which)
    for kw in (dict(dtype=np.float32), dict(dtype=np.float32, dense=R.dense_bf16x3)):
        sc = OB.score(params, spec, x, mask, h, **kw)
        for key, sk in (("logq", "Sq"), ("logp", "Sp"), ("logpx", "Spx")):
            err = np.abs(np.asarray(sc[key], np.float64) - ref[key])
            live = ref[sk] > 0
            assert not np.asarray(sc[key])[~live].any()                       # no observed addend: exactly 0
            assert err.max() <= QUARTER * np.abs(ref[key]).max() and (err[live] / ref[sk][live]).max() <= QUARTER, key
        g = OB.grads(params, spec, x, mask, h, **kw)
        for t in G.TERMS:
            for a, b in zip(g[t], gref[t]):
                r = G.rel_l2(a, b)
                assert (not np.asarray(a).any()) if r is None else r <= QUARTER, (t, r)
    assert not gref["px"][0][:, 0].any() and gref["px"][0][:, 1].any()      # image 0 has no observed pixel


# ------------------------------------------------------------------------- HMC
@pytest.mark.parametrize("name", list(LS.HMC_CASES))
def test_hmc_case_is_the_searchs_and_the_emulation_decides_as_float64(name):
    assert LS.hmc_search(name) == LS.HMC_CASES[name] == G.hmc_entry(name)
    out = G.hmc_case(name)
    big, na, nr, margin = LS.hmc_conditions(out)
    print(f"[{name}] max|dH| {big:.2f}, accepted {na}, rejected {nr}, margin {margin:.2f}")
    assert big < 5.0 and na >= 1 and nr >= 2 and margin >= 0.4 - 1e-12
    spec, params, x, _ = R.case(name)
    step, nl, _ = LS.HMC_CASES[name]
    r, q, H0, H1, lu, acc = out
    _, E0, E1 = G.hmc_step(params, spec, x, R.latents(name, "on"), r, step, nl, dtype=np.float32, dense=R.dense_bf16x3)
    d = np.abs((E1 - E0) - (H1 - H0)).max()
    print(f"[{name}] emulated dH off by {d:.2e}")
    assert d <= 0.1, d


# ------------------------------------------------------------------------- AIS
@pytest.mark.parametrize("name,init", list(LS.AIS_CASES))
def test_ais_case_is_the_searchs_and_meets_the_conditions(name, init):
    assert A.search(name, init) == LS.AIS_CASES[name, init] == A.ais_entry(name, init)
    out = A.ais_case(name, init)
    big, nrej = A.conditions(out)
    print(f"[{name} {init}] max|dH| {big:.2f}, transitions with a rejection {nrej}, accept rate {out['accept'].mean():.2f}")
    assert big < 5.0 and nrej >= 2
    assert np.abs(out["log_u"] + out["dH"]).min() >= 0.4 - 1e-9
    assert (out["log_u"] <= -1e-3).all()
    u = np.exp(out["log_u"]).astype(np.float32)
    assert ((u > 0) & (u < 1)).all()
    assert out["accept"].any() and not out["accept"].all()
    np.testing.assert_array_equal(out["accepts"], out["accept"].sum(0))
    assert (out["accepts"] == 0).any() or (out["accepts"] < T).any()


@pytest.mark.parametrize("name,init", list(LS.AIS_CASES))
def test_ais_emulation_decides_as_float64_and_stays_within_a_quarter(name, init):
    ref, emu = A.ais_case(name, init), A.emulated_case(name, init)
    np.testing.assert_array_equal(emu["accept"], ref["accept"])
    np.testing.assert_array_equal(emu["step"], ref["step"])
    ew = np.abs(emu["log_w"] - ref["log_w"]).max() / np.abs(ref["log_w"]).max()
    eh = [np.abs(a - b).max() / np.abs(b).max() for a, b in zip(emu["h"], ref["h"])]
    print(f"[{name} {init}] emulation: log_w {ew:.2e} of max|ref|, latents {max(eh):.2e} of max|ref|")
    assert ew <= QUARTER and max(eh) <= QUARTER, (ew, eh)


# ---------------------------------------------------------------------- refine
def _of_max(got, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("objective", RF.OBJECTIVES)
@pytest.mark.parametrize("name", LS.REFINE_CASES)
def test_refine_emulation_stays_within_a_quarter(name, objective):
    ref, emu = RF.refine_case(name, objective), RF.emulated_case(name, objective)
    fig = {n: max(_of_max(a, b) for a, b in zip(emu[n], ref[n])) for n in ("mean", "logstd")}
    fig["bound"] = _of_max(emu["bound"], ref["bound"])
    fig["log_w"] = _of_max(emu["log_w"], ref["log_w"])
    fig["grad"] = RF.grad_errors(*emu["grads"][0], ref)
    print(f"[{name} {objective}] " + ", ".join(f"{n} {v:.2e}" for n, v in fig.items()))
    for n, v in fig.items():
        assert v <= QUARTER, (n, v)


@pytest.mark.parametrize("objective", RF.OBJECTIVES)
def test_refine_reference_moves_the_columns_of_the_second_round(objective):
    m0, s0, _ = RF.setting("LZ260")
    ref = RF.refine_case("LZ260", objective)
    assert (np.abs(ref["mean"][0][:, LS.kCols:] - m0[0][:, LS.kCols:]) > 1e-2).all()
    assert (np.abs(ref["logstd"][0][:, LS.kCols:] - s0[0][:, LS.kCols:]) > 1e-2).all()
