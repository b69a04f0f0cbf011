"""The wake-sleep and masked-step shape sweep (tests/step_shape_cases.py) without
a GPU: the constants expected() restates against the library's sources, the
branches the tables reach, the fairness of every input the GPU tests
(tests/test_gpu_step_shapes.py) run on -- the float64 reference in float32
arithmetic within a quarter of every GPU bar, both phases carrying weight, masks
that matter -- and the proof that the parity comparisons bite: deliberately wrong
references miss the bars by a wide margin.

Worst float32-reference figures over all cases (values / loss, whole gradient,
worst tensor): 2.1e-7, 2.6e-6, 9.0e-6 against quarters of 2.5e-5, 2.5e-5,
1.25e-4.  No seed is passed over: every case keeps shape_cases' seed."""
import os
import re

import numpy as np
import pytest

import missing_ref as M
import pathgrad_ref as PR
import shape_cases as S
import step_shape_cases as SS
import wakesleep_ref as W
from oracle import iwae_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "iwae_replication_project_amd", "csrc")

WS = [(n, c) for n in SS.WS_CASES for c in SS.WS_COEFS[n]]             # what the GPU tests run
WS_ALL = [(n, c) for n in SS.WS_CASES for c in W.COEFS]                 # fairness: every coefficient pair
WS_ALL_IDS = [f"{n}-{SS.COEF_ID[c]}" for n, c in WS_ALL]
MASKED = [(n, l) for n in SS.MASKED_CASES for l in SS.MASKED_LOSSES[n]]
MASKED_IDS = [f"{n}-{l}" for n, l in MASKED]
MIX = W.COEFS[2]


# ------------------------------------------------------------ the rules' constants
def test_constants_match_the_sources():
    src = open(os.path.join(CSRC, "iwae_model.hip")).read() + open(os.path.join(CSRC, "iwae_kernels.h")).read()

    def const(name):
        return int(re.search(r"constexpr \w+ (?:\w+ = \d+, )?%s = (\d+)" % name, src).group(1))
    assert const("kRbMaxJobs") == SS.kRbMaxJobs and const("kRbMaxWidth") == SS.kRbMaxWidth
    # ws_use_fused: the gates expected() restates, with the automatic path's row limit
    body = re.search(r"static bool ws_use_fused\(const iwae_handle\* h, long long rows\) \{(.*?)\n\}", src, re.S).group(1)
    assert "h->path == 1 || h->L > kRbMaxJobs || h->masked || !rb_width_ok(h)" in body
    assert "return h->path == 2 || rows <= %d;" % SS.RB_ROWS in body
    assert "ws_use_fused(h, (long long)M + n)" in src
    # use_fused on a masked step: the same rule, and the engine never
    assert "P.Bimg * P.kS <= %d;" % SS.RB_ROWS in src
    assert "if (P.pix) return false;" in src
    # rb_width_ok: fin + 1 and fout + 1 of every Dense but the first and the last
    assert "if (d.fin + 1 > kRbMaxWidth || d.fout + 1 > kRbMaxWidth) return 0;" in src
    # smallm_ok
    assert re.search(r"int smallm_rows = (\d+);", src).group(1) == str(SS.SMALLM_ROWS)
    assert "rows > std::min(h->tune.smallm_rows, %d)" % SS.SMALLM_ROWS in src
    assert "fin + 1 > %d || h->dense[di].fout > %d" % (SS.SMALLM_WIDTH, SS.SMALLM_WIDTH) in src
    # the decisions the row-count cases separate
    assert "const bool direct = fusedp && smallm_ok(h, P.Bimg);" in src
    assert "const bool sm0 = i == 0 && smallm_ok(h, rows);" in src
    assert "const bool per_image = wake && P.kS > 1;" in src
    assert "rows = (i == 0 ? B : M) + n - off;" in src
    # the output layer on bf16x3 products: both steps decide on the wake / sample rows
    assert re.search(r"long long out_x3_rows = (\d+);", src).group(1) == "8192"
    assert "(long long)M >= h->tune.out_x3_rows" in src and "P.Bimg * P.kS >= h->tune.out_x3_rows" in src


def test_cases_reuse_shape_cases_models_and_sit_beside_the_existing_ones():
    for name in SS.MODELS:
        he, hd, le, ld, x_dim, B, k, seed = S.CASES[name]
        assert SS.WS_CASES[name] == (he, hd, le, ld, x_dim, B, k, SS.WS_N[name], seed)
        mB, mk = SS.MASKED_T1 if name == "T1" else (B, k)
        assert SS.MASKED_CASES[name] == (he, hd, le, ld, x_dim, mB, mk, seed)
    for name, (B, k, n) in SS.ROW_CASES.items():
        assert SS.WS_CASES[name] == S.CASES["O2"][:5] + (B, k, n, 1303)
    assert not SS.TRIES
    assert not set(SS.WS_CASES) & set(W.CASES) and not set(SS.MASKED_CASES) & set(M.SHAPES)
    assert list(W.CASES) == ["W1", "W2", "W2w", "W3", "W4"]
    assert list(M.SHAPES) == ["M1", "M2", "M2w", "M50", "M50w", "M784", "M784k"]
    for name, e in SS.WS_CASES.items():
        (he, hd, le, ld), B, k, n, (spec, params, mean, x, eps, (xd, hd_)) = SS.ws_case(name)
        assert (he, hd, le, ld, spec.x_dim, B, k, n) == e[:8]
        assert B * k + n <= 300, name
        assert x.shape == (B, e[4]) and xd.shape == (n, e[4]) and [v.shape for v in hd_] == [(n, d) for d in le]
        # the dreams are wakesleep_ref.make_dreams' at the case's seed + 50000
        again = W.make_dreams(spec, mean, n, np.random.default_rng(e[8] + 50000))
        assert np.array_equal(again[0], xd) and all(np.array_equal(a, b) for a, b in zip(again[1], hd_))
        # and the model, images and noise are shape_cases' own
        if name in SS.MODELS:
            ref = S.make(name)
            assert np.array_equal(O.flatten_params(spec, params), O.flatten_params(ref[0], ref[1]))
            assert np.array_equal(x, ref[3]) and all(np.array_equal(a, b) for a, b in zip(eps, ref[4]))
    for name, e in SS.MASKED_CASES.items():
        arch, B, k, x_dim, (spec, params, _, x, eps, eps2, mask) = SS.masked_case(name)
        assert (list(arch[0]), list(arch[1]), list(arch[2]), list(arch[3]), x_dim, B, k) == e[:7]
        assert B * k <= 300, name
        assert np.array_equal(mask, M.make_mask(B, x_dim, e[7] + 2))
        assert np.isnan(x[mask == 0]).all() and np.isfinite(x[mask != 0]).all()
        assert not mask[0].any() and mask[1].all()


# -------------------------------------------------------------- branch coverage
def test_every_untested_branch_is_reached():
    E = {n: {p: SS.expected(n, e, p) for p in ("auto", "fused", "layerwise")} for n, e in SS.WS_CASES.items()}
    Em = {n: {p: SS.expected(n, e, p) for p in ("auto", "fused", "layerwise")} for n, e in SS.MASKED_CASES.items()}
    # 1. the three gates of ws_use_fused / use_fused: depth, width, a "fused" request that falls to layer-wise
    for X in (E, Em):
        for n in ("D5", "D8", "W512"):
            assert not any(X[n][p]["row_block"] for p in X[n]), n
        for n in ("D4", "W511"):
            assert X[n]["auto"]["row_block"] and X[n]["fused"]["row_block"] and not X[n]["layerwise"]["row_block"], n
        for n in X:
            assert not X[n]["layerwise"]["row_block"]
            assert X[n]["auto"]["row_block"] == X[n]["fused"]["row_block"]         # no case near RB_ROWS
    assert len(SS.WS_CASES["D4"][0]) == SS.kRbMaxJobs == len(SS.WS_CASES["D5"][0]) - 1
    assert SS.WS_CASES["W511"][0][0] + 1 == SS.kRbMaxWidth == SS.WS_CASES["W512"][0][0]
    for n in ("D5", "D8", "W512"):
        assert E[n]["fused"]["fit_counter"] == 37
    # 2. odd widths and widths below 32; x_dim % 4 != 0 under every wake-sleep launch that reads or writes image rows
    he, _, le, _, x_dim = SS.WS_CASES["O2"][:5]
    assert all(w % 2 and w < 32 for w in he + le) and x_dim % 4 == 1
    assert SS.WS_CASES["O1"][4] % 4 == 2 and SS.WS_CASES["O2w"][4] % 4 == 2
    assert E["O1"]["auto"]["x_direct"] and E["O2"]["auto"]["x_direct"]              # the few-row launch reads x
    assert not E["O2w"]["auto"]["x_direct"] and not E["R40p5"]["auto"]["x_direct"]  # copy_x above 32 images
    assert {SS.MASKED_CASES[n][4] % 4 for n in SS.MASKED_CASES} == {0, 1, 2}
    assert sum(SS.MASKED_CASES[n][4] % 2 for n in SS.MASKED_CASES) >= 2             # odd x_dim: T1 (5), O2 (37)
    # 4. the output Dense on bf16x3 products: at the default knob no case, at 16 rows O2w's 66
    assert not any(E[n]["auto"]["out_x3"] for n in E) and not any(Em[n]["auto"]["out_x3"] for n in Em)
    for cases in (SS.WS_CASES, SS.MASKED_CASES):
        e = cases[SS.OUT_X3_CASE]
        assert SS.expected(SS.OUT_X3_CASE, e, "fused", out_x3_rows=SS.OUT_X3_ROWS)["out_x3"]
        assert not SS.expected(SS.OUT_X3_CASE, e, "fused", out_x3_rows=0)["out_x3"]
        assert e[5] * e[6] == 66 and e[1][-1] % 32 != 0 and e[4] % 32 != 0         # widths off 32: the padded split copy


def test_row_count_cases_reach_what_the_table_says():
    """3. of the list, from smallm_ok's rule (rows <= 32, first-layer widths <= 1024) alone."""
    wake, sleep, mix = W.COEFS
    ex = lambda n, coef: SS.expected(n, SS.WS_CASES[n], "auto", coef)
    for n in SS.ROW_CASES:
        e = SS.WS_CASES[n]
        assert all(fin + 1 <= 1024 and fout <= 1024 for fin, fout in SS.dense_layers(e)[:3])
        assert ex(n, mix)["row_block"]
    # R20p20: each phase few-row; under the mix the joint fit has 40 image rows; wake-only and sleep-only keep 20
    r = ex("R20p20", mix)
    assert r["wake_few_row"] and r["sleep_few_row"] and r["fit_rows"] == 40 and not r["fit_few_row"]
    assert ex("R20p20", wake)["fit_rows"] == 20 and ex("R20p20", wake)["fit_few_row"]
    assert ex("R20p20", sleep)["fit_rows"] == 20 and ex("R20p20", sleep)["fit_few_row"]
    # R5p40: x read directly; the dreams beyond the few-row launches (split-K GEMM + row-block job) behind 5 rows
    r = ex("R5p40", mix)
    assert r["x_direct"] and r["wake_few_row"] and not r["sleep_few_row"] and not r["fit_few_row"]
    assert not ex("R5p40", sleep)["fit_few_row"] and ex("R5p40", sleep)["fit_rows"] == 40
    assert ex("R5p40", wake)["fit_few_row"]
    # R40p5: copy_x of a 37-wide image, the dreams few-row behind 40 rows
    r = ex("R40p5", mix)
    assert not r["x_direct"] and not r["wake_few_row"] and r["sleep_few_row"] and not r["fit_few_row"]
    assert ex("R40p5", sleep)["fit_few_row"] and ex("R40p5", sleep)["fit_rows"] == 5
    assert SS.WS_CASES["R40p5"][4] == 37
    # Rk1: per_image false although the wake phase runs
    assert not ex("Rk1", mix)["per_image"] and not ex("Rk1", wake)["per_image"]
    assert all(ex(n, mix)["per_image"] for n in SS.ROW_CASES if n != "Rk1")
    assert not any(ex(n, sleep)["per_image"] for n in SS.ROW_CASES)
    # R32p1: the boundary itself; the fit has 33 rows
    r = ex("R32p1", mix)
    assert SS.WS_CASES["R32p1"][5] == SS.SMALLM_ROWS
    assert r["x_direct"] and r["wake_few_row"] and r["sleep_few_row"] and r["fit_rows"] == 33 and not r["fit_few_row"]
    assert ex("R32p1", wake)["fit_few_row"]
    # the remaining model cases: k >= 2 everywhere but T1, whose k = 1 is a second per_image-false case
    assert SS.WS_CASES["T1"][6] == 1
    # O2w: more than 32 images and more than 32 dreams
    r = SS.expected("O2w", SS.WS_CASES["O2w"], "auto")
    assert not r["wake_few_row"] and not r["sleep_few_row"] and not r["fit_few_row"]


# --------------------------------------------------------- reference fairness
@pytest.mark.parametrize("name,coef", WS_ALL, ids=WS_ALL_IDS)
def test_wake_sleep_float32_reference_within_a_quarter_of_the_gpu_bars(name, coef):
    """A condition on the GPU tests' inputs, not a measurement of the GPU code."""
    fig = SS.ws_figures(name, coef)
    print(f"{name} {coef}: float32 reference values rel {fig[0]:.2e}, whole rel-L2 {fig[1]:.2e}, worst tensor {fig[2]:.2e}")
    assert SS.within(fig, 0.25), fig
    v32, v64 = SS.ws_reference(name, coef, np.float32)[0], SS.ws_reference(name, coef)[0]
    for a, b, c in zip(v32, v64, (1.0,) + coef):
        assert (a == 0) == (b == 0) == (c == 0)


@pytest.mark.parametrize("name,loss", MASKED, ids=MASKED_IDS)
def test_masked_float32_reference_within_a_quarter_of_the_gpu_bars(name, loss):
    fig = SS.masked_figures(name, loss)
    print(f"{name} {loss}: float32 reference loss rel {fig[0]:.2e}, whole rel-L2 {fig[1]:.2e}, worst tensor {fig[2]:.2e}")
    assert SS.within(fig, 0.25), fig


def _worst(family, name):
    if family == "ws":
        figs = [SS.ws_figures(name, c) for c in W.COEFS]
    else:
        figs = [SS.masked_figures(name, l) for l in SS.MASKED_LOSSES[name.split("@")[0]]]
    return max(max(f[0], f[1]) / SS.GPU_REL for f in figs), max(f[2] / SS.GPU_TENSOR for f in figs)


@pytest.mark.parametrize("family,name", [("ws", n) for n in SS.WS_CASES] + [("masked", n) for n in SS.MASKED_CASES])
def test_seed_is_the_first_of_the_fixed_order_the_float32_reference_accepts(family, name):
    """Seeds seed + 1000 j before the one taken miss 0.9 of the quarter; the one taken keeps it."""
    taken = SS.TRIES.get(name if family == "ws" else "M:" + name, 0)
    assert taken < SS.SEED_TRIES
    for j in range(taken + 1):
        a, b = _worst(family, name if j == taken else SS.candidate(family, name, j))
        if j < taken:
            print(f"{family} {name}: seed + {1000 * j} passed over at {a:.3f} / {b:.3f} of the bars")
        assert (max(a, b) <= SS.SELECT * 0.25) == (j == taken), (j, a, b)


def test_zero_gradient_tensors_are_exactly_zero():
    """T1's sleep-only step: an all-zero dream image and zero biases, so the encoder's kernel gradients vanish,
    legitimately.  worst_tensor's rule asks exactly 0 of such a tensor; the float32 reference gives it."""
    spec = SS.ws_case("T1")[4][0]
    xd = SS.ws_case("T1")[4][5][0]
    assert not xd.any()
    sleep = W.COEFS[1]
    g64, g32 = SS.ws_reference("T1", sleep)[1], SS.ws_reference("T1", sleep, np.float32)[1]
    zero = [not t.any() for t in PR.split_tensors(spec, g64)]
    ne = sum(1 for n, _, _ in spec.dense if n.startswith("enc"))
    assert any(zero[:2 * ne])                                         # in the encoder
    for z, t in zip(zero, PR.split_tensors(spec, g32)):
        assert not z or not t.any()
    # the rule: one wrong entry in such a tensor is an infinite error
    bad = np.array(g64)
    i0 = int(np.cumsum([0] + [t.size for t in PR.split_tensors(spec, g64)])[zero.index(True)])
    bad[i0] = 1e-30
    assert M.worst_tensor(spec, bad, g64) == np.inf and M.worst_tensor(spec, np.array(g64), g64) == 0.0


@pytest.mark.parametrize("name", list(SS.WS_CASES))
def test_both_phases_count_in_the_mix(name):
    """c_wake grad L_wake and c_sleep grad L_sleep each at least 1 % of the encoder gradient's norm."""
    spec, params, _, x, eps, dreams = SS.ws_case(name)[4]
    ne = PR.enc_size(spec)
    cw, cs = MIX
    _, _, gw = W.train_step(params, spec, x, eps, dreams, 1.0, 0.0, O.Adam())
    _, _, gs = W.train_step(params, spec, x, eps, dreams, 0.0, 1.0, O.Adam())
    gm = SS.ws_reference(name, MIX)[1]
    np.testing.assert_allclose(cw * gw[:ne] + cs * gs[:ne], gm[:ne], rtol=0, atol=1e-12 * np.abs(gm[:ne]).max())
    total = np.linalg.norm(gm[:ne])
    shares = cw * np.linalg.norm(gw[:ne]) / total, cs * np.linalg.norm(gs[:ne]) / total
    print(f"{name}: wake {shares[0]:.3f}, sleep {shares[1]:.3f} of the encoder gradient's norm")
    assert min(shares) >= 0.01, shares
    assert np.linalg.norm(gm[:ne]) > 1e-3 * np.linalg.norm(gm[ne:])


@pytest.mark.parametrize("name", list(SS.MASKED_CASES))
def test_masked_inputs_are_not_vacuous(name):
    _, B, k, _, (spec, params, _, x, eps, eps2, mask) = SS.masked_case(name)
    partial = [(row != 0).any() and (row == 0).any() for row in mask]
    # make_mask: image 0 all missing, image 1 all observed, the others drawn.  The cases of two images (T1, and
    # D8, W511, W512 at shape_cases' B = 2) therefore have no image with both kinds of pixel; every other case has
    assert any(partial) == (B > 2), name
    assert B > 2 or name in ("T1", "D8", "W511", "W512")
    for loss in SS.MASKED_LOSSES[name]:
        kw = M.loss_kwargs(loss, k, eps2)
        l_m, g_m, _ = SS.masked_reference(name, loss)
        l_1, _, g_1 = M.train_step(params, spec, np.where(mask != 0, x, 0.0), np.ones_like(mask), eps, loss, O.Adam(), **kw)
        d = PR.rel_l2(g_m, g_1)
        print(f"{name} {loss}: masked against unmasked gradient rel-L2 {d:.2e}, loss rel {abs(l_m - l_1) / abs(l_1):.2e}")
        assert d > SS.GPU_REL, d


# ------------------------------------------------- the parity comparisons bite
def _ws_wrong(name, coef, how):
    """A deliberately wrong float64 "reference" of a wake-sleep case."""
    spec, params, _, x, eps, (xd, hd) = SS.ws_case(name)[4]
    n = xd.shape[0]
    cw, cs = coef
    if how == "dream weight c_sleep / (n + 1)":
        cs = cs * n / (n + 1)
    elif how == "one dream row too many":               # the GM_FIT job reads a row behind the dream block
        xd = np.concatenate([xd, xd[:1]])
        hd = [np.concatenate([v, v[-1:]]) for v in hd]
        cs = cs * (n + 1) / n                            # at the weight the n rows carry
    elif how == "dream rows strided by r4(x_dim)":      # pixels of a [n, x_dim] block read at stride r4(x_dim)
        ld = (spec.x_dim + 3) // 4 * 4
        flat = np.concatenate([xd.ravel(), np.zeros(n * ld)])
        xd = np.stack([flat[j * ld:j * ld + spec.x_dim] for j in range(n)])
    elif how == "wake weights of k - 1 samples":        # per_image walks one sample row too few
        c = O.forward(params, spec, x, eps)
        a = W.wake_weights(c["lw"]).copy()
        a[-1] = 0.0
        gw = W.zeros_like_params(params, spec)
        W.wake_value_and_grads(params, spec, x, c["h"], a, gw)
        g = np.array(SS.ws_reference(name, (0.0, coef[1]) if coef[1] else (1.0, 0.0))[1])
        ne = PR.enc_size(spec)
        g[:ne] = (g[:ne] if coef[1] else 0.0) + cw * O.flatten_params(spec, gw)[:ne]
        return SS.ws_reference(name, coef)[0], g
    vals, _, g = W.train_step(params, spec, x, eps, (xd, hd), cw, cs, O.Adam())
    return tuple(float(v) for v in vals), g


WRONG_WS = [(n, c, h) for n in SS.WS_CASES for c in SS.WS_COEFS[n]
            for h in ("dream weight c_sleep / (n + 1)", "one dream row too many", "dream rows strided by r4(x_dim)",
                      "wake weights of k - 1 samples")]


@pytest.mark.parametrize("name,coef,how", WRONG_WS, ids=[f"{n}-{SS.COEF_ID[c]}-{h}" for n, c, h in WRONG_WS])
def test_a_wrong_wake_sleep_reference_misses_the_bars_by_far(name, coef, how):
    """What a wrong kernel would compute, against the float64 reference at the GPU bars: at least ten times
    over one of them.  (A fault the inputs cannot show is skipped over by construction only: a sleep fault
    under the wake-only step, the stride at x_dim % 4 == 0 or n = 1, k - 1 samples at k = 1.)"""
    spec = SS.ws_case(name)[4][0]
    n, k, x_dim = SS.WS_CASES[name][7], SS.WS_CASES[name][6], SS.WS_CASES[name][4]
    sleepy = how != "wake weights of k - 1 samples"
    if (sleepy and coef[1] == 0) or (not sleepy and (coef[0] == 0 or k == 1)):
        return
    if how == "dream rows strided by r4(x_dim)" and (x_dim % 4 == 0 or n == 1):
        return
    ref = SS.ws_reference(name, coef)
    fig = SS.compare(spec, _ws_wrong(name, coef, how), ref)
    print(f"{name} {coef} {how}: values {fig[0]:.2e}, whole {fig[1]:.2e}, worst tensor {fig[2]:.2e}")
    assert not SS.within(fig, 10.0), fig


def test_every_wake_sleep_fault_is_shown_somewhere():
    """The early returns above leave each fault shown on several cases, the odd-x_dim ones included."""
    for how, ok in (("stride", lambda e: e[4] % 4 and e[7] > 1), ("k - 1", lambda e: e[6] > 1)):
        names = [n for n, e in SS.WS_CASES.items() if ok(e)]
        assert {"O1", "O2", "O2w", "R5p40", "R40p5", "R20p20"} <= set(names), how
    assert all(e[4] % 4 for n, e in SS.WS_CASES.items() if n in SS.ROW_CASES)


def _shift(mask):
    return np.roll(mask, 1, axis=1)


@pytest.mark.parametrize("name,loss", MASKED, ids=MASKED_IDS)
def test_a_wrong_masked_reference_misses_the_bars_by_far(name, loss):
    """The mask shifted by one column (a staging kernel striding by r4(x_dim), an epilogue reading the wrong
    column): at least ten times over a bar.  The mask rows of a two-image case (T1, D8, W511, W512) are constant,
    so a column shift cannot show there: their fault is the mask shifted by one row."""
    _, B, k, _, (spec, params, _, x, eps, eps2, mask) = SS.masked_case(name)
    wrong = np.roll(mask, 1, axis=0) if B == 2 else _shift(mask)
    assert not np.array_equal(wrong, mask)
    xz = np.where(mask != 0, x, 0.0)
    l, _, g = M.train_step(params, spec, xz, wrong, eps, loss, O.Adam(), **M.loss_kwargs(loss, k, eps2))
    fig = SS.compare(spec, (float(l), g), SS.masked_reference(name, loss))
    print(f"{name} {loss}: shifted mask: loss {fig[0]:.2e}, whole {fig[1]:.2e}, worst tensor {fig[2]:.2e}")
    assert not SS.within(fig, 10.0), fig
