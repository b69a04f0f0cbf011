"""The host restatement of the device noise (tests/noise_ref.py) without a GPU:
its layouts against explicit loops, the distinctness of the counters the GPU
cases use, the end words of the uniform mapping, the moments of the reference
normals, the constants it restates against the library's sources, and two
conditions on the inputs of tests/test_gpu_noise.py: the oracle run in float32
on the reference noise stays within a quarter of every GPU bar, and no
resampling or pixel draw of the posterior / imputation cases is a near tie."""
import os
import re

import numpy as np
import pytest

import impute_ref as I
import noise_ref as N
import pathgrad_ref as R
from binarize_ref import LAYER as BIN_LAYER, MAX_LAYERS, philox_uniforms
from oracle import iwae_oracle as O

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "iwae_replication_project_amd", "csrc")
KEY = N.key(N.SEED)

# the GPU tests' bars (tests/test_gpu_shapes.py, tests/test_gpu_parity.py)
GPU_REL = 1e-4
GPU_TENSOR = 5e-4
GPU_ADAM_ATOL = 6e-5
GPU_LW = 1e-4
GPU_LOGPX = 1e-3
GPU_STEPS_W = 1e-5
PROBS_TOL = dict(rtol=2e-4, atol=2e-6)
LATENT_TOL = dict(rtol=1e-4, atol=2e-5)


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


# ------------------------------------------------------------ the sources
def test_constants_match_the_sources():
    k, m = _src("iwae_kernels.h"), _src("iwae_model.hip")
    assert "c1 = (layer << 20) | grp, c2 = (unsigned)base, c3 = (unsigned)(base >> 32)" in k
    assert "k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32)" in k
    assert "constexpr float k2m32 = 2.3283064365386963e-10f" in k and 2.3283064365386963e-10 == 2.0 ** -32
    assert "-1.38629436f * __builtin_amdgcn_logf(u0)" in k        # -2 ln 2 * log2 u
    assert abs(-2 * np.log(2) + 1.38629436) < 1e-8
    assert "r0 * __builtin_amdgcn_cosf(u1), r0 * __builtin_amdgcn_sinf(u1)" in k
    assert "r1 * __builtin_amdgcn_cosf(u3), r1 * __builtin_amdgcn_sinf(u3)" in k
    assert "const unsigned ca = half ? c2 : c0, cb = half ? c3 : c1" in k
    assert "h->noise_stream == 0 ? h->user_seed : splitmix64(h->user_seed ^ splitmix64(h->noise_stream))" in m
    for c in ("0x9E3779B97F4A7C15ULL", "0xBF58476D1CE4E5B9ULL", "0x94D049BB133111EBULL"):
        assert c in m
    assert N.splitmix64(0) == 0xE220A8397B1DCDAF                   # the published first output of state 0
    assert "g.layer = IWAE_MAX_LAYERS + j" in m and "IWAE_MAX_LAYERS + L - 1" in m
    assert "w.u_layer = 2 * IWAE_MAX_LAYERS + 1" in m
    assert re.search(r"#define IWAE_MAX_LAYERS 8\b", open(os.path.join(CSRC, "..", "..", "include", "iwae.h")).read())
    assert MAX_LAYERS == 8 and BIN_LAYER == N.BINARIZE_LAYER
    assert "return iwae_set_noise_stream(h, (unsigned long long)rank)" in m


def test_advance_table():
    """The table against the chunk rules it restates, at the GPU tests' arguments."""
    assert N.advance("train_step") == 1 and N.advance("train_steps", nsteps=3) == 3
    assert N.advance("nll", N=5, k=17, chunk=2) == 3
    assert N.advance("nll", N=5, k=17, chunk=2, nll_rows=16) == 9       # 17 = 8 + 8 + 1 per image chunk
    assert N.nll_chunks(5, 130, 2, nll_rows=256) == (2, 128)
    assert N.advance("nll", N=5, k=130, chunk=2, nll_rows=256) == 6
    assert N.advance("nll", N=5, k=17) == 1
    assert N.advance("posterior", N=5, k=17, chunk=2) == 3 and N.advance("posterior", N=5, k=17) == 1
    assert N.advance("encode", N=5, k=17, chunk=2) == 3 and N.advance("impute", N=5, k=17, chunk=4) == 2
    assert N.advance("encoder_means", N=5, n=8) == 1
    assert N.advance("encoder_means", N=3, n=1 << 20) == 3
    assert N.advance("generate", n=4) == 1 and N.advance("generate", n=0) == 0
    assert N.advance("binarize", n=7) == 1 and N.advance("binarize", n=0) == 0
    assert N.advance("reconstruct") == 1 and N.advance("score") == 0
    m = _src("iwae_model.hip")
    assert "int imgs = chunk > 0 ? chunk : (int)std::max<long long>(1, target_rows / k);" in m
    assert "const int kS = (int)std::min<long long>(k, std::max<long long>(1, target_rows / imgs));" in m
    assert "const long long max_rows = 1LL << 20;" in m


# ------------------------------------------------------------------ layouts
def test_uniforms_are_binarize_refs():
    np.testing.assert_array_equal(N.uniforms(KEY, 3, np.arange(7), 22, N.BINARIZE_LAYER), philox_uniforms(KEY, 3, 7, 22))


def test_layouts_round_trip_against_loops():
    B, k, dims = 3, 5, (70, 5)
    e1, e2 = N.eps_forward(KEY, 2, B, k, dims), N.eps_second_draw(KEY, 2, B, k, dims)
    for i, d in enumerate(dims):
        assert e1[i].shape == (k, B, d)
        for s in range(k):
            for b in range(B):
                np.testing.assert_array_equal(e1[i][s, b], N.normals(KEY, 2, [b * k + s], d, i)[0])
                np.testing.assert_array_equal(e2[i][s, b], N.normals(KEY, 2, [(B + b) * k + s], d, i)[0])
    # a single column against a single Philox block
    z = N.box_muller(N.words(KEY, 2, [7], [17], 0))[0, 0]
    np.testing.assert_array_equal(N.normals(KEY, 2, [7], 70, 0)[0, 68:70], z[:2])
    # chunks: images in chunks of 2, samples in chunks of 2; chunk c draws at base0 + c, rows local
    NN, imgs, ks = 5, 2, 2
    eps, chunks = N.eps_chunked(KEY, 4, NN, k, dims, imgs, ks)
    assert chunks == 3 * 3
    c = 0
    for i0 in range(0, NN, imgs):
        n = min(imgs, NN - i0)
        for s0 in range(0, k, ks):
            kl = min(ks, k - s0)
            for i, d in enumerate(dims):
                for s in range(kl):
                    for b in range(n):
                        np.testing.assert_array_equal(eps[i][s0 + s, i0 + b], N.normals(KEY, 4 + c, [b * kl + s], d, i)[0])
            c += 1
    # prior and top latents, SIR and imputation uniforms
    L = len(dims)
    pri = N.eps_prior(KEY, 1, 4, dims)
    assert len(pri) == L - 1 and pri[0].shape == (1, 4, dims[0])
    np.testing.assert_array_equal(pri[0][0, 3], N.normals(KEY, 1, [3], dims[0], MAX_LAYERS)[0])
    np.testing.assert_array_equal(N.eps_top(KEY, 1, 4, dims)[0, 2], N.normals(KEY, 1, [2], dims[1], MAX_LAYERS + L - 1)[0])
    u = N.sir_uniforms(KEY, 6, 5, 2)
    up = N.impute_uniforms(KEY, 6, 5, 22, 2)
    for b in range(5):
        assert u[b] == N.uniforms(KEY, 6 + b // 2, [b % 2], 4, 2 * MAX_LAYERS + 1)[0, 0]
        np.testing.assert_array_equal(up[b], N.uniforms(KEY, 6 + b // 2, [b % 2], 22, 2 * MAX_LAYERS + 2)[0])


def test_counters_are_distinct_over_the_largest_gpu_case():
    """RING_POINT's train step as CIWAE would draw it (twice the rows), every
    layer id in use with its own quad count, four consecutive bases: no two
    draws share a counter."""
    (he, hd, le, ld), x_dim = N.arch("RING")
    _, B, k, _ = N.RING_POINT
    L = len(le)
    use = [(i, 2 * B * k, (d + 3) // 4) for i, d in enumerate(le)]
    use += [(N.prior_layer(j), B * k, (le[L - 2 - j] + 3) // 4) for j in range(L - 1)]
    use += [(N.top_layer(L), B * k, (le[-1] + 3) // 4)]
    use += [(lay, B, (x_dim + 3) // 4) for lay in (N.PIXEL_LAYER, N.IMPUTE_LAYER, N.BINARIZE_LAYER)] + [(N.SIR_LAYER, B, 1)]
    packed = []
    for base in range(4):
        for layer, rows, quads in use:
            r, q = np.meshgrid(np.arange(rows, dtype=np.uint64), np.arange(quads, dtype=np.uint64), indexing="ij")
            c1 = np.uint64(layer << 20) | q
            assert int(c1.max()) < 1 << 32
            packed.append(((np.uint64(base) << np.uint64(56)) | (r << np.uint64(32)) | c1).ravel())
    packed = np.concatenate(packed)
    ids = [u[0] for u in use]
    assert len(set(ids)) == len(ids), ids
    assert np.unique(packed).size == packed.size


# ---------------------------------------------------------------- end words
def test_end_words_give_finite_normals():
    w = np.array([[0], [0], [0xFFFFFF80], [0xFFFFFFFF]], np.uint32)
    u = [N.uniform_from_u32(c) for c in w]
    assert u[0][0] == np.float32(2.0 ** -33) and u[2][0] == np.float32(1.0) and u[3][0] == np.float32(1.0)
    assert N.uniform_from_u32(np.uint32(0xFFFFFF7F)) < np.float32(1.0)
    z = N.box_muller(w)[0]
    assert np.isfinite(z).all()
    assert abs(z[0] - np.sqrt(66 * np.log(2))) < 1e-6 and abs(z[1]) < 1e-7      # angle 2 pi 2^-33
    assert z[2] == 0.0 and z[3] == 0.0                                       # ln 1 = 0: exactly 0, not NaN
    z32 = N.box_muller(w, np.float32)[0]
    assert np.isfinite(z32).all() and z32[2] == 0.0 and z32[3] == 0.0


# ------------------------------------------------------------------ moments
ROWS, D = 4096, 64                    # 262144 normals per (layer, base)


@pytest.fixture(scope="module")
def draws():
    rows = np.arange(ROWS)
    return {(lay, base): N.normals(KEY, base, rows, D, lay) for lay, base in ((0, 0), (1, 0), (0, 1))}


def test_moments_of_the_reference_normals(draws):
    z = draws[0, 0].ravel()
    n = z.size
    stats = {"mean": (z.mean(), 0.0, 1 / np.sqrt(n)), "variance": ((z * z).mean(), 1.0, np.sqrt(2 / n)),
             "fourth moment": ((z ** 4).mean(), 3.0, np.sqrt(96 / n))}          # var z^4 = 105 - 9
    for name, (v, want, se) in stats.items():
        print(f"{name}: {v:.5f} ({(v - want) / se:+.2f} standard errors, n = {n})")
        assert abs(v - want) <= 5 * se, (name, v)


def test_reference_normals_are_uncorrelated(draws):
    z = draws[0, 0]
    blocks = z.reshape(ROWS, D // 4, 4)
    pairs = {f"block values {a},{b}": (blocks[..., a].ravel(), blocks[..., b].ravel())
             for a in range(4) for b in range(a + 1, 4)}
    pairs["adjacent rows"] = (z[:-1].ravel(), z[1:].ravel())
    pairs["adjacent quads"] = (blocks[:, :-1].ravel(), blocks[:, 1:].ravel())
    pairs["layer ids 0, 1"] = (z.ravel(), draws[1, 0].ravel())
    pairs["bases 0, 1"] = (z.ravel(), draws[0, 1].ravel())
    for name, (a, b) in pairs.items():
        c, se = (a * b).mean(), 1 / np.sqrt(a.size)
        print(f"{name}: {c:+.5f} ({c / se:+.2f} standard errors, n = {a.size})")
        assert abs(c) <= 5 * se, (name, c)
        assert not np.array_equal(a, b)


def test_streams_differ():
    a = N.normals(N.key(N.SEED, 0), 0, np.arange(256), 64, 0).ravel()
    b = N.normals(N.key(N.SEED, 1), 0, np.arange(256), 64, 0).ravel()
    c = N.normals(N.key(N.SEED, 3), 0, np.arange(256), 64, 0).ravel()
    for p, q in ((a, b), (a, c), (b, c)):
        assert abs((p * q).mean()) <= 5 / np.sqrt(p.size)


def test_float32_box_muller_distance():
    """The scale to read the GPU's normal error against: numpy's float32 Box-Muller
    on the same uniforms (printed; the bound only says float32 can do it)."""
    worst = 0.0
    for model in N.STAT_MODELS:
        dims = N.arch(model)[0][2]
        for B, k in N.SHAPES:
            for base in (0, 1):
                for a, b in zip(N.eps_forward(KEY, base, B, k, dims), N.eps_forward(KEY, base, B, k, dims, dtype=np.float32)):
                    worst = max(worst, np.abs(a - b).max())
    print(f"numpy float32 Box-Muller against float64 over the direct-observation draws: max abs {worst:.2e}")
    assert worst < 1e-5


# ------------------------------------- float32 oracle against the GPU bars
TRAIN_ALL = N.TRAIN + [N.RING_POINT]


@pytest.mark.parametrize("model,B,k,vid", TRAIN_ALL, ids=["-".join(map(str, c)) for c in TRAIN_ALL])
def test_float32_train_step_within_a_quarter_of_the_gpu_bars(model, B, k, vid):
    spec = N.case(model, B)[1]
    l64, g64, w64 = N.train_reference(model, B, k, vid)
    l32, g32, w32 = N.train_reference(model, B, k, vid, np.float32)
    whole = R.rel_l2(g32, g64)
    per = max(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)
              for a, b in zip(R.split_tensors(spec, g32), R.split_tensors(spec, g64)))
    adam = np.abs(w32 - w64).max()
    print(f"float32 loss rel {abs(l32 - l64) / abs(l64):.2e}, gradient rel-L2 {whole:.2e}, per tensor {per:.2e}, "
          f"post-Adam weights {adam:.2e}")
    assert abs(l32 - l64) <= GPU_REL / 4 * abs(l64)
    assert whole <= GPU_REL / 4, whole
    assert per <= GPU_TENSOR / 4, per
    assert adam <= max(GPU_ADAM_ATOL, 10 * np.abs(g32 - g64).max()) / 4, adam


def test_float32_steps_within_a_quarter_of_the_gpu_bars():
    l64, w64 = N.steps_reference()
    l32, w32 = N.steps_reference(np.float32)
    print(f"float32 three steps: loss rel {np.abs(l32 / l64 - 1).max():.2e}, final weights {np.abs(w32 - w64).max():.2e}")
    assert np.abs(l32 - l64).max() <= GPU_REL / 4 * np.abs(l64).min()
    assert np.abs(w32 - w64).max() <= GPU_STEPS_W / 4
    assert len(set(np.round(l64, 6))) == 3


@pytest.mark.parametrize("model,B,k", N.FORWARD, ids=["-".join(map(str, c)) for c in N.FORWARD])
def test_float32_forward_within_a_quarter_of_the_gpu_bars(model, B, k):
    c64, c32 = N.forward_reference(model, B, k, 1), N.forward_reference(model, B, k, 1, np.float32)
    e = np.abs(c32["lw"] - c64["lw"]).max() / np.abs(c64["lw"]).max()
    lk64, lk32 = O.L_k_from_weights(c64["lw"]), O.L_k_from_weights(c32["lw"].astype(np.float64))
    print(f"float32 log-weights {e:.2e} of max|lw|, L_k rel {abs(lk32 - lk64) / abs(lk64):.2e}")
    assert e <= GPU_LW / 4
    assert abs(lk32 - lk64) <= GPU_REL / 4 * abs(lk64)
    # the second position draws other noise: a call that replays position 0 misses the bar by far
    c0 = N.forward_reference(model, B, k, 0)
    assert np.abs(c0["lw"] - c64["lw"]).max() > 100 * GPU_LW * np.abs(c64["lw"]).max()


def _swap_halves(e):
    """Columns (4g, 4g + 1) <-> (4g + 2, 4g + 3) where both pairs exist: philox_normal2 with the half inverted."""
    out = e.copy()
    for j in range(0, e.shape[-1] - 3, 4):
        out[..., j:j + 2], out[..., j + 2:j + 4] = e[..., j + 2:j + 4], e[..., j:j + 2]
    return out


@pytest.mark.parametrize("model", ["S2", "W2"])
def test_each_addressing_mistake_moves_the_reference_far_past_the_gpu_bars(model):
    """What the GPU tests can see: the oracle on noise addressed in each of the
    wrong ways a drawing kernel could address it differs from the reference by
    at least 100 times the log-weight bar (CIWAE's loss: the loss bar)."""
    B, k = N.SHAPES[0]
    _, spec, params, _, x = N.case(model, B)
    dims = spec.n_latent_encoder
    good = N.eps_forward(KEY, 0, B, k, dims)
    lw = O.forward(params, spec, x, good)["lw"]
    rows = N.sample_rows(B, k)
    wrong = {
        "two layers under one layer id": [good[0], N.normals(KEY, 0, rows, dims[1], 0).reshape(k, B, -1)],
        "rows of two 16-row workgroups share counters":
            [N.normals(KEY, 0, rows % 16, d, i).reshape(k, B, d) for i, d in enumerate(dims)],
        "the sample index alone as the row": [N.normals(KEY, 0, rows % k, d, i).reshape(k, B, d) for i, d in enumerate(dims)],
        "the halves of a block swapped": [_swap_halves(e) for e in good],
        "the previous position's noise": N.eps_forward(KEY, 1, B, k, dims),
        "the key's high word ignored": N.eps_forward(KEY & N.MASK32, 0, B, k, dims),
        "stream key without the inner splitmix64": N.eps_forward(N.splitmix64(N.SEED ^ 1), 0, B, k, dims),
    }
    ref1 = O.forward(params, spec, x, N.eps_forward(N.key(N.SEED, 1), 0, B, k, dims))["lw"]
    for name, eps in wrong.items():
        other = O.forward(params, spec, x, eps)["lw"]
        base = ref1 if name.startswith("stream key") else lw
        e = np.abs(other - base).max() / np.abs(base).max()
        print(f"{model} {name}: log-weights move by {e:.2e} of max|lw|")
        assert e >= 100 * GPU_LW, (name, e)
    l_good, g_good, _ = N.train_reference(model, B, k, "CIWAE")
    l_same, _, g_same = O.train_step(params, spec, x, good, "CIWAE", k, O.Adam(1e-3, 0.9, 0.999, 1e-4), beta=0.3, eps2=good)
    print(f"{model} CIWAE's second draw equal to its first: loss moves by {abs(l_same - l_good) / abs(l_good):.2e}, "
          f"gradient by {R.rel_l2(g_same, g_good):.2e}")
    assert abs(l_same - l_good) >= 3 * GPU_REL * abs(l_good) and R.rel_l2(g_same, g_good) >= 100 * GPU_REL


NLL_ALL = [c + (False,) for c in N.NLL] + [N.NLL_MASKED[:3] + (0, N.NLL_MASKED[3], True)]


@pytest.mark.parametrize("model,NN,k,chunk,rows,masked", NLL_ALL, ids=["-".join(map(str, c)) for c in NLL_ALL])
def test_float32_log_px_within_a_quarter_of_the_gpu_bar(model, NN, k, chunk, rows, masked):
    masks = N.latent_masks(model) if masked else None
    lp64, chunks = N.nll_reference(model, NN, k, chunk, rows, masks=masks)
    lp32, _ = N.nll_reference(model, NN, k, chunk, rows, dtype=np.float32, masks=masks)
    print(f"float32 log p(x): {np.abs(lp32 - lp64).max():.2e} nats over {chunks} chunks")
    assert np.abs(lp32 - lp64).max() <= GPU_LOGPX / 4
    assert chunks == N.advance("nll", N=NN, k=k, chunk=chunk, **({} if rows is None else dict(nll_rows=rows)))
    # a chunk that replayed the previous chunk's base, or rows counted over the whole call, misses the bar
    if chunks > 1 and not masked:
        spec, params, x = N.case(model, NN)[1], N.case(model, NN)[2], N.case(model, NN)[4]
        eps = N.eps_forward(KEY, 0, NN, k, spec.n_latent_encoder)
        wrong = O.log_px_per_image(params, spec, x, k, eps=eps)
        assert np.abs(wrong - lp64).max() > 20 * GPU_LOGPX


@pytest.mark.parametrize("model", N.STAT_MODELS)
def test_float32_statistics_within_a_quarter_of_the_gpu_bars(model):
    B = N.SHAPES[0][0]
    p64, l64 = N.reconstruct_reference(model, B)
    p32, l32 = N.reconstruct_reference(model, B, dtype=np.float32)
    assert (np.abs(p32 - p64) <= (PROBS_TOL["atol"] + PROBS_TOL["rtol"] * np.abs(p64)) / 4).all()
    assert abs(l32 - l64) <= GPU_REL / 4 * abs(l64)
    for a, b in zip(N.encoder_means_reference(model, N.NLL_N, N.MEANS_N, dtype=np.float32),
                    N.encoder_means_reference(model, N.NLL_N, N.MEANS_N)):
        assert (np.abs(a - b) <= (LATENT_TOL["atol"] + LATENT_TOL["rtol"] * np.abs(b)) / 4).all()
    g64, g32 = N.generate_reference(model, 19), N.generate_reference(model, 19, dtype=np.float32)
    assert (np.abs(g32[0] - g64[0]) <= (PROBS_TOL["atol"] + PROBS_TOL["rtol"] * np.abs(g64[0])) / 4).all()
    for a, b in zip(g32[1], g64[1]):
        assert (np.abs(a - b) <= (LATENT_TOL["atol"] + LATENT_TOL["rtol"] * np.abs(b)) / 4).all()


# ---------------------------- posterior / imputation: conditions on the inputs
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("model", N.POSTERIOR_MODELS)
def test_posterior_cases_are_not_vacuous_and_have_no_near_ties(model, masked):
    """The weights spread over several samples; the resampling uniform is 5e-4
    away from every step of the reference's cumulative weights (the GPU test
    takes the index from the DEVICE's weights, whose float32 running sum is
    within (k + 8) 2^-23 = 3e-6 of their float64 sum; 5e-4 leaves the weights
    themselves a relative error of 5e-4, fifty times the measured one); the
    imputation's pixel uniforms are PROBS_TOL away from the selected sample's
    probabilities at all but 1 % of the missing pixels (test_gpu_impute's cap)."""
    NN, k = N.NLL_N, N.POSTERIOR_K
    mask = N.pixel_mask(NN, N.X_DIM) if masked else None
    for imgs in (NN, 2):
        ref = N.posterior_reference(model, NN, k, imgs, mask=mask)
        w = ref["weights"]
        # (plain Glorot weights: some weights are tiny, but every one is a normal float32, so its log is meaningful)
        assert w.min() >= 1e-34 and (ref["ess"] > 1).all() and (ref["ess"] < k).all(), (w.min(), ref["ess"])
        gap = np.abs(np.cumsum(w, axis=1) - ref["u"][:, None].astype(np.float64)).min()
        print(f"{model} chunks of {imgs}: ESS/k {ref['ess'].min() / k:.3f}..{ref['ess'].max() / k:.3f}, min w {w.min():.1e}, "
              f"resampling gap {gap:.2e}, indices {ref['sir_index']}")
        assert gap >= 5e-4
        if masked:
            miss = mask == 0
            p_sel = I.p_sir(ref["sir_index"], ref["cache"])
            u_pix = N.impute_uniforms(KEY, 0, NN, N.X_DIM, imgs).astype(np.float64)
            near = miss & (np.abs(u_pix - p_sel) <= PROBS_TOL["atol"] + PROBS_TOL["rtol"] * p_sel)
            assert near.sum() <= max(1, int(0.01 * miss.sum()))
