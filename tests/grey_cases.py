"""Grey-level pixel cases shared by tests/test_grey_cases.py (CPU) and
tests/test_gpu_grey.py: every kernel that evaluates log p(x|h) chooses at run
time between the binarised form (select sigmoid(+-l), multiply four, one log)
and the two-log form x log p + (1 - x) log(1 - p), over a deciding group of
pixels that differs per kernel.  These cases put grey pixels, and the boundary
between grey and binarised images, where those groups lie.

Models, weights and noise come from pathgrad_ref.make_case (rounded through
float32); x is then replaced by a pattern:

  grey    every pixel uniform in (0, 1) as float32; per image four entries are
          exactly 0, 1, 2^-24 and 1 - 2^-24
  mixed   small cases: image i % 5 == 0 or 4 binarised, 1 grey, 2 binarised but
          for one grey pixel in column 0, 3 binarised but for one grey pixel in
          column x_dim - 1.  Ring cases: image 0 binarised, 1 grey, 2 binarised
          but for one grey pixel in column 783 (workgroup 0 of 128 rows is all
          image 0: the binarised form; every other workgroup the two-log form)
  deep    grey, with three columns of the output Dense's kernel zeroed and their
          biases set to -100, -88 and -87.5, so those logits are exact in every
          row: exp(-l) overflows float32 below -88.72, and 1 / (1 + exp(-l)) is
          a float32 denormal in (-88.72, -87.3].  Their pixels: 0.25; an exact 0
          sharing its quad with grey pixels; an exact 1 sharing its 16-column
          tile with grey pixels.  Negative extremes only: at large positive
          logits the reference's own float32 log1p(-p) loses digits (F:126-F:128)

Nothing had to be changed to keep the float32 oracle within a quarter of the
GPU bars (tests/test_grey_cases.py): seeds are the first tried, the deep
magnitudes the ones named above.

expected_kernels() restates, from a case's numbers alone, which launch counters
(iwae_debug_count) a call must move; tests/test_grey_cases.py checks its
constants against the sources."""
import functools

import numpy as np

import pathgrad_ref as R
from shape_cases import NO_ENGINE_LOSSES, _mirror, split_k

RING_MIN_K = 43            # nring_kernel's pixel cache: kS >= 43 (iwae_model.hip / iwae_nring.hip)
RING_WG_ROWS = 128         # NR_ROWS = 16 * NR_W
RING_NLL_MIN_K = 128       # the NLL's first pass runs nring_kernel from k = 128
WIDE_ROWS = 4097           # tuning default wide_rows
NRING_TRAIN_ROWS = 4096    # tuning default nring_train_rows
TC_BOUND_MAX_K, TC_BOUND_MAX_IMAGES = 256, 64    # use_tc_bound: the bound inside the engine's backward launch

DEEP_BIASES = (-100.0, -88.0, -87.5)
ARCH1 = ([200], [200], [50], [784])
ARCH2 = ([200, 100], [100, 200], [100, 50], [100, 784])


def _small(he, le, x_dim, B, k, seed):
    hd, ld = _mirror(he, le, x_dim)
    return (list(he), hd, list(le), ld, x_dim, B, k, seed)


# name: (he, hd, le, ld, x_dim, B, k, seed)
CASES = {
    "G1": _small([24], [6], 20, 5, 7, 1701),
    "G2": _small([31, 17], [7, 3], 37, 5, 7, 1702),
    "G3": _small([37, 23, 13], [11, 6, 2], 64, 4, 9, 1703),
    "GW": _small([31, 17], [7, 3], 37, 9, 8, 1704),
    "R1": (*ARCH1, 784, 3, 192, 1705),
    "R2": (*ARCH2, 784, 3, 192, 1706),
}
SMALL = ("G1", "G2", "G3", "GW")
RING = ("R1", "R2")
DEEP_CASES = ("G1", "G2", "R2")
ALL_LOSS_CASES = ("G1", "G2")
PATTERNS = {n: ("grey", "mixed") + (("deep",) if n in DEEP_CASES else ()) for n in CASES}

# tuning knobs a case runs with; GW: 72 rows on the engine's 32- and 64-row workgroups
# (below wide_rows tc_rt row tiles; from wide_rows the forward launch runs 4, the backward wide_rt)
GW_KNOBS = {"rt2": dict(tc_rt=2), "wide2": dict(wide_rows=64, wide_rt=2), "wide4": dict(wide_rows=64, wide_rt=4)}
# ring cases: 576 rows run the ring train forward with nring_train_rows lowered to 512
RING_KNOBS = {
    "ring-b3": dict(nring_train_rows=512, nring_train=1, nring_bwd=3, tc_bound=0),
    "ring-b3-tcb": dict(nring_train_rows=512, nring_train=1, nring_bwd=3),
    "ring-b0": dict(nring_train_rows=512, nring_train=1, nring_bwd=0, tc_bound=0),
    "engine": dict(nring_train_rows=512, nring_train=0, nring_bwd=3),
}


def deep_columns(x_dim):
    """The three constructed columns: any; one whose quad holds grey pixels; the
    last one (its 16-column tile holds grey pixels; alone in a ragged quad when
    x_dim % 4 == 1)."""
    return (5, 10, x_dim - 1)


def special_columns(x_dim, image):
    """Columns of an image's exact 0, 1, 2^-24 and 1 - 2^-24 in the grey pattern."""
    c0 = 0 if image % 2 else x_dim - 7
    return tuple(range(c0, c0 + 4))


SPECIALS = (0.0, 1.0, 2.0 ** -24, 1.0 - 2.0 ** -24)
DEEP_PIXELS = (0.25, 0.0, 1.0)


def loss_variants(name, pattern):
    """(id, loss, model keywords) of every train-step loss a (case, pattern) runs."""
    if pattern.startswith("deep"):
        return [("IWAE", "IWAE", {}), ("L_alpha", "L_alpha", dict(alpha=0.3))]
    out = [("IWAE", "IWAE", {})]
    if name in ALL_LOSS_CASES:
        k1, k2 = split_k(CASES[name][6])
        out += [("VAE", "VAE", {}), ("CIWAE", "CIWAE", dict(beta=0.3)), ("L_alpha", "L_alpha", dict(alpha=0.3)),
                ("L_power_neg", "L_power_p", dict(p=-1.5)), ("VAE_V1", "VAE_V1", {}),
                ("MIWAE", "MIWAE", dict(k1=k1, k2=k2)), ("PIWAE", "PIWAE", dict(k1=k1, k2=k2))]
    if name == "G2":
        out += [("IWAE_DREG", "IWAE_DREG", {})]
    return out


def variant(name, pattern, vid):
    return next(v for v in loss_variants(name, pattern) if v[0] == vid)


def _grey_image(rng, x_dim, image):
    row = rng.uniform(0.0, 1.0, x_dim).astype(np.float32)
    row = np.clip(row, np.float32(2.0 ** -20), np.float32(1.0 - 2.0 ** -20))    # strictly inside (0, 1)
    for c, v in zip(special_columns(x_dim, image), SPECIALS):
        row[c] = np.float32(v)
    return row.astype(np.float64)


@functools.lru_cache(maxsize=None)
def make(name, pattern):
    """(spec, params, mean, x, eps) in float64; parameters, pixels and noise are
    float32 values.  Shared: do not modify."""
    he, hd, le, ld, x_dim, B, k, seed = CASES[name]
    spec, params, mean, xbin, eps = R.make_case((he, hd, le, ld), B, k, seed, x_dim=x_dim)
    rng = np.random.default_rng(seed + 100)
    grey = np.stack([_grey_image(rng, x_dim, i) for i in range(B)])
    if pattern == "grey":
        x = grey
    elif pattern == "binary":                     # the all-binarised batch the mixed-batch property compares with
        x = xbin.copy()
    elif pattern == "mixed":
        x = xbin.copy()
        for i in range(B):
            kind = i if name in RING else i % 5
            if kind == 1:
                x[i] = grey[i]
            elif kind == 2:
                x[i, x_dim - 1 if name in RING else 0] = np.float64(np.float32(0.3))
            elif kind == 3:
                x[i, x_dim - 1] = np.float64(np.float32(0.7))
    elif pattern.startswith("deep"):
        # "deep": all three columns; "deep0" / "deep1" / "deep2": one of them alone
        # (what one constructed pixel gives, apart from the other two)
        if name not in DEEP_CASES:
            raise KeyError((name, pattern))
        which = range(3) if pattern == "deep" else [int(pattern[4:])]
        x = grey.copy()
        W, b = params["out.l3"]
        W, b = W.copy(), b.copy()
        for j in which:
            c = deep_columns(x_dim)[j]
            W[:, c] = 0.0
            b[c] = DEEP_BIASES[j]
            x[:, c] = DEEP_PIXELS[j]
        params = dict(params)
        params["out.l3"] = [W, b]
    else:
        raise KeyError(pattern)
    x.setflags(write=False)
    return spec, params, mean, x, eps


def binarised_images(name):
    """The wholly binarised images of a mixed batch."""
    B = CASES[name][5]
    return [i for i in range(B) if (i if name in RING else i % 5) in (0, 4)]


def impute_mask(name):
    """[B, x_dim] float32, 0 = missing: 30 % of the pixels, drawn once per case."""
    x_dim, B, seed = CASES[name][4], CASES[name][5], CASES[name][7]
    return (np.random.default_rng(seed + 200).random((B, x_dim)) >= 0.3).astype(np.float32)


def grey_pixels(name, pattern):
    """Boolean [B, x_dim]: the pixels that are neither 0 nor 1."""
    x = make(name, pattern)[3]
    return (x != 0.0) & (x != 1.0)


@functools.lru_cache(maxsize=None)
def second_draw(name):
    """CIWAE's second, independent noise draw of a case (float32-rounded)."""
    from oracle import iwae_oracle as O
    seed = CASES[name][7]
    k, B = CASES[name][6], CASES[name][5]
    rng = np.random.default_rng(seed + 5000)
    return [e.astype(np.float32).astype(np.float64) for e in O.draw_eps(make(name, "grey")[0], k, B, rng)]


def reference_step(name, pattern, vid, dtype=None):
    """(loss, flat gradient, flat post-Adam weights) of a train step (Adam lr 1e-3,
    eps 1e-4) by the oracle in `dtype` arithmetic (default float64)."""
    from oracle import iwae_oracle as O
    dtype = dtype or np.float64
    _, loss, kw = variant(name, pattern, vid)
    spec, params, _, x, eps = make(name, pattern)
    k = CASES[name][6]
    p = O.cast_params(params, dtype)
    x, eps = x.astype(dtype), [e.astype(dtype) for e in eps]
    opt = O.Adam(1e-3, 0.9, 0.999, 1e-4)
    if loss in R.LOSSES:
        out = R.train_step(p, spec, x, eps, loss, opt)
    else:
        kw = dict(kw)
        if loss == "CIWAE":
            kw["eps2"] = [e.astype(dtype) for e in second_draw(name)]
        out = O.train_step(p, spec, x, eps, loss, k, opt, **kw)
    return float(out[0]), np.asarray(out[2], np.float64), np.asarray(O.flatten_params(spec, out[1]), np.float64)


def forward_reference(name, pattern, dtype=np.float64):
    """(log-weights [k, B], L_k, E_q log p(x|h), log p(x) per image, L_alpha at
    alpha = 0.3) by the oracle in `dtype` arithmetic."""
    from oracle import iwae_oracle as O
    spec, params, _, x, eps = make(name, pattern)
    k = CASES[name][6]
    p = O.cast_params(params, dtype)
    x, eps = x.astype(dtype), [e.astype(dtype) for e in eps]
    c = O.forward(p, spec, x, eps, need_bce=True)
    lw = c["lw"]
    eq = float(np.mean(c["bce_row"]))
    la = 0.7 * eq + 0.3 * float(O.L_from_weights(lw))
    return lw, float(O.L_k_from_weights(lw)), eq, O.log_px_per_image(p, spec, x, k, eps=eps), la


def expected_kernels(name, loss="IWAE", path="auto", knobs=None, p=1.0):
    """Which launch counters a train step (ids 2 train engine, 13 row-block
    forward, 4 / 5 / 6 ring train forward, nrb, nre) and an injected-noise log_px
    (ids 0 fused NLL, 3 ring NLL) must move: True, False, or None where the
    table does not say."""
    he, hd, le, ld, x_dim, B, k, seed = CASES[name]
    knobs = knobs or {}
    L = len(he)
    rows = (2 * B if loss == "CIWAE" else B) * k
    on_engine = (path == "auto" and loss not in NO_ENGINE_LOSSES and not (loss == "L_power_p" and p < 0) and L <= 3)
    row_block = path != "layerwise" and not on_engine
    ring_shape = name in RING
    ring_fwd = (on_engine and ring_shape and knobs.get("nring_train", 1) != 0 and k >= RING_MIN_K
                and rows >= knobs.get("nring_train_rows", NRING_TRAIN_ROWS) and loss != "L_alpha")
    tc_bound = (knobs.get("tc_bound", 1) != 0 and k <= TC_BOUND_MAX_K and B <= TC_BOUND_MAX_IMAGES
                and loss not in ("L_alpha", "VAE_V1"))
    # (with the bound inside the engine's backward launch that launch runs job O' and
    # E' itself; whether it does also depends on the plan's LDS: not restated here)
    nrb = None if ring_fwd and tc_bound else ring_fwd and knobs.get("nring_bwd", 3) != 0
    nre = None if nrb is None else nrb and knobs.get("nring_bwd", 3) == 3 and L == 2
    # the engine launches nothing only when the ring kernels take every sample-row job
    engine = None if ring_fwd else on_engine
    wide = on_engine and rows >= knobs.get("wide_rows", WIDE_ROWS)
    fwd_rows = 16 * (4 if wide else knobs.get("tc_rt", 1))     # rows tc_bern's `bin` is decided over
    nll_fused = path != "layerwise"
    nll_ring = nll_fused and ring_shape and knobs.get("nring", 1) != 0 and k >= RING_NLL_MIN_K
    return {2: engine, 13: row_block, 4: ring_fwd, 5: nrb, 6: nre, 0: nll_fused, 3: nll_ring, "fwd_rows": fwd_rows}
