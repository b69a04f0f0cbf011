"""Named (images, samples) points at the edges of the bound code's decisions on
the sample axis (csrc/iwae_bound.h, bound_kernel in csrc/iwae_elem.hip, the
in-launch bound of the engine's backward launch), shared by
tests/test_sample_cases.py (CPU) and tests/test_gpu_samples.py:

  K17     an image of 17 rows straddles the 16-row workgroups of the in-launch bound
  K63 / K64 / K65   the lane stride: q = lane; q < k; q += 64 runs once / once, full / twice
  K128    even k for the median; MIWAE / PIWAE with k1 = 64, k2 = 2
  K130    k1 = 65 > 64, k2 = 2: the inner loops over k1 run twice
  K256 / K257   either side of use_tc_bound's sample limit
  K1024 / K1025 either side of the LDS-staged limit (above it LwView re-reads the global row)
  B64 / B65     either side of the in-launch bound's image limit; one workgroup either way
  M65     65 images, 8255 rows: bound_kernel on several workgroups (ticket, contrib[] re-sum)
  C33     CIWAE only: 66 images, 8250 rows, several workgroups with Bsplit inside one's stride
  M1025   IWAE only, default path only: several workgroups, each image unstaged

on two small models, S1 (one stochastic layer) and S2 (two), decoders mirrored
as in shape_cases._mirror, x_dim = 20; and two constructed inputs on S2:

  WIDE    B = 3, k = 96, the output layer's last kernel times 8: log-weights
          spread over 60 to 100 nats per image, so exp(lw - max) underflows to
          0 in float32 for part of an image's samples
  TIE64 / TIE65   L_median with the two middle order statistics (k even), or
          the median and the next one (k odd), bit-identical rows: in every
          image the noise of the largest-lw sample is overwritten, in every
          layer, with that of the sample at rank (k - 1) // 2

Each case's seed was picked by a search on the CPU so that, in every image, the
order statistics beside the median's are 2e-4 max|lw| away from it or further
(median_gaps; tests/test_sample_cases.py checks it); M65's 65 images get
there by drawing the noise of single images again (REDRAWN).  Where k > 64 the
samples of each image are then reordered so that the last index, which only the
last pass of a lane-strided loop reaches, carries the image's largest
log-weight or its median (_place_last).

expected_bound() restates from a case's numbers alone where its bound is
computed: inside the engine's backward launch (use_tc_bound's numeric limits in
csrc/iwae_model.hip) or by bound_kernel on one or several workgroups
(launch_bound's grid rule in csrc/iwae_elem.hip).  use_tc_bound's last
condition, on the LDS the engine's plan leaves, depends on the model's widths
and is not restated: LDS_FALLBACK lists the cases it takes the in-launch bound
from, as measured."""
import functools

import numpy as np

import pathgrad_ref as R
import shape_cases as S
from oracle import iwae_oracle as O

# limits, by their place in the sources (tests/test_sample_cases.py checks them)
TC_BOUND_K = 256          # use_tc_bound: P.kS > 256
TC_BOUND_IMAGES = 64      # use_tc_bound: P.Bimg > 64
BOUND_WAVES = 16          # kBoundWaves: launch_bound's one workgroup serves up to 4 * 16 images ...
BOUND_ROWS = 8192         # ... or up to 8192 rows
STAGED_K = 1024           # bound_images: staged = kS <= 1024; make_plan's limit of L_median / MIWAE / PIWAE
ENGINE_ROWS = 1 << 18     # use_engine
MEDIAN_BAR = 2 * 1e-4     # of max|lw|: twice the GPU tests' log-weight bar (two rows may each move by it)
WIDE_SPREAD = (60.0, 90.0)  # nats: every image's max - min of lw at least the first, some image's the second

X_DIM = 20
# name: (encoder hidden, encoder latent)
MODELS = {"S1": ([24], [6]), "S2": ([20, 12], [6, 4]),
          # hidden 64: the smallest multiple of 32 at which a one-layer model's engine plan
          # leaves the in-launch bound its LDS at k = 256 (K256 only)
          "S3": ([64], [6])}

# name: (B, k, the branch it sits at)
POINTS = {
    "K17": (3, 17, "an image straddles 16-row workgroups of the in-launch bound"),
    "K63": (2, 63, "lane stride: the last lane idle"),
    "K64": (2, 64, "lane stride: one full pass"),
    "K65": (2, 65, "lane stride: a second pass of one lane"),
    "K128": (2, 128, "even k for the median; k1 = 64, k2 = 2"),
    "K130": (2, 130, "k1 = 65 > 64, k2 = 2"),
    "K256": (2, 256, "use_tc_bound's sample limit, inside"),
    "K257": (2, 257, "use_tc_bound's sample limit, outside; k1 = 257"),
    "K1024": (3, 1024, "the LDS-staged limit, inside"),
    "K1025": (2, 1025, "the LDS-staged limit, outside: LwView reads the global row"),
    "B64": (64, 4, "the in-launch bound's image limit, inside"),
    "B65": (65, 4, "the in-launch bound's image limit, outside; one workgroup (260 rows)"),
    "M65": (65, 127, "8255 rows: bound_kernel on several workgroups"),
    "C33": (33, 125, "CIWAE: Bimg = 66, 8250 rows, several workgroups, Bsplit = 33 inside one's stride"),
    "M1025": (65, 1025, "several workgroups and unstaged; 66625 rows: beyond the row-block path's automatic limit"),
}
SPLITS = {"K17": (17, 1), "K128": (64, 2), "K130": (65, 2)}
S2_POINTS = ("K65", "K130", "K257", "K1025", "M65")
PATHGRAD_CASES = ("K65-S2", "K257-S2")

ALL_LOSSES = ("VAE", "IWAE", "CIWAE", "L_alpha", "L_median", "L_power_p", "L_power_neg", "VAE_V1", "MIWAE", "PIWAE")
POINT_LOSSES = {
    "K17": ("IWAE", "L_median", "MIWAE"),
    "K1025": ("VAE", "IWAE", "CIWAE", "L_alpha", "L_power_p", "L_power_neg", "VAE_V1"),
    "C33": ("CIWAE",),
    "M1025": ("IWAE",),
}
WIDE_LOSSES = ("IWAE", "L_power_p", "L_power_neg", "MIWAE", "CIWAE", "IWAE_DREG")
WIDE_SCALE = 8.0

# case: seed, by the search of the module docstring (seeds 1301, 1302, ... in turn)
SEEDS = {
    "K17-S1": 1301, "K63-S1": 1301, "K64-S1": 1301, "K65-S1": 1301, "K65-S2": 1302, "K128-S1": 1301,
    "K130-S1": 1301, "K130-S2": 1304, "K256-S1": 1307, "K256-S3": 1301, "K257-S1": 1301, "K257-S2": 1310,
    "K1024-S1": 2020, "K1025-S1": 1301, "K1025-S2": 1301, "B64-S1": 1303, "B65-S1": 1302, "M65-S1": 1304,
    "M65-S2": 1302, "C33-S1": 1301, "M1025-S1": 1301, "WIDE": 1301, "TIE64": 1301, "TIE65": 1303,
}
# 65 images of 127 samples: no seed serves them all, so the noise of each image that
# misses the bar is drawn again, from (seed, image, attempt), until every image meets it
REDRAWN = ("M65-S1", "M65-S2")


def _case(model, B, k, seed):
    he, le = MODELS[model]
    hd, ld = S._mirror(he, le, X_DIM)
    return (list(he), hd, list(le), ld, X_DIM, B, k, seed)


def _table():
    out, point = {}, {}
    for pt, (B, k, _) in POINTS.items():
        models = ["S1"] + (["S2"] if pt in S2_POINTS else []) + (["S3"] if pt == "K256" else [])
        for mdl in models:
            name = f"{pt}-{mdl}"
            out[name], point[name] = _case(mdl, B, k, SEEDS[name]), pt
    out["WIDE"] = _case("S2", 3, 96, SEEDS["WIDE"])
    out["TIE64"] = _case("S2", 3, 64, SEEDS["TIE64"])
    out["TIE65"] = _case("S2", 3, 65, SEEDS["TIE65"])
    return out, point


# name: (he, hd, le, ld, x_dim, B, k, seed), as shape_cases.CASES; POINT_OF: its row of POINTS
CASES, POINT_OF = _table()
CONSTRUCTED = ("WIDE", "TIE64", "TIE65")
TIES = ("TIE64", "TIE65")


def loss_variants(name):
    """(id, loss, model keywords) of every train-step loss a case runs
    (parameters as shape_cases.loss_variants)."""
    k = CASES[name][6]
    k1, k2 = S.split_k(k)
    if name == "WIDE":
        ids, (k1, k2) = WIDE_LOSSES, (48, 2)
    elif name in TIES:
        ids = ("L_median",)
    else:
        pt = POINT_OF[name]
        ids = POINT_LOSSES.get(pt, ALL_LOSSES) + (("IWAE_STL", "IWAE_DREG") if name in PATHGRAD_CASES else ())
        k1, k2 = SPLITS.get(pt, (k1, k2))
    kw = {"CIWAE": dict(beta=0.3), "L_alpha": dict(alpha=0.3), "L_power_p": dict(p=2.5), "L_power_neg": dict(p=-1.5),
          "MIWAE": dict(k1=k1, k2=k2), "PIWAE": dict(k1=k1, k2=k2)}
    return [(v, "L_power_p" if v == "L_power_neg" else v, kw.get(v, {})) for v in ids]


def variant(name, vid):
    return next(v for v in loss_variants(name) if v[0] == vid)


CASE_LOSS = [(n, v[0]) for n in CASES for v in loss_variants(n)]


def _lw(spec, params, x, eps):
    return O.forward(params, spec, x, eps)["lw"]


def _place_last(spec, params, x, eps):
    """Within each image, swap the noise of two samples so that index k - 1 -- reached
    only by the last pass of every lane-strided loop -- holds the sample of the
    largest log-weight (even images) or of the median's rank (k - 1) // 2 (odd
    images): a pass left out then costs the bound's heaviest row, not a negligible one."""
    lw = _lw(spec, params, x, eps)
    k, B = lw.shape
    order = np.argsort(lw, axis=0, kind="stable")
    for b in range(B):
        src = order[k - 1 if b % 2 == 0 else (k - 1) // 2, b]
        for e in eps:
            e[[src, k - 1], b] = e[[k - 1, src], b]


def _make(name, seed):
    he, hd, le, ld, x_dim, B, k, _ = CASES[name]
    spec, params, mean, x, eps = R.make_case((he, hd, le, ld), B, k, seed, x_dim=x_dim)
    if name == "WIDE":
        w, b = params["out.l3"]
        params["out.l3"] = [(w * WIDE_SCALE).astype(np.float32).astype(np.float64), b]
    if name in REDRAWN:
        lw = _lw(spec, params, x, eps)
        bar = 1.5 * MEDIAN_BAR * np.abs(lw).max()
        for b in np.flatnonzero(_gaps(lw, False).min(axis=0) < bar):
            for attempt in range(1, 300):
                rng = np.random.default_rng([seed, int(b), attempt])
                for e in eps:
                    e[:, b, :] = rng.standard_normal(e[:, b, :].shape).astype(np.float32)
                if _gaps(_lw(spec, params, x[b:b + 1], [e[:, b:b + 1] for e in eps]), False).min() >= bar:
                    break
    if k > 64 and name not in TIES:
        _place_last(spec, params, x, eps)
    if name in TIES:
        lw = _lw(spec, params, x, eps)
        order = np.argsort(lw, axis=0, kind="stable")
        for b in range(B):
            top, mid = order[k - 1, b], order[(k - 1) // 2, b]
            for e in eps:
                e[top, b, :] = e[mid, b, :]
    return spec, params, mean, x, eps


@functools.lru_cache(maxsize=None)
def make(name):
    """(spec, params, mean, x, eps) of a case in float64, parameters and noise
    rounded through float32 (pathgrad_ref.make_case).  Shared: do not modify."""
    out = _make(name, CASES[name][7])
    for e in out[4]:
        e.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def second_draw(name):
    """CIWAE's second, independent noise draw of a case (float32-rounded)."""
    he, hd, le, ld, x_dim, B, k, seed = CASES[name]
    rng = np.random.default_rng(seed + 5000)
    spec, params, _, x, _ = make(name)
    eps = [e.astype(np.float32).astype(np.float64) for e in O.draw_eps(spec, k, B, rng)]
    if k > 64:
        _place_last(spec, params, x, eps)
    return eps


@functools.lru_cache(maxsize=None)
def log_weights(name):
    """The oracle's float64 log-weights [k, B] of a case's first draw."""
    spec, params, _, x, eps = make(name)
    lw = _lw(spec, params, x, eps)
    lw.setflags(write=False)
    return lw


def _gaps(lw, tie):
    k = lw.shape[0]
    lo, hi = O.median_indices(k)
    if tie and k % 2:                 # the copy holds rank hi + 1: the gap above the tied pair
        hi += 1
    srt = np.sort(lw, axis=0)
    return np.stack([srt[lo] - srt[lo - 1], srt[hi + 1] - srt[hi]])


def median_gaps(name):
    """Per image, the gaps between the order statistics lo - 1, lo and hi, hi + 1
    of the oracle's log-weights, [2, B], and the bar on them: twice the GPU
    tests' log-weight bar, 2 * 1e-4 max|lw| (two rows may each move by it).
    TIE: the tied rows count as one, the gaps are those around them."""
    lw = log_weights(name)
    return _gaps(lw, name in TIES), MEDIAN_BAR * np.abs(lw).max()


def search_seed(name, first=1301, tries=20000):
    """The first seed from `first` whose draw meets median_gaps' bar in every
    image (how SEEDS was made; cases without L_median keep `first`)."""
    median = "L_median" in [v[0] for v in loss_variants(name)]
    for seed in range(first, first + tries):
        spec, params, _, x, eps = _make(name, seed)
        lw = _lw(spec, params, x, eps)
        spread = lw.max(axis=0) - lw.min(axis=0)
        if name == "WIDE" and not (spread.min() >= WIDE_SPREAD[0] and spread.max() >= WIDE_SPREAD[1]):
            continue
        if not median or _gaps(lw, name in TIES).min() >= MEDIAN_BAR * np.abs(lw).max():
            return seed
    raise RuntimeError(name)


def reference_step(name, vid, dtype=None):
    """(loss, flat gradient, flat post-Adam weights) of a case's train step (Adam
    lr 1e-3, eps 1e-4) by the oracle in `dtype` arithmetic (default float64):
    shape_cases.reference_step on this table."""
    dtype = dtype or np.float64
    _, loss, kw = variant(name, vid)
    spec, params, _, x, eps = make(name)
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


def reference_bound(name, vid):
    """The float64 value of a case's bound (forward only)."""
    _, loss, kw = variant(name, vid)
    spec, params, _, x, eps = make(name)
    kw = dict(kw)
    if loss == "CIWAE":
        kw["eps2"] = second_draw(name)
    if loss in R.LOSSES:                          # the path-gradient losses report IWAE's value
        loss = "IWAE"
    return float(O.objective_and_grads(params, spec, x, eps, loss, CASES[name][6], with_grads=False, **kw)[0])


# cases whose numbers allow the in-launch bound on the default path but whose engine
# plan leaves less LDS than 64 + 8 r4(k) floats: bound_kernel runs (measured on an MI355X)
LDS_FALLBACK = ("K256-S1",)


def on_engine(name, vid, path="auto"):
    """use_engine on these models (their widths fit the engine's LDS by far)."""
    _, loss, kw = variant(name, vid)
    he, B, k = CASES[name][0], CASES[name][5], CASES[name][6]
    rows = (2 * B if loss == "CIWAE" else B) * k
    return (path == "auto" and loss not in S.NO_ENGINE_LOSSES and not (loss == "L_power_p" and kw["p"] < 0)
            and len(he) <= S.kTcMaxLayers and rows <= ENGINE_ROWS)


def expected_bound(name, vid, path="auto", tc_bound=True):
    """Where a train step of this case computes its bound: ("in-launch", 0) in the
    engine's backward launch, or ("standalone", n) by bound_kernel on n = 1 or
    n > 1 workgroups.  From use_engine / use_tc_bound's numeric limits and
    launch_bound's grid rule; the LDS condition aside (LDS_FALLBACK)."""
    _, loss, kw = variant(name, vid)
    he, hd, le, ld, x_dim, B, k, seed = CASES[name]
    Bimg = 2 * B if loss == "CIWAE" else B
    rows = Bimg * k
    engine = on_engine(name, vid, path)
    need_bce_or_kl = loss in ("L_alpha", "VAE_V1")
    if engine and tc_bound and k <= TC_BOUND_K and Bimg <= TC_BOUND_IMAGES and not need_bce_or_kl:
        return "in-launch", 0
    one = Bimg <= 4 * BOUND_WAVES or rows <= BOUND_ROWS
    return "standalone", 1 if one else -(-Bimg // BOUND_WAVES)


def rejected(loss, k):
    """make_plan: the losses whose reductions need the LDS copy stop at k = 1024."""
    return loss in ("L_median", "MIWAE", "PIWAE") and k > STAGED_K


# ------------------------------------------------------------ NLL reductions
# lse_kernel reads 8 x 256 rows per pass (2047 / 2049: either side of one pass);
# the weight-ring kernel serves kS >= 128 only (127 / 128)
NLL_KS = (1, 63, 65, 127, 128, 2047, 2049)
NLL_B = 3
NLL_SEED = {"S1": 1401, "S2": 1402}


@functools.lru_cache(maxsize=None)
def nll_case(model, k):
    """(he, hd, le, ld), (spec, params, mean, x, eps) of a log p(x) case: B = 3 images, k samples."""
    he, hd, le, ld = _case(model, NLL_B, k, 0)[:4]
    return (he, hd, le, ld), R.make_case((he, hd, le, ld), NLL_B, k, NLL_SEED[model] + k, x_dim=X_DIM)


@functools.lru_cache(maxsize=None)
def nll_reference(model, k, dtype=np.float64):
    spec, params, _, x, eps = nll_case(model, k)[1]
    out = O.log_px_per_image(O.cast_params(params, dtype), spec, x.astype(dtype), k, eps=[e.astype(dtype) for e in eps])
    out.setflags(write=False)
    return out
