"""The models of tests/shape_cases.py under the two families of train steps that
came after its sweep, shared by tests/test_step_shape_cases.py (CPU) and
tests/test_gpu_step_shapes.py:

  the reweighted wake-sleep step (iwae_wake_sleep_step / _grad), WS_CASES:
    T1 O1 O2 O2w E3 D4 D5 D8 W511 W512   shape_cases' model, x_dim, (B, k) and seed, with WS_N dream pairs
    R20p20   20 x 3 wake rows + 20 dreams: each phase on the few-row launches, the joint fit (40 image rows) not
    R5p40    x read directly; 40 dreams through the split-K GEMM and a row-block job behind 5 image rows
    R40p5    copy_x of a 37-wide image; 5 dreams on the few-row launch behind 40 image rows
    Rk1      k = 1: per_image false, kS = 1 and nk_img = 0 in layer 0's GM_FIT job
    R32p1    B = 32 = smallm_rows exactly; the joint fit has 33 rows
  (the R cases on O2's model -- x_dim 37, widths 31 and 17, d = 7 and 3 -- at seed ROW_SEED);

  the pixel-masked train step (iwae_train_step_masked), MASKED_CASES: the same ten models, mask =
  missing_ref.make_mask(B, x_dim, seed + 2), x with NaN at the missing entries.  T1 runs at B = 2, k = 3: at
  B = 1 its only image is all missing and the loss's relative error ill-conditioned (3e-2 between the float32
  and float64 references).

The cases sit in the second registries of wakesleep_ref and missing_ref under these names, so
wakesleep_ref.case and missing_ref.shape_case serve them while wakesleep_ref.CASES, missing_ref.SHAPES and the
tests parametrized over them stay as they are.

expected() restates the library's dispatch (csrc/iwae_model.hip: ws_use_fused, use_fused, rb_width_ok,
smallm_ok, do_wake_sleep, ws_sleep_forward, ws_encoder_fit) from a case's numbers alone;
tests/test_step_shape_cases.py checks its constants against the sources.

Seeds.  A case keeps shape_cases' seed unless the float64 reference run in float32 misses a quarter of a GPU
bar on it; it then takes the first of seed + 1000 j, j = 1 .. 7, at which it keeps it, read with
latent_shape_cases' margin (SELECT = 0.9 of the quarter; the assertion stays at the quarter).  TRIES records j
per case: every case keeps its first seed (tests/test_step_shape_cases.py re-derives this)."""
import functools

import numpy as np

import missing_ref as M
import pathgrad_ref as PR
import shape_cases as S
import wakesleep_ref as W
from oracle import iwae_oracle as O
from shape_cases import RB_ROWS, SMALLM_ROWS, SMALLM_WIDTH, kRbMaxJobs, kRbMaxWidth

MODELS = ("T1", "O1", "O2", "O2w", "E3", "D4", "D5", "D8", "W511", "W512")
WS_N = {"T1": 1, "O1": 5, "O2": 9, "O2w": 35, "E3": 6, "D4": 5, "D5": 5, "D8": 3, "W511": 3, "W512": 3}
ROW_MODEL, ROW_SEED = "O2", 1303
# name: (B, k, n)
ROW_CASES = {"R20p20": (20, 3, 20), "R5p40": (5, 3, 40), "R40p5": (40, 2, 5), "Rk1": (6, 1, 4), "R32p1": (32, 2, 1)}
ALL_COEF_CASES = ("O2", "O2w", "D4") + tuple(ROW_CASES)
MASKED_T1 = (2, 3)                                  # (B, k) of the masked T1
EXTRA_LOSS_CASES = ("O2", "D4")
EXTRA_LOSSES = ("L_alpha", "IWAE_DREG")
BOUND_CASES = ("O2", "O2w", "D4", "D5")
OUT_X3_CASE, OUT_X3_ROWS = "O2w", 16

# the GPU bars (tests/test_gpu_wakesleep.py and tests/test_gpu_missing.py: values / loss and whole gradient
# relative, each tensor of its largest entry) and the quarter the float32 reference must keep
GPU_REL, GPU_TENSOR = 1e-4, 5e-4
SELECT = 0.9
SEED_TRIES = 8
TRIES = {}                                          # name: j of seed + 1000 j (absent: 0)


def _seed(seed, tries):
    return seed + 1000 * tries


# name: (he, hd, le, ld, x_dim, B, k, n, seed)
WS_CASES = {}
for _n in MODELS:
    _he, _hd, _le, _ld, _xd, _B, _k, _s = S.CASES[_n]
    WS_CASES[_n] = (_he, _hd, _le, _ld, _xd, _B, _k, WS_N[_n], _seed(_s, TRIES.get(_n, 0)))
for _n, (_B, _k, _nd) in ROW_CASES.items():
    _he, _hd, _le, _ld, _xd = S.CASES[ROW_MODEL][:5]
    WS_CASES[_n] = (_he, _hd, _le, _ld, _xd, _B, _k, _nd, _seed(ROW_SEED, TRIES.get(_n, 0)))

# name: (he, hd, le, ld, x_dim, B, k, seed)
MASKED_CASES = {}
for _n in MODELS:
    _he, _hd, _le, _ld, _xd, _B, _k, _s = S.CASES[_n]
    if _n == "T1":
        _B, _k = MASKED_T1
    MASKED_CASES[_n] = (_he, _hd, _le, _ld, _xd, _B, _k, _seed(_s, TRIES.get("M:" + _n, 0)))

WS_COEFS = {n: (W.COEFS if n in ALL_COEF_CASES else W.COEFS[2:]) for n in WS_CASES}
COEF_ID = {W.COEFS[0]: "wake", W.COEFS[1]: "sleep", W.COEFS[2]: "mix"}
MASKED_LOSSES = {n: ("IWAE",) + (EXTRA_LOSSES if n in EXTRA_LOSS_CASES else ()) for n in MASKED_CASES}


def register_ws(name, entry):
    he, hd, le, ld, x_dim, B, k, n, seed = entry
    W.EXTRA_CASES[name] = (he, hd, le, ld, B, k, n, seed, x_dim)


def register_masked(name, entry):
    he, hd, le, ld, x_dim, B, k, seed = entry
    assert hd == he[::-1] and ld == le[-2::-1] + [x_dim]          # missing_ref.shape_case mirrors the decoder itself
    M.EXTRA_SHAPES[name] = (he, hd, le, x_dim, B, k, seed)


for _n, _e in WS_CASES.items():
    assert _n not in W.CASES
    register_ws(_n, _e)
for _n, _e in MASKED_CASES.items():
    assert _n not in M.SHAPES
    register_masked(_n, _e)


def candidate(family, name, tries):
    """The registered name of a case at its seed after `tries` steps of the fixed order (0: the table's first)."""
    cname = f"{name}@{tries}"
    if family == "ws":
        e = WS_CASES[name]
        base = e[8] - 1000 * TRIES.get(name, 0)
        register_ws(cname, e[:8] + (_seed(base, tries),))
    else:
        e = MASKED_CASES[name]
        base = e[7] - 1000 * TRIES.get("M:" + name, 0)
        register_masked(cname, e[:7] + (_seed(base, tries),))
    return cname


# ------------------------------------------------------------ the dispatch, restated
def dense_layers(entry):
    """(fin, fout) of the library's Dense layers in its order (shape_cases.dense_layers, from a tuple)."""
    he, hd, le, ld, x_dim = entry[:5]
    L = len(he)
    out = []
    for i in range(L):
        fin = x_dim if i == 0 else le[i - 1]
        out += [(fin, he[i]), (he[i], he[i]), (he[i], 2 * le[i])]
    for j in range(L - 1):
        out += [(le[L - 1 - j], hd[j]), (hd[j], hd[j]), (hd[j], 2 * ld[j])]
    return out + [(le[0], hd[L - 1]), (hd[L - 1], hd[L - 1]), (hd[L - 1], x_dim)]


def rb_width_ok(entry):
    """Every Dense but the input and the output layer within the row-block kernels' LDS row."""
    return all(fin + 1 <= kRbMaxWidth and fout + 1 <= kRbMaxWidth for fin, fout in dense_layers(entry)[1:-1])


def smallm_ok(entry, rows):
    """The first encoder layer of `rows` image rows on the few-row launches."""
    return rows <= SMALLM_ROWS and all(fin + 1 <= SMALLM_WIDTH and fout <= SMALLM_WIDTH
                                       for fin, fout in dense_layers(entry)[:3])


def expected(name, entry, path, coef=W.COEFS[2], out_x3_rows=8192):
    """Which kernels a call on this case must use, from its numbers alone.  entry: a WS_CASES tuple (9 fields)
    or a MASKED_CASES tuple (8); path: "auto", "fused" or "layerwise"; coef = (c_wake, c_sleep).
      row_block     on the f32 row-block kernels (wake-sleep: GM_FIT counter 36, else 37; masked: counter 13)
      fit_counter   the wake-sleep call's GM_FIT counter
      out_x3        the output Dense on bf16x3 products
    and for a wake-sleep case on the row-block kernels (all False otherwise):
      x_direct      the wake forward's few-row launch reads the caller's x (else copy_x stages it)
      wake_few_row / sleep_few_row / fit_few_row   the first encoder layer of the wake images, of the dream
                    images, and the joint fit's dY2 / dY1 of layer 0 on the few-row launches
      fit_rows      image rows of layer 0's GM_FIT job
      per_image     layer 0's job walks kS sample rows per wake image"""
    L = len(entry[0])
    B, k = entry[5], entry[6]
    ws = len(entry) == 9
    n = entry[7] if ws else 0
    cw, cs = coef if ws else (0.0, 0.0)
    nd = n if cs > 0 else 0                                     # (a zero coefficient leaves its phase out)
    rows = B * k + nd
    row_block = path != "layerwise" and L <= kRbMaxJobs and rb_width_ok(entry) and (path == "fused" or rows <= RB_ROWS)
    out = dict(row_block=row_block, out_x3=out_x3_rows > 0 and B * k >= out_x3_rows)
    if not ws:
        return out
    wake = cw > 0
    fit_rows = B + nd - (0 if wake else B)
    out.update(fit_counter=36 if row_block else 37, fit_rows=fit_rows,
               x_direct=row_block and smallm_ok(entry, B),
               wake_few_row=row_block and smallm_ok(entry, B),
               sleep_few_row=row_block and nd > 0 and smallm_ok(entry, nd),
               fit_few_row=row_block and smallm_ok(entry, fit_rows),
               per_image=wake and k > 1)
    return out


# ------------------------------------------------------------------ references
ws_case = functools.lru_cache(maxsize=None)(W.case)
masked_case = functools.lru_cache(maxsize=None)(M.shape_case)


def _opt():
    return O.Adam(1e-3, 0.9, 0.999, 1e-4)


@functools.lru_cache(maxsize=None)
def ws_reference(name, coef, dtype=np.float64):
    """((L_theta, L_wake, L_sleep), flat gradient, post-Adam flat weights) of a wake-sleep case by
    wakesleep_ref.train_step in `dtype` arithmetic, as float64 arrays.  Shared: read-only."""
    c = ws_case(name)[4]
    if dtype is not np.float64:
        c = W.cast_case(c, dtype)
    spec, params, _, x, eps, dreams = c
    vals, new, g = W.train_step(params, spec, x, eps, dreams, coef[0], coef[1], _opt())
    g = np.asarray(g, np.float64)
    w = np.asarray(O.flatten_params(spec, new), np.float64)
    g.setflags(write=False)
    w.setflags(write=False)
    return tuple(float(v) for v in vals), g, w


@functools.lru_cache(maxsize=None)
def masked_reference(name, loss, dtype=np.float64):
    """(loss, flat gradient, post-Adam flat weights) of a masked case by missing_ref.train_step in `dtype`."""
    _, _, k, _, (spec, params, _, x, eps, eps2, mask) = masked_case(name)
    if dtype is not np.float64:
        params = O.cast_params(params, dtype)
        x, eps, eps2 = x.astype(dtype), [e.astype(dtype) for e in eps], [e.astype(dtype) for e in eps2]
    l, new, g = M.train_step(params, spec, x, mask, eps, loss, _opt(), **M.loss_kwargs(loss, k, eps2))
    g = np.asarray(g, np.float64)
    w = np.asarray(O.flatten_params(spec, new), np.float64)
    g.setflags(write=False)
    w.setflags(write=False)
    return float(l), g, w


def value_errors(got, ref):
    """Relative error per value; a value that is exactly 0 in the reference (an absent phase) must be exactly 0."""
    return [abs(a - b) / abs(b) if b != 0 else (0.0 if a == 0 else np.inf) for a, b in zip(got, ref)]


def compare(spec, got, ref):
    """(worst value error, whole-gradient relative L2, worst tensor by missing_ref.worst_tensor's rule) of
    (values, gradient, ...) tuples; a scalar loss counts as one value."""
    gv = got[0] if isinstance(got[0], tuple) else (got[0],)
    rv = ref[0] if isinstance(ref[0], tuple) else (ref[0],)
    return max(value_errors(gv, rv)), float(PR.rel_l2(got[1], ref[1])), M.worst_tensor(spec, got[1], ref[1])


def ws_figures(name, coef):
    """The float32 run of the reference against float64: (values, whole gradient, worst tensor)."""
    return compare(ws_case(name)[4][0], ws_reference(name, coef, np.float32), ws_reference(name, coef))


def masked_figures(name, loss):
    return compare(masked_case(name)[4][0], masked_reference(name, loss, np.float32), masked_reference(name, loss))


def within(fig, share):
    """The figures of compare() within `share` of the GPU bars."""
    return fig[0] <= share * GPU_REL and fig[1] <= share * GPU_REL and fig[2] <= share * GPU_TENSOR
