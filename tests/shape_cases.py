"""Named model shapes at the edges of the host code's width- and depth-dependent
decisions, shared by tests/test_shape_cases.py (CPU) and tests/test_gpu_shapes.py:

  T1      every dimension at its minimum; one sample row
  O1      x_dim % 4 == 2 read directly by the few-row launch; hidden 33; d = 5
  O2      odd x_dim; every width odd and below 32 (narrow row-block backward, 2 layers); d = 3
  O2w     33 images with x_dim % 4 != 0: the staged-copy branch of gemm_direct;
          widths beside 64; d = 33
  E3      the engine at its maximum depth (kTcMaxLayers), k = 9 = 3 * 3
  D4      the row-block maximum depth (kRbMaxJobs); 24 Dense layers; k = 6 = 3 * 2
  D5      beyond the row-block limit: layer-wise only; the NLL kernel's stage limit
  D8      IWAE_MAX_LAYERS
  W511 / W512   either side of kRbMaxWidth
  W1024   hidden 1024: beyond the few-row launches' width (smallm_ok) and the
          fused update's tile table (kUpdMaxTiles) with the engine still on
  WX      hidden WX_H: the smallest multiple of 64 whose engine plan does not fit the LDS
  E2t     264 odd-width sample rows: the combined image-row backward + update launch

expected_paths() restates the library's dispatch rules (csrc/iwae_model.hip:
use_engine, tc_fits, use_fused, rb_width_ok, use_update, smallm_ok, gemm_direct,
mega_plan) from a case's numbers alone; tests/test_shape_cases.py checks its
constants against the sources."""
import functools

import pathgrad_ref as R

# limits of the library, by their names in csrc/iwae_model.hip / csrc/iwae_kernels.h
kTcMaxLayers = 3          # engine: stochastic layers
kRbMaxJobs = 4            # row-block kernels: stochastic layers
kRbMaxWidth = 512         # row-block kernels: fin + 1 and fout + 1 of every Dense but the first and the last
kUpdMaxJobs = 20          # fused update / wide weight-gradient pass: Dense layers
kUpdMaxTiles = 384        # fused update: 64 x 64 tiles over all Dense layers
kMgMaxBufs = 12           # fused NLL kernel: LDS buffers (L + 1)
kMgMaxStages = 24         # fused NLL kernel: Dense stages after the first encoder layer (6 L - 3)
kTcLdsBytes = 160 * 1024  # LDS of a workgroup (engine and NLL plans)
UPD_ROWS = 4096           # tuning default upd_rows
SMALLM_ROWS = 32          # tuning default smallm_rows: images of the few-row launches
SMALLM_WIDTH = 1024       # smallm_ok: fin + 1 and fout of the first encoder layer's three Dense
TCU_ROWS = 256            # engine_train_body: sample rows from which the combined launch runs
RB_ROWS = 65536           # use_fused on the auto path

NO_ENGINE_LOSSES = ("VAE_V1", "IWAE_STL", "IWAE_DREG")


def _r32(v):
    return (v + 31) // 32 * 32


def _mirror(he, le, x_dim):
    return list(he)[::-1], list(le)[::-1][1:] + [x_dim]


def _plane_ld(width):
    """Row stride (bf16) of an LDS buffer: 8 mod 16 dwords (tc_layout, mega_plan's first pass)."""
    sdw = (max(width, 32) + 1) // 2
    while sdw % 16 != 8:
        sdw += 1
    return 2 * sdw


def engine_lds_bytes_1layer(H, d, x_dim):
    """tc_layout at rt = 1 (16 rows) of the widest launch of a 1-layer engine
    step, plus the per-row accumulators: buffer widths as tc_build_jobs needs them
    (ldF = r32(fin + 1), ldG = r32(fout))."""
    launches = [
        [max(_r32(d + 1), _r32(H + 1)), _r32(H + 1)],            # forward job O: o1 -> o2 -> o3
        [max(_r32(x_dim), _r32(H)), _r32(H)],                    # backward job O'
        [_r32(H + 1), _r32(H + 1)],                              # image-row job I: l2 -> head
        [max(_r32(2 * d), 2 * d), _r32(H), 256],                 # image-row job I' and its reduction scratch
    ]
    worst = max(sum(2 * 16 * _plane_ld(w) * 2 for w in bufs) for bufs in launches)
    return (worst + 15) // 16 * 16 + (4 + 4 * 8) * 16 * 4


def _wx_width():
    H = 64
    while engine_lds_bytes_1layer(H, 8, 16) <= kTcLdsBytes:
        H += 64
    return H


# H + 1 pads to H + 32 columns, whose stride of 8 mod 16 dwords is H + 48 bf16: two
# such buffers of 16 rows, hi and lo planes, take 128 (H + 48) bytes beside 2304 bytes
# of accumulators; 128 * 1264 + 2304 = 164096 > 163840 first at H = 1216.
WX_H = _wx_width()


def _case(he, le, x_dim, B, k, seed):
    hd, ld = _mirror(he, le, x_dim)
    return (list(he), hd, list(le), ld, x_dim, B, k, seed)


# name: (he, hd, le, ld, x_dim, B, k, seed)
CASES = {
    "T1": _case([1], [1], 5, 1, 1, 1201),
    "O1": _case([33], [5], 30, 3, 5, 1202),
    "O2": _case([31, 17], [7, 3], 37, 5, 7, 1203),
    "O2w": _case([65, 63], [33, 9], 66, 33, 2, 1204),
    "E3": _case([37, 23, 13], [11, 6, 2], 64, 4, 9, 1205),
    "D4": _case([24, 20, 16, 12], [10, 8, 6, 4], 32, 3, 6, 1206),
    "D5": _case([20, 16, 12, 10, 8], [8, 6, 5, 4, 3], 32, 3, 4, 1207),
    "D8": _case([8] * 8, [3] * 8, 16, 2, 3, 1208),
    "W511": _case([511], [4], 16, 2, 3, 1209),
    "W512": _case([512], [4], 16, 2, 3, 1210),
    "W1024": _case([1024], [8], 16, 2, 3, 1211),
    "WX": _case([WX_H], [8], 16, 2, 3, 1212),
    "E2t": _case([35, 29], [9, 5], 42, 33, 8, 1213),
}
# the cases every loss runs on, and the two of them the path-gradient losses run on
LOSS_CASES = ("O2", "O2w", "E3", "D4")
PATHGRAD_CASES = ("O2", "D4")


def split_k(k):
    """(k1, k2) with k1 * k2 = k: the most balanced split (k1 >= k2; a prime k: (k, 1))."""
    k2 = max(f for f in range(1, int(k ** 0.5) + 1) if k % f == 0)
    return k // k2, k2


def loss_variants(name):
    """(id, loss, model keywords) of every train-step loss a case runs."""
    k = CASES[name][6]
    out = [("IWAE", "IWAE", {})]
    if name in LOSS_CASES:
        k1, k2 = split_k(k)
        out += [("VAE", "VAE", {}), ("CIWAE", "CIWAE", dict(beta=0.3)), ("L_alpha", "L_alpha", dict(alpha=0.3)),
                ("L_median", "L_median", {}), ("L_power_p", "L_power_p", dict(p=2.5)),
                ("L_power_neg", "L_power_p", dict(p=-1.5)), ("VAE_V1", "VAE_V1", {}),
                ("MIWAE", "MIWAE", dict(k1=k1, k2=k2)), ("PIWAE", "PIWAE", dict(k1=k1, k2=k2))]
    if name in PATHGRAD_CASES:
        out += [("IWAE_STL", "IWAE_STL", {}), ("IWAE_DREG", "IWAE_DREG", {})]
    return out


@functools.lru_cache(maxsize=None)
def make(name):
    """(spec, params, mean, x, eps) of a case in float64, parameters and noise
    rounded through float32 (pathgrad_ref.make_case).  Shared: do not modify."""
    he, hd, le, ld, x_dim, B, k, seed = CASES[name]
    return R.make_case((he, hd, le, ld), B, k, seed, x_dim=x_dim)


@functools.lru_cache(maxsize=None)
def second_draw(name):
    """CIWAE's second, independent noise draw of a case (float32-rounded)."""
    import numpy as np
    from oracle import iwae_oracle as O
    he, hd, le, ld, x_dim, B, k, seed = CASES[name]
    rng = np.random.default_rng(seed + 5000)
    return [e.astype(np.float32).astype(np.float64) for e in O.draw_eps(make(name)[0], k, B, rng)]


def variant(name, vid):
    return next(v for v in loss_variants(name) if v[0] == vid)


def reference_step(name, vid, dtype=None):
    """(loss, flat gradient, flat post-Adam weights) of a case's train step (Adam
    lr 1e-3, eps 1e-4) by the oracle in `dtype` arithmetic (default float64)."""
    import numpy as np
    from oracle import iwae_oracle as O
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


def dense_layers(name):
    """(fin, fout) of the library's Dense layers in its order: per stochastic
    layer l1, l2 and the head (mu | std, 2 d columns); encoder, decoder, output MLP."""
    he, hd, le, ld, x_dim = CASES[name][:5]
    L = len(he)
    out = []
    for i in range(L):
        fin = x_dim if i == 0 else le[i - 1]
        out += [(fin, he[i]), (he[i], he[i]), (he[i], 2 * le[i])]
    for j in range(L - 1):
        out += [(le[L - 1 - j], hd[j]), (hd[j], hd[j]), (hd[j], 2 * ld[j])]
    return out + [(le[0], hd[L - 1]), (hd[L - 1], hd[L - 1]), (hd[L - 1], x_dim)]


def _engine_fits(name):
    he, hd, le, ld, x_dim = CASES[name][:5]
    if len(he) == 1:
        return engine_lds_bytes_1layer(he[0], le[0], x_dim) <= kTcLdsBytes
    # deeper models: at most L + 1 buffers (forward job E), none wider than the widest
    # padded operand or the reduction scratch; every such case here fits by far
    w = max(256, max(_r32(max(fin + 1, fout)) for fin, fout in dense_layers(name)))
    bound = (len(he) + 1) * 2 * 16 * _plane_ld(w) * 2 + (4 + 4 * 8) * 16 * 4
    if bound > kTcLdsBytes:
        raise NotImplementedError("engine LDS fit of a deep and wide model")
    return True


def _mega_fits(name):
    """mega_plan: L + 1 buffers; conservative width as _engine_fits, exact for 1 layer."""
    he, hd, le, ld, x_dim = CASES[name][:5]
    L = len(he)
    if L == 1:
        widths = [max(_r32(le[0] + 1), he[0], _r32(he[0] + 1)), max(he[0], _r32(he[0] + 1))]
    else:
        widths = [max(_r32(max(fin + 1, fout)) for fin, fout in dense_layers(name))] * (L + 1)
    bf16 = sum(2 * 16 * _plane_ld(w) for w in widths)
    fits = ((bf16 + 3) // 2 // 2 * 2 + 2 * 16 + 8 * 16) * 4 <= kTcLdsBytes
    if L > 1 and not fits:
        raise NotImplementedError("NLL LDS fit of a deep and wide model")
    return fits


def expected_paths(name, loss="IWAE", kernel_path="auto", precision="bf16x3", p=1.0):
    """Which kernels a call on this case must use, from its numbers alone:
    engine, row_block, update (fused update launch), combined (image-row backward
    + update in one launch), few_row (first encoder layer on the few-row
    launches), x_direct (the step's first kernel reads the caller's x),
    nll_fused (the fused NLL kernel serves log_px).  p: L_power_p's exponent."""
    he, hd, le, ld, x_dim, B, k, seed = CASES[name]
    L = len(he)
    dense = dense_layers(name)
    x3 = precision == "bf16x3"
    Bimg = 2 * B if loss == "CIWAE" else B
    rows = Bimg * k
    # use_engine (+ tc_fits)
    engine = (x3 and kernel_path in ("auto", "engine") and loss not in NO_ENGINE_LOSSES
              and not (loss == "L_power_p" and p < 0) and L <= kTcMaxLayers
              and le[0] <= 2048 and rows <= 1 << 18 and _engine_fits(name))
    # use_fused / rb_width_ok: every Dense but the input and the output layer
    widths_ok = all(fin + 1 <= kRbMaxWidth and fout + 1 <= kRbMaxWidth for fin, fout in dense[1:-1])
    fused_ok = kernel_path != "layerwise" and L <= kRbMaxJobs and widths_ok and (kernel_path == "fused" or rows <= RB_ROWS)
    row_block = fused_ok and not engine
    # use_update
    tiles = sum(-(-(fin + 1) // 64) * -(-fout // 64) for fin, fout in dense)
    update = engine and rows <= UPD_ROWS and tiles <= kUpdMaxTiles and len(dense) <= kUpdMaxJobs
    # smallm_ok, gemm_direct, do_train's direct
    smallm = Bimg <= SMALLM_ROWS and all(fin + 1 <= SMALLM_WIDTH and fout <= SMALLM_WIDTH for fin, fout in dense[:3])
    few_row = (engine or row_block) and smallm
    x_direct = Bimg == B and (few_row or (engine and not smallm and x_dim % 4 == 0))
    # nll_mega_ok / mega_plan
    nll_fused = (x3 and kernel_path != "layerwise" and L + 1 <= kMgMaxBufs and 6 * L - 3 <= kMgMaxStages
                 and _mega_fits(name))
    return dict(engine=engine, row_block=row_block, update=update, combined=update and rows >= TCU_ROWS,
                few_row=few_row, x_direct=x_direct, nll_fused=nll_fused)
