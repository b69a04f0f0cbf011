"""Model shapes at the edges of the row-chain engine's op loop (csrc/iwae_train.hip:
the per-op hot records, the unit counters of the weight pipeline, the padding
written per op or up front), shared by tests/test_engine_op_cases.py (CPU) and
tests/test_gpu_engine_ops.py:

  Ea   21 sample rows: a ragged second workgroup; every Dense op has at most 4
       column tiles, so most waves own no unit and take the hand-over of the next
       op's units; forward padding of 1, 31 and 32 columns, a backward op with none
  Eb   9 against 8 column tiles (wave 0 owns two units, the rest one); k = 160
       against 128: two against one k chunk
  Ec   exactly one full workgroup; 17 tiles (three units and more per wave: the
       A / B register sets); three k chunks; x_dim >= 241: the output layer split
       over jobs O1 / O2 (first tile t0 > 0)
  Et   264 rows, 33 images: the image-row jobs I and I', the combined launch
  E3b  three stochastic layers: the longest jobs E / E'

engine_ops() restates, from a case's numbers alone, the Dense ops the engine
runs and their geometry (tc_build_jobs, tc_dense_op, tc_resolve_hot)."""
import functools

import pathgrad_ref as R
import shape_cases as S

TC_NW = 8            # waves of an engine workgroup
TC_KCHUNK = 128      # k of one weight fetch unit (TC_KS = 4 steps of 32)

# name: (he, hd, le, ld, x_dim, B, k, seed)
CASES = {
    "Ea": S._case([33, 31], [32, 5], 40, 3, 7, 2301),
    "Eb": S._case([129, 127], [33, 17], 130, 2, 9, 2302),
    "Ec": S._case([257, 128], [64, 32], 260, 1, 16, 2303),
    "Et": S._case([129, 33], [31, 9], 66, 33, 8, 2304),
    "E3b": S._case([48, 33, 17], [32, 16, 3], 50, 2, 11, 2305),
}
EXTRA_LOSS_CASES = ("Ea", "Et")      # also PIWAE (the backward launch runs twice) and L_alpha (the BCE epilogue)
GRAPH_CASE = "Ec"                    # device noise: eager against a captured graph


def loss_variants(name):
    """(id, loss, model keywords) of the train-step losses a case runs."""
    out = [("IWAE", "IWAE", {})]
    if name in EXTRA_LOSS_CASES:
        k1, k2 = S.split_k(CASES[name][6])
        out += [("PIWAE", "PIWAE", dict(k1=k1, k2=k2)), ("L_alpha", "L_alpha", dict(alpha=0.3))]
    return out


def variant(name, vid):
    return next(v for v in loss_variants(name) if v[0] == vid)


@functools.lru_cache(maxsize=None)
def make(name):
    """(spec, params, mean, x, eps) of a case in float64, parameters and noise
    rounded through float32 (pathgrad_ref.make_case).  Shared: do not modify."""
    he, hd, le, ld, x_dim, B, k, seed = CASES[name]
    return R.make_case((he, hd, le, ld), B, k, seed, x_dim=x_dim)


def reference_step(name, vid, dtype=None):
    """(loss, flat gradient, flat post-Adam weights) of a case's train step (Adam
    lr 1e-3, eps 1e-4) by the oracle in `dtype` arithmetic (default float64)."""
    import numpy as np
    from oracle import iwae_oracle as O
    dtype = dtype or np.float64
    _, loss, kw = variant(name, vid)
    spec, params, _, x, eps = make(name)
    k = CASES[name][6]
    opt = O.Adam(1e-3, 0.9, 0.999, 1e-4)
    out = O.train_step(O.cast_params(params, dtype), spec, x.astype(dtype), [e.astype(dtype) for e in eps], loss, k,
                       opt, **kw)
    return float(out[0]), np.asarray(out[2], np.float64), np.asarray(O.flatten_params(spec, out[1]), np.float64)


def _r32(v):
    return (v + 31) // 32 * 32


def engine_ops(name):
    """The engine's Dense ops of a case: dicts with dir ('fwd' / 'bwd'), job,
    ntile (column tiles of N), nch (k chunks), units (per wave), pad (columns of
    padding behind the output, None: no LDS output) and t0 (first tile)."""
    he, hd, le, ld, x_dim, B, k, seed = CASES[name]
    L = len(he)
    rows = B * k

    def units(ntile, nch, t0=0):
        return [max(0, -(-(ntile - t0 - w) // TC_NW)) * nch for w in range(TC_NW)]

    def fwd(job, fin, fout, head, has_out, t0=0, ntile=None):
        N = 8 * -(-fout // 4) if head else fout          # heads: [mu quad | zs quad] groups of 8, fout = d
        nt = ntile if ntile is not None else -(-N // 16)
        nch = -(-_r32(fin + 1) // TC_KCHUNK)
        # an LDS output of width fout (heads: the d sampled columns) is read as the next op's k = r32(fout + 1)
        pad = _r32(fout + 1) - fout if has_out else None
        return dict(dir="fwd", job=job, ntile=nt, nch=nch, units=units(nt, nch, t0), pad=pad, t0=t0)

    def bwd(job, fin, fout, last):
        # dX = dZ W^T: N = fin, k = fout (heads: 2 d), padded to the next op's k = r32(fin)
        nt = -(-fin // 16)
        nch = -(-_r32(fout) // TC_KCHUNK)
        return dict(dir="bwd", job=job, ntile=nt, nch=nch, units=units(nt, nch), pad=None if last else _r32(fin) - fin,
                    t0=0)

    ops = []
    # forward: first encoder layer's l2 and head on image rows (job I, or folded), then job E, then O1 / O2
    ops += [fwd("I", he[0], he[0], False, True), fwd("I", he[0], le[0], True, False)]
    for i in range(1, L):
        ops += [fwd("E", le[i - 1], he[i], False, True), fwd("E", he[i], he[i], False, True),
                fwd("E", he[i], le[i], True, True)]
    for j in range(L - 1):
        ops += [fwd("E", le[L - 1 - j], hd[j], False, True), fwd("E", hd[j], hd[j], False, True),
                fwd("E", hd[j], ld[j], True, False)]
    H = hd[L - 1]
    ntile = -(-x_dim // 16)
    nsplit = 2 if ntile >= 16 and rows <= 2048 else 1
    for part in range(nsplit):
        t0 = part * (ntile // nsplit)
        t1 = ntile if part + 1 == nsplit else (part + 1) * (ntile // nsplit)
        job = "O%d" % (part + 1)
        ops += [fwd(job, le[0], H, False, True), fwd(job, H, H, False, True),
                fwd(job, H, x_dim, False, False, t0=t0, ntile=t1)]
    # backward: job O', job E' (prior layers, then encoder layers L-1 .. 1), job I'
    ops += [bwd("O'", H, x_dim, False), bwd("O'", H, H, False), bwd("O'", le[0], H, True)]
    for j in range(L - 1):
        ops += [bwd("E'", hd[j], 2 * ld[j], False), bwd("E'", hd[j], hd[j], False), bwd("E'", le[L - 1 - j], hd[j], True)]
    for i in range(L - 1, 0, -1):
        ops += [bwd("E'", he[i], 2 * le[i], False), bwd("E'", he[i], he[i], False), bwd("E'", le[i - 1], he[i], True)]
    ops += [bwd("I'", he[0], 2 * le[0], False), bwd("I'", he[0], he[0], True)]
    return ops


def job_ops(name, job):
    """Ops of one job, the elementwise ones included (SAMPLE0 / LOADG / GBWD_*)."""
    L = len(CASES[name][0])
    dense = sum(1 for o in engine_ops(name) if o["job"] == job)
    extra = {"E": 1, "E'": 2 * (L - 1), "O'": 1, "I": 1, "I'": 1}.get(job, 1)
    return dense + extra
