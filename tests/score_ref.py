"""Float64 reference of the densities of caller-supplied latents (iwae_score):
log q(h|x), log p(h), log p(x|h) and p(h_1) per row, on the oracle's own
functions (O._stoch_forward, O.normal_log_prob; the Bernoulli and PROB_SCALE /
PROB_SHIFT lines restate O.forward's), plus the cases and latent sets the CPU
and GPU tests share.

Formulas (F:60 / F:70, F:134-F:142, F:123-F:129), h = [h_1 .. h_L], each [k, B, d_i]:
  logq  = log N(h_1; enc_0(x)) + sum_{i>=1} log N(h_{i+1}; enc_i(h_i))
  logp  = log N(h_L; 0, 1) + sum_j log N(h_{L-1-j}; dec_j(h_{L-j}))
  logpx = sum_pixels log Bern(x | p(h_1)),  p = sigmoid(logit) (1 - 1e-6) + 1e-7
"""
import functools

import numpy as np

from oracle import iwae_oracle as O
import pathgrad_ref as PR

X_DIM = PR.X_DIM

# name: (arch, B, k, seed, x_dim, lstd bias shift)
CASES = {name: ((he, hd, le, ld), B, k, seed, X_DIM, 0.0) for name, (he, hd, le, ld, B, k, seed) in PR.SHAPES.items()}
_S2 = PR.SHAPES["S2"]
# several tiles per image, image boundaries inside tiles, above the k at which the ring would serve an NLL
CASES["K130"] = (tuple(_S2[:4]), 3, 130, 966, X_DIM, 0.0)
CASES["C784"] = (([200], [200], [50], [784]), 20, 5, 977, 784, 0.0)
# scales of about e^-3, as in a trained encoder.  The seed is chosen by the CPU emulation of bf16x3 alone
# (test_score_ref.py::test_sharp_case_emulation_stays_within_the_max_bar): with prior latents log p(h) is a small
# sum (max|ref| about 13) of terms whose means carry the products' rounding times 1 / scale = e^3, and the
# emulation itself lands at 0.6 to 1.3 of the 1e-4 bar over seeds 988 .. 991; 990 is the lowest (0.56).
CASES["SH"] = (tuple(_S2[:4]), _S2[4], _S2[5], 990, X_DIM, -3.0)
LATENTS = ("on", "off", "prior")
# a second registry of the same tuples, filled by the modules that bring cases of their own
# (tests/latent_shape_cases.py): case(), latents() and reference() find them, CASES and every test
# parametrized over it stay as they are
EXTRA_CASES = {}


def entry(name):
    """The case's tuple, from CASES or from the second registry."""
    return CASES[name] if name in CASES else EXTRA_CASES[name]


def f32r(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def case(name):
    """(spec, params, x, eps): float32-representable float64 arrays."""
    arch, B, k, seed, x_dim, shift = entry(name)
    spec, params, _, x, eps = PR.make_case(arch, B, k, seed, x_dim=x_dim)
    if shift:
        params = {n: [w, f32r(b + shift) if n.endswith(".lstd") else b] for n, (w, b) in params.items()}
    return spec, params, x, eps


@functools.lru_cache(maxsize=None)
def latents(name, which, rounded=True):
    """One latent set of a case, [k, B, d_i] per layer; rounded through float32 unless told otherwise."""
    spec, params, x, eps = case(name)
    _, B, k, seed, _, _ = entry(name)
    L = spec.L
    if which == "on":                     # O.forward's own h for the case's eps
        h = O.forward(params, spec, x, eps)["h"]
    elif which == "off":                  # independent of the model
        rng = np.random.default_rng(seed + 1)
        h = [1.5 * rng.standard_normal((k, B, d)) for d in spec.n_latent_encoder]
    elif which == "prior":                # ancestral samples through the oracle's decoder layers
        rng = np.random.default_rng(seed + 2)
        h = [None] * L
        h[L - 1] = rng.standard_normal((k, B, spec.n_latent_encoder[L - 1]))
        for j in range(L - 1):
            di = O._stoch_forward(params, f"dec{j}", h[L - 1 - j])
            h[L - 2 - j] = rng.standard_normal(di["mu"].shape) * di["scale"] + di["mu"]
    else:
        raise ValueError(which)
    return [f32r(v) for v in h] if rounded else list(h)


def to_bf16(a):
    """float32 -> the nearest bfloat16 (ties to even), as float32."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(a))


def split(a):
    a = np.asarray(a, dtype=np.float32)
    hi = to_bf16(a)
    return hi, to_bf16(a - hi)


def dense_bf16x3(X, W, b):
    """X W + b as the kernels form it: a.b = a_hi b_hi + a_hi b_lo + a_lo b_hi on
    the bf16 hi / lo split of both operands (the bias row among the weights),
    float32 accumulate."""
    xh, xl = split(X)
    wh, wl = split(W)
    bh, bl = split(b)
    return (xl @ wh + xh @ wl) + xh @ wh + (bl + bh)


def _stoch(params, prefix, X, dense):
    if dense is None:
        return O._stoch_forward(params, prefix, X)
    W1, b1 = params[prefix + ".l1"]; W2, b2 = params[prefix + ".l2"]
    Wm, bm = params[prefix + ".lmu"]; Ws, bs = params[prefix + ".lstd"]
    y2 = np.tanh(dense(np.tanh(dense(X, W1, b1)), W2, b2))
    return dict(mu=dense(y2, Wm, bm), scale=np.exp(dense(y2, Ws, bs)) + X.dtype.type(O.SCALE_EPS))


def score(params, spec, x, h, dtype=np.float64, dense=None, split_targets=False):
    """Per row [k, B]: logq, logp, logpx, their scales Sq, Sp, Spx (the sum of the
    absolute values of the term's per-coordinate / per-pixel addends) and probs
    [k, B, x_dim].  dtype float32 runs the same lines in float32; dense: the
    matrix products' emulation (dense_bf16x3), densities in float32;
    split_targets: the densities evaluated at hi + lo of the split latent
    instead of the float32 value."""
    L = spec.L
    dt = np.dtype(dtype).type
    params = O.cast_params(params, dtype)
    x = np.asarray(x, dtype=dtype)
    h = [np.asarray(v, dtype=dtype) for v in h]
    tgt = h
    if split_targets:
        tgt = [np.add(*split(v)).astype(dtype) for v in h]

    def lp_sum(t, loc, scale):
        lp = O.normal_log_prob(t, loc, scale)[0]
        return lp.sum(-1), np.abs(lp).sum(-1)
    logq = Sq = None
    X = x
    for i in range(L):
        q = _stoch(params, f"enc{i}", X, dense)
        v, a = lp_sum(tgt[i], q["mu"], q["scale"])                # F:60, F:70
        logq, Sq = (v, a) if i == 0 else (logq + v, Sq + a)      # F:73
        X = h[i]
    W1, b1 = params["out.l1"]; W2, b2 = params["out.l2"]; W3, b3 = params["out.l3"]
    if dense is None:
        logit = np.tanh(np.tanh(h[0] @ W1 + b1) @ W2 + b2) @ W3 + b3
    else:
        logit = dense(np.tanh(dense(np.tanh(dense(h[0], W1, b1)), W2, b2)), W3, b3)
    s = 1.0 / (1.0 + np.exp(-logit))
    p = s * dt(O.PROB_SCALE) + dt(O.PROB_SHIFT)                  # F:126
    xb = x[None]
    terms = np.log1p(-p) * (1 - xb) + np.log(p) * xb             # F:127-F:128
    logpx, Spx = terms.sum(-1), np.abs(terms).sum(-1)
    logp, Sp = lp_sum(tgt[L - 1], dt(0.0), dt(1.0))              # F:135-F:136
    for j in range(L - 1):
        d = _stoch(params, f"dec{j}", h[L - 1 - j], dense)       # F:139
        v, a = lp_sum(tgt[L - 2 - j], d["mu"], d["scale"])       # F:140
        logp, Sp = logp + v, Sp + a                              # F:141
    return dict(logq=logq, logp=logp, logpx=logpx, probs=p, Sq=Sq, Sp=Sp, Spx=Spx)


@functools.lru_cache(maxsize=None)
def reference(name, which):
    """The float64 reference of a case's latent set: computed once, shared, read-only."""
    spec, params, x, _ = case(name)
    out = score(params, spec, x, latents(name, which))
    for v in out.values():
        v.setflags(write=False)
    return out


# the three Decoder methods of the reference (F:123-F:145), by their definitions
def get_log_pxIh(params, spec, x, h):
    return score(params, spec, x, h)["logpx"]


def get_log_ph(params, spec, h):
    spec_x = np.zeros((h[0].shape[1], spec.x_dim))
    return score(params, spec, spec_x, h)["logp"]


def get_log_pxh(params, spec, x, h):
    return get_log_pxIh(params, spec, x, h) + get_log_ph(params, spec, h)
