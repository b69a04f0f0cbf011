"""Float64 reference of the gradients of the scored densities with respect to
the latents (iwae_score_grad), on score_ref.py's cases and latent sets, the
emulation of the bf16x3 path, and the HMC reference built on them.

With z = (t - mu) / s, s = exp(zs) + 1e-6 and t a head's target latent:
  d log N / dt = -z / s,  d / dmu = z / s,  d / dzs = (z^2 - 1) (s - 1e-6) / s,
the head gradients carried back through head -> l2 -> l1 (tanh' = 1 - y^2) to
the latent the chain reads.
  log q:      h_1 gets its target term only (mu_0, s_0 depend on x); chain i >= 1
              gives h_{i+1} its target term and h_i the chain's dX
  log p(h):   -h_L, and each prior chain's target term and dX
  log p(x|h): dlogit = (x / p - (1 - x) / (1 - p)) (1 - 1e-6) sig (1 - sig),
              p = sig (1 - 1e-6) + 1e-7, back through the output MLP to h_1
"""
import functools

import numpy as np

from oracle import iwae_oracle as O
import score_ref as R

TERMS = ("q", "ph", "px")


def _mm(A, W, dense):
    """A W: exact, or as the kernels' bf16x3 product (no bias row)."""
    if dense is None:
        return A @ W
    return dense(A, W, np.zeros(W.shape[1], np.float32))


def _forward(params, prefix, X, dense):
    if dense is None:
        return O._stoch_forward(params, prefix, X)
    W1, b1 = params[prefix + ".l1"]; W2, b2 = params[prefix + ".l2"]
    Wm, bm = params[prefix + ".lmu"]; Ws, bs = params[prefix + ".lstd"]
    y1 = np.tanh(dense(X, W1, b1))
    y2 = np.tanh(dense(y1, W2, b2))
    # the head is one Dense with columns (mu | zs)
    P = dense(y2, np.concatenate([Wm, Ws], 1), np.concatenate([bm, bs]))
    d = Wm.shape[1]
    e = np.exp(P[..., d:])
    return dict(X=X, y1=y1, y2=y2, mu=P[..., :d], e=e, scale=e + X.dtype.type(O.SCALE_EPS))


def _chain(params, prefix, X, t, dense, with_dx=True):
    """One Gaussian chain scored at target t: (target gradient, dX or None)."""
    c = _forward(params, prefix, X, dense)
    s = c["scale"]
    z = t / s - c["mu"] / s
    tg = -z / s
    if not with_dx:
        return tg, None
    W1 = params[prefix + ".l1"][0]; W2 = params[prefix + ".l2"][0]
    Wh = np.concatenate([params[prefix + ".lmu"][0], params[prefix + ".lstd"][0]], 1)
    dP = np.concatenate([z / s, (z * z - 1) * c["e"] / s], -1)
    dY2 = _mm(dP, Wh.T, dense) * (1 - c["y2"] * c["y2"])
    dY1 = _mm(dY2, W2.T, dense) * (1 - c["y1"] * c["y1"])
    return tg, _mm(dY1, W1.T, dense)


def grads(params, spec, x, h, dtype=np.float64, dense=None):
    """{"q" | "ph" | "px": [L arrays [k, B, d_i]]}: the three gradient terms.
    dtype float32 runs the same lines in float32; dense: the matrix products'
    emulation (score_ref.dense_bf16x3), forward and backward-data."""
    L = spec.L
    dt = np.dtype(dtype).type
    params = O.cast_params(params, dtype)
    x = np.asarray(x, dtype=dtype)
    h = [np.asarray(v, dtype=dtype) for v in h]
    k = h[0].shape[0]
    zero = lambda: [np.zeros_like(v) for v in h]
    gq, gp, gx = zero(), zero(), zero()
    # log q
    tg, _ = _chain(params, "enc0", x, h[0], dense, with_dx=False)       # [B, d] heads broadcast over k
    gq[0] = gq[0] + tg
    for i in range(1, L):
        tg, dx = _chain(params, f"enc{i}", h[i - 1], h[i], dense)
        gq[i] = gq[i] + tg
        gq[i - 1] = gq[i - 1] + dx
    # log p(h)
    gp[L - 1] = gp[L - 1] - h[L - 1]
    for j in range(L - 1):
        tg, dx = _chain(params, f"dec{j}", h[L - 1 - j], h[L - 2 - j], dense)
        gp[L - 2 - j] = gp[L - 2 - j] + tg
        gp[L - 1 - j] = gp[L - 1 - j] + dx
    # log p(x | h_1)
    W1, b1 = params["out.l1"]; W2, b2 = params["out.l2"]; W3, b3 = params["out.l3"]
    if dense is None:
        y1 = np.tanh(h[0] @ W1 + b1); y2 = np.tanh(y1 @ W2 + b2); logit = y2 @ W3 + b3
    else:
        y1 = np.tanh(dense(h[0], W1, b1)); y2 = np.tanh(dense(y1, W2, b2)); logit = dense(y2, W3, b3)
    sg = 1.0 / (1.0 + np.exp(-logit))
    p = sg * dt(O.PROB_SCALE) + dt(O.PROB_SHIFT)
    xb = np.broadcast_to(x[None], (k,) + x.shape)
    dlogit = (xb / p - (1 - xb) / (1 - p)) * dt(O.PROB_SCALE) * (sg * (1 - sg))
    dY2 = _mm(dlogit, W3.T, dense) * (1 - y2 * y2)
    dY1 = _mm(dY2, W2.T, dense) * (1 - y1 * y1)
    gx[0] = gx[0] + _mm(dY1, W1.T, dense)
    return {"q": gq, "ph": gp, "px": gx}


@functools.lru_cache(maxsize=None)
def reference(name, which):
    """The float64 gradient terms of a case's latent set: computed once, shared, read-only."""
    spec, params, x, _ = R.case(name)
    out = grads(params, spec, x, R.latents(name, which))
    for t in out.values():
        for v in t:
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def emulated(name, which):
    """The bf16x3 emulation's gradient terms (float32 lines, emulated products)."""
    spec, params, x, _ = R.case(name)
    return grads(params, spec, x, R.latents(name, which), dtype=np.float32, dense=R.dense_bf16x3)


def rel_l2(got, ref, scale=None):
    """Relative L2 error of one layer's array; None where the reference is identically zero."""
    ref = np.asarray(ref, np.float64)
    den = np.linalg.norm(ref) if scale is None else scale
    if den == 0.0:
        return None
    return float(np.linalg.norm(np.asarray(got, np.float64) - ref) / den)


def combine(g, coef):
    """(sum_t c_t g_t per layer, sum_t |c_t| ||g_t|| per layer) for coef = (c_q, c_ph, c_px)."""
    L = len(g["q"])
    tot = [sum(c * np.asarray(g[t][i], np.float64) for c, t in zip(coef, TERMS)) for i in range(L)]
    scale = [sum(abs(c) * np.linalg.norm(np.asarray(g[t][i], np.float64)) for c, t in zip(coef, TERMS)) for i in range(L)]
    return tot, scale


@functools.lru_cache(maxsize=None)
def emulation_figures(name, which):
    """{term: worst relative L2 error over the layers} of the bf16x3 emulation against the reference."""
    ref, emu = reference(name, which), emulated(name, which)
    out = {}
    for t in TERMS:
        r = [rel_l2(a, b) for a, b in zip(emu[t], ref[t])]
        out[t] = max(v for v in r if v is not None)
    return out


# ------------------------------------------------------------------------ HMC
def log_joint(params, spec, x, h, **kw):
    s = R.score(params, spec, x, h, **kw)
    return np.asarray(s["logp"], np.float64) + np.asarray(s["logpx"], np.float64)


def hmc_step(params, spec, x, h, r, step, n_leapfrog, **kw):
    """One leapfrog trajectory (half kick, drift, half kick; identity mass) from
    (h, r) under log p(x, h): (proposal, H_old, H_new), each chain (s, b) its
    own, float64 state; kw selects the arithmetic of the densities and gradients."""
    def g(hs):
        t = grads(params, spec, x, hs, **kw)
        return [np.asarray(a, np.float64) + np.asarray(b, np.float64) for a, b in zip(t["ph"], t["px"])]
    q = [np.array(v, np.float64) for v in h]
    r = [np.array(v, np.float64) for v in r]
    H_old = -log_joint(params, spec, x, q, **kw) + 0.5 * sum((v * v).sum(-1) for v in r)
    gr = g(q)
    for _ in range(n_leapfrog):
        r = [a + 0.5 * step * b for a, b in zip(r, gr)]
        q = [a + step * b for a, b in zip(q, r)]
        gr = g(q)
        r = [a + 0.5 * step * b for a, b in zip(r, gr)]
    H_new = -log_joint(params, spec, x, q, **kw) + 0.5 * sum((v * v).sum(-1) for v in r)
    return q, H_old, H_new


# name: (step size, leapfrog steps, momentum seed): the float64 trajectory has |dH| < 5 on every chain
# and the emulated dH stays within 0.1 nats of it (tests/test_scoregrad_ref.py asserts both)
# (the encoder's own samples of these untrained models sit where the energy error is mostly negative: the step
# is as large as |dH| < 5 allows and the seed is the first of 4101.. at which two odd chains reject)
HMC_CASES = {"S2": (0.22, 4, 4119), "C784": (0.6, 5, 4103)}
# a second registry of the same tuples (tests/latent_shape_cases.py); HMC_CASES and its tests stay as they are
EXTRA_HMC_CASES = {}


def hmc_entry(name):
    return HMC_CASES[name] if name in HMC_CASES else EXTRA_HMC_CASES[name]


@functools.lru_cache(maxsize=None)
def hmc_case(name):
    """(momenta, proposal, H_old, H_new, log u, accept) of the case's "on" latents."""
    return hmc_run(name, *hmc_entry(name))


def hmc_run(name, step, nl, seed):
    """hmc_case at a given (step size, leapfrog steps, momentum seed)."""
    spec, params, x, _ = R.case(name)
    h = R.latents(name, "on")
    rng = np.random.default_rng(seed)
    r = [R.f32r(rng.standard_normal(v.shape)) for v in h]
    q, H0, H1 = hmc_step(params, spec, x, h, r, step, nl)
    dH = H1 - H0
    k, B = dH.shape
    chain = np.arange(k * B).reshape(k, B)
    # no chain at the margin: accepted by 0.4 nats on even chains, rejected by 0.4 on odd ones where u < 1 allows
    lu = -dH - 0.4
    rej = (chain % 2 == 1) & (-dH + 0.4 < 0)
    lu = np.where(rej, -dH + 0.4, lu)
    return r, q, H0, H1, lu, lu < -dH
