"""Float64 reference of training with missing pixels (Mattei & Frellsen 2019,
MIWAE), built on the oracle's own functions (oracle/iwae_oracle.py) as
pathgrad_ref.py is, plus the cases the CPU and GPU tests share.

mask [B, x_dim]: non-zero = observed.  The encoder sees where(mask, x, 0); the
log weights keep the Bernoulli terms of the observed pixels only,

    lw[s][b] = log p(h) + sum_j [mask_bj != 0] log Bern(x_bj | p_j) - log q(h | x (.) mask),

and so does the Keras-BCE row term of L_alpha / VAE_V1.  Every loss is the
oracle's function of these lw.  The gradient needs no new backward: with the
cache's sigmoid s set to 0 at the missing pixels, O.backward's
dlogit = dp * c * s (1 - s) vanishes exactly there, which is the masked
gradient (finite differences: tests/test_missing_ref.py)."""
import numpy as np

import pathgrad_ref as R
from oracle import iwae_oracle as O

ALPHA = 0.7
BETA = 0.5
ARCH2 = ([40, 24], [24, 40], [10, 6])

# name: (encoder hidden, decoder hidden, encoder latent, x_dim, B, k, seed)
SHAPES = {
    "M1": ([16], [16], [6], 64, 3, 5, 1911),
    "M2": (*ARCH2, 64, 5, 7, 1922),
    "M2w": (*ARCH2, 64, 33, 2, 1933),
    "M50": (*ARCH2, 50, 4, 3, 1944),
    "M50w": (*ARCH2, 50, 33, 3, 1955),      # x_dim % 4 != 0 and more than 32 images: the unmasked step stages x too
    "M784": ([200], [200], [50], 784, 20, 5, 1966),
    # 9540 sample rows: 75 x 7 tiles of 128 x 128 >= 512, where the tiled GEMM takes its 2 x 2-MFMA-tile kernel
    # (74.5 row tiles), and >= 8192, where a train step runs the output layer on bf16x3 products
    "M784k": ([200], [200], [50], 784, 20, 477, 1977),
}
# a second registry of the same tuples, filled by the modules that bring cases of their own
# (tests/step_shape_cases.py): shape_case() finds them, SHAPES and every test parametrized over it stay as they are
EXTRA_SHAPES = {}


def make_mask(B, x_dim, seed, p_obs=0.5):
    """Image 0 entirely missing, image 1 entirely observed, Bernoulli(p_obs) elsewhere."""
    rng = np.random.default_rng(seed)
    mask = (rng.random((B, x_dim)) < p_obs).astype(np.float64)
    mask[0] = 0.0
    if B > 1:
        mask[1] = 1.0
    return mask


def with_holes(x, mask, fill=np.nan):
    """x with ``fill`` written at the missing entries."""
    out = np.array(x, copy=True)
    out[mask == 0] = fill
    return out


def shape_case(name):
    """(arch, B, k, x_dim, (spec, params, mean, x, eps, eps2, mask)); x holds NaN where missing."""
    he, hd, le, x_dim, B, k, seed = SHAPES[name] if name in SHAPES else EXTRA_SHAPES[name]
    arch = (he, hd, le, le[-2::-1] + [x_dim])
    spec, params, mean, x, eps = R.make_case(arch, B, k, seed, x_dim=x_dim)
    rng = np.random.default_rng(seed + 1)
    eps2 = [e.astype(np.float32).astype(np.float64) for e in O.draw_eps(spec, k, B, rng)]
    mask = make_mask(B, x_dim, seed + 2)
    return arch, B, k, x_dim, (spec, params, mean, with_holes(x, mask), eps, eps2, mask)


def forward(params, spec, x, mask, eps, need_bce=False):
    """O.forward's cache of the masked model (lw, logpx, bce_row and s corrected)."""
    dt = x.dtype.type
    obs = np.asarray(mask) != 0
    xz = np.where(obs, x, dt(0))
    c = O.forward(params, spec, xz, eps, need_bce=need_bce)
    p, xb, mb = c["p"], xz[None], obs[None]
    t = np.log1p(-p) * (1 - xb) + np.log(p) * xb
    logpx = np.where(mb, t, dt(0)).sum(-1)
    c["lw"] = (c["logp"] + logpx) - c["logq"]
    c["logpx"] = logpx
    if need_bce:
        pc = np.clip(p, dt(O.KERAS_EPS), dt(1 - O.KERAS_EPS))
        b = xb * np.log(pc + dt(O.KERAS_EPS)) + (1 - xb) * np.log(1 - pc + dt(O.KERAS_EPS))
        c["bce_row"] = np.where(mb, b, dt(0)).sum(-1)
    c["s"] = np.where(mb, c["s"], dt(0))
    return c


def _add(g1, g2):
    return {n: [g1[n][0] + g2[n][0], g1[n][1] + g2[n][1]] for n in g1}


def objective_and_grads(params, spec, x, mask, eps, loss, p=1.0, alpha=ALPHA, beta=BETA, k1=None, k2=None, eps2=None,
                        with_grads=True):
    """(J, gradients) of the masked objective; dispatch as O.objective_and_grads
    and, for the path-gradient losses, pathgrad_ref.objective_and_grads."""
    if loss in ("VAE", "IWAE", "L_power_p", "L_median", "MIWAE"):
        c = forward(params, spec, x, mask, eps)
        lw = c["lw"]
        J = {"VAE": O.L_from_weights, "IWAE": O.L_k_from_weights, "L_median": O.L_median_from_weights,
             "L_power_p": lambda w: O.L_power_p_from_weights(w, p),
             "MIWAE": lambda w: O.MIWAE_from_weights(w, k1, k2)}[loss](lw)
        if not with_grads:
            return J, None
        return J, O.backward(params, spec, c, O.bound_grad(lw, loss, p=p, k1=k1, k2=k2))
    if loss == "PIWAE":
        c = forward(params, spec, x, mask, eps)
        lw = c["lw"]
        J = O.L_k_from_weights(lw)
        if not with_grads:
            return J, None
        g_dec = O.backward(params, spec, c, O.bound_grad(lw, "IWAE"), want=("dec",))
        g_enc = O.backward(params, spec, c, O.bound_grad(lw, "MIWAE", k1=k1, k2=k2), want=("enc",))
        return J, _add(g_dec, g_enc)
    if loss == "CIWAE":
        c1 = forward(params, spec, x, mask, eps)
        c2 = forward(params, spec, x, mask, eps2)
        J = beta * O.L_from_weights(c1["lw"]) + (1 - beta) * O.L_k_from_weights(c2["lw"])
        if not with_grads:
            return J, None
        g1 = O.backward(params, spec, c1, beta * O.bound_grad(c1["lw"], "VAE"))
        g2 = O.backward(params, spec, c2, (1 - beta) * O.bound_grad(c2["lw"], "IWAE"))
        return J, _add(g1, g2)
    if loss in ("L_alpha", "VAE_V1"):
        c = forward(params, spec, x, mask, eps, need_bce=True)
        lw = c["lw"]
        Eq = np.mean(c["bce_row"])
        if loss == "L_alpha":
            J = (1 - alpha) * Eq + alpha * O.L_from_weights(lw)
            a, bc, kl = np.full_like(lw, alpha / lw.size), np.full_like(lw, (1 - alpha) / lw.size), 0.0
        else:
            J = Eq - O.kl_v1(c)
            a, bc, kl = np.zeros_like(lw), np.full_like(lw, 1.0 / lw.size), -1.0
        if not with_grads:
            return J, None
        return J, O.backward(params, spec, c, a, bce_coef=bc, kl_coef=kl)
    if loss in R.LOSSES:
        c = forward(params, spec, x, mask, eps)
        lw = c["lw"]
        J = O.L_k_from_weights(lw)
        if not with_grads:
            return J, None
        g_dec = O.backward(params, spec, c, O.bound_grad(lw, "IWAE"), want=("dec",))
        g_enc = R.path_enc_grads(params, spec, c, R.enc_weights(lw, loss))
        return J, {n: g_enc[n] if n.startswith("enc") else g_dec[n] for n, _, _ in spec.dense}
    raise ValueError(f"unknown loss_function {loss!r}")


def train_step(params, spec, x, mask, eps, loss, opt, **kw):
    """(loss = -J, new parameters, flat gradient of the loss): O.train_step's contract."""
    J, gJ = objective_and_grads(params, spec, x, mask, eps, loss, **kw)
    dt = x.dtype
    flat_g = -O.flatten_params(spec, gJ).astype(dt)
    new_flat = opt.apply(O.flatten_params(spec, params).astype(dt), flat_g)
    return -J, O.unflatten_params(spec, new_flat, dtype=dt), flat_g


def surrogate(ps, pd, spec, x, mask, eps, a):
    """pathgrad_ref.surrogate of the masked model: sum(a * lw) with the
    encoder's sampling on ps and every density on pd."""
    L = spec.L
    obs = np.asarray(mask) != 0
    xz = np.where(obs, x, 0.0)
    X, h, logq = xz, [], 0.0
    for i in range(L):
        qs = O._stoch_forward(ps, f"enc{i}", X)
        hi = eps[i] * qs["scale"] + qs["mu"]
        qd = O._stoch_forward(pd, f"enc{i}", X)
        logq = logq + O.normal_log_prob(hi, qd["mu"], qd["scale"])[0].sum(-1)
        h.append(hi)
        X = hi
    W1, b1 = pd["out.l1"]; W2, b2 = pd["out.l2"]; W3, b3 = pd["out.l3"]
    logit = np.tanh(np.tanh(h[0] @ W1 + b1) @ W2 + b2) @ W3 + b3
    p = 1.0 / (1.0 + np.exp(-logit)) * O.PROB_SCALE + O.PROB_SHIFT
    xb = xz[None]
    logpx = np.where(obs[None], np.log1p(-p) * (1 - xb) + np.log(p) * xb, 0.0).sum(-1)
    logp = O.normal_log_prob(h[-1], 0.0, 1.0)[0].sum(-1)
    for i in range(L - 1):
        di = O._stoch_forward(pd, f"dec{i}", h[L - 1 - i])
        logp = logp + O.normal_log_prob(h[L - 2 - i], di["mu"], di["scale"])[0].sum(-1)
    return float(np.sum(a * ((logp + logpx) - logq)))


def loss_kwargs(loss, k, eps2=None):
    """The loss parameters the tests use: alpha 0.7, beta 0.5, and for PIWAE
    k1 = 1, k2 = k (every k factors so; the encoder then gets the VAE
    weighting and the decoder IWAE's: two different backward passes)."""
    if loss == "PIWAE":
        return {"k1": 1, "k2": k}
    if loss == "CIWAE":
        return {"beta": BETA, "eps2": eps2}
    if loss == "L_alpha":
        return {"alpha": ALPHA}
    return {}


def worst_tensor(spec, g, ref):
    """Largest error of a parameter tensor relative to the tensor's largest
    reference entry.  A tensor the loss gives no gradient (VAE_V1: the decoder's
    prior layers) must be exactly zero: 0 there, inf otherwise."""
    worst = 0.0
    for a, b in zip(R.split_tensors(spec, g), R.split_tensors(spec, ref)):
        err, scale = np.abs(a - b).max(), np.abs(b).max()
        worst = max(worst, err / scale if scale > 0 else (0.0 if err == 0 else np.inf))
    return float(worst)
