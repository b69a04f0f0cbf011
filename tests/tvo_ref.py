"""Float64 reference of the thermodynamic variational objective (TVO; Masrani,
Le & Wood 2019) and of the step that descends it, built on the oracle's own
functions (oracle/iwae_oracle.py) and the wake-sleep reference's weighted
regression (tests/wakesleep_ref.py), plus the cases and partitions the CPU and
GPU tests share.

For one image with log weights lw_s, s < k, and a partition
0 = beta_0 < ... < beta_J = 1 with D_j = beta_{j+1} - beta_j:
  wn^(j)_s = softmax_s(beta_j lw_s),          m_j = sum_s wn^(j)_s lw_s,
  lower = sum_{j<J} D_j m_j,                  upper = sum_{j<J} D_j m_{j+1},
  iwae  = logsumexp_s lw_s - log k,
  a_theta_s = sum_{j<J} D_j wn^(j)_s [1 + beta_j (lw_s - m_j)],
  a_phi_s   = sum_{j<J} D_j wn^(j)_s [(1 - beta_j) (lw_s - m_j) - 1].
The step descends L_tvo = -(1/B) sum_b lower_b at fixed samples: the decoder
takes -(1/B) sum a_theta grad [log p(h) + log p(x | h_1)], every encoder layer
the gradient of -(1/B) sum a_phi log q(h | x) with a_phi and h constants."""
import numpy as np

import pathgrad_ref as PR
import wakesleep_ref as W
from oracle import iwae_oracle as O

X_DIM = W.X_DIM


def schedule(n_part, beta1=0.025):
    """beta_0 = 0, beta_1 .. beta_J log-uniform from beta1 to 1, as float32 values."""
    b = np.zeros(n_part + 1, dtype=np.float32)
    b[1:] = np.logspace(np.log10(beta1), 0.0, n_part) if n_part > 1 else 1.0
    b[-1] = 1.0
    return b


PARTS = {
    "P1": np.array([0.0, 1.0], dtype=np.float32),
    "P2": np.array([0.0, 0.3, 1.0], dtype=np.float32),
    "P5": schedule(5),
    "P64": np.linspace(0.0, 1.0, 65).astype(np.float32),
}

# name: (encoder hidden, decoder hidden, encoder latent, decoder latent, B, k, seed)
CASES = {
    "T1": ([16], [16], [6], [X_DIM], 3, 5, 2011),                                 # 15 rows, a partial tile
    "T2": ([40, 24], [24, 40], [10, 6], [10, X_DIM], 7, 5, 2022),                 # ragged rows, an upper layer
    "T2w": ([40, 24], [24, 40], [10, 6], [10, X_DIM], 33, 2, 2033),               # first layer beyond the few-row launches
    "T3": ([40, 24, 16], [16, 24, 40], [12, 10, 6], [10, 12, X_DIM], 4, 6, 2044),   # a middle layer
    "T4": ([48, 32], [32, 48], [70, 5], [70, X_DIM], 2, 9, 2055),                 # d = 70 > 64
    "Tk1": ([40, 24], [24, 40], [10, 6], [10, X_DIM], 7, 1, 2066),                # k = 1
}
# the partitions each case runs on (GPU parity and the float32 fairness check)
CASE_PARTS = [(c, p) for c in CASES for p in ("P1", "P5")] + [("T2", "P2"), ("T2", "P64")]

# T1's model at B = 65, k = 127 (8255 rows): the smallest batch beyond bound_grid's one-workgroup rule
# (B > 64 and B k > 8192), where the last workgroup to arrive sums the batch values; run on P5
MULTI = (CASES["T1"][:4], 65, 127, 2077)


def multi_case():
    arch, B, k, seed = MULTI
    return arch, B, k, PR.make_case(tuple(arch), B, k, seed)


def tvo_terms(lw, betas):
    """lw [k, ...] (sample axis first), betas [J + 1]: dict of lower, upper,
    iwae [...] and a_theta, a_phi [k, ...], in lw's float type."""
    dt = lw.dtype
    b = np.asarray(betas).astype(dt)
    k = lw.shape[0]
    mx = lw.max(axis=0, keepdims=True)
    d = lw - mx
    J = b.size - 1
    wn, m = [], []
    for j in range(J + 1):
        e = np.exp(b[j] * d)
        w = e / e.sum(axis=0, keepdims=True)
        wn.append(w)
        m.append((w * lw).sum(axis=0))
    lower = sum((b[j + 1] - b[j]) * m[j] for j in range(J))
    upper = sum((b[j + 1] - b[j]) * m[j + 1] for j in range(J))
    iwae = np.log(np.exp(d).sum(axis=0) / dt.type(k)) + mx[0]
    a_theta = sum((b[j + 1] - b[j]) * wn[j] * (1 + b[j] * (lw - m[j])) for j in range(J))
    a_phi = sum((b[j + 1] - b[j]) * wn[j] * ((1 - b[j]) * (lw - m[j]) - 1) for j in range(J))
    return dict(lower=lower, upper=upper, iwae=iwae, a_theta=a_theta, a_phi=a_phi)


def decoder_grads(params, spec, c, a):
    """Gradient of -sum_bs a_bs [log p(h_bs) + log p(x_b | h_1,bs)] in the decoder's
    parameters at the forward cache's fixed latents (a [k, B]); zero elsewhere."""
    g = O.backward(params, spec, c, a, want=("dec",))
    return {n: [-g[n][0], -g[n][1]] for n, _, _ in spec.dense}


def encoder_value_and_grads(params, spec, x, h, a, grads=None):
    """The encoder's surrogate -sum_bs a_bs log q(h_bs | x_b) of the constants
    (h, a), a plain function of the encoder's parameters; adds its gradient to
    grads.  (The wake phase's regression, with weights of either sign.)"""
    return W.wake_value_and_grads(params, spec, x, h, a, grads)


def values_and_grads(params, spec, x, eps, betas):
    """((L_tvo, L_upper, L_iwae), gradient dict of the step)."""
    c = O.forward(params, spec, x, eps)
    B = x.shape[0]
    t = tvo_terms(c["lw"], betas)
    dt = x.dtype.type
    out = decoder_grads(params, spec, c, t["a_theta"] / dt(B))
    ge = W.zeros_like_params(params, spec)
    encoder_value_and_grads(params, spec, x, c["h"], t["a_phi"] / dt(B), ge)
    for n, _, _ in spec.dense:
        if n.startswith("enc"):
            out[n] = ge[n]
    return (-t["lower"].mean(), -t["upper"].mean(), -t["iwae"].mean()), out


def train_step(params, spec, x, eps, betas, opt):
    """((L_tvo, L_upper, L_iwae), new parameters, flat gradient), with the oracle's Adam."""
    vals, g = values_and_grads(params, spec, x, eps, betas)
    dt = x.dtype
    flat_g = O.flatten_params(spec, g).astype(dt)
    new_flat = opt.apply(O.flatten_params(spec, params).astype(dt), flat_g)
    return vals, O.unflatten_params(spec, new_flat, dtype=dt), flat_g


def case(name):
    """((he, hd, le, ld), B, k, (spec, params, mean, x, eps))."""
    he, hd, le, ld, B, k, seed = CASES[name]
    return (he, hd, le, ld), B, k, PR.make_case((he, hd, le, ld), B, k, seed)


def cast_case(c, dtype):
    spec, params, mean, x, eps = c
    return spec, O.cast_params(params, dtype), mean, x.astype(dtype), [e.astype(dtype) for e in eps]
