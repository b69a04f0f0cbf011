"""Float64 reference of the reweighted wake-sleep step (Bornschein & Bengio
2015; Le et al. 2019), built on the oracle's own functions
(oracle/iwae_oracle.py), plus the cases the CPU and GPU tests share.

The step reports three values and leaves one gradient:
  L_theta = -L_k, the IWAE loss; the decoder's parameters get its gradient;
  L_wake  = -(1/B) sum_b sum_s sm_bs log q(h_bs | x_b), sm = softmax_s(log w)
            and every h held constant;
  L_sleep = -(1/n) sum_j log q(h^j | x^j) over n dream pairs (constants);
the encoder's parameters get c_wake grad L_wake + c_sleep grad L_sleep.  The
latent an encoder layer reads is data: each layer is a weighted regression of
its own, no gradient flows from one layer into another.  A coefficient of
exactly 0 leaves its phase out: it is not evaluated and its value is 0."""
import numpy as np

import pathgrad_ref as PR
from oracle import iwae_oracle as O

X_DIM = PR.X_DIM
COEFS = ((1.0, 0.0), (0.0, 1.0), (0.5, 0.5))

# name: (encoder hidden, decoder hidden, encoder latent, decoder latent, B, k, n dreams, seed)
CASES = {
    "W1": ([16], [16], [6], [64], 3, 5, 7, 1911),                                # 15 rows, every width < 32, 7 dream rows
    "W2": ([40, 24], [24, 40], [10, 6], [10, 64], 7, 5, 19, 1922),               # ragged rows, an upper layer
    "W2w": ([40, 24], [24, 40], [10, 6], [10, 64], 33, 2, 33, 1933),             # > 32 wake and dream image rows
    "W3": ([40, 24, 16], [16, 24, 40], [12, 10, 6], [10, 12, 64], 4, 6, 5, 1944),   # a middle layer
    "W4": ([48, 32], [32, 48], [70, 5], [70, 64], 2, 9, 3, 1955),                # d = 70 > 64
}
# a second registry, filled by the modules that bring cases of their own (tests/step_shape_cases.py), of the same
# tuples with x_dim appended: case() finds them, CASES and every test parametrized over it stay as they are
EXTRA_CASES = {}


def enc_names(spec):
    return [n for n, _, _ in spec.dense if n.startswith("enc")]


def zeros_like_params(params, spec):
    return {n: [np.zeros_like(params[n][0]), np.zeros_like(params[n][1])] for n, _, _ in spec.dense}


def fit_layer(params, i, X, H, a, grads=None):
    """Encoder layer i as a weighted regression: returns sum_r a_r log q(H_r | X_r)
    per row ([...] like a) -- and, with grads, adds the gradient of
    -sum_r a_r log q(H_r | X_r) in the layer's parameters (X, H, a constants).
    X [B, fin] with H, a [k, B, ...] (layer 0 of the wake phase: the image is
    shared by its k rows), or X, H, a with the same leading dims."""
    q = O._stoch_forward(params, f"enc{i}", X)
    lp, z = O.normal_log_prob(H, q["mu"], q["scale"])
    if grads is not None:
        sc = q["scale"]
        dmu = -a[..., None] * (z / sc)
        dsc = -a[..., None] * ((z * z - 1) / sc)          # _stoch_backward chains ds/dzs = exp(zs) = s - 1e-6
        if X.ndim < H.ndim:
            dmu, dsc = dmu.sum(0), dsc.sum(0)
        O._stoch_backward(params, f"enc{i}", q, dmu, dsc, grads, False)
    return lp.sum(-1)


def wake_weights(lw):
    """sm / B, [k, B]: the wake rows' weights at c_wake = 1."""
    return O.bound_grad(lw, "IWAE")


def wake_value_and_grads(params, spec, x, h, a, grads=None):
    """L_wake of the constants (h, a = sm / B) as a plain function of the
    encoder's parameters; adds its gradient to grads."""
    val = x.dtype.type(0)
    for i in range(spec.L):
        X = x if i == 0 else h[i - 1]
        val = val - (a * fit_layer(params, i, X, h[i], a, grads)).sum()
    return val


def sleep_value_and_grads(params, spec, dreams, grads=None):
    """L_sleep of the dream pairs (x_d [n, x_dim], [h_1 .. h_L] each [n, d_i])."""
    xd, hd = dreams
    n = xd.shape[0]
    a = np.full(n, 1.0 / n, dtype=xd.dtype)
    val = xd.dtype.type(0)
    for i in range(spec.L):
        X = xd if i == 0 else hd[i - 1]
        val = val - (a * fit_layer(params, i, X, hd[i], a, grads)).sum()
    return val


def values_and_grads(params, spec, x, eps, dreams, c_wake, c_sleep):
    """((L_theta, L_wake, L_sleep), gradient dict of the step): the decoder's
    entries are the gradient of L_theta, the encoder's of
    c_wake L_wake + c_sleep L_sleep."""
    dt = x.dtype.type
    c = O.forward(params, spec, x, eps)
    lw = c["lw"]
    J = O.L_k_from_weights(lw)
    g_dec = O.backward(params, spec, c, O.bound_grad(lw, "IWAE"), want=("dec",))
    gw, gs = zeros_like_params(params, spec), zeros_like_params(params, spec)
    L_wake = L_sleep = dt(0)
    if c_wake != 0:
        L_wake = wake_value_and_grads(params, spec, x, c["h"], wake_weights(lw), gw)
    if c_sleep != 0:
        L_sleep = sleep_value_and_grads(params, spec, dreams, gs)
    out = {}
    for n, _, _ in spec.dense:
        if n.startswith("enc"):
            out[n] = [dt(c_wake) * gw[n][0] + dt(c_sleep) * gs[n][0], dt(c_wake) * gw[n][1] + dt(c_sleep) * gs[n][1]]
        else:
            out[n] = [-g_dec[n][0], -g_dec[n][1]]
    return (-J, L_wake, L_sleep), out


def train_step(params, spec, x, eps, dreams, c_wake, c_sleep, opt):
    """((L_theta, L_wake, L_sleep), new parameters, flat gradient), with the oracle's Adam."""
    vals, g = values_and_grads(params, spec, x, eps, dreams, c_wake, c_sleep)
    dt = x.dtype
    flat_g = O.flatten_params(spec, g).astype(dt)
    new_flat = opt.apply(O.flatten_params(spec, params).astype(dt), flat_g)
    return vals, O.unflatten_params(spec, new_flat, dtype=dt), flat_g


def make_dreams(spec, mean, n, rng):
    """Host-made dream pairs: binary x, h_i ~ 0.7 N(0, 1), rounded through
    float32.  They need not come from the model."""
    xd = (rng.random((n, spec.x_dim)) < mean).astype(np.float64)
    hd = [(0.7 * rng.standard_normal((n, d))).astype(np.float32).astype(np.float64) for d in spec.n_latent_encoder]
    return xd, hd


def make_case(arch, B, k, n, seed, x_dim=X_DIM):
    """(spec, params, mean, x, eps, dreams) of one case."""
    spec, params, mean, x, eps = PR.make_case(arch, B, k, seed, x_dim=x_dim)
    dreams = make_dreams(spec, mean, n, np.random.default_rng(seed + 50000))
    return spec, params, mean, x, eps, dreams


def case(name):
    if name in EXTRA_CASES:
        he, hd, le, ld, B, k, n, seed, x_dim = EXTRA_CASES[name]
        return (he, hd, le, ld), B, k, n, make_case((he, hd, le, ld), B, k, n, seed, x_dim=x_dim)
    he, hd, le, ld, B, k, n, seed = CASES[name]
    return (he, hd, le, ld), B, k, n, make_case((he, hd, le, ld), B, k, n, seed)


def cast_case(c, dtype):
    """A case's arrays in another float type (spec and mean as they are)."""
    spec, params, mean, x, eps, (xd, hd) = c
    return (spec, O.cast_params(params, dtype), mean, x.astype(dtype), [e.astype(dtype) for e in eps],
            (xd.astype(dtype), [v.astype(dtype) for v in hd]))
