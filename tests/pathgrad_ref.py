"""Float64 reference of the path-gradient estimators IWAE_STL (Roeder et al.
2017) and IWAE_DREG (Tucker et al. 2019), built on the oracle's own functions
(oracle/iwae_oracle.py), plus the cases the CPU and GPU tests share.

Both losses report -L_k and give the decoder the IWAE gradient.  The encoder's
gradient is that of sum(a_enc * log w) through the sampling path
h_i = mu_i + s_i eps_i only, with a_enc = softmax_k(lw) / B (STL) or its
square times B, softmax_k(lw)^2 / B (DReG), held constant."""
import numpy as np

from oracle import iwae_oracle as O

LOSSES = ("IWAE_STL", "IWAE_DREG")
X_DIM = 64

# name: (encoder hidden, decoder hidden, encoder latent, decoder latent, B, k, seed)
SHAPES = {
    "S1": ([16], [16], [6], [64], 3, 5, 911),
    "S2": ([40, 24], [24, 40], [10, 6], [10, 64], 5, 7, 922),
    "S2w": ([40, 24], [24, 40], [10, 6], [10, 64], 33, 2, 933),
    "S3": ([40, 24, 16], [16, 24, 40], [12, 10, 6], [10, 12, 64], 4, 9, 944),
    "S4": ([48, 32], [32, 48], [70, 5], [70, 64], 2, 17, 955),
}


def enc_weights(lw, loss):
    """a_enc [k, B]: the row weights of the encoder's path gradient."""
    sm = O.bound_grad(lw, "IWAE") * lw.shape[1]           # softmax over k
    if loss == "IWAE_STL":
        return sm / lw.shape[1]
    if loss == "IWAE_DREG":
        return sm * sm / lw.shape[1]
    raise ValueError(loss)


def path_enc_grads(params, spec, c, a, density=True):
    """Encoder gradients of sum(a * lw) through the sampling path only.
    c = O.forward(...), a = a_enc [k, B].  density=False drops the chain that
    carries the density partials of q(h_i | h_{i-1}) down to h_{i-1} (wrong on
    purpose: the tests use it to show their inputs tell the two apart).
    Only the encoder entries of the result are meaningful."""
    L = spec.L
    x = c["x"][None]
    h, eps = c["h"], c["eps"]

    def zeros():
        return {n: [np.zeros_like(params[n][0]), np.zeros_like(params[n][1])] for n, _, _ in spec.dense}
    grads, junk = zeros(), zeros()
    dh = [np.zeros_like(v) for v in h]
    s, p = c["s"], c["p"]
    dlogit = a[..., None] * (x / p - (1 - x) / (1 - p)) * x.dtype.type(O.PROB_SCALE) * (s * (1 - s))
    W1, W2, W3 = params["out.l1"][0], params["out.l2"][0], params["out.l3"][0]
    do1 = ((dlogit @ W3.T) * (1 - c["o2"] ** 2)) @ W2.T
    dh[0] += (do1 * (1 - c["o1"] ** 2)) @ W1.T
    dlp = a[..., None]
    dh[L - 1] += dlp * (-h[L - 1])
    for i in range(L - 1):
        di = c["dec"][i]
        t, src = L - 2 - i, L - 1 - i
        z, sc = di["z"], di["scale"]
        dh[t] += dlp * (-z / sc)
        dh[src] += O._stoch_backward(params, f"dec{i}", di, dlp * (z / sc), dlp * ((z * z - 1) / sc), junk, True)
    dlq = -a[..., None]
    for i in reversed(range(L)):
        qi = c["enc"][i]
        z, sc = qi["z"], qi["scale"]
        dht = dh[i] + dlq * (-z / sc)
        if i == 0:
            O._stoch_backward(params, "enc0", qi, dht.sum(0), (dht * eps[0]).sum(0), grads, False)
        else:
            dXp = O._stoch_backward(params, f"enc{i}", qi, dht, dht * eps[i], grads, True)
            dh[i - 1] += dXp
            if density:
                dh[i - 1] += O._stoch_backward(params, f"enc{i}", qi, dlq * (z / sc), dlq * ((z * z - 1) / sc),
                                               junk, True)
    return grads


def objective_and_grads(params, spec, x, eps, loss, density=True):
    """(J = L_k, gradients of the estimator's surrogate objective), the
    counterpart of O.objective_and_grads for the two path-gradient losses."""
    c = O.forward(params, spec, x, eps)
    lw = c["lw"]
    J = O.L_k_from_weights(lw)
    g_dec = O.backward(params, spec, c, O.bound_grad(lw, "IWAE"), want=("dec",))
    g_enc = path_enc_grads(params, spec, c, enc_weights(lw, loss), density)
    out = {}
    for n, _, _ in spec.dense:
        out[n] = g_enc[n] if n.startswith("enc") else g_dec[n]
    return J, out


def train_step(params, spec, x, eps, loss, opt, density=True):
    """(loss = -J, new parameters, flat gradient of the loss): O.train_step's contract."""
    J, gJ = objective_and_grads(params, spec, x, eps, loss, density)
    dt = x.dtype
    flat_g = -O.flatten_params(spec, gJ).astype(dt)
    new_flat = opt.apply(O.flatten_params(spec, params).astype(dt), flat_g)
    return -J, O.unflatten_params(spec, new_flat, dtype=dt), flat_g


def surrogate(ps, pd, spec, x, eps, a):
    """sum(a * lw) with the encoder's SAMPLING run on the parameters ps and
    every density (log q, log p, log p(x|h)) on pd: its gradient in ps at
    ps = pd is the path gradient (a constant)."""
    L = spec.L
    X, h, logq = x, [], 0.0
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
    xb = x[None]
    logpx = (np.log1p(-p) * (1 - xb) + np.log(p) * xb).sum(-1)
    logp = O.normal_log_prob(h[-1], 0.0, 1.0)[0].sum(-1)
    for i in range(L - 1):
        di = O._stoch_forward(pd, f"dec{i}", h[L - 1 - i])
        logp = logp + O.normal_log_prob(h[L - 2 - i], di["mu"], di["scale"])[0].sum(-1)
    return float(np.sum(a * ((logp + logpx) - logq)))


def make_case(arch, B, k, seed, x_dim=X_DIM):
    """Oracle-side inputs of one case, parameters and noise rounded through
    float32 (tests/test_gpu_configs.py::_case at another x_dim)."""
    he, hd, le, ld = arch
    rng = np.random.default_rng(seed)
    mean = rng.uniform(0.01, 0.4, x_dim)
    spec = O.ModelSpec(he, hd, le, ld, x_dim=x_dim)
    params = O.glorot_init(spec, rng, out_bias=O.output_bias_from_mean(mean))
    params = {n: [w.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64)]
              for n, (w, b) in params.items()}
    x = (rng.random((B, x_dim)) < mean).astype(np.float64)
    eps = [e.astype(np.float32).astype(np.float64) for e in O.draw_eps(spec, k, B, rng)]
    return spec, params, mean, x, eps


def shape_case(name):
    he, hd, le, ld, B, k, seed = SHAPES[name]
    return (he, hd, le, ld), B, k, make_case((he, hd, le, ld), B, k, seed)


def split_tensors(spec, flat):
    """The flat parameter-order vector as its tensors (kernel, bias per Dense)."""
    out, o = [], 0
    for shp in spec.param_shapes():
        n = int(np.prod(shp))
        out.append(flat[o:o + n])
        o += n
    assert o == flat.size
    return out


def enc_size(spec):
    return sum(fin * fout + fout for n, fin, fout in spec.dense if n.startswith("enc"))


def rel_l2(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-30))
