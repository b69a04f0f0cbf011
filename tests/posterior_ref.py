"""Float64 reference of the importance-weighted posterior (iwae_posterior),
built on oracle.iwae_oracle.forward, whose cache holds every sample's latents
``h`` ([k, B, d_i] per layer), pixel probabilities ``p`` ([k, B, x_dim]) and
log weights ``lw`` ([k, B]).

Everything here is image-major like the device outputs: weights are [B, k]."""
import numpy as np


def weights(lw):
    """lw [k, B] -> (w [B, k], logpx [B], ess [B]): w = softmax_k(lw),
    logpx = m + log sum e - log k, ess = (sum e)^2 / sum e^2."""
    lw = np.asarray(lw, np.float64)
    k = lw.shape[0]
    m = lw.max(axis=0)
    e = np.exp(lw - m)
    se = e.sum(axis=0)
    return (e / se).T.copy(), m + np.log(se) - np.log(k), se * se / (e * e).sum(axis=0)


def combine(w, cache):
    """Weighted means under ANY weights w [B, k]: (h_mean, probs) with
    h_mean[i] [B, d_i] = sum_s w[b, s] h_i[s, b] and probs [B, x_dim] likewise
    of p(x | h_1)."""
    w = np.asarray(w, np.float64)
    h_mean = [np.einsum("bs,sbd->bd", w, np.asarray(h, np.float64)) for h in cache["h"]]
    return h_mean, np.einsum("bs,sbd->bd", w, np.asarray(cache["p"], np.float64))


def combine_abs(w, cache):
    """sum_s w[b, s] |v_s|: the scale of combine()'s rounding error per element."""
    w = np.asarray(w, np.float64)
    return ([np.einsum("bs,sbd->bd", w, np.abs(h)) for h in cache["h"]],
            np.einsum("bs,sbd->bd", w, np.abs(cache["p"])))


def sir_index(w, u):
    """min{ j : sum_{s <= j} w[b, s] > u[b] }, clamped to k - 1; w [B, k], u [B]."""
    w = np.asarray(w, np.float64)
    c = np.cumsum(w, axis=1)
    idx = np.array([np.searchsorted(c[b], u[b], side="right") for b in range(w.shape[0])])
    return np.minimum(idx, w.shape[1] - 1)


def sir_latents(idx, cache):
    """The latents [B, d_i] per layer of sample idx[b] of image b."""
    b = np.arange(len(idx))
    return [np.asarray(h, np.float64)[idx, b] for h in cache["h"]]


def posterior(params, spec, x, eps, u=None):
    """Everything iwae_posterior returns, in float64, from one oracle forward."""
    from oracle import iwae_oracle as O
    c = O.forward(params, spec, np.asarray(x, np.float64), [np.asarray(e, np.float64) for e in eps])
    w, logpx, ess = weights(c["lw"])
    h_mean, probs = combine(w, c)
    out = dict(cache=c, lw=c["lw"], weights=w, log_px=logpx, ess=ess, h_mean=h_mean, probs=probs)
    if u is not None:
        out["sir_index"] = sir_index(w, np.asarray(u, np.float64))
        out["h_sir"] = sir_latents(out["sir_index"], c)
    return out
