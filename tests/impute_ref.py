"""Float64 reference of missing-pixel imputation (iwae_impute), built on
oracle.iwae_oracle.forward of the zero-imputed image x * mask: its cache gives
every sample's latents ``h``, pixel probabilities ``p``, ``logp`` and ``logq``;
the likelihood is recomputed over the observed pixels alone.

mask [B, x_dim]: non-zero = observed.  Image-major like posterior_ref."""
import numpy as np

import posterior_ref as R


def forward(params, spec, x, mask, eps):
    """The oracle forward of where(mask, x, 0) with ``lw`` (and ``logpx``)
    replaced by the masked ones.  Missing entries of x are selected away."""
    from oracle import iwae_oracle as O
    obs = np.asarray(mask) != 0
    xz = np.where(obs, np.asarray(x, np.float64), 0.0)
    c = O.forward(params, spec, xz, [np.asarray(e, np.float64) for e in eps])
    p, xb = c["p"], xz[None]
    c["logpx"] = ((np.log1p(-p) * (1 - xb) + np.log(p) * xb) * obs[None]).sum(-1)
    c["lw"] = (c["logp"] + c["logpx"]) - c["logq"]
    c["x"] = xz
    return c


def x_mean(x, mask, probs):
    """x where observed, the weighted probabilities where missing."""
    return np.where(np.asarray(mask) != 0, np.asarray(x, np.float64), probs)


def p_sir(idx, cache):
    """p(x | h_1) [B, x_dim] of sample idx[b] of image b."""
    return np.asarray(cache["p"], np.float64)[idx, np.arange(len(idx))]


def x_draw(x, mask, p_sel, u_pix):
    """x where observed, (u_pix < p) as 0.0 / 1.0 where missing."""
    return np.where(np.asarray(mask) != 0, np.asarray(x, np.float64),
                    (np.asarray(u_pix, np.float64) < p_sel).astype(np.float64))


def impute(params, spec, x, mask, eps, u=None, u_pix=None):
    """Everything iwae_impute returns, in float64."""
    c = forward(params, spec, x, mask, eps)
    w, logpx, ess = R.weights(c["lw"])
    h_mean, probs = R.combine(w, c)
    out = dict(cache=c, lw=c["lw"], weights=w, log_px=logpx, ess=ess, h_mean=h_mean, probs=probs,
               x_mean=x_mean(c["x"], mask, probs))
    if u is not None:
        out["sir_index"] = R.sir_index(w, np.asarray(u, np.float64))
        out["h_sir"] = R.sir_latents(out["sir_index"], c)
        if u_pix is not None:
            out["x_draw"] = x_draw(c["x"], mask, p_sir(out["sir_index"], c), u_pix)
    return out
