"""Float64 reference of the pixel-masked scoring family (iwae_score_masked,
iwae_score_grad_masked, iwae_ais_masked, iwae_refine_masked and the facade's
hmc_observed), on the oracle's functions as score_ref.py, scoregrad_ref.py,
ais_ref.py and refine_ref.py are, with the cases the CPU and GPU tests share.

mask [B, x_dim]: non-zero = observed.  The model is missing_ref.py's and
impute_ref.py's:
  the encoder sees where(mask, x, 0), so log q is log q(h | x (.) mask);
  log p(x|h_1) = sum_j [mask_bj != 0] log Bern(x_bj | p_j(h_1));
  dlogit of a missing pixel is 0;  log p(h) does not change.
Missing entries of x are selected away, never multiplied: the cases' x holds
NaN there.  Every function keeps its original's dtype= / dense= hooks, and with
an all-ones mask runs its original's lines on its original's operands
(tests/test_observed_ref.py asserts the equality, exactly)."""
import functools

import numpy as np

from oracle import iwae_oracle as O
import ais_ref as A
import missing_ref as M
import pathgrad_ref as PR
import refine_ref as RF
import score_ref as R
import scoregrad_ref as G

LATENTS = R.LATENTS
_S2 = R.CASES["S2"]
O50_ARCH = (_S2[0][0], _S2[0][1], _S2[0][2], _S2[0][3][:-1] + [50])

# name: (base case of score_ref or None, architecture, B, k, seed, x_dim, grey).  The base's parameters,
# images and noise are the case's own; the mask is missing_ref.make_mask(B, x_dim, seed + 2): image 0
# entirely missing, image 1 entirely observed, Bernoulli(0.5) elsewhere.
CASES = {"O" + b: (b,) + tuple(R.CASES[b][:5]) + (False,) for b in ("S1", "S2", "S3", "K130", "C784")}
# x_dim % 4 != 0: the staged copies' padding columns
CASES["O50"] = (None, O50_ARCH, _S2[1], _S2[2], 9250, 50, False)
# grey-level observed pixels in (0, 1) on the odd images: the two-log branch beside a binarised neighbour
CASES["OG"] = ("S2",) + tuple(_S2[:5]) + (True,)


# a second registry of the same tuples (tests/latent_shape_cases.py); CASES and its tests stay as they are
EXTRA_CASES = {}


def entry(name):
    return CASES[name] if name in CASES else EXTRA_CASES[name]


def observed(x, mask, dtype=np.float64):
    """where(mask, x, 0): what the encoder sees (the holes selected away)."""
    return np.where(np.asarray(mask) != 0, np.asarray(x, dtype=dtype), np.dtype(dtype).type(0))


@functools.lru_cache(maxsize=None)
def case(name):
    """(spec, params, x, mask, eps, x_full): x holds NaN at the holes, x_full the complete images."""
    base, arch, B, k, seed, x_dim, grey = entry(name)
    if base is not None:
        spec, params, x_full, eps = R.case(base)
    else:
        spec, params, _, x_full, eps = PR.make_case(arch, B, k, seed, x_dim=x_dim)
    if grey:
        rng = np.random.default_rng(seed + 3)
        x_full = np.array(x_full)
        x_full[1::2] = R.f32r(rng.uniform(0.05, 0.95, x_full[1::2].shape))
    mask = M.make_mask(B, x_dim, seed + 2)
    x = M.with_holes(x_full, mask)
    for v in (x, mask, x_full):
        v.setflags(write=False)
    return spec, params, x, mask, eps, x_full


def arch(name):
    return entry(name)[1]


@functools.lru_cache(maxsize=None)
def latents(name, which, rounded=True):
    """score_ref.latents for the masked model: "on" are the encoder's samples at where(mask, x, 0)."""
    spec, params, x, mask, eps, _ = case(name)
    _, _, B, k, seed, _, _ = entry(name)
    L = spec.L
    if which == "on":
        h = O.forward(params, spec, observed(x, mask), eps)["h"]
    elif which == "off":
        rng = np.random.default_rng(seed + 1)
        h = [1.5 * rng.standard_normal((k, B, d)) for d in spec.n_latent_encoder]
    elif which == "prior":
        rng = np.random.default_rng(seed + 2)
        h = [None] * L
        h[L - 1] = rng.standard_normal((k, B, spec.n_latent_encoder[L - 1]))
        for j in range(L - 1):
            di = O._stoch_forward(params, f"dec{j}", h[L - 1 - j])
            h[L - 2 - j] = rng.standard_normal(di["mu"].shape) * di["scale"] + di["mu"]
    else:
        raise ValueError(which)
    return [R.f32r(v) for v in h] if rounded else list(h)


# ------------------------------------------------------------------- score
def score(params, spec, x, mask, h, dtype=np.float64, dense=None, split_targets=False):
    """score_ref.score of the masked model: logq at where(mask, x, 0), logp and
    probs (every pixel's) as they are, logpx / Spx over the observed addends."""
    obs = np.asarray(mask) != 0
    xz = observed(x, mask, dtype)
    out = R.score(params, spec, xz, h, dtype=dtype, dense=dense, split_targets=split_targets)
    p, xb = out["probs"], xz[None]
    terms = np.log1p(-p) * (1 - xb) + np.log(p) * xb             # F:127-F:128
    terms = np.where(obs[None], terms, np.dtype(dtype).type(0))
    out["logpx"], out["Spx"] = terms.sum(-1), np.abs(terms).sum(-1)
    return out


@functools.lru_cache(maxsize=None)
def reference(name, which):
    """The float64 reference of a case's latent set: computed once, shared, read-only."""
    spec, params, x, mask, _, _ = case(name)
    out = score(params, spec, x, mask, latents(name, which))
    for v in out.values():
        v.setflags(write=False)
    return out


# --------------------------------------------------------------- gradients
def grads(params, spec, x, mask, h, dtype=np.float64, dense=None):
    """scoregrad_ref.grads of the masked model: the q and ph terms at where(mask,
    x, 0), the px term with the dlogit of a missing pixel selected to 0."""
    obs = np.asarray(mask) != 0
    xz = observed(x, mask, dtype)
    out = G.grads(params, spec, xz, h, dtype=dtype, dense=dense)
    dt = np.dtype(dtype).type
    params = O.cast_params(params, dtype)
    h = [np.asarray(v, dtype=dtype) for v in h]
    k = h[0].shape[0]
    gx = [np.zeros_like(v) for v in h]
    W1, b1 = params["out.l1"]; W2, b2 = params["out.l2"]; W3, b3 = params["out.l3"]
    if dense is None:
        y1 = np.tanh(h[0] @ W1 + b1); y2 = np.tanh(y1 @ W2 + b2); logit = y2 @ W3 + b3
    else:
        y1 = np.tanh(dense(h[0], W1, b1)); y2 = np.tanh(dense(y1, W2, b2)); logit = dense(y2, W3, b3)
    sg = 1.0 / (1.0 + np.exp(-logit))
    p = sg * dt(O.PROB_SCALE) + dt(O.PROB_SHIFT)
    xb = np.broadcast_to(xz[None], (k,) + xz.shape)
    dlogit = (xb / p - (1 - xb) / (1 - p)) * dt(O.PROB_SCALE) * (sg * (1 - sg))
    dlogit = np.where(obs[None], dlogit, dt(0))
    dY2 = G._mm(dlogit, W3.T, dense) * (1 - y2 * y2)
    dY1 = G._mm(dY2, W2.T, dense) * (1 - y1 * y1)
    gx[0] = gx[0] + G._mm(dY1, W1.T, dense)
    out["px"] = gx
    return out


@functools.lru_cache(maxsize=None)
def grad_reference(name, which):
    spec, params, x, mask, _, _ = case(name)
    out = grads(params, spec, x, mask, latents(name, which))
    for t in out.values():
        for v in t:
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def grad_emulated(name, which):
    spec, params, x, mask, _, _ = case(name)
    return grads(params, spec, x, mask, latents(name, which), dtype=np.float32, dense=R.dense_bf16x3)


# ------------------------------------------------------------------------ HMC
def log_joint(params, spec, x, mask, h, **kw):
    s = score(params, spec, x, mask, h, **kw)
    return np.asarray(s["logp"], np.float64) + np.asarray(s["logpx"], np.float64)


def hmc_step(params, spec, x, mask, h, r, step, n_leapfrog, **kw):
    """scoregrad_ref.hmc_step under log p(x_obs, h): (proposal, H_old, H_new)."""
    def g(hs):
        t = grads(params, spec, x, mask, hs, **kw)
        return [np.asarray(a, np.float64) + np.asarray(b, np.float64) for a, b in zip(t["ph"], t["px"])]
    q = [np.array(v, np.float64) for v in h]
    r = [np.array(v, np.float64) for v in r]
    H_old = -log_joint(params, spec, x, mask, q, **kw) + 0.5 * sum((v * v).sum(-1) for v in r)
    gr = g(q)
    for _ in range(n_leapfrog):
        r = [a + 0.5 * step * b for a, b in zip(r, gr)]
        q = [a + step * b for a, b in zip(q, r)]
        gr = g(q)
        r = [a + 0.5 * step * b for a, b in zip(r, gr)]
    H_new = -log_joint(params, spec, x, mask, q, **kw) + 0.5 * sum((v * v).sum(-1) for v in r)
    return q, H_old, H_new


HMC_STEPS = (0.3, 0.26, 0.22)
HMC_SEEDS = tuple(range(4101, 4161))
HMC_LEAPFROG = 4
# name: (step size, leapfrog steps, momentum seed): the first of HMC_STEPS x HMC_SEEDS (steps outer) at which
# the float64 trajectory has |dH| < 5 on every chain and scoregrad_ref.hmc_case's rule for log u (accepted by
# 0.4 nats on even chains, rejected by 0.4 on odd ones whose dH allows u < 1) accepts some chains and rejects
# at least two (hmc_search(); tests/test_observed_ref.py re-checks)
HMC_CASES = {"OS2": (0.3, 4, 4122)}


def _hmc_run(name, step, nl, seed):
    spec, params, x, mask, _, _ = case(name)
    h = latents(name, "on")
    rng = np.random.default_rng(seed)
    r = [R.f32r(rng.standard_normal(v.shape)) for v in h]
    q, H0, H1 = hmc_step(params, spec, x, mask, h, r, step, nl)
    dH = H1 - H0
    k, B = dH.shape
    chain = np.arange(k * B).reshape(k, B)
    lu = -dH - 0.4
    rej = (chain % 2 == 1) & (-dH + 0.4 < 0)
    lu = np.where(rej, -dH + 0.4, lu)
    return r, q, H0, H1, lu, lu < -dH


def hmc_conditions(out):
    """(max |dH|, accepted chains, rejected chains, smallest margin |log u + dH|)."""
    _, _, H0, H1, lu, acc = out
    dH = H1 - H0
    return float(np.abs(dH).max()), int(acc.sum()), int((~acc).sum()), float(np.abs(lu + dH).min())


def hmc_search(name):
    for step in HMC_STEPS:
        for seed in HMC_SEEDS:
            big, na, nr, _ = hmc_conditions(_hmc_run(name, step, HMC_LEAPFROG, seed))
            if big < 5.0 and na >= 1 and nr >= 2:
                return step, HMC_LEAPFROG, seed
    return None


@functools.lru_cache(maxsize=None)
def hmc_case(name):
    """(momenta, proposal, H_old, H_new, log u, accept) of the case's "on" latents."""
    return _hmc_run(name, *HMC_CASES[name])


# ------------------------------------------------------------------------ AIS
def _state(params, spec, x, mask, h, init, coef, kw):
    """ais_ref._state of the masked model: (U, Delta, g) at h under coef."""
    sc = score(params, spec, x, mask, h, **kw)
    val = {"q": np.asarray(sc["logq"], np.float64), "ph": np.asarray(sc["logp"], np.float64),
           "px": np.asarray(sc["logpx"], np.float64)}
    gt = grads(params, spec, x, mask, h, **kw)
    U = 0.0
    g = [np.zeros(v.shape) for v in h]
    for c, t in zip(coef, G.TERMS):
        if c == 0.0:
            continue
        U = U - c * val[t]
        g = [a + c * np.asarray(b, np.float64) for a, b in zip(g, gt[t])]
    delta = val["px"] if init == "prior" else (val["ph"] + val["px"]) - val["q"]
    return U, delta, g


def ais_run(params, spec, x, mask, h0, betas, init, step, n_leapfrog, adapt, momenta, log_u, log_w0=None,
            accepts0=None, **kw):
    """ais_ref.run of the masked model (its arguments, its dict)."""
    h = [np.array(v, np.float64) for v in h0]
    k, B = h[0].shape[:2]
    T = len(betas) - 1
    inc, dec, smin, smax = (np.float32(v) for v in adapt)
    eps = np.broadcast_to(np.asarray(step, np.float32), (k, B)).copy()
    log_w = np.zeros((k, B)) if log_w0 is None else np.array(log_w0, np.float64)
    accepts = np.zeros((k, B)) if accepts0 is None else np.array(accepts0, np.float64)
    dHs, accs, lus = [], [], []
    for t in range(1, T + 1):
        beta = float(betas[t])
        coef = A.coefs(init, beta)
        U_old, delta, g = _state(params, spec, x, mask, h, init, coef, kw)
        log_w = log_w + (float(betas[t]) - float(betas[t - 1])) * delta
        r = [np.array(v, np.float64) for v in momenta[t - 1]]
        H_old = U_old + 0.5 * sum((v * v).sum(-1) for v in r)
        e = eps.astype(np.float64)[..., None]
        r = [a + 0.5 * e * b for a, b in zip(r, g)]
        q = [a + e * b for a, b in zip(h, r)]
        for l in range(1, n_leapfrog + 1):
            U_new, _, g = _state(params, spec, x, mask, q, init, coef, kw)
            if l < n_leapfrog:
                r = [a + e * b for a, b in zip(r, g)]
                q = [a + e * b for a, b in zip(q, r)]
            else:
                r = [a + 0.5 * e * b for a, b in zip(r, g)]
        H_new = U_new + 0.5 * sum((v * v).sum(-1) for v in r)
        dH = H_new - H_old
        lu = log_u(t, dH) if callable(log_u) else np.asarray(log_u[t - 1], np.float64)
        acc = lu < -dH
        h = [np.where(acc[..., None], a, b) for a, b in zip(q, h)]
        accepts = accepts + acc
        eps = np.clip(eps * np.where(acc, inc, dec).astype(np.float32), smin, smax).astype(np.float32)
        dHs.append(dH); accs.append(acc); lus.append(lu)
    logpx, ess = A.finish(log_w)
    return dict(h=h, log_w=log_w, accepts=accepts, step=eps, dH=np.array(dHs), accept=np.array(accs),
                log_u=np.array(lus), logpx=logpx, ess=ess)


# (case, init): (step, momentum seed): the first of ais_ref's STEPS x SEEDS (steps outer) at which the float64
# run on ais_ref's BETAS, N_LEAPFROG and ADAPT meets ais_ref's conditions: |dH| < 5 on every chain and
# transition, rejections in at least two transitions (ais_search(); tests/test_observed_ref.py re-checks);
# log u is ais_ref.log_u_rule's: no decision within 0.4 nats of its margin
AIS_CASES = {("OS2", "q"): (0.2, 5006), ("OC784", "prior"): (0.5, 5001)}


def momenta_of(name, seed, T):
    h = latents(name, "on")
    rng = np.random.default_rng(seed)
    return [[R.f32r(rng.standard_normal(v.shape)) for v in h] for _ in range(T)]


def _ais_case(name, init, step, seed, **kw):
    spec, params, x, mask, _, _ = case(name)
    mom = momenta_of(name, seed, len(A.BETAS) - 1)
    out = ais_run(params, spec, x, mask, latents(name, A.START[init]), A.BETAS, init, step, A.N_LEAPFROG, A.ADAPT, mom,
                  kw.pop("log_u", A.log_u_rule), **kw)
    out["momenta"] = mom
    return out


def ais_search(name, init):
    for step in A.STEPS:
        for seed in A.SEEDS:
            big, nrej = A.conditions(_ais_case(name, init, step, seed))
            if big < 5.0 and nrej >= 2:
                return step, seed
    return None


@functools.lru_cache(maxsize=None)
def ais_case(name, init):
    """The float64 run of a case (ais_run's dict plus "momenta"): computed once, shared, read-only."""
    out = _ais_case(name, init, *AIS_CASES[name, init])
    for v in out.values():
        RF._freeze(v)
    return out


@functools.lru_cache(maxsize=None)
def ais_emulated(name, init):
    """The same momenta and log u through the float32 + bf16x3 emulation of the densities and gradients."""
    return _ais_case(name, init, *AIS_CASES[name, init], log_u=ais_case(name, init)["log_u"], dtype=np.float32,
                     dense=R.dense_bf16x3)


# --------------------------------------------------------------- refinement
def refine_weights(params, spec, x, mask, mean, logstd, eps, rounded=True, **kw):
    """refine_ref.weights of the masked model: (h, log_w [k, B]) of one pass."""
    h = RF.sample(mean, logstd, eps, rounded)
    sc = score(params, spec, x, mask, h, **kw)
    return h, (np.asarray(sc["logp"], np.float64) + np.asarray(sc["logpx"], np.float64)) - RF.log_q(eps, logstd)


def refine_objective_and_grads(params, spec, x, mask, mean, logstd, eps, objective, rounded=True, **kw):
    """refine_ref.objective_and_grads of the masked model: (value [B], G^m, G^ls)."""
    h, lw = refine_weights(params, spec, x, mask, mean, logstd, eps, rounded, **kw)
    k = lw.shape[0]
    if objective == "ELBO":
        a = np.full(lw.shape, 1.0 / k)
    else:
        e = np.exp(lw - lw.max(0))
        a = e / e.sum(0)
    gt = grads(params, spec, x, mask, h, **kw)
    g = [np.asarray(p, np.float64) + np.asarray(q, np.float64) for p, q in zip(gt["ph"], gt["px"])]
    Gm = [(a[..., None] * v).sum(0) for v in g]
    Gl = [(a[..., None] * v * np.asarray(e, np.float64)).sum(0) * np.exp(np.asarray(ls, np.float64)) + 1.0
          for v, e, ls in zip(g, eps, logstd)]
    return RF.value(lw, objective), Gm, Gl


def refine_run(params, spec, x, mask, mean0, logstd0, eps, objective, n_iters, lr=RF.LR, betas=RF.BETAS,
               epsilon=RF.EPS_HAT, ls_range=RF.LS_RANGE, evaluate=True, step0=0, adam0=None, state_dtype=np.float64, **kw):
    """refine_ref.run of the masked model (its arguments; its dict without the gradient scales)."""
    sd = np.dtype(state_dtype).type
    L = len(mean0)
    mean = [np.array(v, state_dtype) for v in mean0]
    logstd = [np.array(v, state_dtype) for v in logstd0]
    if adam0 is None or step0 == 0:
        adam = [np.zeros(mean[i // 4].shape, state_dtype) for i in range(4 * L)]
    else:
        adam = [np.array(v, state_dtype) for v in adam0]
    b1, b2 = (float(np.float32(b)) for b in betas)
    omb1, omb2, eh = sd(np.float32(1) - np.float32(b1)), sd(np.float32(1) - np.float32(b2)), sd(np.float32(epsilon))
    lo, hi = sd(np.float32(ls_range[0])), sd(np.float32(ls_range[1]))
    bound, gr = [], []
    for t in range(n_iters):
        val, Gm, Gl = refine_objective_and_grads(params, spec, x, mask, mean, logstd, eps[t], objective, **kw)
        bound.append(val)
        gr.append((Gm, Gl))
        n = step0 + t + 1
        lr_n = sd(np.float32(float(np.float32(lr)) * np.sqrt(1.0 - b2 ** n) / (1.0 - b1 ** n)))
        for i in range(L):
            for p, g, j in ((mean, Gm[i], 0), (logstd, Gl[i], 2)):
                g = g.astype(state_dtype)
                m1 = adam[4 * i + j] = adam[4 * i + j] + (g - adam[4 * i + j]) * omb1
                m2 = adam[4 * i + j + 1] = adam[4 * i + j + 1] + (g * g - adam[4 * i + j + 1]) * omb2
                p[i] = p[i] + (m1 * lr_n) / (np.sqrt(m2) + eh)
            logstd[i] = np.clip(logstd[i], lo, hi)
    out = dict(mean=mean, logstd=logstd, adam=adam, bound=np.array(bound).reshape(n_iters, -1), grads=gr)
    if evaluate:
        h, lw = refine_weights(params, spec, x, mask, mean, logstd, eps[n_iters], **kw)
        lp, ess = A.finish(lw)
        out.update(h=h, log_w=lw, logpx=lp, ess=ess)
    return out


@functools.lru_cache(maxsize=None)
def refine_setting(name, seed=RF.SEED, passes=RF.T + 1):
    """refine_ref.setting on the case's "on" latents: (means, logstds, eps)."""
    spec = case(name)[0]
    _, _, B, k = entry(name)[:4]
    means = [R.f32r(np.asarray(v).mean(0)) for v in latents(name, "on")]
    logstds = [np.full(v.shape, RF.LS0) for v in means]
    rng = np.random.default_rng(seed)
    eps = [[R.f32r(rng.standard_normal((k, B, d))) for d in spec.n_latent_encoder] for _ in range(passes)]
    for v in means + logstds + [e for p in eps for e in p]:
        v.setflags(write=False)
    return means, logstds, eps


@functools.lru_cache(maxsize=None)
def refine_case(name, objective, n_iters=RF.T):
    """The float64 run of a case in refine_ref's fixed setting: computed once, shared, read-only."""
    spec, params, x, mask, _, _ = case(name)
    m0, s0, eps = refine_setting(name)
    out = refine_run(params, spec, x, mask, m0, s0, eps[:n_iters] + eps[RF.T:], objective, n_iters)
    for v in out.values():
        RF._freeze(v)
    return out


@functools.lru_cache(maxsize=None)
def refine_emulated(name, objective):
    """The same run through the float32 + bf16x3 emulation, parameters and moments in float32."""
    spec, params, x, mask, _, _ = case(name)
    m0, s0, eps = refine_setting(name)
    return refine_run(params, spec, x, mask, m0, s0, eps, objective, RF.T, state_dtype=np.float32, dtype=np.float32,
                      dense=R.dense_bf16x3)
