"""Float64 reference of per-image variational refinement (iwae_refine), on
score_ref.score and scoregrad_ref.grads, with the cases and the fixed setting
the CPU and GPU tests share.

q*(h) = prod_i N(h_i; m_i, exp(ls_i)^2) per image; per pass and row (s, b):
  h_i    = float32(exp(ls_i) eps_i + m_i)          (the value the gradient pass sees)
  log q* = sum_ij (-eps^2 / 2 - ls_ij) - D / 2 log 2 pi
  log w  = log p(h) + log p(x|h_1) - log q*
  ELBO:   value mean_s log w_s,             a_s = 1 / k
  IWAE:   value logsumexp_s log w_s - log k, a_s = softmax_s(log w)
  G^m  = sum_s a_s g_s,  G^ls = (sum_s a_s g_s eps_s) exp(ls) + 1,  g = d(log p(h) + log p(x|h_1)) / dh
  Adam ascent, step n = step0 + t + 1: m1 += (1 - b1) (G - m1); m2 += (1 - b2) (G^2 - m2);
  p += lr_n m1 / (sqrt(m2) + eps_hat), lr_n = lr sqrt(1 - b2^n) / (1 - b1^n); ls clipped to its range
then one evaluation pass on fresh noise: log_w, logpx = logsumexp - log k, ess."""
import functools

import numpy as np

from oracle import iwae_oracle as O
import ais_ref as A
import noise_ref as NR
import pathgrad_ref as PR
import score_ref as R
import scoregrad_ref as G

OBJECTIVES = ("ELBO", "IWAE")
NOISE_LAYER = 2 * NR.MAX_LAYERS + 13          # layer i's noise: philox_normal4 under NOISE_LAYER + i
SHAPES = ("S1", "S2", "S3", "S4", "C784", "K300")
# the cases of this file's own, on S1's architecture: two images of 300 samples (a 256-wide sample loop wraps;
# 64 sample groups and 16 waves wrap several times) and, beside the issue's list, one image of 1100 samples (the
# workgroup-wide loops of 1024 threads wrap)
OWN = {"K300": (tuple(PR.SHAPES["S1"][:4]), 2, 300, 7300, R.X_DIM),
       "K1100": (tuple(PR.SHAPES["S1"][:4]), 1, 1100, 7311, R.X_DIM)}
EXTRA = ("K1100",)

T = 4
LR = 0.05
BETAS = (0.9, 0.999)
EPS_HAT = 1e-3            # (at 1e-7 the first step is +- lr sign(g): discontinuous where g is about 0)
LS_RANGE = (-12.0, 4.0)
LS0 = -1.0
SEED = 7001


@functools.lru_cache(maxsize=None)
def case(name):
    """(spec, params, x, B, k): float32-representable float64 arrays."""
    if name in OWN:
        arch, B, k, seed, x_dim = OWN[name]
        spec, params, _, x, _ = PR.make_case(arch, B, k, seed, x_dim=x_dim)
        return spec, params, x, B, k
    spec, params, x, _ = R.case(name)
    return spec, params, x, R.entry(name)[1], R.entry(name)[2]


def arch(name):
    return OWN[name][0] if name in OWN else R.entry(name)[0]


@functools.lru_cache(maxsize=None)
def setting(name, seed=SEED, passes=T + 1):
    """(means, logstds, eps): the per-image sample mean of the case's "on" latents
    rounded to float32, logstd -1, and `passes` lists of injected noise [k, B, d_i]."""
    spec, params, x, B, k = case(name)
    if name in OWN:
        arch_, _, _, cseed, x_dim = OWN[name]
        on = O.forward(params, spec, x, PR.make_case(arch_, B, k, cseed, x_dim=x_dim)[4])["h"]
    else:
        on = R.latents(name, "on")
    means = [R.f32r(np.asarray(v).mean(0)) for v in on]
    logstds = [np.full(v.shape, LS0) for v in means]
    rng = np.random.default_rng(seed)
    eps = [[R.f32r(rng.standard_normal((k, B, d))) for d in spec.n_latent_encoder] for _ in range(passes)]
    for v in means + logstds + [e for p in eps for e in p]:
        v.setflags(write=False)
    return means, logstds, eps


def log_q(eps, logstd):
    """log q* [k, B] of the samples drawn with eps at logstd."""
    D = sum(v.shape[-1] for v in logstd)
    return sum((-0.5 * np.asarray(e, np.float64) ** 2 - np.asarray(ls, np.float64)[None]).sum(-1)
               for e, ls in zip(eps, logstd)) - 0.5 * D * np.log(2 * np.pi)


def sample(mean, logstd, eps, rounded=True):
    h = [np.exp(np.asarray(ls, np.float64))[None] * np.asarray(e, np.float64) + np.asarray(m, np.float64)[None]
         for m, ls, e in zip(mean, logstd, eps)]
    return [R.f32r(v) for v in h] if rounded else h


def weights(params, spec, x, mean, logstd, eps, rounded=True, **kw):
    """(h, log_w [k, B]) of one pass; rounded=False keeps h in float64 (a smooth function of the parameters)."""
    h = sample(mean, logstd, eps, rounded)
    sc = R.score(params, spec, x, h, **kw)
    return h, (np.asarray(sc["logp"], np.float64) + np.asarray(sc["logpx"], np.float64)) - log_q(eps, logstd)


def value(lw, objective):
    if objective == "ELBO":
        return lw.mean(0)
    return A.finish(lw)[0]


def objective_and_grads(params, spec, x, mean, logstd, eps, objective, scales=None, rounded=True, **kw):
    """(value [B], G^m, G^ls): the objective on the pass's samples and its total
    reparameterised gradients.  scales: a dict that receives "m" and "ls", per
    layer the scale a gradient error is measured against: test_gpu_scoregrad's
    combined-gradient scale sum_t ||g_t|| of the rows' gradients (g_t eps sigma
    for ls), times max_b ||a_b||_2, the factor by which the sum over samples
    can carry a row error into a parameter (Cauchy-Schwarz; 1 / sqrt(k) for the ELBO)."""
    h, lw = weights(params, spec, x, mean, logstd, eps, rounded, **kw)
    k = lw.shape[0]
    if objective == "ELBO":
        a = np.full(lw.shape, 1.0 / k)
    else:
        e = np.exp(lw - lw.max(0))
        a = e / e.sum(0)
    gt = G.grads(params, spec, x, h, **kw)
    g = [np.asarray(p, np.float64) + np.asarray(q, np.float64) for p, q in zip(gt["ph"], gt["px"])]
    Gm = [(a[..., None] * v).sum(0) for v in g]
    Gl = [(a[..., None] * v * np.asarray(e, np.float64)).sum(0) * np.exp(np.asarray(ls, np.float64)) + 1.0
          for v, e, ls in zip(g, eps, logstd)]
    if scales is not None:
        amp = np.sqrt((a * a).sum(0)).max()
        es = [np.asarray(e, np.float64) * np.exp(np.asarray(ls, np.float64)) for e, ls in zip(eps, logstd)]
        scales["m"] = [amp * sum(np.linalg.norm(np.asarray(gt[t][i], np.float64)) for t in ("ph", "px")) for i in range(len(g))]
        scales["ls"] = [amp * sum(np.linalg.norm(np.asarray(gt[t][i], np.float64) * es[i]) for t in ("ph", "px"))
                        for i in range(len(g))]
    return value(lw, objective), Gm, Gl


def run(params, spec, x, mean0, logstd0, eps, objective, n_iters, lr=LR, betas=BETAS, epsilon=EPS_HAT, ls_range=LS_RANGE,
        evaluate=True, step0=0, adam0=None, state_dtype=np.float64, **kw):
    """The run.  eps[p][i]: pass p's noise [k, B, d_i] (n_iters passes, then the
    evaluation's when `evaluate`); adam0: 4 L arrays as iwae_refine takes them
    (step0 > 0).  kw selects the arithmetic of the densities and gradients
    (score_ref.score's dtype / dense); parameters and moments are carried in
    state_dtype.  Returns a dict: mean, logstd, adam (4 L arrays), bound
    [n_iters, B], grads (per iteration (G^m, G^ls)), grad_scales (the first
    iteration's, objective_and_grads's), and with `evaluate` h, log_w [k, B], logpx, ess."""
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
    bound, grads, scales = [], [], {}
    for t in range(n_iters):
        val, Gm, Gl = objective_and_grads(params, spec, x, mean, logstd, eps[t], objective, scales if t == 0 else None, **kw)
        bound.append(val)
        grads.append((Gm, Gl))
        n = step0 + t + 1
        lr_n = sd(np.float32(float(np.float32(lr)) * np.sqrt(1.0 - b2 ** n) / (1.0 - b1 ** n)))
        for i in range(L):
            for p, g, j in ((mean, Gm[i], 0), (logstd, Gl[i], 2)):
                g = g.astype(state_dtype)
                m1 = adam[4 * i + j] = adam[4 * i + j] + (g - adam[4 * i + j]) * omb1
                m2 = adam[4 * i + j + 1] = adam[4 * i + j + 1] + (g * g - adam[4 * i + j + 1]) * omb2
                p[i] = p[i] + (m1 * lr_n) / (np.sqrt(m2) + eh)
            logstd[i] = np.clip(logstd[i], lo, hi)
    out = dict(mean=mean, logstd=logstd, adam=adam, bound=np.array(bound).reshape(n_iters, -1), grads=grads,
               grad_scales=scales)
    if evaluate:
        h, lw = weights(params, spec, x, mean, logstd, eps[n_iters], **kw)
        lp, ess = A.finish(lw)
        out.update(h=h, log_w=lw, logpx=lp, ess=ess)
    return out


def _freeze(v):
    if isinstance(v, np.ndarray):
        v.setflags(write=False)
    elif isinstance(v, (list, tuple)):
        for a in v:
            _freeze(a)


@functools.lru_cache(maxsize=None)
def refine_case(name, objective, n_iters=T):
    """The float64 run of a case in the fixed setting: computed once, shared, read-only."""
    spec, params, x, _, _ = case(name)
    m0, s0, eps = setting(name)
    out = run(params, spec, x, m0, s0, eps[:n_iters] + eps[T:], objective, n_iters)
    for v in out.values():
        _freeze(v)
    return out


def grad_errors(Gm, Gl, ref):
    """Worst relative L2 error over the layers of first-iteration gradients against a run()'s, of its grad_scales."""
    rm, rl = ref["grads"][0]
    sc = ref["grad_scales"]
    return max(max(G.rel_l2(a, b, s) for a, b, s in zip(Gm, rm, sc["m"])),
               max(G.rel_l2(a, b, s) for a, b, s in zip(Gl, rl, sc["ls"])))


@functools.lru_cache(maxsize=None)
def emulated_case(name, objective):
    """The same run through the float32 + bf16x3 emulation, parameters and moments in float32."""
    spec, params, x, _, _ = case(name)
    m0, s0, eps = setting(name)
    return run(params, spec, x, m0, s0, eps, objective, T, state_dtype=np.float32, dtype=np.float32, dense=R.dense_bf16x3)


# ------------------------------------------------------------ device noise
def device_noise(name, seed, passes, base0=0):
    """eps[p][i] [k, B, d_i] as iwae_refine draws it: row = b k + s, base0 + p, layer id NOISE_LAYER + i."""
    spec, _, _, B, k = case(name)
    rows = NR.sample_rows(B, k)
    key = NR.key(seed)
    return [[NR.normals(key, base0 + p, rows, d, NOISE_LAYER + i).reshape(k, B, d)
             for i, d in enumerate(spec.n_latent_encoder)] for p in range(passes)]


@functools.lru_cache(maxsize=None)
def noise_case(name, objective, seed, base0, n_iters=2):
    spec, params, x, _, _ = case(name)
    m0, s0, _ = setting(name)
    eps = device_noise(name, seed, n_iters + 1, base0)
    out = run(params, spec, x, m0, s0, eps, objective, n_iters)
    out["eps"] = eps
    return out
