"""Float64 reference of annealed importance sampling on the latents (iwae_ais),
on score_ref.score and scoregrad_ref.grads, with the cases the CPU and GPU
tests share.

Every chain is one (sample s, image b) row; all layers move jointly, identity
mass.  Transition t = 1 .. T at beta = betas[t], coefficients (c_q, c_ph, c_px)
and Delta:
  init "prior": (0, 1, beta),              Delta = log p(x|h_1)
  init "q":     (1 - beta, beta, beta),    Delta = log p(h) + log p(x|h_1) - log q(h|x)
  1. g, U_old = -(c_q log q + c_ph log p(h) + c_px log p(x|h)) and Delta at the state
  2. log_w += (betas[t] - betas[t-1]) Delta
  3. r ~ N(0, I); H_old = U_old + |r|^2 / 2; r += eps/2 g; q = state + eps r
  4. n_leapfrog gradients at q: after each but the last r += eps g, q += eps r;
     after the last r += eps/2 g, H_new = U(q) + |r|^2 / 2; accept iff log u < H_old - H_new
  5. on accept state <- q, accepts += 1
  6. eps <- clip(eps (accept ? inc : dec), step_min, step_max), carried in float32
then logpx = logsumexp_s log_w - log k and ess = (sum e)^2 / sum e^2, e = exp(log_w - max).
A term whose coefficient is 0 is left out of U and g."""
import functools

import numpy as np

from oracle import iwae_oracle as O
import noise_ref as NR
import score_ref as R
import scoregrad_ref as G

INITS = ("prior", "q")
MOM_LAYER = 2 * NR.MAX_LAYERS + 4        # momenta of layer i: philox_normal4 under MOM_LAYER + i
U_LAYER = 2 * NR.MAX_LAYERS + 12         # the accept uniform: value 0 of quad 0


def coefs(init, beta):
    return (0.0, 1.0, beta) if init == "prior" else (1.0 - beta, beta, beta)


def ais_schedule_sigmoid(T, rad=4.0):
    """Wu et al.'s schedule in float64 (the facade's ais_schedule restates it)."""
    s = lambda v: 1.0 / (1.0 + np.exp(-v))
    t = np.arange(T + 1) / T
    return (s(rad * (2 * t - 1)) - s(-rad)) / (s(rad) - s(-rad))


def _state(params, spec, x, h, init, coef, kw):
    """(U, Delta, g) at h under coef."""
    sc = R.score(params, spec, x, h, **kw)
    val = {"q": np.asarray(sc["logq"], np.float64), "ph": np.asarray(sc["logp"], np.float64),
           "px": np.asarray(sc["logpx"], np.float64)}
    gt = G.grads(params, spec, x, h, **kw)
    U = 0.0
    g = [np.zeros(v.shape) for v in h]
    for c, t in zip(coef, G.TERMS):
        if c == 0.0:
            continue
        U = U - c * val[t]
        g = [a + c * np.asarray(b, np.float64) for a, b in zip(g, gt[t])]
    delta = val["px"] if init == "prior" else (val["ph"] + val["px"]) - val["q"]
    return U, delta, g


def run(params, spec, x, h0, betas, init, step, n_leapfrog, adapt, momenta, log_u, log_w0=None, accepts0=None, **kw):
    """The chain.  h0: L arrays [k, B, d_i]; betas: T + 1 values; step: a number or
    float32 [k, B]; adapt = (inc, dec, step_min, step_max); momenta[t - 1]: L arrays
    like h0; log_u: [T, k, B], or a function (t, dH [k, B]) -> log u [k, B] (the
    cases build u from the reference's own dH).  kw selects the arithmetic of the
    densities and gradients (score_ref.score's dtype / dense); the state is float64.
    Returns a dict: h, log_w, accepts, step (float32), dH [T, k, B], accept [T, k, B],
    log_u [T, k, B], logpx [B], ess [B]."""
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
        coef = coefs(init, beta)
        U_old, delta, g = _state(params, spec, x, h, init, coef, kw)
        log_w = log_w + (float(betas[t]) - float(betas[t - 1])) * delta
        r = [np.array(v, np.float64) for v in momenta[t - 1]]
        H_old = U_old + 0.5 * sum((v * v).sum(-1) for v in r)
        e = eps.astype(np.float64)[..., None]
        r = [a + 0.5 * e * b for a, b in zip(r, g)]
        q = [a + e * b for a, b in zip(h, r)]
        for l in range(1, n_leapfrog + 1):
            U_new, _, g = _state(params, spec, x, q, init, coef, kw)
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
    logpx, ess = finish(log_w)
    return dict(h=h, log_w=log_w, accepts=accepts, step=eps, dH=np.array(dHs), accept=np.array(accs),
                log_u=np.array(lus), logpx=logpx, ess=ess)


def finish(log_w):
    """(logpx [B], ess [B]) of log_w [k, B], float64."""
    lw = np.asarray(log_w, np.float64)
    m = lw.max(0)
    e = np.exp(lw - m)
    return m + np.log(e.sum(0)) - np.log(lw.shape[0]), e.sum(0) ** 2 / (e * e).sum(0)


# ------------------------------------------------------------------- cases
BETAS = (0.0, 0.1, 0.4, 0.8, 1.0)
N_LEAPFROG = 3
ADAPT = (1.25, 0.5, 0.01, 2.0)
STEPS = (0.5, 0.4, 0.3, 0.2, 0.15, 0.1)
SEEDS = tuple(range(5001, 5007))
SHAPES = ("S1", "S2", "S3", "S4", "K130", "C784")
START = {"prior": "prior", "q": "on"}

# (shape case, init): (step, momentum seed): the first of STEPS x SEEDS (steps outer) at which the float64
# run has |dH| < 5 on every chain and transition and rejects in at least two transitions (search();
# tests/test_ais_ref.py asserts both conditions on every entry)
AIS_CASES = {
    ("S1", "prior"): (0.5, 5002), ("S1", "q"): (0.5, 5001),
    ("S2", "prior"): (0.2, 5002), ("S2", "q"): (0.2, 5004),
    ("S3", "prior"): (0.15, 5001), ("S3", "q"): (0.2, 5001),
    ("S4", "prior"): (0.2, 5001), ("S4", "q"): (0.2, 5001),
    ("K130", "prior"): (0.15, 5001), ("K130", "q"): (0.15, 5002),
    ("C784", "prior"): (0.5, 5001), ("C784", "q"): (0.4, 5001),
}


# a second registry of (step, momentum seed), filled by tests/latent_shape_cases.py under the same search;
# AIS_CASES and the tests parametrized over it stay as they are
EXTRA_AIS_CASES = {}


def ais_entry(name, init):
    return AIS_CASES[name, init] if (name, init) in AIS_CASES else EXTRA_AIS_CASES[name, init]


def momenta_of(name, seed, T):
    h = R.latents(name, "on")
    rng = np.random.default_rng(seed)
    return [[R.f32r(rng.standard_normal(v.shape)) for v in h] for _ in range(T)]


def log_u_rule(t, dH):
    """No decision within 0.4 nats of its margin: accepted by 0.4, but chains with
    (s B + b + t) odd whose dH allows it (u < 1) rejected by 0.4; u <= exp(-1e-3)."""
    k, B = dH.shape
    chain = np.arange(k * B).reshape(k, B)
    lu = -dH - 0.4
    rej = ((chain + t) % 2 == 1) & (dH > 0.4)
    return np.minimum(np.where(rej, -dH + 0.4, lu), -1e-3)


def _run_case(name, init, step, seed, **kw):
    spec, params, x, _ = R.case(name)
    mom = momenta_of(name, seed, len(BETAS) - 1)
    out = run(params, spec, x, R.latents(name, START[init]), BETAS, init, step, N_LEAPFROG, ADAPT, mom,
              kw.pop("log_u", log_u_rule), **kw)
    out["momenta"] = mom
    return out


def conditions(out):
    """(max |dH|, transitions with a rejection) of a run."""
    return float(np.abs(out["dH"]).max()), int((~out["accept"]).any(axis=(1, 2)).sum())


def search(name, init):
    for step in STEPS:
        for seed in SEEDS:
            big, nrej = conditions(_run_case(name, init, step, seed))
            if big < 5.0 and nrej >= 2:
                return step, seed
    return None


@functools.lru_cache(maxsize=None)
def ais_case(name, init):
    """The float64 run of a case (run()'s dict plus "momenta"): computed once, shared, read-only."""
    step, seed = ais_entry(name, init)
    out = _run_case(name, init, step, seed)
    for v in out.values():
        for a in (v if isinstance(v, list) else [v]):
            for b in (a if isinstance(a, list) else [a]):
                b.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def emulated_case(name, init):
    """The same momenta and log u through the float32 + bf16x3 emulation of the densities and gradients."""
    step, seed = ais_entry(name, init)
    return _run_case(name, init, step, seed, log_u=ais_case(name, init)["log_u"], dtype=np.float32, dense=R.dense_bf16x3)


# ------------------------------------------------------------ device noise
# (shape case, init): (step, seed of set_seed): T = 2 transitions on the library's own Philox momenta and
# accept uniforms from position 0; the seed is the first of 6001.. at which every chain's decision margin
# |log u + dH| in the float64 run is at least 0.05 nats and both decisions occur (search_noise();
# asserted in tests/test_ais_ref.py)
NOISE_BETAS = (0.0, 0.5, 1.0)
NOISE_MARGIN = 0.05
NOISE_CASES = {("S2", "q"): (0.2, 6025), ("S3", "prior"): (0.15, 6035)}


def device_noise(name, seed, T, base0=0):
    """(momenta[t - 1][i] [k, B, d_i], u [T, k, B] float32) as iwae_ais draws them: row = b k + s, base0 + t - 1."""
    _, B, k = R.entry(name)[:3]
    dims = R.case(name)[0].n_latent_encoder
    rows = NR.sample_rows(B, k)
    key = NR.key(seed)
    mom = [[NR.normals(key, base0 + t, rows, d, MOM_LAYER + i).reshape(k, B, d) for i, d in enumerate(dims)]
           for t in range(T)]
    u = np.stack([NR.uniforms(key, base0 + t, rows, 1, U_LAYER)[:, 0].reshape(k, B) for t in range(T)])
    return mom, u


def _run_noise(name, init, step, seed):
    spec, params, x, _ = R.case(name)
    mom, u = device_noise(name, seed, len(NOISE_BETAS) - 1)
    out = run(params, spec, x, R.latents(name, START[init]), NOISE_BETAS, init, step, N_LEAPFROG, ADAPT, mom,
              np.log(u.astype(np.float64)))
    out["momenta"], out["u"] = mom, u
    return out


def noise_margin(out):
    return float(np.abs(out["log_u"] + out["dH"]).min())


def search_noise(name, init, step):
    for seed in range(6001, 6065):
        out = _run_noise(name, init, step, seed)
        if noise_margin(out) >= NOISE_MARGIN and out["accept"].any() and not out["accept"].all():
            return seed
    return None


@functools.lru_cache(maxsize=None)
def noise_case(name, init):
    step, seed = NOISE_CASES[name, init]
    return _run_noise(name, init, step, seed)
