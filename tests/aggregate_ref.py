"""Float64 reference of the aggregate posterior (iwae_aggregate), plain numpy,
and the cases the CPU and GPU tests share.

Definitions, for R query rows h [R, d], M components (mu, s) [M, d]:
  t(r,m,j) = -1/2 z^2 - log s_mj - 1/2 log 2 pi,   z = (h_rj - mu_mj) (1 / s_mj)
  J(r,m)   = sum_j t(r,m,j)
  log_q_agg[r]    = logsumexp_m J(r,m) - log M
  log_q_dim[r,j]  = logsumexp_m t(r,m,j) - log M
  log_q_own[r]    = J(r, r mod P),   log_q_own_dim[r,j] = t(r, r mod P, j)
The logsumexp is two-pass (max over m, then the sum of exp).  With
dtype=float32 the same lines run in float32 the way the kernels do: 1 / s and
log s formed once, J summed in column order, the logsumexp online over m.

The row scale S_r is the sum over j of the absolute values of the three addends
of t(r, m*, j), 1/2 z^2 + |log s| + 1/2 log 2 pi, at the row's dominant
reference m* = argmax_m J(r,m): what the rounding of a float32 evaluation of
the row's result scales with (as score_ref's Sq, Sp do for their densities).
The GPU bars are 1e-4 max|ref| over an output and 1e-4 S_r per row.
"""
import functools
import zlib

import numpy as np

HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)
REL = 1e-4                                  # test_gpu_score.py's bars

D1S = (1, 3, 50, 64, 65, 200)
MS = (1, 2, 63, 64, 65, 1000)
RS = (1, 15, 17, 257)


def f32r(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def _covering():
    """Every (d1, M), (d1, R) and (M, R) pair at least once: R's index is (i + j) mod 4 on
    the 6 x 6 grid of (d1, M), plus the named shapes that grid does not hold."""
    out = {}
    for i, d in enumerate(D1S):
        for j, M in enumerate(MS):
            out[f"d{d}_M{M}_R{RS[(i + j) % 4]}"] = (d, M, RS[(i + j) % 4])
    for d, M, R in ((1, 1, 1), (65, 65, 17), (200, 1000, 257), (64, 1000, 1)):
        out[f"d{d}_M{M}_R{R}"] = (d, M, R)
    return out


# name: (d1, M, R); inputs() draws them
SHAPES = _covering()
# edge inputs: name: (d1, M, R, kind)
EDGES = {
    "small": (50, 65, 130, "small"),        # scales 1e-3, means far apart: off-image terms underflow
    "wide": (50, 65, 130, "wide"),          # scales 10: every reference term comparable
    "poison": (50, 65, 17, "poison"),       # row 5 of the latents is NaN
    "m1": (65, 1, 17, "plain"),             # one component: the aggregate is the own term
    "own": (3, 5, 15, "plain"),             # [k = 3][N = 5][d1] latents, own image r mod 5
    "d260": (260, 13, 17, "plain"),         # more than 256 units: a second unit chunk (of 4) in the per-unit kernel
    "d260s": (260, 1000, 5, "plain"),       # ... with the references split
}
ALL = {**{n: v + ("plain",) for n, v in SHAPES.items()}, **EDGES}


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(h [R, d], mu [M, d], s [M, d], P): float32-representable float64 arrays; row r is a
    draw from component r mod M, and P = M."""
    d, M, R, kind = ALL[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))     # a case's inputs do not depend on the table around it
    mu = rng.standard_normal((M, d))
    s = np.exp(-1.0 + 0.5 * rng.standard_normal((M, d)))
    if kind == "small":
        mu = 3.0 * mu
        s = np.full((M, d), 1e-3)
    elif kind == "wide":
        s = np.full((M, d), 10.0) * np.exp(0.1 * rng.standard_normal((M, d)))
    mu, s = f32r(mu), f32r(s)
    o = np.arange(R) % M
    h = f32r(mu[o] + s[o] * rng.standard_normal((R, d)))
    if kind == "poison":
        h[5] = np.nan
    for a in (h, mu, s):
        a.setflags(write=False)
    return h, mu, s, M


def aggregate(h, mu, s, P=0, dtype=np.float64):
    """dict(log_q_agg [R], log_q_dim [R, d], S [R], and with P > 0 log_q_own [R],
    log_q_own_dim [R, d])."""
    dt = np.dtype(dtype).type
    f32 = np.dtype(dtype) == np.float32
    h, mu, s = (np.asarray(a, dtype=dtype) for a in (h, mu, s))
    R, d = h.shape
    M = mu.shape[0]
    rs = dt(1.0) / s
    lc = -(np.log(s) + dt(HALF_LOG_2PI))

    def t_of(m):                                             # t(:, m, :) [R, d] and its addends' magnitudes
        z = (h - mu[m]) * rs[m]
        hz = dt(0.5) * z * z
        return lc[m] - hz, hz + np.abs(np.log(s[m])) + dt(HALF_LOG_2PI)

    def j_of(t):
        return np.cumsum(t, axis=-1)[:, -1] if f32 else t.sum(-1)

    with np.errstate(invalid="ignore", over="ignore"):
        if f32:                                              # online, one exp per value, as the kernels
            mj, sj = np.full(R, -np.inf, dtype), np.zeros(R, dtype)
            md, sd = np.full((R, d), -np.inf, dtype), np.zeros((R, d), dtype)

            def push(m_, s_, v):
                dv = np.where(v == -np.inf, dt(-np.inf), v - m_)
                e = np.exp(-np.abs(dv))
                up = dv > 0
                s_[...] = np.where(up, s_ * e + dt(1.0), s_ + e)
                m_[...] = np.where(up, v, m_)
            for m in range(M):
                t, _ = t_of(m)
                push(mj, sj, j_of(t))
                push(md, sd, t)
        else:                                                # two passes
            mj, md = np.full(R, -np.inf), np.full((R, d), -np.inf)
            for m in range(M):
                t, _ = t_of(m)
                mj, md = np.fmax(mj, j_of(t)), np.fmax(md, t)
            bj, bd = np.where(np.isfinite(mj), mj, 0.0), np.where(np.isfinite(md), md, 0.0)
            sj, sd = np.zeros(R), np.zeros((R, d))
            for m in range(M):
                t, _ = t_of(m)
                sj, sd = sj + np.exp(j_of(t) - bj), sd + np.exp(t - bd)
        with np.errstate(divide="ignore"):
            out = dict(log_q_agg=mj + np.log(sj) - dt(np.log(M)), log_q_dim=md + np.log(sd) - dt(np.log(M)))
        # the dominant reference of each row and its scale (float64 lines whatever dtype)
        best, S = np.full(R, -np.inf), np.zeros(R)
        for m in range(M):
            t, a = t_of(m)
            J = np.nan_to_num(j_of(t).astype(np.float64), nan=np.inf)    # a poisoned row: any scale will do
            S = np.where(J > best, a.sum(-1), S)
            best = np.fmax(best, J)
        out["S"] = S
        if P > 0:
            o = np.arange(R) % P
            z = (h - mu[o]) * rs[o]
            t = lc[o] - dt(0.5) * z * z
            out["log_q_own"], out["log_q_own_dim"] = j_of(t), t
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 reference of a case: computed once, shared, read-only."""
    h, mu, s, P = inputs(name)
    out = aggregate(h, mu, s, P)
    for v in out.values():
        v.setflags(write=False)
    return out


OUTPUTS = ("log_q_agg", "log_q_dim", "log_q_own", "log_q_own_dim")


def errors(got, ref):
    """{output: (max error / max|ref|, max over rows of the row's max error / S_r)} over the
    rows the reference has finite, in units of the bars (<= 1 passes)."""
    S = ref["S"]
    out = {}
    for n in OUTPUTS:
        if n not in got:
            continue
        g, r = np.asarray(got[n], dtype=np.float64), ref[n]
        ok = np.isfinite(r.reshape(len(S), -1)).all(-1)
        err = np.abs(g - r).reshape(len(S), -1)[ok].max(-1)
        out[n] = (err.max() / (REL * np.abs(r[ok]).max()), (err / (REL * S[ok])).max())
    return out


def information(log_q, log_ph, log_q_own, log_q_agg):
    """(kl, mi, marginal_kl): the ELBO-surgery means over all rows, float64."""
    lq, lp, own, agg = (np.asarray(a, dtype=np.float64) for a in (log_q, log_ph, log_q_own, log_q_agg))
    return (lq - lp).mean(), (own - agg).mean(), (lq - own + agg - lp).mean()
