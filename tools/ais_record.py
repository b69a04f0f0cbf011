"""AIS record: on the configs[1] architecture
(784-200-200-100-100-50), N = 100 images, k = 50, 4 leapfrogs, microseconds
per transition of
  (a) five iwae_score_grad calls with a transition's coefficients and outputs
      (beta = 0.5; from the prior: (0, 1, beta), log_ph and log_px; from q:
      (1 - beta, beta, beta), all three values): the floor, nothing between
      the gradient launches,
  (b) iwae_ais over T = 200 transitions (the sigmoid schedule, device noise,
      adapting steps), from the prior and from q, per transition,
  (c) one Flexible_Model.hmc iteration per call (the facade this replaces on
      the way to AIS, its synchronizes included),
the arms alternating in one process.  Each figure brackets at least 0.2 s of
enqueued work with events on the model's stream, after a warm-up; five
repeats, median and spread.  Writes one JSON record.
    python tools/ais_record.py [out.json]"""
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from iwae_replication_project_amd import Flexible_Model, _lib, ais_schedule  # noqa: E402

HE, HD, LE, LD = [200, 100], [100, 200], [100, 50], [100, 784]
N, K, T, LEAPFROGS, REPEATS, MIN_SECONDS = 100, 50, 200, 4, 5, 0.2
BETA, STEP = 0.5, 0.05


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "ais_record.json")
    rng = np.random.default_rng(0)
    mean = rng.uniform(0.02, 0.4, 784)
    m = Flexible_Model(HE, HD, LE, LD, dataset_bias=mean, loss_function="IWAE", k=K, seed=1)
    dev = m.device
    x = torch.from_numpy((rng.random((N, 784)) < mean).astype(np.float32)).to(dev)
    gen = torch.Generator(device=dev).manual_seed(K)
    lat0 = [torch.randn(K, N, d, device=dev, generator=gen) for d in LE]
    lat = [t.clone() for t in lat0]                       # (a), (c): fixed latents
    chains = {init: [t.clone() for t in lat0] for init in (0, 1)}      # (b): the chains' own state
    grads = [torch.empty_like(t) for t in lat]
    terms = [torch.empty(N, K, device=dev) for _ in range(3)]
    outs = {n: torch.empty(N, K, device=dev) for n in ("log_w", "accepts")}
    lpx, ess = torch.empty(N, device=dev), torch.empty(N, device=dev)
    torch.cuda.synchronize()
    arr, n = _lib.fptr_array(lat)
    garr, ng = _lib.fptr_array(grads)
    q, ph, px = [_lib.fptr(t) for t in terms]
    betas = ais_schedule(T)
    P = _lib.fptr

    def floor(init):
        c = (ctypes.c_float * 3)(*((1 - BETA, BETA, BETA) if init else (0.0, 1.0, BETA)))
        for _ in range(LEAPFROGS + 1):
            m._call(m._lib.iwae_score_grad(m._h, P(x), N, K, 0, arr, n, c, garr, ng, q if init else None, ph, px))

    def ais(init):
        cfg = _lib.IwaeAisConfig(init=init, n_temps=T, n_leapfrog=LEAPFROGS, accumulate=0, step=STEP, adapt_inc=1.02,
                                 adapt_dec=0.98, step_min=1e-4, step_max=1.0)
        carr, cn = _lib.fptr_array(chains[init])
        m._call(m._lib.iwae_ais(m._h, P(x), N, K, 0, carr, cn, ctypes.byref(cfg), betas.ctypes.data_as(_lib.FP), None, 0,
                                None, None, P(outs["log_w"]), P(outs["accepts"]), P(lpx), P(ess)))

    # name, function, transitions per call
    variants = [("a_floor_prior", lambda: floor(0), 1), ("a_floor_q", lambda: floor(1), 1),
                ("b_ais_prior", lambda: ais(0), T), ("b_ais_q", lambda: ais(1), T),
                ("c_hmc_facade", lambda: m.hmc(x, lat, STEP, LEAPFROGS), 1)]

    def timed(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(m._stream)
        for _ in range(calls):
            fn()
        e1.record(m._stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    def counts():
        return [int(m._lib.iwae_debug_count(m._h, i)) for i in (25, 26, 27, 28)]

    calls = {}
    for name, fn, _ in variants:                   # warm-up, then the call count that fills MIN_SECONDS
        for _ in range(2):
            fn()
        m._stream.synchronize()
        t = timed(fn, 2) / 2
        calls[name] = max(1, int(MIN_SECONDS * 1.3 / t) + 1)
    c0 = counts()
    ais(0)
    c1 = counts()
    times = {name: [] for name, _, _ in variants}
    for _ in range(REPEATS):
        for name, fn, per in variants:             # alternating
            s = timed(fn, calls[name])
            assert s >= MIN_SECONDS, (name, s)
            times[name].append(s / (calls[name] * per))
    m.check_kernel_status()
    d = [b - a for a, b in zip(c0, c1)]
    rec = dict(arch="784-200-200-100-100-50", images=N, k=K, leapfrogs=LEAPFROGS, transitions_per_ais_call=T,
               repeats=REPEATS, device=torch.cuda.get_device_name(dev),
               gradient_path="fused" if d[0] > 0 else "layer-wise",
               per_ais_call=dict(gradient_passes=d[0] + d[1], transitions=d[2], begin_step_end_launches=d[3]),
               ais_q_accept_rate=round(float(outs["accepts"].mean()) / T, 3), variants={})
    for name, ts in times.items():
        us = [t * 1e6 for t in ts]
        rec["variants"][name] = dict(calls_per_repeat=calls[name], us_per_transition=[round(v, 1) for v in us],
                                     median_us=round(statistics.median(us), 1), spread_us=round(max(us) - min(us), 1))
    v = {n: r["median_us"] for n, r in rec["variants"].items()}
    for init in ("prior", "q"):
        rec[f"b_over_a_{init}"] = round(v[f"b_ais_{init}"] / v[f"a_floor_{init}"], 4)
        rec[f"b_minus_a_{init}_us"] = round(v[f"b_ais_{init}"] - v[f"a_floor_{init}"], 1)
        rec[f"c_over_b_{init}"] = round(v["c_hmc_facade"] / v[f"b_ais_{init}"], 4)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(rec, open(out_path, "w"), indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
