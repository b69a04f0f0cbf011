"""Refinement record: on the configs[1] architecture
(784-200-200-100-100-50), N = 100 images, k = 50, microseconds per refinement
iteration of
  (a) one bare iwae_score_grad call under (0, 1, 1) with log_ph and log_px (what
      an iteration's gradient pass is): the floor, and an unchanged kernel,
  (b) iwae_refine over T = 200 iterations, ELBO and IWAE_k, device noise, no
      evaluation pass, per iteration,
  (c) one iteration of the torch loop a caller had to write around
      Flexible_Model.score_grad (ELBO; its synchronizes included),
the arms alternating in one process.  Each figure brackets at least 0.2 s of
enqueued work with events on the model's stream, after a warm-up; five
repeats, median and spread.  Writes one JSON record.
    python tools/refine_record.py [out.json]"""
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from iwae_replication_project_amd import Flexible_Model, _lib  # noqa: E402

HE, HD, LE, LD = [200, 100], [100, 200], [100, 50], [100, 784]
N, K, T, REPEATS, MIN_SECONDS = 100, 50, 200, 5, 0.2
LR = 0.01


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "refine_record.json")
    rng = np.random.default_rng(0)
    mean = rng.uniform(0.02, 0.4, 784)
    m = Flexible_Model(HE, HD, LE, LD, dataset_bias=mean, loss_function="IWAE", k=K, seed=1)
    dev = m.device
    x = torch.from_numpy((rng.random((N, 784)) < mean).astype(np.float32)).to(dev)
    gen = torch.Generator(device=dev).manual_seed(K)
    lat = [torch.randn(K, N, d, device=dev, generator=gen) for d in LE]
    grads = [torch.empty_like(t) for t in lat]
    terms = [torch.empty(N, K, device=dev) for _ in range(2)]
    par = {o: ([torch.zeros(N, d, device=dev) for d in LE], [torch.full((N, d), -1.0, device=dev) for d in LE]) for o in (0, 1)}
    bound = torch.empty(T, N, device=dev)
    torch.cuda.synchronize()
    arr, n = _lib.fptr_array(lat)
    garr, ng = _lib.fptr_array(grads)
    ph, px = [_lib.fptr(t) for t in terms]
    P = _lib.fptr
    coef = (ctypes.c_float * 3)(0.0, 1.0, 1.0)

    def floor():
        m._call(m._lib.iwae_score_grad(m._h, P(x), N, K, 0, arr, n, coef, garr, ng, None, ph, px))

    def refine(objective):
        cfg = _lib.IwaeRefineConfig(objective=objective, n_iters=T, step0=0, lr=LR, beta1=0.9, beta2=0.999, epsilon=1e-7,
                                    logstd_min=-12.0, logstd_max=4.0)
        marr, nm = _lib.fptr_array(par[objective][0])
        sarr, _ = _lib.fptr_array(par[objective][1])
        m._call(m._lib.iwae_refine(m._h, P(x), N, K, 0, marr, sarr, nm, ctypes.byref(cfg), None, 0, None, 0, P(bound),
                                   None, 0, None, None, None))

    tm = [torch.zeros(N, d, device=dev) for d in LE]
    ts = [torch.full((N, d), -1.0, device=dev) for d in LE]
    mom = [torch.zeros(N, d, device=dev) for d in LE for _ in range(4)]
    step = [0]

    def torch_loop():
        with torch.cuda.stream(m._stream):
            eps = [torch.randn(K, N, d, device=dev) for d in LE]
            h = [torch.addcmul(a, b.exp(), e) for a, b, e in zip(tm, ts, eps)]
        g = m.score_grad(x, h)["grad"]
        step[0] += 1
        lr_n = LR * (1 - 0.999 ** step[0]) ** 0.5 / (1 - 0.9 ** step[0])
        with torch.cuda.stream(m._stream):
            for i in range(len(LE)):
                G = (g[i].mean(0), (g[i] * eps[i]).mean(0) * ts[i].exp() + 1.0)
                for j, p in enumerate((tm[i], ts[i])):
                    m1, m2 = mom[4 * i + 2 * j], mom[4 * i + 2 * j + 1]
                    m1.lerp_(G[j], 0.1)
                    m2.lerp_(G[j] * G[j], 0.001)
                    p.add_(lr_n * m1 / (m2.sqrt() + 1e-7))
                ts[i].clamp_(-12.0, 4.0)

    # name, function, iterations per call
    variants = [("a_floor", floor, 1), ("b_refine_elbo", lambda: refine(0), T), ("b_refine_iwae", lambda: refine(1), T),
                ("c_torch_loop", torch_loop, 1)]

    def timed(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(m._stream)
        for _ in range(calls):
            fn()
        e1.record(m._stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    def counts():
        return [int(m._lib.iwae_debug_count(m._h, i)) for i in (25, 26, 29, 30)]

    calls = {}
    for name, fn, _ in variants:                   # warm-up, then the call count that fills MIN_SECONDS
        for _ in range(2):
            fn()
        m._stream.synchronize()
        t = timed(fn, 2) / 2
        calls[name] = max(1, int(MIN_SECONDS * 1.3 / t) + 1)
    c0 = counts()
    refine(0)
    c1 = counts()
    times = {name: [] for name, _, _ in variants}
    for _ in range(REPEATS):
        for name, fn, per in variants:             # alternating
            s = timed(fn, calls[name])
            assert s >= MIN_SECONDS, (name, s)
            times[name].append(s / (calls[name] * per))
    m.check_kernel_status()
    d = [b - a for a, b in zip(c0, c1)]
    rec = dict(arch="784-200-200-100-100-50", images=N, k=K, iterations_per_refine_call=T, repeats=REPEATS,
               device=torch.cuda.get_device_name(dev), gradient_path="fused" if d[0] > 0 else "layer-wise",
               per_refine_call=dict(gradient_passes=d[0] + d[1], iterations=d[2], begin_step_end_launches=d[3]),
               last_elbo_bound_mean=round(float(bound[-1].mean()), 3), variants={})
    for name, ts_ in times.items():
        us = [t * 1e6 for t in ts_]
        rec["variants"][name] = dict(calls_per_repeat=calls[name], us_per_iteration=[round(v, 1) for v in us],
                                     median_us=round(statistics.median(us), 1), spread_us=round(max(us) - min(us), 1))
    v = {n: r["median_us"] for n, r in rec["variants"].items()}
    for o in ("elbo", "iwae"):
        rec[f"b_over_a_{o}"] = round(v[f"b_refine_{o}"] / v["a_floor"], 4)
        rec[f"b_minus_a_{o}_us"] = round(v[f"b_refine_{o}"] - v["a_floor"], 1)
    rec["c_over_b_elbo"] = round(v["c_torch_loop"] / v["b_refine_elbo"], 4)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(rec, open(out_path, "w"), indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
