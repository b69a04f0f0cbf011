"""Score-gradient record: on the configs[1] architecture
(784-200-200-100-100-50), N = 100 images, k = 50 and k = 5000, standard-normal
latents, the time of
  (a) iwae_score, all three terms, fused (score_kernel): the yardstick,
  (a_lw) the same through the layer-wise kernels (kernel_path="layerwise"): what
      the gradient passes below add their backward to,
  (b) iwae_score_grad with (0, 1, 1), gradients only, automatic path,
  (c) iwae_score_grad with (-1, 1, 1) and all three values, automatic path,
  (d) (c) under kernel_path="layerwise",
  (e) one Flexible_Model.hmc iteration with 4 leapfrogs, per call (the facade,
      its synchronizes included),
the arms alternating in one process.  The record says which path each
gradient arm took (debug counts 25 / 26).  Each figure brackets at least 0.2 s
of enqueued work with events on the model's stream, after a warm-up; five
repeats, median and spread.  Writes one JSON record.
    python tools/scoregrad_record.py [out.json]"""
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
N, KS, REPEATS, MIN_SECONDS = 100, (50, 5000), 5, 0.2


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "scoregrad_record.json")
    rng = np.random.default_rng(0)
    mean = rng.uniform(0.02, 0.4, 784)
    auto = Flexible_Model(HE, HD, LE, LD, dataset_bias=mean, loss_function="IWAE", k=50, seed=1)
    layer = Flexible_Model(HE, HD, LE, LD, dataset_bias=mean, loss_function="IWAE", k=50, seed=1,
                           kernel_path="layerwise")
    layer.set_weights(auto.get_weights())
    x = torch.from_numpy((rng.random((N, 784)) < mean).astype(np.float32)).to(auto.device)
    rec_out = dict(arch="784-200-200-100-100-50", images=N, latents="standard normal, [k][N][d]", repeats=REPEATS,
                   device=torch.cuda.get_device_name(auto.device), k={})

    def timed(m, fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(m._stream)
        for _ in range(calls):
            fn()
        e1.record(m._stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    def counts(m):
        return [int(m._lib.iwae_debug_count(m._h, i)) for i in (23, 24, 25, 26)]

    for k in KS:
        gen = torch.Generator(device=auto.device).manual_seed(k)
        lat = [torch.randn(k, N, d, device=auto.device, generator=gen) for d in LE]
        grads = [torch.empty_like(t) for t in lat]
        terms = [torch.empty(N, k, device=auto.device) for _ in range(3)]
        torch.cuda.synchronize()
        arr, n = _lib.fptr_array(lat)
        garr, ng = _lib.fptr_array(grads)
        q, ph, px = [_lib.fptr(t) for t in terms]

        def score(m):
            m._call(m._lib.iwae_score(m._h, _lib.fptr(x), N, k, 0, arr, n, q, ph, px, None, 0))

        def grad(m, coef, values):
            c = (ctypes.c_float * 3)(*coef)
            m._call(m._lib.iwae_score_grad(m._h, _lib.fptr(x), N, k, 0, arr, n, c, garr, ng,
                                           q if values else None, ph if values else None, px if values else None))

        variants = [("a_score_fused", auto, lambda: score(auto)),
                    ("a_lw_score_layerwise", layer, lambda: score(layer)),
                    ("b_grad_011", auto, lambda: grad(auto, (0, 1, 1), False)),
                    ("c_grad_m111_values", auto, lambda: grad(auto, (-1, 1, 1), True)),
                    ("d_grad_m111_values_layerwise", layer, lambda: grad(layer, (-1, 1, 1), True)),
                    ("e_hmc_4_leapfrogs", auto, lambda: auto.hmc(x, lat, 0.05, 4))]
        calls = {}
        for name, m, fn in variants:               # warm-up, then the call count that fills MIN_SECONDS
            for _ in range(2):
                fn()
            m._stream.synchronize()
            t = timed(m, fn, 3) / 3
            n1 = max(3, int(0.25 * MIN_SECONDS / t) + 1)        # a longer look: the first calls run slow
            t = timed(m, fn, n1) / n1
            calls[name] = max(3, int(MIN_SECONDS * 1.3 / t) + 1)
        c0 = counts(auto)
        grad(auto, (0, 1, 1), False)
        c1 = counts(auto)
        path = "fused" if c1[2] > c0[2] else "layer-wise"
        times = {name: [] for name, _, _ in variants}
        for _ in range(REPEATS):
            for name, m, fn in variants:           # alternating
                s = timed(m, fn, calls[name])
                assert s >= MIN_SECONDS, (name, s)
                times[name].append(s / calls[name])
        for m in (auto, layer):
            m.check_kernel_status()
        rk = dict(variants={}, gradient_path_auto=path, chunks_per_gradient_call=sum(c1[2:]) - sum(c0[2:]))
        for name, ts in times.items():
            us = [t * 1e6 for t in ts]
            rk["variants"][name] = dict(calls_per_repeat=calls[name], us_per_call=[round(v, 1) for v in us],
                                        median_us=round(statistics.median(us), 1),
                                        spread_us=round(max(us) - min(us), 1))
        v = {n: d["median_us"] for n, d in rk["variants"].items()}
        rk["b_over_a"] = round(v["b_grad_011"] / v["a_score_fused"], 4)
        rk["c_over_a"] = round(v["c_grad_m111_values"] / v["a_score_fused"], 4)
        rk["d_over_c"] = round(v["d_grad_m111_values_layerwise"] / v["c_grad_m111_values"], 4)
        rk["c_over_a_lw"] = round(v["c_grad_m111_values"] / v["a_lw_score_layerwise"], 4)
        rk["e_over_5b"] = round(v["e_hmc_4_leapfrogs"] / (5 * v["b_grad_011"]), 4)
        rec_out["k"][str(k)] = rk
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(rec_out, open(out_path, "w"), indent=1)
    print(json.dumps(rec_out))


if __name__ == "__main__":
    main()
