"""Importance-weighted posterior record: on the configs[1]
architecture (784-200-200-100-100-50), N = 100 images, k = 50 and k = 5000,
device noise, the time of
  (a)  iwae_nll alone (the first pass's forward and log-sum-exp),
  (b)  iwae_posterior with every output on the fused path (post_kernel),
  (b1) the same call asked for weights, ess and log_px only (no second pass:
       (b) - (b1) is what the second pass and its merge cost),
  (c)  iwae_posterior with every output through the layer-wise fallback
       (kernel_path="layerwise": its first pass is the layer-wise forward),
the variants alternating in one process.  Each figure brackets at least 0.2 s of
enqueued work with events on the model's stream (the native calls, without the
facade's per-call synchronize), after a warm-up; five repeats, median and
spread.  Writes one JSON record.
    python tools/posterior_record.py [out.json]"""
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
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "posterior_record.json")
    rng = np.random.default_rng(0)
    mean = rng.uniform(0.02, 0.4, 784)
    models = {p: Flexible_Model(HE, HD, LE, LD, dataset_bias=mean, loss_function="IWAE", k=50, seed=1, kernel_path=p)
              for p in ("auto", "layerwise")}
    models["layerwise"].set_weights(models["auto"].get_weights())
    fused, layer = models["auto"], models["layerwise"]
    x = torch.from_numpy((rng.random((N, 784)) < mean).astype(np.float32)).to(fused.device)
    rec_out = dict(arch="784-200-200-100-100-50", images=N, noise="device (Philox)", repeats=REPEATS,
                   device=torch.cuda.get_device_name(fused.device), k={})

    def timed(m, fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(m._stream)
        for _ in range(calls):
            fn()
        e1.record(m._stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    for k in KS:
        bufs = {}
        for name, m in models.items():
            with torch.cuda.stream(m._stream):
                bufs[name] = dict(hm=[torch.empty(N, d, device=m.device) for d in LE],
                                  hs=[torch.empty(N, d, device=m.device) for d in LE],
                                  probs=torch.empty(N, 784, device=m.device), w=torch.empty(N, k, device=m.device),
                                  ess=torch.empty(N, device=m.device), lpx=torch.empty(N, device=m.device))
        torch.cuda.synchronize()

        def nll(m, name):
            m._call(m._lib.iwae_nll(m._h, _lib.fptr(x), N, k, 0, _lib.fptr(bufs[name]["lpx"])))

        def post(m, name, second):
            b = bufs[name]
            marr, nm = _lib.fptr_array(b["hm"] if second else [])
            sarr, ns = _lib.fptr_array(b["hs"] if second else [])
            m._call(m._lib.iwae_posterior(m._h, _lib.fptr(x), N, k, 0, None, 0, None, marr, nm,
                                          _lib.fptr(b["probs"]) if second else None, 784 if second else 0, sarr, ns,
                                          _lib.fptr(b["w"]), _lib.fptr(b["ess"]), _lib.fptr(b["lpx"])))

        variants = [("a_nll", fused, lambda: nll(fused, "auto")),
                    ("b_posterior_fused", fused, lambda: post(fused, "auto", True)),
                    ("b1_weights_only_fused", fused, lambda: post(fused, "auto", False)),
                    ("c_posterior_layerwise", layer, lambda: post(layer, "layerwise", True))]
        calls = {}
        for name, m, fn in variants:               # warm-up, then the call count that fills MIN_SECONDS
            for _ in range(2):
                fn()
            m._stream.synchronize()
            t = timed(m, fn, 3) / 3
            n1 = max(3, int(0.25 * MIN_SECONDS / t) + 1)        # a longer look: the first calls run slow
            t = timed(m, fn, n1) / n1
            calls[name] = max(3, int(MIN_SECONDS * 1.3 / t) + 1)
        c0 = [int(fused._lib.iwae_debug_count(fused._h, i)) for i in (17, 18)]
        l0 = [int(layer._lib.iwae_debug_count(layer._h, i)) for i in (17, 18)]
        times = {name: [] for name, _, _ in variants}
        for _ in range(REPEATS):
            for name, m, fn in variants:           # alternating
                s = timed(m, fn, calls[name])
                assert s >= MIN_SECONDS, (name, s)
                times[name].append(s / calls[name])
        for m in models.values():
            m.check_kernel_status()
        c1 = [int(fused._lib.iwae_debug_count(fused._h, i)) for i in (17, 18)]
        l1 = [int(layer._lib.iwae_debug_count(layer._h, i)) for i in (17, 18)]
        assert c1[0] - c0[0] == REPEATS * calls["b_posterior_fused"] and c1[1] == c0[1], (c0, c1)   # one chunk per call
        assert l1[0] == l0[0] and l1[1] > l0[1], (l0, l1)
        rk = dict(variants={}, layerwise_chunks_per_call=(l1[1] - l0[1]) // (REPEATS * calls["c_posterior_layerwise"]))
        for name, ts in times.items():
            us = [t * 1e6 for t in ts]
            rk["variants"][name] = dict(calls_per_repeat=calls[name], us_per_call=[round(v, 1) for v in us],
                                        median_us=round(statistics.median(us), 1),
                                        spread_us=round(max(us) - min(us), 1))
        v = {n: d["median_us"] for n, d in rk["variants"].items()}
        rk["b_over_a"] = round(v["b_posterior_fused"] / v["a_nll"], 4)
        rk["b1_over_a"] = round(v["b1_weights_only_fused"] / v["a_nll"], 4)
        rk["second_pass_over_a"] = round((v["b_posterior_fused"] - v["b1_weights_only_fused"]) / v["a_nll"], 4)
        rk["c_over_a"] = round(v["c_posterior_layerwise"] / v["a_nll"], 4)
        rec_out["k"][str(k)] = rk
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(rec_out, open(out_path, "w"), indent=1)
    print(json.dumps(rec_out))


if __name__ == "__main__":
    main()
