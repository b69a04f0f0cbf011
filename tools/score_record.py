"""Scoring record: on the configs[1] architecture
(784-200-200-100-100-50), N = 100 images, k = 50 and k = 5000, the time of
  (a) iwae_nll_eps on injected noise with IWAE_KNOB_NRING = 0: mega_fwd_kernel on
      the same rows, the yardstick (code this feature does not change),
  (b) iwae_score, all three terms, fused (score_kernel),
  (c) iwae_score, log_ph alone (the prior chain only),
  (d) iwae_score, all three terms, through the layer-wise fallback
      (kernel_path="layerwise"),
the arms alternating in one process.  Each figure brackets at least 0.2 s of
enqueued work with events on the model's stream (the native calls, without the
facade's per-call synchronize), after a warm-up; five repeats, median and
spread.  Writes one JSON record.
    python tools/score_record.py [out.json]"""
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
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "score_record.json")
    rng = np.random.default_rng(0)
    mean = rng.uniform(0.02, 0.4, 784)
    fused = Flexible_Model(HE, HD, LE, LD, dataset_bias=mean, loss_function="IWAE", k=50, seed=1, tuning={"nring": 0})
    layer = Flexible_Model(HE, HD, LE, LD, dataset_bias=mean, loss_function="IWAE", k=50, seed=1,
                           kernel_path="layerwise")
    layer.set_weights(fused.get_weights())
    x = torch.from_numpy((rng.random((N, 784)) < mean).astype(np.float32)).to(fused.device)
    rec_out = dict(arch="784-200-200-100-100-50", images=N, latents="standard normal, [k][N][d]", repeats=REPEATS,
                   device=torch.cuda.get_device_name(fused.device), k={})

    def timed(m, fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(m._stream)
        for _ in range(calls):
            fn()
        e1.record(m._stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    def count(m, i):
        return int(m._lib.iwae_debug_count(m._h, i))

    for k in KS:
        gen = torch.Generator(device=fused.device).manual_seed(k)
        lat = [torch.randn(k, N, d, device=fused.device, generator=gen) for d in LE]
        terms = [torch.empty(N, k, device=fused.device) for _ in range(3)]
        lpx = torch.empty(N, device=fused.device)
        torch.cuda.synchronize()
        arr, n = _lib.fptr_array(lat)

        def nll_eps():
            fused._call(fused._lib.iwae_nll_eps(fused._h, _lib.fptr(x), N, k, arr, n, _lib.fptr(lpx)))

        def score(m, all_terms):
            q, ph, px = [_lib.fptr(t) for t in terms]
            m._call(m._lib.iwae_score(m._h, _lib.fptr(x) if all_terms else None, N, k, 0, arr, n,
                                      q if all_terms else None, ph, px if all_terms else None, None, 0))

        variants = [("a_nll_eps_mega", fused, nll_eps),
                    ("b_score_fused", fused, lambda: score(fused, True)),
                    ("c_score_log_ph_fused", fused, lambda: score(fused, False)),
                    ("d_score_layerwise", layer, lambda: score(layer, True))]
        calls = {}
        for name, m, fn in variants:               # warm-up, then the call count that fills MIN_SECONDS
            for _ in range(2):
                fn()
            m._stream.synchronize()
            t = timed(m, fn, 3) / 3
            n1 = max(3, int(0.25 * MIN_SECONDS / t) + 1)        # a longer look: the first calls run slow
            t = timed(m, fn, n1) / n1
            calls[name] = max(3, int(MIN_SECONDS * 1.3 / t) + 1)
        c0 = [count(fused, i) for i in (0, 3, 23, 24)]
        l0 = [count(layer, i) for i in (23, 24)]
        times = {name: [] for name, _, _ in variants}
        for _ in range(REPEATS):
            for name, m, fn in variants:           # alternating
                s = timed(m, fn, calls[name])
                assert s >= MIN_SECONDS, (name, s)
                times[name].append(s / calls[name])
        for m in (fused, layer):
            m.check_kernel_status()
        c1 = [count(fused, i) for i in (0, 3, 23, 24)]
        l1 = [count(layer, i) for i in (23, 24)]
        assert c1[0] - c0[0] == REPEATS * calls["a_nll_eps_mega"] and c1[1] == c0[1], (c0, c1)   # mega_fwd_kernel, no ring
        assert c1[2] - c0[2] == REPEATS * (calls["b_score_fused"] + calls["c_score_log_ph_fused"]) and c1[3] == c0[3]
        assert l1[0] == l0[0] and l1[1] - l0[1] == REPEATS * calls["d_score_layerwise"], (l0, l1)
        rk = dict(variants={})
        for name, ts in times.items():
            us = [t * 1e6 for t in ts]
            rk["variants"][name] = dict(calls_per_repeat=calls[name], us_per_call=[round(v, 1) for v in us],
                                        median_us=round(statistics.median(us), 1),
                                        spread_us=round(max(us) - min(us), 1))
        v = {n: d["median_us"] for n, d in rk["variants"].items()}
        rk["b_over_a"] = round(v["b_score_fused"] / v["a_nll_eps_mega"], 4)
        rk["c_over_a"] = round(v["c_score_log_ph_fused"] / v["a_nll_eps_mega"], 4)
        rk["d_over_a"] = round(v["d_score_layerwise"] / v["a_nll_eps_mega"], 4)
        rec_out["k"][str(k)] = rk
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(rec_out, open(out_path, "w"), indent=1)
    print(json.dumps(rec_out))


if __name__ == "__main__":
    main()
