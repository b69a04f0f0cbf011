"""Generation record: on the configs[1] architecture
(784-200-200-100-100-50) and n = 10,000 rows with device noise, the time of
  (a) Flexible_Model.sample on the fused gen_kernel,
  (b) the same through the layer-wise fallback (kernel_path="layerwise"),
  (c) reconstructed_x_probs on 10,000 images (the existing layer-wise path: an
      encoder pass and a BCE pass on top of the same decoder chain),
the three alternating in one process.  Each figure brackets at least 0.2 s of
enqueued work with events on the model's stream (the native calls, without the
facade's per-call synchronize), after a warm-up; five repeats, median and
spread.  Writes one JSON record.
    python tools/gen_record.py [out.json]"""
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from iwae_replication_project_amd import Flexible_Model, _lib  # noqa: E402

HE, HD, LE, LD = [200, 100], [100, 200], [100, 50], [100, 784]
N, REPEATS, MIN_SECONDS = 10000, 5, 0.2


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "gen_record.json")
    rng = np.random.default_rng(0)
    mean = rng.uniform(0.02, 0.4, 784)
    models = {p: Flexible_Model(HE, HD, LE, LD, dataset_bias=mean, loss_function="IWAE", k=50, seed=1, kernel_path=p)
              for p in ("auto", "layerwise")}
    models["layerwise"].set_weights(models["auto"].get_weights())
    fused, layer = models["auto"], models["layerwise"]
    x = torch.from_numpy((rng.random((N, 784)) < mean).astype(np.float32)).to(fused.device)
    bufs = {}
    for name, m in models.items():
        with torch.cuda.stream(m._stream):
            bufs[name] = (torch.empty(N, 784, device=m.device), torch.empty(N, 784, device=m.device),
                          torch.empty(1, device=m.device))
    torch.cuda.synchronize()

    def gen(m, name):
        probs, pixels, _ = bufs[name]
        m._call(m._lib.iwae_generate(m._h, N, None, None, 0, None, _lib.fptr(probs), 784, _lib.fptr(pixels), 784,
                                     None, 0))

    def rec(m, name):
        probs, _, loss = bufs[name]
        m._call(m._lib.iwae_reconstruct(m._h, _lib.fptr(x), N, None, 0, _lib.fptr(probs), 784, _lib.fptr(loss)))

    variants = [("a_fused_sample", fused, lambda: gen(fused, "auto")),
                ("b_layerwise_sample", layer, lambda: gen(layer, "layerwise")),
                ("c_reconstructed_x_probs", fused, lambda: rec(fused, "auto"))]

    def timed(m, fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(m._stream)
        for _ in range(calls):
            fn()
        e1.record(m._stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    calls = {}
    for name, m, fn in variants:                   # warm-up, then the call count that fills MIN_SECONDS
        for _ in range(3):
            fn()
        m._stream.synchronize()
        t = timed(m, fn, 20) / 20
        calls[name] = max(20, int(MIN_SECONDS * 1.1 / t) + 1)
    c0 = int(fused._lib.iwae_debug_count(fused._h, 10))
    times = {name: [] for name, _, _ in variants}
    for _ in range(REPEATS):
        for name, m, fn in variants:               # alternating
            s = timed(m, fn, calls[name])
            assert s >= MIN_SECONDS, (name, s)
            times[name].append(s / calls[name])
    for m in models.values():
        m.check_kernel_status()
    assert int(fused._lib.iwae_debug_count(fused._h, 10)) - c0 == REPEATS * calls["a_fused_sample"]
    assert int(layer._lib.iwae_debug_count(layer._h, 10)) == 0
    rec_out = dict(arch="784-200-200-100-100-50", rows=N, noise="device (Philox)", repeats=REPEATS,
                   device=torch.cuda.get_device_name(fused.device), variants={})
    for name, ts in times.items():
        us = [t * 1e6 for t in ts]
        rec_out["variants"][name] = dict(calls_per_repeat=calls[name], us_per_call=[round(v, 2) for v in us],
                                         median_us=round(statistics.median(us), 2),
                                         spread_us=round(max(us) - min(us), 2),
                                         rows_per_s=round(N / statistics.median(ts)))
    v = rec_out["variants"]
    rec_out["fused_over_reconstruct"] = round(v["a_fused_sample"]["median_us"] / v["c_reconstructed_x_probs"]["median_us"], 4)
    rec_out["fused_no_slower_than_reconstruct"] = v["a_fused_sample"]["median_us"] <= v["c_reconstructed_x_probs"]["median_us"]
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(rec_out, open(out_path, "w"), indent=1)
    print(json.dumps(rec_out))


if __name__ == "__main__":
    main()
