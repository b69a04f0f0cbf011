"""Path-gradient record: on configs[1] (2L 784-200-200-100-100-50,
k = 50, batch 20, device noise, graphs on) the time per train step of
  IWAE on the default path (the bf16x3 engine), IWAE and PIWAE (k1 = k2: 10 x 5)
  on the fused row-block kernels, IWAE_STL and IWAE_DREG (default path: the
  row-block kernels),
measured two ways: `steps` = train_steps over 32 batches (fit's inner loop; the
engine replays one 32-step graph, the other paths one graph per step) and
`step` = train_step calls without a host synchronize.  The variants alternate
in one process; each figure brackets at least 0.2 s of enqueued work with
events on the model's stream after a warm-up; five repeats, median and spread.
Then the median encoder / decoder gradient SNR of IWAE, IWAE_STL and IWAE_DREG
from get_gradient_snr (R = 1000, k = 64, batch 20, one seed): informational.
    python tools/pathgrad_record.py [out.json]"""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from iwae_replication_project_amd import Adam, Flexible_Model  # noqa: E402

B, K, NB, REPEATS, MIN_SECONDS = 20, 50, 32, 5, 0.2
VARIANTS = [("iwae_engine", "IWAE", {}),
            ("iwae_fused", "IWAE", dict(kernel_path="fused")),
            ("piwae_fused", "PIWAE", dict(kernel_path="fused", k1=10, k2=5)),
            ("iwae_stl", "IWAE_STL", {}),
            ("iwae_dreg", "IWAE_DREG", {})]


def timed(m, fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(m._stream)
    for _ in range(calls):
        fn()
    e1.record(m._stream)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "pathgrad_record.json")
    x, pi = bench.synthetic_images(B * NB, 1)
    models, fns = {}, {}
    for name, loss, kw in VARIANTS:
        m = Flexible_Model(bench.HE, bench.HD, bench.LE, bench.LD, dataset_bias=pi, loss_function=loss, k=K, seed=1,
                           use_graphs=True, **kw)
        m.compile(Adam(learning_rate=1e-3, epsilon=1e-4))
        xd = m._x(x)
        models[name] = m
        fns[name] = {"steps": (lambda m=m, xd=xd: m.train_steps(xd, B, sync=False), NB),
                     "step": (lambda m=m, xd=xd: m.train_step(xd[:B], sync=False), 1)}
    counters = {name: [int(m._lib.iwae_debug_count(m._h, i)) for i in (2, 11)] for name, m in models.items()}
    calls = {}
    for name, m in models.items():                 # warm-up (workspace, captures), then the call counts
        for mode, (fn, per) in fns[name].items():
            for _ in range(3):
                fn()
            m._stream.synchronize()
            t = timed(m, fn, 5) / 5
            calls[name, mode] = max(5, int(MIN_SECONDS * 1.1 / t) + 1)
    times = {key: [] for key in calls}
    for _ in range(REPEATS):
        for name, m in models.items():             # alternating
            for mode, (fn, per) in fns[name].items():
                s = timed(m, fn, calls[name, mode])
                assert s >= MIN_SECONDS, (name, mode, s)
                times[name, mode].append(s / (calls[name, mode] * per))
    rec = dict(arch="784-200-200-100-100-50", batch=B, k=K, noise="device (Philox)", graphs=True, repeats=REPEATS,
               device=torch.cuda.get_device_name(models["iwae_engine"].device), variants={})
    for name, m in models.items():
        m.check_kernel_status()
        adv = [int(m._lib.iwae_debug_count(m._h, i)) - c for i, c in zip((2, 11), counters[name])]
        v = dict(loss=m.loss_function, engine_launches=adv[0], path_gradient_jobs=adv[1])
        for mode in ("steps", "step"):
            us = [t * 1e6 for t in times[name, mode]]
            v[mode] = dict(calls_per_repeat=calls[name, mode], us_per_step=[round(u, 2) for u in us],
                           median_us=round(statistics.median(us), 2), spread_us=round(max(us) - min(us), 2))
        rec["variants"][name] = v
    assert rec["variants"]["iwae_engine"]["engine_launches"] > 0
    for name in ("iwae_fused", "piwae_fused", "iwae_stl", "iwae_dreg"):
        assert rec["variants"][name]["engine_launches"] == 0, name
    for name in ("iwae_stl", "iwae_dreg"):
        assert rec["variants"][name]["path_gradient_jobs"] > 0, name
    med = {n: {mode: v[mode]["median_us"] for mode in ("steps", "step")} for n, v in rec["variants"].items()}
    rec["ratios"] = {mode: dict(stl_over_fused_iwae=round(med["iwae_stl"][mode] / med["iwae_fused"][mode], 3),
                                dreg_over_fused_piwae=round(med["iwae_dreg"][mode] / med["piwae_fused"][mode], 3),
                                stl_over_engine=round(med["iwae_stl"][mode] / med["iwae_engine"][mode], 3),
                                dreg_over_engine=round(med["iwae_dreg"][mode] / med["iwae_engine"][mode], 3))
                     for mode in ("steps", "step")}
    # gradient SNR (informational): R draws at fixed weights, k = 64
    xs = x[:B]
    snr = {}
    for loss in ("IWAE", "IWAE_STL", "IWAE_DREG"):
        m = Flexible_Model(bench.HE, bench.HD, bench.LE, bench.LD, dataset_bias=pi, loss_function=loss, k=64, seed=2)
        s, _ = m.get_gradient_snr(xs, R=1000, seed=7)
        names = [d[0] for d in m.dense for _ in (0, 1)]
        flat = [np.asarray(a).ravel() for a in s]
        enc = np.concatenate([f for f, nm in zip(flat, names) if nm.startswith("enc")])
        dec = np.concatenate([f for f, nm in zip(flat, names) if not nm.startswith("enc")])
        snr[loss] = dict(median_encoder=round(float(np.median(enc[np.isfinite(enc)])), 4),
                         median_decoder=round(float(np.median(dec[np.isfinite(dec)])), 4))
    rec["snr"] = dict(R=1000, k=64, batch=B, seed=7, weights="untrained (glorot, seed 2)", **snr)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(rec, open(out_path, "w"), indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
