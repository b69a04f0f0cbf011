"""Wake-sleep record: on configs[1] (2L 784-200-200-100-100-50,
k = 50, batch 20, 20 dreams of the step's own, device noise) the time per step of
  wake_sleep_step at (1, 0), (0, 1) and (0.5, 0.5) on the fused row-block kernels
  beside an IWAE_DREG and an IWAE train_step forced to the same path,
every variant enqueued call by call without a host synchronize and without
graphs (the wake-sleep step is not captured, so the train steps are not either:
the same launch-by-launch mode on the same build).  The variants alternate in
one process; each figure brackets at least 0.2 s of enqueued work with events
on the model's stream after a warm-up; five repeats, median and spread, clocks
as found.
    python tools/wakesleep_record.py [out.json]"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from iwae_replication_project_amd import Adam, Flexible_Model  # noqa: E402

B, K, N_DREAM, REPEATS, MIN_SECONDS = 20, 50, 20, 5, 0.2
IDS = (2, 36, 38)        # engine launches, GM_FIT row-block jobs, own dream generations
VARIANTS = [("ws_wake", "IWAE", (1.0, 0.0)),
            ("ws_sleep", "IWAE", (0.0, 1.0)),
            ("ws_mix", "IWAE", (0.5, 0.5)),
            ("iwae_dreg", "IWAE_DREG", None),
            ("iwae", "IWAE", None)]


def timed(m, fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(m._stream)
    for _ in range(calls):
        fn()
    e1.record(m._stream)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "wakesleep_record.json")
    x, pi = bench.synthetic_images(B, 1)
    models, fns = {}, {}
    for name, loss, coef in VARIANTS:
        m = Flexible_Model(bench.HE, bench.HD, bench.LE, bench.LD, dataset_bias=pi, loss_function=loss, k=K, seed=1,
                           use_graphs=False, kernel_path="fused")
        m.compile(Adam(learning_rate=1e-3, epsilon=1e-4))
        xd = m._x(x)
        models[name] = m
        if coef is None:
            fns[name] = lambda m=m, xd=xd: m.train_step(xd, sync=False)
        else:
            n = N_DREAM if coef[1] > 0 else None
            fns[name] = lambda m=m, xd=xd, c=coef, n=n: m.wake_sleep_step(xd, c[0], c[1], n_dream=n, sync=False)
    counters = {name: [int(m._lib.iwae_debug_count(m._h, i)) for i in IDS] for name, m in models.items()}
    calls = {}
    for name, m in models.items():                 # warm-up (workspace, code objects), then the call counts
        for _ in range(5):
            fns[name]()
        m._stream.synchronize()
        t = timed(m, fns[name], 10) / 10
        calls[name] = max(10, int(MIN_SECONDS * 1.1 / t) + 1)
    times = {name: [] for name in models}
    for _ in range(REPEATS):
        for name, m in models.items():             # alternating
            s = timed(m, fns[name], calls[name])
            assert s >= MIN_SECONDS, (name, s)
            times[name].append(s / calls[name])
    rec = dict(arch="784-200-200-100-100-50", batch=B, k=K, n_dream=N_DREAM, noise="device (Philox)", graphs=False,
               kernel_path="fused", repeats=REPEATS, device=torch.cuda.get_device_name(models["iwae"].device), variants={})
    for name, m in models.items():
        m.check_kernel_status()
        adv = [int(m._lib.iwae_debug_count(m._h, i)) - c for i, c in zip(IDS, counters[name])]
        us = [t * 1e6 for t in times[name]]
        rec["variants"][name] = dict(loss=m.loss_function, engine_launches=adv[0], fit_jobs=adv[1], own_dreams=adv[2],
                                     calls_per_repeat=calls[name], us_per_step=[round(u, 2) for u in us],
                                     median_us=round(statistics.median(us), 2), spread_us=round(max(us) - min(us), 2))
        assert adv[0] == 0, name
    for name in ("ws_wake", "ws_sleep", "ws_mix"):
        assert rec["variants"][name]["fit_jobs"] > 0, name
    assert rec["variants"]["ws_wake"]["own_dreams"] == 0 and rec["variants"]["ws_mix"]["own_dreams"] > 0
    med = {n: v["median_us"] for n, v in rec["variants"].items()}
    rec["ratios"] = {f"{a}_over_{b}": round(med[a] / med[b], 3)
                     for a in ("ws_wake", "ws_sleep", "ws_mix") for b in ("iwae", "iwae_dreg")}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(rec, open(out_path, "w"), indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
