"""TVO record: on configs[1] (2L 784-200-200-100-100-50, k = 50,
batch 20, device noise) the time per step of
  tvo_step over the partitions P1 = [0, 1], P5 = tvo_schedule(5) and P64 (65
  equal steps) on the fused row-block kernels
  beside wake_sleep_step(1, 0) and an IWAE train_step forced to the same path,
every variant enqueued call by call without a host synchronize and without
graphs (the TVO step is not captured, so the others are not either: the same
launch-by-launch mode on the same build).  The variants alternate in one
process; each figure brackets at least 0.2 s of enqueued work with events on
the model's stream after a warm-up; five repeats, median and spread, clocks as
found.
    python tools/tvo_record.py [out.json]
    python tools/tvo_record.py --loop P5 2000          # one partition alone, for a kernel trace
    python tools/tvo_record.py --kernel-stats kernel_stats.csv P5 [out.json]
                                                       # tvo_kernel's own time from that trace into the record"""
import csv
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from iwae_replication_project_amd import Adam, Flexible_Model, tvo_schedule  # noqa: E402

B, K, REPEATS, MIN_SECONDS = 20, 50, 5, 0.2
IDS = (2, 36, 42, 43)        # engine launches, GM_FIT row-block jobs, TVO calls, tvo_kernel launches
PARTS = {"P1": tvo_schedule(1), "P5": tvo_schedule(5), "P64": np.linspace(0.0, 1.0, 65).astype(np.float32)}
VARIANTS = [("tvo_P1", "P1"), ("tvo_P5", "P5"), ("tvo_P64", "P64"), ("ws_wake", None), ("iwae", None)]
DEFAULT_OUT = os.path.join("profiles", "tvo_record.json")


def make(name, part, x, pi):
    m = Flexible_Model(bench.HE, bench.HD, bench.LE, bench.LD, dataset_bias=pi, loss_function="IWAE", k=K, seed=1,
                       use_graphs=False, kernel_path="fused")
    m.compile(Adam(learning_rate=1e-3, epsilon=1e-4))
    xd = m._x(x)
    if part is not None:
        bt = PARTS[part]
        return m, lambda: m.tvo_step(xd, betas=bt, sync=False)
    if name == "ws_wake":
        return m, lambda: m.wake_sleep_step(xd, 1.0, 0.0, sync=False)
    return m, lambda: m.train_step(xd, sync=False)


def timed(m, fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(m._stream)
    for _ in range(calls):
        fn()
    e1.record(m._stream)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def loop(part, n):
    x, pi = bench.synthetic_images(B, 1)
    m, fn = make("tvo_" + part, part, x, pi)
    for _ in range(n):
        fn()
    m._stream.synchronize()
    m.check_kernel_status()


def kernel_stats(path, part, out_path):
    rec = json.load(open(out_path))
    for row in csv.DictReader(open(path)):
        if "tvo_kernel" in row["Name"]:
            rec.setdefault("tvo_kernel_us", {})[part] = dict(
                calls=int(row["Calls"]), average_us=round(float(row["AverageNs"]) * 1e-3, 3),
                min_us=round(float(row["MinNs"]) * 1e-3, 3), max_us=round(float(row["MaxNs"]) * 1e-3, 3),
                source="rocprofv3 --kernel-trace --stats, a run of its own (tvo_record.py --loop)")
    json.dump(rec, open(out_path, "w"), indent=1)
    print(json.dumps(rec.get("tvo_kernel_us", {})))


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else DEFAULT_OUT
    x, pi = bench.synthetic_images(B, 1)
    models, fns = {}, {}
    for name, part in VARIANTS:
        models[name], fns[name] = make(name, part, x, pi)
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
    rec = dict(arch="784-200-200-100-100-50", batch=B, k=K, noise="device (Philox)", graphs=False,
               kernel_path="fused", repeats=REPEATS, device=torch.cuda.get_device_name(models["iwae"].device),
               partitions={p: [round(float(v), 6) for v in b] if len(b) <= 6 else f"{len(b)} equal steps" for p, b in PARTS.items()},
               variants={})
    for name, m in models.items():
        m.check_kernel_status()
        adv = [int(m._lib.iwae_debug_count(m._h, i)) - c for i, c in zip(IDS, counters[name])]
        us = [t * 1e6 for t in times[name]]
        rec["variants"][name] = dict(engine_launches=adv[0], fit_jobs=adv[1], tvo_calls=adv[2], tvo_launches=adv[3],
                                     calls_per_repeat=calls[name], us_per_step=[round(u, 2) for u in us],
                                     median_us=round(statistics.median(us), 2), spread_us=round(max(us) - min(us), 2))
        assert adv[0] == 0, name
    for name, part in VARIANTS:
        v = rec["variants"][name]
        assert (v["tvo_calls"] > 0 and v["tvo_calls"] == v["tvo_launches"]) == (part is not None), name
    med = {n: v["median_us"] for n, v in rec["variants"].items()}
    rec["ratios"] = {f"{a}_over_{b}": round(med[a] / med[b], 3)
                     for a in ("tvo_P1", "tvo_P5", "tvo_P64") for b in ("ws_wake", "iwae")}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(rec, open(out_path, "w"), indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--loop":
        loop(sys.argv[2], int(sys.argv[3]))
    elif len(sys.argv) > 1 and sys.argv[1] == "--kernel-stats":
        kernel_stats(sys.argv[2], sys.argv[3], sys.argv[4] if len(sys.argv) > 4 else DEFAULT_OUT)
    else:
        main()
