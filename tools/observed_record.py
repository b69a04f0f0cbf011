"""Pixel-mask record: on the configs[1] architecture
(784-200-200-100-100-50), N = 100 images, k = 50 and k = 5000, standard-normal
latents, half the pixels observed (Bernoulli(0.5) per pixel), the time of

(a) iwae_score_grad_masked against iwae_score_grad at this commit, (-1, 1, 1)
    with all three values, on the automatic path and under
    kernel_path="layerwise", the arms alternating in one process; and the staging
    launch's own share, by difference: a log p(h)-only scoring call with the
    images and the mask given (the staging launch and the small kernel) minus the
    same call without images (the small kernel alone), over the masked gradient
    call; the unmasked call's copy is measured the same way;

(b) with --parent-tree DIR (a built checkout of the parent commit): the unmasked
    iwae_score_grad under (0, 1, 1), gradients only, and one iwae_ais transition
    (init q, 10 leapfrogs, injected noise) at the parent commit and at this one.
    Each repeat is a fresh process importing the package of its tree; the two
    trees alternate, PARENT_REPEATS repeats each.  The record says whether this
    commit's median lies inside the min-max spread of the parent's repeats.

Each figure brackets at least 0.2 s of enqueued work with events on the model's
stream, after a warm-up; five repeats in (a), nine in (b), median and spread.  Writes one JSON record.
    python tools/observed_record.py [out.json] [--parent-tree DIR]"""
import ctypes
import json
import os
import statistics
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
HE, HD, LE, LD = [200, 100], [100, 200], [100, 50], [100, 784]
N, KS, REPEATS, MIN_SECONDS = 100, (50, 5000), 5, 0.2
PARENT_REPEATS = 9                # part (b): processes per tree (the parent's min-max spread is the yardstick)
AIS_LEAPFROG = 10


def timed(m, fn, calls):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(m._stream)
    for _ in range(calls):
        fn()
    e1.record(m._stream)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def calibrate(m, fn):
    """Warm-up, then the call count that fills MIN_SECONDS."""
    for _ in range(2):
        fn()
    m._stream.synchronize()
    t = timed(m, fn, 3) / 3
    n1 = max(3, int(0.25 * MIN_SECONDS / t) + 1)            # a longer look: the first calls run slow
    t = timed(m, fn, n1) / n1
    return max(3, int(MIN_SECONDS * 1.3 / t) + 1)


def summary(ts, calls):
    us = [t * 1e6 for t in ts]
    return dict(calls_per_repeat=calls, us_per_call=[round(v, 1) for v in us], median_us=round(statistics.median(us), 1),
                min_us=round(min(us), 1), max_us=round(max(us), 1))


def setup(tree, kernel_path=None):
    sys.path.insert(0, tree)
    import torch
    from iwae_replication_project_amd import Flexible_Model, _lib
    rng = np.random.default_rng(0)
    mean = rng.uniform(0.02, 0.4, 784)
    kw = {} if kernel_path is None else dict(kernel_path=kernel_path)
    m = Flexible_Model(HE, HD, LE, LD, dataset_bias=mean, loss_function="IWAE", k=50, seed=1, **kw)
    x = torch.from_numpy((rng.random((N, 784)) < mean).astype(np.float32)).to(m.device)
    mask = torch.from_numpy((rng.random((N, 784)) < 0.5).astype(np.float32)).to(m.device)
    return torch, _lib, m, x, mask


def buffers(torch, _lib, m, k):
    gen = torch.Generator(device=m.device).manual_seed(k)
    lat = [torch.randn(k, N, d, device=m.device, generator=gen) for d in LE]
    grads = [torch.empty_like(t) for t in lat]
    terms = [torch.empty(N, k, device=m.device) for _ in range(3)]
    torch.cuda.synchronize()
    return lat, grads, terms


# ------------------------------------------------------------------ part (a)
def masked_against_unmasked(tree):
    torch, _lib, auto, x, mask = setup(tree)
    layer = setup(tree, "layerwise")[2]
    layer.set_weights(auto.get_weights())
    out = {}
    P = _lib.fptr

    def counts(m):
        return [int(m._lib.iwae_debug_count(m._h, i)) for i in (25, 26, 33, 34)]

    for k in KS:
        lat, grads, terms = buffers(torch, _lib, auto, k)
        arr, n = _lib.fptr_array(lat)
        garr, ng = _lib.fptr_array(grads)
        q, ph, px = [P(t) for t in terms]
        c = (ctypes.c_float * 3)(-1.0, 1.0, 1.0)

        def plain(m):
            m._call(m._lib.iwae_score_grad(m._h, P(x), N, k, 0, arr, n, c, garr, ng, q, ph, px))

        def masked(m):
            m._call(m._lib.iwae_score_grad_masked(m._h, P(x), P(mask), N, k, 0, arr, n, c, garr, ng, q, ph, px))

        def ph_only(m, with_x, with_mask):                  # a scoring call of log p(h) alone
            if with_mask:
                m._call(m._lib.iwae_score_grad_masked(m._h, P(x), P(mask), N, k, 0, arr, n, c, None, 0, None, ph, None))
            else:
                m._call(m._lib.iwae_score_grad(m._h, P(x) if with_x else None, N, k, 0, arr, n, c, None, 0, None, ph, None))

        variants = [("unmasked_fused", auto, lambda: plain(auto)), ("masked_fused", auto, lambda: masked(auto)),
                    ("unmasked_layerwise", layer, lambda: plain(layer)), ("masked_layerwise", layer, lambda: masked(layer)),
                    ("ph_only_no_images", auto, lambda: ph_only(auto, False, False)),
                    ("ph_only_copy", auto, lambda: ph_only(auto, True, False)),
                    ("ph_only_staging", auto, lambda: ph_only(auto, True, True))]
        calls = {name: calibrate(m, fn) for name, m, fn in variants}
        c0 = counts(auto)
        plain(auto)
        masked(auto)
        d = [b - a for a, b in zip(c0, counts(auto))]
        times = {name: [] for name, _, _ in variants}
        for _ in range(REPEATS):
            for name, m, fn in variants:                    # alternating
                s = timed(m, fn, calls[name])
                assert s >= MIN_SECONDS, (name, s)
                times[name].append(s / calls[name])
        for m in (auto, layer):
            m.check_kernel_status()
        rk = dict(variants={name: summary(ts, calls[name]) for name, ts in times.items()},
                  unmasked_path_auto="fused" if d[0] else "layer-wise", masked_path_auto="fused" if d[2] else "layer-wise")
        v = {name: s["median_us"] for name, s in rk["variants"].items()}
        rk["masked_over_unmasked_fused"] = round(v["masked_fused"] / v["unmasked_fused"], 4)
        rk["masked_over_unmasked_layerwise"] = round(v["masked_layerwise"] / v["unmasked_layerwise"], 4)
        rk["staging_us_by_difference"] = round(v["ph_only_staging"] - v["ph_only_no_images"], 1)
        rk["copy_us_by_difference"] = round(v["ph_only_copy"] - v["ph_only_no_images"], 1)
        rk["staging_share_of_masked_fused"] = round(rk["staging_us_by_difference"] / v["masked_fused"], 4)
        rk["staging_share_of_masked_layerwise"] = round(rk["staging_us_by_difference"] / v["masked_layerwise"], 4)
        out[str(k)] = rk
    return out, torch.cuda.get_device_name(auto.device)


# ------------------------------------------------------------------ part (b)
def worker(tree):
    """One repeat in a fresh process on the package of `tree`: {k: {arm: seconds per call}} as JSON."""
    torch, _lib, m, x, _ = setup(tree)
    P = _lib.fptr
    res = {}
    for k in KS:
        lat, grads, _ = buffers(torch, _lib, m, k)
        arr, n = _lib.fptr_array(lat)
        garr, ng = _lib.fptr_array(grads)
        c = (ctypes.c_float * 3)(0.0, 1.0, 1.0)
        state = [t.clone() for t in lat]
        sarr, ns = _lib.fptr_array(state)
        mom = [torch.randn_like(t) for t in lat]
        marr, nm = _lib.fptr_array(mom)
        u = torch.rand(N, k, device=m.device)
        lw = torch.empty(N, k, device=m.device)
        cfg = _lib.IwaeAisConfig(init=1, n_temps=1, n_leapfrog=AIS_LEAPFROG, accumulate=0, step=0.01, adapt_inc=1.0,
                                 adapt_dec=1.0, step_min=1e-4, step_max=1.0)
        betas = np.asarray([0.5, 0.5], np.float32)

        def grad():
            m._call(m._lib.iwae_score_grad(m._h, P(x), N, k, 0, arr, n, c, garr, ng, None, None, None))

        def ais():
            m._call(m._lib.iwae_ais(m._h, P(x), N, k, 0, sarr, ns, ctypes.byref(cfg), betas.ctypes.data_as(_lib.FP), marr, nm,
                                    P(u), None, P(lw), None, None, None))

        rk = {}
        for name, fn in (("score_grad_011", grad), ("ais_transition", ais)):
            calls = calibrate(m, fn)
            s = timed(m, fn, calls)
            assert s >= MIN_SECONDS, (name, s)
            rk[name] = s / calls
        m.check_kernel_status()
        res[str(k)] = rk
    print("RECORD " + json.dumps(res), flush=True)


def against_parent(tree, parent_tree):
    runs = {"parent": [], "this": []}
    for _ in range(PARENT_REPEATS):
        for which, t in (("parent", parent_tree), ("this", tree)):      # alternating, a fresh process each
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", t], check=True, capture_output=True,
                               text=True, timeout=600)
            line = [l for l in p.stdout.splitlines() if l.startswith("RECORD ")][-1]
            runs[which].append(json.loads(line[len("RECORD "):]))
    out = {}
    for k in KS:
        rk = {}
        for arm in ("score_grad_011", "ais_transition"):
            a = summary([r[str(k)][arm] for r in runs["parent"]], None)
            b = summary([r[str(k)][arm] for r in runs["this"]], None)
            for s in (a, b):
                del s["calls_per_repeat"]
            rk[arm] = dict(parent=a, this=b, this_over_parent=round(b["median_us"] / a["median_us"], 4),
                           this_median_inside_parent_spread=bool(a["min_us"] <= b["median_us"] <= a["max_us"]))
        out[str(k)] = rk
    return out


def main():
    args = sys.argv[1:]
    tree = os.path.abspath(os.path.join(HERE, ".."))
    if args[:1] == ["--worker"]:
        return worker(os.path.abspath(args[1]))
    parent = None
    if "--parent-tree" in args:
        i = args.index("--parent-tree")
        parent = os.path.abspath(args[i + 1])
        del args[i:i + 2]
    out_path = args[0] if args else os.path.join("profiles", "observed_record.json")
    a, device = masked_against_unmasked(tree)
    rec = dict(arch="784-200-200-100-100-50", images=N, observed_fraction=0.5, latents="standard normal, [k][N][d]",
               repeats=REPEATS, device=device, masked_against_unmasked=a)
    if parent is not None:
        rec["unmasked_against_parent"] = dict(repeats=PARENT_REPEATS, k=against_parent(tree, parent))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(rec, open(out_path, "w"), indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
