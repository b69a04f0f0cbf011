"""Bitwise record of the train step's routes (a recorder, not a test): for each
row of ROWS a fresh model with a fixed seed runs three steps on fixed x with
injected noise (eager launches), then three with device noise (Philox from the
model's seed: captured graphs where the row has them on), and the row's record
is the SHA-256 of the losses, weights, gradients, Adam m / v and the Adam step,
plus what the steps added to iwae_debug_count ids 0-16.  The rows reach every
way a train step ends ("How a train step ends") and every mode
of the update and Adam launches at small shapes: where a route needs more than
upd_rows sample rows the knob is lowered instead of the batch raised.  Routes
differ in rounding, so equal digests from two builds of the library mean every
row still takes the same route with the same arguments.
    IWAE_HIP_LIB=<lib.so> python tools/step_digest.py out.json
    python tools/step_digest.py --compare parent.json new.json profiles/update_tail_digests.json
(--compare writes both records side by side and exits 1 on any difference.)"""
import ctypes
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ARCH2 = ([200, 100], [100, 200], [100, 50], [100, 784])      # tests/test_gpu_state.py
ARCH1 = ([200], [200], [50], [784])
BEYOND = {"upd_rows": 512}                                   # B = 20, k = 50: 1,000 sample rows
RING = {"upd_rows": 512, "nring_train_rows": 512}            # B = 40 (above the few-row launches): 2,000 rows
PIWAE = dict(loss="PIWAE", k=64, kw=dict(k1=8, k2=8))

# name -> B, k, and optionally arch, loss, kw (model arguments), tune, dp, mode
ROWS = {
    "01_b20_k50_combined_launch": dict(B=20, k=50),
    "02_b20_k5_two_launches": dict(B=20, k=5),
    "03_b7_k64_ragged": dict(B=7, k=64),
    "03b_b40_k50_image_row_forward": dict(B=40, k=50),
    "03c_b20_k50_one_layer": dict(B=20, k=50, arch=ARCH1),
    "03d_b20_k50_tcu_off": dict(B=20, k=50, tune={"tcu": 0}),
    "04_graphs_off": dict(B=20, k=50, kw=dict(use_graphs=False)),
    "04b_train_steps_multi_step_graph": dict(B=20, k=50, mode="train_steps"),
    "05_forward_backward": dict(B=20, k=50, mode="forward_backward"),
    "05b_forward_backward_beyond_upd_rows": dict(B=20, k=50, mode="forward_backward", tune=BEYOND),
    "06_piwae_one_1": dict(B=20, tune={"piwae_one": 1}, **PIWAE),
    "07_piwae_one_0": dict(B=20, tune={"piwae_one": 0}, **PIWAE),
    "07b_piwae_one_layer": dict(B=20, arch=ARCH1, **PIWAE),
    "07c_piwae_dw_kernel": dict(B=20, tune=dict(BEYOND, dw_wide=1), **PIWAE),
    "07d_piwae_slab_pass": dict(B=20, tune=dict(BEYOND, dw_wide=0), **PIWAE),
    "07e_piwae_grouped_gemms": dict(B=20, tune={"upd": 0, "upd_slabs": 0}, **PIWAE),
    "08_beyond_upd_rows_dw_wide_1": dict(B=20, k=50, tune=dict(BEYOND, dw_wide=1)),
    "09_beyond_upd_rows_dw_wide_0": dict(B=20, k=50, tune=dict(BEYOND, dw_wide=0)),
    "10_beyond_upd_rows_upd_apply_0": dict(B=20, k=50, tune=dict(BEYOND, upd_apply=0)),
    "10b_ring_forward": dict(B=40, k=50, tune=RING),
    # (the bound as a launch of its own, as beyond 64 images: the ring kernels run the backward)
    "10c_ring_forward_nring_bwd_2": dict(B=40, k=50, tune=dict(RING, tc_bound=0, nring_bwd=2)),
    "10d_ring_forward_nring_bwd_3": dict(B=40, k=50, tune=dict(RING, tc_bound=0, nring_bwd=3)),
    "10e_beyond_upd_rows_one_layer": dict(B=20, k=50, arch=ARCH1, tune=BEYOND),
    "11_grouped_gemms_adam_fx": dict(B=20, k=50, tune={"upd": 0, "upd_slabs": 0}),
    "12_kernel_path_layerwise": dict(B=20, k=50, kw=dict(kernel_path="layerwise")),
    "13_kernel_path_fused": dict(B=20, k=50, kw=dict(kernel_path="fused")),
    "14_kernel_path_fused_piwae": dict(B=20, kw=dict(kernel_path="fused", k1=8, k2=8), loss="PIWAE", k=64),
    "14b_kernel_path_layerwise_piwae": dict(B=20, kw=dict(kernel_path="layerwise", k1=8, k2=8), loss="PIWAE", k=64),
    "15_library_comm_bucketed_fused_update": dict(B=20, k=50, dp="library"),
    "15b_library_comm_train_steps": dict(B=20, k=50, dp="library", mode="train_steps"),
    "16_library_comm_beyond_upd_rows": dict(B=20, k=50, dp="library", tune=BEYOND),
    "16b_library_comm_slab_pass": dict(B=20, k=50, dp="library", tune=dict(BEYOND, dw_wide=0)),
    "16c_library_comm_adam_launch": dict(B=20, k=50, dp="library", tune={"upd": 0, "upd_slabs": 0}),
    "16d_library_comm_kernel_path_fused": dict(B=20, k=50, dp="library", kw=dict(kernel_path="fused")),
    "17_caller_reduced_forward_backward_apply_adam": dict(B=20, k=50, dp="torch"),
    "17b_caller_reduced_beyond_upd_rows": dict(B=20, k=50, dp="torch", tune=BEYOND),
    # (one rank of a claimed world of two, nothing reduced: B_local * g over the B_local in the buffer's tail)
    "17c_caller_reduced_weighted": dict(B=20, k=50, dp="weighted", mode="apply_adam_0"),
    "17d_caller_reduced_weighted_beyond_upd_rows": dict(B=20, k=50, dp="weighted", mode="apply_adam_0", tune=BEYOND),
    "17e_caller_reduced_weighted_adam_launch": dict(B=20, k=50, dp="weighted", mode="apply_adam_0",
                                                    tune={"upd": 0, "upd_slabs": 0}),
    "18_iwae_stl": dict(B=20, k=50, loss="IWAE_STL"),
    # live profiling (bench.py --full): the replays run on scratch copies, the model's state must not move
    "19_profile_adam_launch": dict(B=20, k=50, tune={"upd": 0, "upd_slabs": 0}, mode="profile_12"),
    "19b_profile_update_launch": dict(B=20, k=50, tune={"tcu": 0}, mode="profile_15"),
    "19c_profile_combined_launch": dict(B=20, k=50, mode="profile_16"),
}
STEPS = 3


def run_row(spec):
    import torch
    from iwae_replication_project_amd import Adam, Flexible_Model
    from iwae_replication_project_amd import distributed as D
    arch, loss, B, k = spec.get("arch", ARCH2), spec.get("loss", "IWAE"), spec["B"], spec["k"]
    mode = spec.get("mode", "train_step")
    rng = np.random.default_rng(67)
    x = (rng.random((4 * B, 784)) < 0.2).astype(np.float32)
    eps = [[rng.standard_normal((k, B, d)).astype(np.float32) for d in arch[2]] for _ in range(STEPS)]
    t0 = time.perf_counter()
    m = Flexible_Model(*arch, dataset_bias=None, loss_function=loss, k=k, seed=13, tuning=spec.get("tune"),
                       **spec.get("kw", {}))
    m.compile(Adam(learning_rate=1e-3, epsilon=1e-4))
    lib, h = m._lib, m._h
    if spec.get("dp") == "weighted":
        from iwae_replication_project_amd import _lib
        m._call(lib.iwae_dp_init(h, 0, 2, None))
        g, n = _lib.FP(), ctypes.c_longlong(0)
        m._call(lib.iwae_grad_buffer(h, ctypes.byref(g), ctypes.byref(n)))
        with torch.cuda.stream(m._stream):
            gbuf = torch.zeros(int(n.value) + 4, device=m.device)     # the gradient + the batch-size tail
        m._call(lib.iwae_bind_grad_buffer(h, _lib.fptr(gbuf), gbuf.numel()))
    elif spec.get("dp"):
        D.enable_data_parallel(m, comm=spec["dp"])
    c0 = [int(lib.iwae_debug_count(h, i)) for i in range(17)]
    losses, extra = [], {}

    def step(e):
        if mode in ("forward_backward", "apply_adam_0"):
            xd = m._x(x[:B])
            lc = m._lc()
            arr, n, keep = m._eps(e, B, lc.k)
            m._forward_backward(lc, xd, B, arr, n)
            if mode == "apply_adam_0":
                m._apply_adam(0.0)
            m._stream.synchronize()
            return float(m._loss_buf.item())
        return m.train_step(x[:B], eps=e)[loss]

    if mode == "train_steps":
        losses += [float(v) for v in m.train_steps(x, B)]
        losses += [float(v) for v in m.train_steps(x, B)]
    elif mode.startswith("profile_"):
        m._call(lib.iwae_profile_gemm(h, int(mode.split("_")[1]), 0))
        losses.append(step(None))
        ms, fl = ctypes.c_double(), ctypes.c_double()
        extra["replay_rc"] = int(lib.iwae_profile_replay(h, 2, ctypes.byref(ms), ctypes.byref(fl)))
        m._call(lib.iwae_profile_gemm(h, -1, -1))
        losses.append(step(None))
    else:
        losses += [step(eps[s]) for s in range(STEPS)]
        losses += [step(None) for _ in range(STEPS)]
    m.check_kernel_status()
    torch.cuda.synchronize()
    am, av, astep = m.get_optimizer_state()
    sha = hashlib.sha256()
    for a in [np.asarray(losses, np.float32)] + m.get_weights() + m.get_gradients() + [am, av]:
        sha.update(np.ascontiguousarray(a, np.float32).tobytes())
    sha.update(str(astep).encode())
    counters = [int(lib.iwae_debug_count(h, i)) - c for i, c in enumerate(c0)]
    return dict(sha256=sha.hexdigest(), adam_step=astep, loss_first=repr(losses[0]), loss_last=repr(losses[-1]),
                counters=counters, seconds=round(time.perf_counter() - t0, 3), **extra)


def compare(a_path, b_path, out_path):
    a, b = json.load(open(a_path)), json.load(open(b_path))
    keys = ("sha256", "adam_step", "counters", "replay_rc")
    differ = [r for r in sorted(set(a["rows"]) | set(b["rows"]))
              if any(a["rows"].get(r, {}).get(k) != b["rows"].get(r, {}).get(k) for k in keys)]
    rec = dict(what="tools/step_digest.py: two builds of the library, same rows, run in one GPU visit",
               equal=not differ, differing_rows=differ, parent=a, new=b)
    json.dump(rec, open(out_path, "w"), indent=1)
    print(f"[step_digest] {len(a['rows'])} / {len(b['rows'])} rows, differing: {differ or 'none'}")
    return 1 if differ else 0


def main():
    if sys.argv[1] == "--compare":
        sys.exit(compare(*sys.argv[2:5]))
    import torch
    from iwae_replication_project_amd import _lib
    _lib.load()
    rec = dict(library=os.path.basename(os.environ.get("IWAE_HIP_LIB", "libiwae_hip.so")),
               device=torch.cuda.get_device_name(0), steps_per_noise=STEPS, rows={})
    only = os.environ.get("ROWS")
    for name, spec in ROWS.items():
        if only and not any(name.startswith(p) for p in only.split(",")):
            continue
        rec["rows"][name] = run_row(spec)
        print(name, json.dumps(rec["rows"][name]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    json.dump(rec, open(sys.argv[1], "w"), indent=1)


if __name__ == "__main__":
    main()
