"""Dynamic-binarisation record.

1. Kernel time of iwae_binarize on N = 60000 x 784 grey levels: device events
   around LAUNCHES back-to-back native calls after a warm-up, REPEATS times,
   median and spread, for every combination of
     input   mnist_blob  ~80 % exact zeros, the rest inside a central 16 x 16
                         box of the 28 x 28 image (zeros contiguous, as MNIST's
                         background), ~3 % exact ones
             mnist_iid   the same value histogram, positions independent
             dense       every grey level in (0, 1): Philox on every quad
             zeros       all 0: no quad depends on u
     path    vec (x 16-byte aligned) / scalar (x offset by one float)
     rows    identity (perm NULL) / a random permutation
   on the in-tree library and, if a second library is given (a variant of
   iwae_binarize.hip built with tools/build_variant.sh), on that one too in the
   same run, with the outputs of the two compared bit for bit.  That is how the
   branch around the Philox rounds of quads that do not depend on u was
   measured and dropped: profiles/binarize_skip_ab.json.
   Algorithmic bytes: 4 N 784 read + 8 N of indices (with a perm) + 4 N 784
   written; share of the 6.3 TB/s achievable HBM rate; dense against zeros says
   whether bytes or the Philox ALU work bounds the kernel.
2. Epoch wall time, 2-layer model 784-200-200-100-100-50, B = 100, k = 50,
   IWAE, device noise: (a) data.stochastic_binarize (numpy) + fit, (b)
   fit(binarize=True) on the device-resident grey levels; alternating in one
   process, each epoch ending in fit's synchronize, after one warm-up epoch of
   each.
    python tools/binarize_record.py [out.json] [variant.so]"""
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from iwae_replication_project_amd import Adam, Flexible_Model, _lib, data  # noqa: E402
from iwae_replication_project_amd.flexible_iwae import ctypes_stream  # noqa: E402

HE, HD, LE, LD = [200, 100], [100, 200], [100, 50], [100, 784]
N, XD, LAUNCHES, WARM, REPEATS, EPOCHS = 60000, 784, 20, 3, 5, 3
HBM = 6.3e12


def grey_levels(kind, rng):
    if kind == "zeros":
        return np.zeros((N, XD), np.float32)
    if kind == "dense":
        return rng.uniform(0.01, 0.99, (N, XD)).astype(np.float32)
    box = np.zeros((28, 28), bool)
    box[6:22, 6:22] = True                                   # 256 of 784 pixels
    inside = np.flatnonzero(box.reshape(-1))
    x = np.zeros((N, XD), np.float32)
    v = rng.random((N, inside.size)).astype(np.float32)
    v[rng.random(v.shape) < 0.39] = 0.0                      # 256 / 784 * 0.61 = 20 % non-zero
    v[(v > 0) & (rng.random(v.shape) < 0.15)] = 1.0          # 3 % of all pixels exactly 1
    x[:, inside] = v
    if kind == "mnist_iid":
        x = rng.permuted(x, axis=1)
    return x


def raw_handle(lib, stream):
    """A 1-layer handle of `lib` on `stream` (the binarisation reads x_dim, seed and stream only)."""
    cfg = _lib.IwaeConfig()
    cfg.n_stochastic, cfg.x_dim = 1, XD
    cfg.n_hidden_encoder[0], cfg.n_latent_encoder[0] = 8, 4
    cfg.n_hidden_decoder[0], cfg.n_latent_decoder[0] = 8, XD
    h = lib.iwae_create(cfg, torch.cuda.current_device())
    assert h, lib.iwae_create_error()
    assert lib.iwae_set_stream(h, ctypes_stream(stream)) == 0 and lib.iwae_set_seed(h, 1) == 0
    return h


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "binarize_record.json")
    variant = sys.argv[2] if len(sys.argv) > 2 else None
    rng = np.random.default_rng(0)
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.Stream(device=dev)
    libs = {"in_tree": _lib.load()}
    if variant:
        libs["variant"] = _lib.load(variant)
    handles = {name: raw_handle(lib, stream) for name, lib in libs.items()}
    rec = dict(device=torch.cuda.get_device_name(dev), rows=N, x_dim=XD, launches_per_figure=LAUNCHES, repeats=REPEATS,
               hbm_rate_assumed_TBps=HBM / 1e12, kernel={}, variant_library=bool(variant))

    with torch.cuda.stream(stream):
        xbuf = torch.empty(N * XD + 4, device=dev)
        views = {"vec": xbuf[:N * XD].view(N, XD), "scalar": xbuf[1:N * XD + 1].view(N, XD)}
        out = torch.empty(N, XD, device=dev)
        ref = torch.empty(N, XD, device=dev)
        perm = torch.randperm(N, generator=torch.Generator().manual_seed(1)).to(dev)
    assert views["vec"].data_ptr() % 16 == 0 and views["scalar"].data_ptr() % 16 == 4
    pp = ctypes.cast(ctypes.c_void_p(perm.data_ptr()), ctypes.POINTER(ctypes.c_longlong))

    def call(name, xv, p, dst):
        rc = libs[name].iwae_binarize(handles[name], _lib.fptr(xv), N, p, N, None, _lib.fptr(dst), XD)
        assert rc == 0, libs[name].iwae_last_error(handles[name])

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(LAUNCHES):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / LAUNCHES          # us per call (the launch and the position's advance)

    for kind in ("mnist_blob", "mnist_iid", "dense", "zeros"):
        x = grey_levels(kind, rng)
        rk = dict(zero_share=round(float((x == 0).mean()), 4), one_share=round(float((x == 1).mean()), 4), arms={})
        for path, xv in views.items():
            with torch.cuda.stream(stream):
                xv.copy_(torch.from_numpy(x))
            for rows, p in (("identity", None), ("perm", pp)):
                nbytes = 8 * N * XD + (8 * N if p else 0)
                for name in libs:
                    for _ in range(WARM):
                        call(name, xv, p, out)
                    stream.synchronize()
                    us = [timed(lambda: call(name, xv, p, out)) for _ in range(REPEATS)]
                    med = statistics.median(us)
                    rk["arms"][f"{name}/{path}/{rows}"] = dict(
                        us_per_call=[round(v, 1) for v in us], median_us=round(med, 1),
                        spread_us=round(max(us) - min(us), 1), algorithmic_bytes=nbytes,
                        TBps=round(nbytes / med / 1e6, 3), share_of_hbm_rate=round(nbytes / (med * 1e-6) / HBM, 3))
                if variant:                                  # same key, same position: the same bits
                    for name, dst in (("in_tree", out), ("variant", ref)):
                        assert libs[name].iwae_set_seed(handles[name], 7) == 0
                        call(name, xv, p, dst)
                    stream.synchronize()
                    assert torch.equal(out, ref), (kind, path, rows)
                    rk["arms"][f"in_tree/{path}/{rows}"]["bits_equal_variant"] = True
        rec["kernel"][kind] = rk
    k = rec["kernel"]
    d, z = k["dense"]["arms"]["in_tree/vec/identity"]["median_us"], k["zeros"]["arms"]["in_tree/vec/identity"]["median_us"]
    rec["dense_over_zeros_vec_identity"] = round(d / z, 3)
    rec["bound"] = ("ALU (Philox rounds) where the grey levels are strictly inside (0, 1), bytes where they are not"
                    if d / z > 1.15 else "bytes")
    counts = {name: int(lib.iwae_debug_count(handles[name], 22)) for name, lib in libs.items()}
    rec["launches_counted"] = counts
    for name, lib in libs.items():
        assert lib.iwae_synchronize(handles[name]) == 0
        lib.iwae_destroy(handles[name])
    del xbuf, views, out, ref

    # ---- epoch wall time
    x = grey_levels("mnist_blob", rng)
    m = Flexible_Model(HE, HD, LE, LD, dataset_bias=None, loss_function="IWAE", k=50, seed=1)
    m.compile(optimizer=Adam(learning_rate=1e-3, epsilon=1e-4))
    xd = m._x(x)
    host_rng = np.random.default_rng(2)

    def host_route():
        t0 = time.perf_counter()
        xs = data.stochastic_binarize(x, host_rng)
        t1 = time.perf_counter()
        m.fit(xs, epochs=1, batch_size=100)
        return time.perf_counter() - t0, t1 - t0

    def device_route():
        t0 = time.perf_counter()
        m.fit(xd, epochs=1, batch_size=100, binarize=True)
        return time.perf_counter() - t0

    host_route(), device_route()                             # warm-up: graph captures, allocator
    ta, tnp, tb = [], [], []
    for _ in range(EPOCHS):
        a, b_np = host_route()
        ta.append(a), tnp.append(b_np)
        tb.append(device_route())
    m.check_kernel_status()
    rec["epoch"] = dict(arch="784-200-200-100-100-50", batch=100, k=50, loss="IWAE", steps_per_epoch=N // 100,
                        a_host_binarize_plus_fit_s=[round(v, 4) for v in ta],
                        a_numpy_draw_alone_s=[round(v, 4) for v in tnp],
                        b_fit_binarize_s=[round(v, 4) for v in tb],
                        a_median_s=round(statistics.median(ta), 4), b_median_s=round(statistics.median(tb), 4),
                        b_over_a=round(statistics.median(tb) / statistics.median(ta), 4))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(rec, open(out_path, "w"), indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
