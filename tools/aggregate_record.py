"""Aggregate-posterior record: d1 = 50 units, M = 10,000
reference components, R = 10,000 and R = 500,000 query rows (injected loc / scale
/ latents: scales of about e^-1, row r drawn from component r mod M), the time of
  (a) iwae_aggregate, log_q_agg alone (agg_joint_kernel; plain VALU, see below),
  (b) iwae_aggregate, log_q_agg and log_q_dim (agg_joint_kernel + agg_dim_kernel),
  (c) the straightforward torch implementation of (a) on the same device: the
      difference form broadcast over reference chunks sized to 1 GiB of float32
      ([R][chunk][d1]), torch.logsumexp per chunk, merged across chunks by
      torch.logaddexp,
  (d) the same for (b),
the arms alternating in one process.  Before timing, (c) and (d) are checked
against the kernels: max|diff| <= 1e-4 max|value| and, per row, <= 1e-4 d1 (1/2
log 2 pi), a lower bound of the row scale S_r of tests/aggregate_ref.py (so a
stricter bar).  Each figure brackets at least 0.2 s of enqueued work with events
on the model's stream (the native calls, without the facade's synchronize),
after a warm-up; five repeats, median and spread; pairs (r, m) per second and
exp per second (R M joint, R M d1 more per unit) as a share of the device's
transcendental rate, taken as 8 lanes per clock per SIMD (v_exp_f32 issues over
8 cycles per wave) x 4 SIMDs x CUs x 2.4 GHz.  Writes one JSON record.
    python tools/aggregate_record.py [out.json]"""
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from iwae_replication_project_amd import Flexible_Model, _lib  # noqa: E402

D1, M, RS, REPEATS, MIN_SECONDS = 50, 10000, (10000, 500000), 5, 0.2
CHUNK_BYTES = 1 << 30
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
JOINT_SUM = ("VALU: the square of a difference is not a product of a row factor and a reference factor, so the "
             "matrix cores could only serve the expanded form h^2 a - 2 h b + c, which the definition rules out")


def torch_aggregate(h, mu, s, per_unit):
    R, d = h.shape
    mc = max(1, CHUNK_BYTES // 4 // (R * d))
    rs, lc = 1.0 / s, -(torch.log(s) + HALF_LOG_2PI)
    aj = ad = None
    for m0 in range(0, mu.shape[0], mc):
        z = (h[:, None, :] - mu[None, m0:m0 + mc]) * rs[None, m0:m0 + mc]
        t = lc[None, m0:m0 + mc] - 0.5 * z * z
        lj = torch.logsumexp(t.sum(-1), dim=1)
        aj = lj if aj is None else torch.logaddexp(aj, lj)
        if per_unit:
            ld = torch.logsumexp(t, dim=1)
            ad = ld if ad is None else torch.logaddexp(ad, ld)
    logm = math.log(mu.shape[0])
    return aj - logm, (ad - logm if per_unit else None)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "aggregate_record.json")
    m = Flexible_Model([200], [200], [D1], [784], dataset_bias=None, loss_function="IWAE", k=50, seed=1)
    dev = m.device
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    exp_rate = 8 * 4 * n_cu * 2.4e9
    gen = torch.Generator(device=dev).manual_seed(0)
    mu = torch.randn(M, D1, device=dev, generator=gen)
    s = torch.exp(-1.0 + 0.5 * torch.randn(M, D1, device=dev, generator=gen))
    rec = dict(d1=D1, M=M, repeats=REPEATS, device=torch.cuda.get_device_name(dev), compute_units=n_cu,
               exp_per_second_taken_as_peak=exp_rate, joint_sum=JOINT_SUM, torch_chunk_bytes=CHUNK_BYTES, R={})

    def timed(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(m._stream)
        for _ in range(calls):
            fn()
        e1.record(m._stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    for R in RS:
        o = torch.arange(R, device=dev) % M
        h = (mu[o] + s[o] * torch.randn(R, D1, device=dev, generator=gen)).contiguous()
        agg, dim = torch.empty(R, device=dev), torch.empty(R, D1, device=dev)
        torch.cuda.synchronize()

        def kernel(per_unit):
            m._call(m._lib.iwae_aggregate(m._h, None, M, 0, _lib.fptr(mu), _lib.fptr(s), _lib.fptr(h), R, 0,
                                          _lib.fptr(agg), _lib.fptr(dim) if per_unit else None, None, None))

        def yard(per_unit):
            with torch.cuda.stream(m._stream):
                return torch_aggregate(h, mu, s, per_unit)

        # the yardstick computes what the kernels compute
        kernel(True)
        tj, td = yard(True)
        m._stream.synchronize()
        check = {}
        for name, got, ref in (("log_q_agg", agg, tj), ("log_q_dim", dim, td)):
            err = (got.double() - ref.double()).abs()
            of_max = float(err.max() / ref.double().abs().max())
            of_row = float(err.max() / (D1 * HALF_LOG_2PI))
            assert of_max <= 1e-4 and of_row <= 1e-4, (R, name, of_max, of_row)
            check[name] = dict(of_max_ref=of_max, of_row_scale_bound=of_row)
        del tj, td

        variants = [("a_kernel_joint", lambda: kernel(False)), ("b_kernel_joint_and_per_unit", lambda: kernel(True)),
                    ("c_torch_joint", lambda: yard(False)), ("d_torch_joint_and_per_unit", lambda: yard(True))]
        calls = {}
        for name, fn in variants:                  # warm-up, then the call count that fills MIN_SECONDS
            fn()
            m._stream.synchronize()
            t = timed(fn, 1)
            if t < 0.25 * MIN_SECONDS:             # a longer look: the first calls run slow
                n1 = int(0.25 * MIN_SECONDS / t) + 1
                t = timed(fn, n1) / n1
            calls[name] = max(1, int(MIN_SECONDS * 1.3 / t) + 1)
        c0 = [int(m._lib.iwae_debug_count(m._h, i)) for i in (40, 41)]
        times = {name: [] for name, _ in variants}
        for _ in range(REPEATS):
            for name, fn in variants:              # alternating
                sec = timed(fn, calls[name])
                assert sec >= MIN_SECONDS, (name, sec)
                times[name].append(sec / calls[name])
        m.check_kernel_status()
        c1 = [int(m._lib.iwae_debug_count(m._h, i)) for i in (40, 41)]
        ka, kb = calls["a_kernel_joint"], calls["b_kernel_joint_and_per_unit"]
        assert c1[0] - c0[0] == REPEATS * (ka + kb) and c1[1] - c0[1] == REPEATS * kb, (c0, c1)
        rr = dict(check_against_torch=check, variants={})
        pairs = float(R) * M
        for name, ts in times.items():
            ms = [t * 1e3 for t in ts]
            med = statistics.median(ts)
            exps = pairs * (1 + D1) if "per_unit" in name else pairs
            rr["variants"][name] = dict(calls_per_repeat=calls[name], ms_per_call=[round(v, 3) for v in ms],
                                        median_ms=round(med * 1e3, 3), spread_ms=round(max(ms) - min(ms), 3),
                                        pairs_per_second=pairs / med, exp_per_second=exps / med,
                                        exp_share_of_peak=round(exps / med / exp_rate, 4))
        v = {n: d["median_ms"] for n, d in rr["variants"].items()}
        rr["torch_over_kernel_joint"] = round(v["c_torch_joint"] / v["a_kernel_joint"], 2)
        rr["torch_over_kernel_per_unit"] = round(v["d_torch_joint_and_per_unit"] / v["b_kernel_joint_and_per_unit"], 2)
        rr["kernel_beats_torch"] = bool(rr["torch_over_kernel_joint"] > 1 and rr["torch_over_kernel_per_unit"] > 1)
        rec["R"][str(R)] = rr
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(rec, open(out_path, "w"), indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
