"""iwae_aggregate is part of the C ABI, the ctypes binding, the facade and the
build manifest; the facade's argument rules and the restated split rule (no GPU
needed)."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "iwae.h")
PKG = os.path.join(ROOT, "iwae_replication_project_amd")


def test_header_declares_iwae_aggregate():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+iwae_aggregate\s*\(([^)]*)\)", src)
    assert m, "include/iwae.h does not declare iwae_aggregate"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["iwae_handle* h", "const float* x_ref", "int M", "int chunk", "float* loc", "float* scale",
                    "const float* lat1", "long long R", "int own_period", "float* log_q_agg", "float* log_q_dim",
                    "float* log_q_own", "float* log_q_own_dim"]


def test_ctypes_signature_matches_the_header():
    from iwae_replication_project_amd import _lib
    res, args = _lib.SIGNATURES["iwae_aggregate"]
    i, FP = ctypes.c_int, _lib.FP
    assert res is i
    assert args == [_lib.H, FP, i, i, FP, FP, FP, ctypes.c_longlong, i, FP, FP, FP, FP]
    assert ctypes.sizeof(ctypes.c_longlong) == 8


def test_header_documents_counters_39_to_41():
    src = open(HEADER).read()
    doc = src[src.rindex("/*", 0, src.index("long long iwae_debug_count")):src.index("long long iwae_debug_count")]
    doc = doc.replace("\n * ", " ")
    m38 = re.search(r"\b38\b\s+dream", doc)
    m39 = re.search(r"\b39\b\s+calls\s+that\s+enqueued", doc)
    m40 = re.search(r"\b40\b\s+agg_joint_kernel\s+launches", doc)
    m41 = re.search(r"\b41\b\s+agg_dim_kernel\s+launches", doc)
    assert m38 and m39 and m40 and m41 and m38.start() < m39.start() < m40.start() < m41.start()


def test_header_documents_the_rules():
    src = " ".join(open(HEADER).read().replace(" * ", " ").split())
    doc = src[src.index("The aggregate posterior q(h_1)"):src.index("int iwae_aggregate(")]
    for phrase in ("difference form", "does not depend on chunk, bit for bit", "two calls with different R need not agree",
                   "No float atomics", "poisons its own row only", "IWAE_EINVAL", "Out of scope", "2^22 floats"):
        assert phrase in doc, phrase


def test_library_exports_iwae_aggregate():
    from iwae_replication_project_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "build the library first (__graft_entry__.build())"
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\bT iwae_aggregate\b", out)


def test_manifest_lists_the_aggregate_source():
    import __graft_entry__ as G
    assert "iwae_aggregate.hip" in G.SOURCES
    assert os.path.exists(os.path.join(PKG, "csrc", "iwae_aggregate.hip"))


def test_facade_signatures():
    from iwae_replication_project_amd import Flexible_Model
    sig = inspect.signature(Flexible_Model.log_q_aggregate)
    assert list(sig.parameters) == ["self", "h1", "x_ref", "loc", "scale", "own_period", "want", "chunk"]
    assert sig.parameters["want"].default == ("log_q_agg",) and sig.parameters["own_period"].default == 0
    sig = inspect.signature(Flexible_Model.aggregate_posterior)
    assert list(sig.parameters) == ["self", "x", "k", "x_ref", "eps", "chunk", "per_unit"]
    assert sig.parameters["per_unit"].default is False
    sig = inspect.signature(Flexible_Model.information_statistics)
    assert list(sig.parameters) == ["self", "x", "k", "eps", "chunk", "per_unit"]
    assert sig.parameters["per_unit"].default is True


def test_facade_argument_rules():
    from iwae_replication_project_amd.flexible_iwae import check_aggregate_args as chk
    d, M = 5, 7
    comp = [(M, d), (M, d)]
    assert chk((11, d), d, True, [], M, 0, "log_q_agg") == (11, ("log_q_agg",))
    assert chk((3, 4, d), d, False, comp, M, 4, ("log_q_own", "loc")) == (12, ("log_q_own", "loc"))
    bad = [
        ((11, d), d, True, comp, M, 0, ("log_q_agg",)),            # both x_ref and (loc, scale)
        ((11, d), d, False, [], M, 0, ("log_q_agg",)),             # neither
        ((11, d), d, False, comp[:1], M, 0, ("log_q_agg",)),       # only one of loc, scale
        ((11, d), d, False, [(M, d), (M, d + 1)], M, 0, ("log_q_agg",)),
        ((11, d), d, True, [], M, M + 1, ("log_q_agg",)),          # own_period > M
        ((11, d), d, True, [], M, -1, ("log_q_agg",)),
        ((11, d), d, True, [], M, 0, ("log_q_own",)),              # own outputs with period 0
        ((11, d), d, True, [], M, 0, ("log_q_agg", "log_q_own_dim")),
        ((d,), d, True, [], M, 0, ("log_q_agg",)),                 # wrong h1 rank
        ((2, 3, 4, d), d, True, [], M, 0, ("log_q_agg",)),
        ((11, d + 1), d, True, [], M, 0, ("log_q_agg",)),          # wrong width
        ((11, d), d, True, [], M, 0, ("loc",)),                    # no density asked for
        ((11, d), d, True, [], M, 0, ("log_q",)),                  # unknown name
    ]
    for args in bad:
        with pytest.raises(ValueError):
            chk(*args)


def test_split_rule_restated_matches_the_source():
    from iwae_replication_project_amd.flexible_iwae import aggregate_split
    src = open(os.path.join(PKG, "csrc", "iwae_kernels.h")).read()
    consts = {n: int(v) for n, v in re.findall(r"constexpr int (kAgg\w+) = (\d+);", src)}
    assert consts == dict(kAggJointRows=64, kAggJointRefs=64, kAggJointCols=32, kAggDimTile=4096, kAggDimUnits=256,
                          kAggWgs=1024, kAggMaxSeg=1024)
    assert aggregate_split(1, 1000, 64) == (16, 16)                # one tile per segment on both kernels
    assert aggregate_split(1, 1, 1) == (1, 1)
    assert aggregate_split(500000, 10000, 50) == (1, 1)            # enough rows: no split
    assert aggregate_split(10000, 10000, 50) == (7, 3)
    # the partial workspace stays below the documented bounds wherever the references are split
    for R in (1, 63, 64, 65, 1000, 4097, 65535, 65536, 262143):
        for d in (1, 3, 50, 200, 256, 257, 1000):
            for M in (2, 1000, 1 << 24):
                sj, sd = aggregate_split(R, M, d)
                assert sj == 1 or 2 * sj * R < 1 << 18, (R, M, d, sj)
                assert sd == 1 or 2 * sd * R * d < 1 << 22, (R, M, d, sd)
