"""Dynamic binarisation is part of the C ABI, the ctypes binding, the facade,
the training driver and the build manifest (no GPU needed)."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "iwae.h")
PKG = os.path.join(ROOT, "iwae_replication_project_amd")


def test_header_declares_iwae_binarize():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+iwae_binarize\s*\(([^)]*)\)", src)
    assert m, "include/iwae.h does not declare iwae_binarize"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["iwae_handle* h", "const float* x", "long long n_src", "const long long* perm", "int n",
                    "const float* u", "float* out", "int ld_out"]
    assert src.index("iwae_generate") < src.index("iwae_binarize") < src.index("iwae_posterior")


def test_header_documents_counter_22_after_21():
    src = open(HEADER).read()
    doc = src[src.rindex("/*", 0, src.index("long long iwae_debug_count")):src.index("long long iwae_debug_count")]
    m21, m22 = re.search(r"\b21\b[^;]*masked Bernoulli", doc), re.search(r"\b22\b[^;]*binarize_kernel", doc)
    assert m21 and m22 and m21.start() < m22.start()


def test_no_binarize_knob():
    src = open(HEADER).read()
    assert not re.search(r"IWAE_KNOB_\w*BINAR", src)
    from iwae_replication_project_amd import _lib
    assert not [k for k in _lib.KNOBS if "binar" in k]


def test_library_exports_iwae_binarize():
    from iwae_replication_project_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "build the library first (__graft_entry__.build())"
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\bT iwae_binarize\b", out)


def test_ctypes_signature_matches_the_header():
    from iwae_replication_project_amd import _lib
    assert "iwae_binarize" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["iwae_binarize"]
    assert res is ctypes.c_int
    assert args == [_lib.H, _lib.FP, ctypes.c_longlong, ctypes.POINTER(ctypes.c_longlong), ctypes.c_int, _lib.FP,
                    _lib.FP, ctypes.c_int]


def test_manifest_lists_the_binarize_source():
    import __graft_entry__ as G
    assert "iwae_binarize.hip" in G.SOURCES
    assert os.path.exists(os.path.join(PKG, "csrc", "iwae_binarize.hip"))


def test_facade_and_driver_keywords():
    from iwae_replication_project_amd import Flexible_Model, data
    sig = inspect.signature(Flexible_Model.binarize)
    assert list(sig.parameters) == ["self", "x", "perm", "u", "out"]
    assert all(sig.parameters[p].default is None for p in ("perm", "u", "out"))
    assert inspect.signature(Flexible_Model.fit).parameters["binarize"].default is False
    assert inspect.signature(data.train_schedule).parameters["binarize"].default is False


class _Opt:
    learning_rate = 0.0


class _StandIn:
    """A model whose fit accepts only today's keywords."""

    def __init__(self):
        self.optimizer = _Opt()
        self.calls = []

    def _push_adam(self):
        pass

    def fit(self, x, epochs, batch_size, verbose):
        self.calls.append((x, epochs, batch_size, verbose))


def test_train_schedule_rejects_both_binarisations():
    from iwae_replication_project_amd import data
    m = _StandIn()
    with pytest.raises(ValueError, match="binarize"):
        data.train_schedule(m, np.zeros((4, 784), np.float32), stages=1, binarize=True,
                            stochastic_rng=np.random.default_rng(0))
    assert m.calls == []


def test_train_schedule_with_both_off_calls_fit_as_before():
    from iwae_replication_project_amd import data
    m = _StandIn()
    x = np.zeros((4, 784), np.float32)
    data.train_schedule(m, x, stages=2, batch_size=3, passes=lambda i: i)
    assert len(m.calls) == 3
    assert all(c[0] is x and c[1:] == (1, 3, 0) for c in m.calls)
    m = _StandIn()
    data.train_schedule(m, x + 0.5, stages=1, batch_size=2, stochastic_rng=np.random.default_rng(0))
    (xs, ep, bs, vb), = m.calls
    assert (ep, bs, vb) == (1, 2, 0) and set(np.unique(xs)) <= {0.0, 1.0}
