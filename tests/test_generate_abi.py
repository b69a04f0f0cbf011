"""Generation from the prior is part of the C ABI, the ctypes binding, the
facade and the build manifest (no GPU needed)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "iwae.h")
PKG = os.path.join(ROOT, "iwae_replication_project_amd")


def test_header_declares_iwae_generate():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+iwae_generate\s*\(([^)]*)\)", src)
    assert m, "include/iwae.h does not declare iwae_generate"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 12, args
    assert args[0].startswith("iwae_handle*") and args[1] == "int n"


def test_library_exports_iwae_generate():
    from iwae_replication_project_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "build the library first (__graft_entry__.build())"
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\bT iwae_generate\b", out)


def test_ctypes_signature_matches_the_header():
    import ctypes
    from iwae_replication_project_amd import _lib
    assert "iwae_generate" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["iwae_generate"]
    assert res is ctypes.c_int
    assert args == [_lib.H, ctypes.c_int, _lib.FP, _lib.FPP, ctypes.c_int, _lib.FP, _lib.FP, ctypes.c_int, _lib.FP,
                    ctypes.c_int, _lib.FPP, ctypes.c_int]


def test_facade_has_generate_x_and_sample():
    from iwae_replication_project_amd import Flexible_Model
    assert callable(getattr(Flexible_Model, "generate_x", None))
    assert callable(getattr(Flexible_Model, "sample", None))


def test_manifest_lists_the_generation_source():
    import __graft_entry__ as G
    assert "iwae_generate.hip" in G.SOURCES
    assert os.path.exists(os.path.join(PKG, "csrc", "iwae_generate.hip"))
