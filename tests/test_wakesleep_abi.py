"""iwae_wake_sleep_step / iwae_wake_sleep_grad are part of the C ABI, the ctypes
binding and the facade (no GPU needed)."""
import ctypes
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "iwae.h")
PKG = os.path.join(ROOT, "iwae_replication_project_amd")
NAMES = ("iwae_wake_sleep_step", "iwae_wake_sleep_grad")
ARGS = ["iwae_handle* h", "const iwae_ws_config* cfg", "const float* x", "int B", "const float* const* eps", "int n_eps",
        "const float* dream_x", "const float* const* dream_lat", "int n_dream_lat", "float* values_dev"]


def _code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_both_entries_after_nll_masked():
    src = _code()
    for name in NAMES:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", src)
        assert m, f"include/iwae.h does not declare {name}"
        assert [" ".join(a.split()) for a in m.group(1).split(",")] == ARGS
    assert (src.index("int iwae_nll_masked(") < src.index("int iwae_wake_sleep_step(")
            < src.index("int iwae_wake_sleep_grad(") < src.index("int iwae_debug_gemm("))


def test_header_declares_the_config_struct():
    src = _code()
    m = re.search(r"typedef\s+struct\s+iwae_ws_config\s*\{(.*?)\}\s*iwae_ws_config\s*;", src, flags=re.S)
    assert m, "include/iwae.h does not define iwae_ws_config"
    fields = [" ".join(f.split()) for f in m.group(1).split(";") if f.strip()]
    assert fields == ["int k", "int n_dream", "float c_wake, c_sleep"]
    assert src.index("iwae_ws_config;") < src.index("int iwae_wake_sleep_step(")


def test_struct_size_matches_a_compiled_probe(tmp_path):
    from iwae_replication_project_amd import _lib
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "iwae.h"\n'
                     'int main(void){printf("%zu %zu %zu %zu\\n", sizeof(iwae_ws_config), offsetof(iwae_ws_config, n_dream),'
                     'offsetof(iwae_ws_config, c_wake), offsetof(iwae_ws_config, c_sleep)); return 0;}')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    C = _lib.IwaeWsConfig
    assert got == [ctypes.sizeof(C), C.n_dream.offset, C.c_wake.offset, C.c_sleep.offset]
    assert got[0] == 16


def test_library_exports_both_symbols():
    from iwae_replication_project_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "build the library first (__graft_entry__.build())"
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for name in NAMES:
        assert re.search(r"\bT " + name + r"\b", out), name


def test_ctypes_signatures_match_the_header():
    from iwae_replication_project_amd import _lib
    i, f, FP, FPP = ctypes.c_int, ctypes.c_float, _lib.FP, _lib.FPP
    assert _lib.IwaeWsConfig._fields_ == [("k", i), ("n_dream", i), ("c_wake", f), ("c_sleep", f)]
    for name in NAMES:
        res, args = _lib.SIGNATURES[name]
        assert res is i
        assert args == [_lib.H, ctypes.POINTER(_lib.IwaeWsConfig), FP, i, FPP, i, FP, FPP, i, FP]
    assert list(_lib.SIGNATURES)[-2:] == list(NAMES)          # appended at the end


def test_header_documents_counters_35_to_38_after_34():
    src = open(HEADER).read()
    doc = src[src.rindex("/*", 0, src.index("long long iwae_debug_count")):src.index("long long iwae_debug_count")]
    doc = " ".join(re.sub(r"^ \* ?", "", doc, flags=re.M).split())
    m34 = re.search(r"\b34\s+masked\s+layer-wise\s+score-gradient", doc)
    m35 = re.search(r"\b35\s+calls\s+that\s+enqueued\s+work", doc)
    m36 = re.search(r"\b36\s+GM_FIT\s+jobs\s+issued\s+on\s+rb_bwd_kernel", doc)
    m37 = re.search(r"\b37\s+GM_FIT\s+launches\s+of\s+gauss_bwd_enc_kernel", doc)
    m38 = re.search(r"\b38\s+dream\s+generations", doc)
    unknown = doc.index("-1 for an unknown")
    assert m34 and m35 and m36 and m37 and m38
    assert m34.start() < m35.start() < m36.start() < m37.start() < m38.start() < unknown


def test_header_documents_the_rules():
    src = " ".join(re.sub(r"^ \* ?", "", open(HEADER).read(), flags=re.M).split())
    doc = src[src.index("One reweighted wake-sleep step"):src.index("int iwae_wake_sleep_step(")]
    for phrase in ("L_theta", "L_wake", "L_sleep", "bit for bit", "IWAE_EINVAL", "noise position", "GM_FIT",
                   "never the bf16x3 engine", "iwae_set_graphs does not apply", "deterministic", "2^30",
                   "data-parallel world > 1", "iwae_generate"):
        assert phrase in doc, phrase


def test_no_new_loss_id_or_knob():
    from iwae_replication_project_amd import _lib
    assert _lib.LOSS_IDS == {"VAE": 0, "IWAE": 1, "VAE_V1": 2, "L_alpha": 3, "L_power_p": 4, "L_median": 5, "CIWAE": 6,
                             "MIWAE": 7, "PIWAE": 8, "IWAE_STL": 9, "IWAE_DREG": 10}
    assert len(_lib.KNOBS) == 37 and sorted(_lib.KNOBS.values()) == list(range(1, 10)) + list(range(11, 36)) + [41, 42, 43]
    src = open(HEADER).read()
    assert not re.search(r"IWAE_(KNOB|LOSS)_\w*(WAKE|SLEEP|RWS|DREAM)", src)
    m = re.search(r"typedef\s+struct\s+iwae_loss_config\s*\{(.*?)\}", _code(), flags=re.S)
    assert [" ".join(f.split()) for f in m.group(1).split(";") if f.strip()] == \
        ["int loss", "int k", "float p", "float alpha", "float beta", "int k1", "int k2"]


def _function_source(text, start_marker, end_marker):
    return text[text.index(start_marker):text.index(end_marker)]


def test_new_host_and_kernel_code_is_plain_and_deterministic():
    model = open(os.path.join(PKG, "csrc", "iwae_model.hip")).read()
    elem = open(os.path.join(PKG, "csrc", "iwae_elem.hip")).read()
    host = _function_source(model, "// ------------------------------------------------ reweighted wake-sleep step",
                            "int iwae_debug_gemm(")
    kern = _function_source(elem, "// ------------------------------------------------------- wake-sleep step",
                            "constexpr int kBoundWaves")
    assert "do_wake_sleep" in host and "ws_values_kernel" in kern
    for word in ("getenv", "atomicAdd", "printf"):
        assert word not in host and word not in kern, word


def test_facade_signatures():
    from iwae_replication_project_amd import Flexible_Model
    sig = inspect.signature(Flexible_Model.wake_sleep_step)
    assert list(sig.parameters) == ["self", "x", "c_wake", "c_sleep", "n_dream", "dreams", "k", "eps", "sync", "update"]
    d = {n: p.default for n, p in sig.parameters.items()}
    assert d["c_wake"] == 1.0 and d["c_sleep"] == 0.0 and d["n_dream"] is None and d["dreams"] is None
    assert d["k"] is None and d["eps"] is None and d["sync"] is True and d["update"] is True
    assert "mask" not in sig.parameters
    sig = inspect.signature(Flexible_Model.wake_sleep_steps)
    assert list(sig.parameters)[:3] == ["self", "x", "batch_size"] and "mask" not in sig.parameters
    sig = inspect.signature(Flexible_Model.train_step)       # the train step is as it was
    assert list(sig.parameters) == ["self", "x", "eps", "sync", "mask"]
