"""iwae_tvo_step / iwae_tvo_grad / iwae_tvo_weights are part of the C ABI, the
ctypes binding and the facade (no GPU needed)."""
import ctypes
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "iwae.h")
PKG = os.path.join(ROOT, "iwae_replication_project_amd")
STEP_NAMES = ("iwae_tvo_step", "iwae_tvo_grad")
STEP_ARGS = ["iwae_handle* h", "const iwae_tvo_config* cfg", "const float* betas", "const float* x", "int B",
             "const float* const* eps", "int n_eps", "float* values_dev"]
WEIGHTS_ARGS = ["iwae_handle* h", "const float* lw", "int N", "int k", "const float* betas", "int n_part",
                "float* lower", "float* upper", "float* iwae", "float* a_theta", "float* a_phi"]


def _code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _args(src, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", src)
    assert m, f"include/iwae.h does not declare {name}"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_the_entries_between_wake_sleep_and_diagnostics():
    src = _code()
    for name in STEP_NAMES:
        assert _args(src, name) == STEP_ARGS
    assert _args(src, "iwae_tvo_weights") == WEIGHTS_ARGS
    assert (src.index("int iwae_wake_sleep_grad(") < src.index("int iwae_tvo_step(") < src.index("int iwae_tvo_grad(")
            < src.index("int iwae_tvo_weights(") < src.index("int iwae_debug_gemm("))


def test_header_declares_the_config_struct():
    src = _code()
    m = re.search(r"typedef\s+struct\s+iwae_tvo_config\s*\{(.*?)\}\s*iwae_tvo_config\s*;", src, flags=re.S)
    assert m, "include/iwae.h does not define iwae_tvo_config"
    assert [" ".join(f.split()) for f in m.group(1).split(";") if f.strip()] == ["int k", "int n_part"]
    assert src.index("iwae_tvo_config;") < src.index("int iwae_tvo_step(")


def test_struct_size_matches_a_compiled_probe(tmp_path):
    from iwae_replication_project_amd import _lib
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "iwae.h"\n'
                     'int main(void){printf("%zu %zu %zu\\n", sizeof(iwae_tvo_config), offsetof(iwae_tvo_config, k),'
                     'offsetof(iwae_tvo_config, n_part)); return 0;}')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    C = _lib.IwaeTvoConfig
    assert got == [ctypes.sizeof(C), C.k.offset, C.n_part.offset]
    assert got[0] == 8


def test_library_exports_the_symbols():
    from iwae_replication_project_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "build the library first (__graft_entry__.build())"
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for name in STEP_NAMES + ("iwae_tvo_weights",):
        assert re.search(r"\bT " + name + r"\b", out), name


def test_ctypes_signatures_match_the_header():
    from iwae_replication_project_amd import _lib
    i, FP, FPP = ctypes.c_int, _lib.FP, _lib.FPP
    assert _lib.IwaeTvoConfig._fields_ == [("k", i), ("n_part", i)]
    for name in STEP_NAMES:
        res, args = _lib.SIGNATURES[name]
        assert res is i
        assert args == [_lib.H, ctypes.POINTER(_lib.IwaeTvoConfig), FP, FP, i, FPP, i, FP]
    res, args = _lib.SIGNATURES["iwae_tvo_weights"]
    assert res is i and args == [_lib.H, FP, i, i, FP, i, FP, FP, FP, FP, FP]
    # inserted before the wake-sleep entries, which stay last
    names = list(_lib.SIGNATURES)
    assert names[-5:-2] == ["iwae_tvo_step", "iwae_tvo_grad", "iwae_tvo_weights"]
    assert names[-2:] == ["iwae_wake_sleep_step", "iwae_wake_sleep_grad"]


def test_header_documents_counters_42_and_43_after_41():
    src = open(HEADER).read()
    doc = src[src.rindex("/*", 0, src.index("long long iwae_debug_count")):src.index("long long iwae_debug_count")]
    doc = " ".join(re.sub(r"^ \* ?", "", doc, flags=re.M).split())
    m41 = re.search(r"\b41\s+agg_dim_kernel\s+launches", doc)
    m42 = re.search(r"\b42\s+iwae_tvo_step\s+/\s+iwae_tvo_grad\s+calls\s+that\s+enqueued\s+work", doc)
    m43 = re.search(r"\b43\s+tvo_kernel\s+launches", doc)
    also = re.search(r"GM_FIT\s+launches\s+also\s+count\s+under\s+36\s+/\s+37", doc)
    unknown = doc.index("-1 for an unknown")
    assert m41 and m42 and m43 and also
    assert m41.start() < m42.start() < m43.start() < also.start() < unknown


def test_header_documents_the_rules():
    src = " ".join(re.sub(r"^ \* ?", "", open(HEADER).read(), flags=re.M).split())
    doc = src[src.index("One TVO step on x"):src.index("int iwae_tvo_step(")]
    for phrase in ("L_tvo", "L_upper", "L_iwae", "a_theta", "a_phi", "lower <= iwae <= upper", "IWAE_EINVAL",
                   "noise position", "GM_FIT", "never the bf16x3 engine", "iwae_set_graphs does not apply",
                   "Deterministic", "2^30", "data-parallel world > 1", "strictly ascending", "[1, 64]"):
        assert phrase in doc, phrase
    doc = src[src.index("The same kernel on caller log weights"):src.index("int iwae_tvo_weights(")]
    for phrase in ("2^20", "2^30", "every output NULL", "noise position", "NaN", "neighbours"):
        assert phrase in doc, phrase


def test_no_new_loss_id_or_knob():
    from iwae_replication_project_amd import _lib
    assert "TVO" not in _lib.LOSS_IDS and len(_lib.LOSS_IDS) == 11 and len(_lib.KNOBS) == 37
    assert not re.search(r"IWAE_(KNOB|LOSS)_\w*(TVO|THERMO)", open(HEADER).read())


def test_new_code_is_plain_and_deterministic():
    model = open(os.path.join(PKG, "csrc", "iwae_model.hip")).read()
    kern = open(os.path.join(PKG, "csrc", "iwae_tvo.hip")).read()
    host = model[model.index("// ------------------------------------------ thermodynamic variational objective"):
                 model.index("int iwae_debug_gemm(")]
    assert "do_tvo" in host and "tvo_kernel" in kern
    for word in ("getenv", "atomicAdd", "printf"):
        assert word not in host and word not in kern, word
    manifest = open(os.path.join(PKG, "csrc", "SOURCES.txt")).read().split()
    assert "iwae_tvo.hip" in manifest


def test_facade_signatures():
    from iwae_replication_project_amd import Flexible_Model, tvo_schedule
    sig = inspect.signature(tvo_schedule)
    assert list(sig.parameters) == ["n_part", "beta1"] and sig.parameters["beta1"].default == 0.025
    sig = inspect.signature(Flexible_Model.tvo_step)
    assert list(sig.parameters) == ["self", "x", "betas", "n_part", "k", "eps", "sync", "update"]
    d = {n: p.default for n, p in sig.parameters.items()}
    assert d["betas"] is None and d["n_part"] is None and d["k"] is None and d["eps"] is None
    assert d["sync"] is True and d["update"] is True
    sig = inspect.signature(Flexible_Model.tvo_steps)
    assert list(sig.parameters) == ["self", "x", "batch_size", "betas", "n_part", "k", "sync"]
    sig = inspect.signature(Flexible_Model.tvo_bounds)
    assert list(sig.parameters) == ["self", "lw", "betas", "want"]
    assert sig.parameters["want"].default == ("lower", "upper", "iwae")
    sig = inspect.signature(Flexible_Model.get_L_TVO)
    assert list(sig.parameters) == ["self", "x", "k", "betas", "eps"]
    for fn in (Flexible_Model.tvo_step, Flexible_Model.tvo_steps, Flexible_Model.tvo_bounds, Flexible_Model.get_L_TVO):
        assert "mask" not in inspect.signature(fn).parameters
    sig = inspect.signature(Flexible_Model.train_step)       # the train step is as it was
    assert list(sig.parameters) == ["self", "x", "eps", "sync", "mask"]
