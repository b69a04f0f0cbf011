"""CPU checks of tests/engine_op_cases.py: each case still reaches the edge of
the engine's op loop it is there for (restated from the case's numbers, so a
later edit of a case cannot silently lose it), and the same train step in
float32 arithmetic stays within a quarter of every GPU bar
(tests/test_gpu_engine_ops.py), as tests/test_shape_cases.py shows for its cases."""
import numpy as np
import pytest

import engine_op_cases as E
import pathgrad_ref as R
import shape_cases as S

# the GPU tests' bars (tests/test_gpu_engine_ops.py = tests/test_gpu_shapes.py)
GPU_REL, GPU_TENSOR, GPU_ADAM_ATOL = 1e-4, 5e-4, 6e-5

CASE_LOSS = [(n, v[0]) for n in E.CASES for v in E.loss_variants(n)]


def _ops(name, **kw):
    return [o for o in E.engine_ops(name) if all(o[k] == v for k, v in kw.items())]


def test_cases_are_small_mirrored_and_on_the_engine():
    for name, (he, hd, le, ld, x_dim, B, k, seed) in E.CASES.items():
        assert B * k <= 300, name
        assert hd == he[::-1] and ld == le[::-1][1:] + [x_dim], name
        assert len(he) <= S.kTcMaxLayers and B * k <= S.UPD_ROWS, name
    assert len({c[7] for c in E.CASES.values()}) == len(E.CASES)
    assert set(E.EXTRA_LOSS_CASES) <= set(E.CASES) and E.GRAPH_CASE in E.CASES


def test_Ea_ragged_rows_idle_waves_and_padding_widths():
    he, hd, le, ld, x_dim, B, k, seed = E.CASES["Ea"]
    rows = B * k
    assert rows == 21 and -(-rows // 16) == 2 and rows % 16 == 5        # a ragged second workgroup
    # at most 4 column tiles per op: at least half the waves own no unit and take the hand-over
    for o in E.engine_ops("Ea"):
        assert o["ntile"] <= 4 and sum(u == 0 for u in o["units"]) >= 4, o
    assert any(o["ntile"] in (2, 3) for o in E.engine_ops("Ea"))
    assert {o["pad"] for o in _ops("Ea", dir="fwd")} >= {1, 31}
    assert E._r32(le[0] + 1) - le[0] == 32                                # h1 (SAMPLE0): 32 columns of padding
    assert E._r32(2 * le[0]) == 2 * le[0]                                 # dP0 (GBWD0): none


def test_Eb_nine_against_eight_tiles_and_one_against_two_k_chunks():
    ops = E.engine_ops("Eb")
    assert {o["ntile"] for o in ops} >= {8, 9}
    nine = next(o for o in ops if o["ntile"] == 9)
    assert nine["units"][0] == 2 * nine["nch"] and set(nine["units"][1:]) == {nine["nch"]}
    eight = next(o for o in ops if o["ntile"] == 8)
    assert set(eight["units"]) == {eight["nch"]}
    assert {o["nch"] for o in ops} >= {1, 2}
    assert {o["nch"] for o in _ops("Eb", dir="fwd")} >= {1, 2} and {o["nch"] for o in _ops("Eb", dir="bwd")} >= {1, 2}


def test_Ec_one_full_workgroup_deep_units_three_chunks_and_split_output():
    he, hd, le, ld, x_dim, B, k, seed = E.CASES["Ec"]
    assert B * k == 16
    ops = E.engine_ops("Ec")
    assert any(o["ntile"] == 17 and max(o["units"]) >= 3 * o["nch"] for o in ops)    # units 2, 3, ...: sets A / B
    assert max(o["nch"] for o in ops) == 3
    assert x_dim >= 241 and _ops("Ec", job="O1") and _ops("Ec", job="O2")
    o2 = _ops("Ec", job="O2")[-1]
    assert o2["t0"] == 8 and o2["ntile"] == 17 and _ops("Ec", job="O1")[-1]["ntile"] == 8
    # both directions have ops without any padding (widths that are multiples of 32)
    assert any(o["pad"] == 0 for o in _ops("Ec", dir="bwd"))


def test_Et_image_row_jobs_and_the_combined_launch():
    he, hd, le, ld, x_dim, B, k, seed = E.CASES["Et"]
    assert B * k == 264 and B * k >= S.TCU_ROWS and B > S.SMALLM_ROWS
    assert _ops("Et", job="I") and _ops("Et", job="I'")
    assert not _ops("Et", job="O2")


def test_E3b_longest_jobs():
    assert len(E.CASES["E3b"][0]) == S.kTcMaxLayers
    assert E.job_ops("E3b", "E") == 13 and E.job_ops("E3b", "E'") == 16
    assert all(E.job_ops(n, "E") <= 13 for n in E.CASES)


@pytest.mark.parametrize("name,vid", CASE_LOSS, ids=["-".join(c) for c in CASE_LOSS])
def test_float32_reference_within_a_quarter_of_the_gpu_bars(name, vid):
    """A condition on the GPU tests' inputs, not a measurement of the GPU code:
    the reference's own train step in float32 arithmetic against float64."""
    spec = E.make(name)[0]
    l64, g64, w64 = E.reference_step(name, vid)
    l32, g32, w32 = E.reference_step(name, vid, np.float32)
    whole = R.rel_l2(g32, g64)
    per = max(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)
              for a, b in zip(R.split_tensors(spec, g32), R.split_tensors(spec, g64)))
    adam = np.abs(w32 - w64).max()
    print(f"{name} {vid}: float32 loss rel {abs(l32 - l64) / abs(l64):.2e}, gradient rel-L2 {whole:.2e}, "
          f"per tensor {per:.2e}, post-Adam weights {adam:.2e}")
    assert abs(l32 - l64) <= GPU_REL / 4 * abs(l64)
    assert whole <= GPU_REL / 4, whole
    assert per <= GPU_TENSOR / 4, per
    assert adam <= max(GPU_ADAM_ATOL, 10 * np.abs(g32 - g64).max()) / 4, adam
