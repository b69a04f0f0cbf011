"""CPU checks of the first-layer group tests' inputs (tests/group_cases.py):
the float64 references the GPU tests compare against are finite, and every
image is one the references handle as the existing cases' images are."""
import numpy as np

import group_cases as GC
import observed_ref as OB
import score_ref as R
import scoregrad_ref as G


def test_shape_reaches_a_group_boundary_inside_the_call():
    starts = list(range(0, GC.N, GC.CHUNK))
    sup = GC.CHUNK * max(1, GC.GROUP // GC.CHUNK)                 # whole chunks per group, as ChunkWalk's
    groups = sorted({i0 - i0 % sup for i0 in starts})
    assert groups == [0, 4] and starts == [0, 2, 4, 6]            # a chunk starts the second group mid-call
    assert GC.N - starts[-1] == 1 and GC.N - groups[-1] == 3      # a one-image chunk; a ragged last group


def test_score_references_are_finite():
    name = GC.GROUP_CASE
    spec, _, x, _ = R.case(name)
    assert x.shape == (GC.N, spec.x_dim) and spec.L == 2
    ref, g = R.reference(name, "off"), G.reference(name, "off")
    assert ref["logq"].shape == (GC.K, GC.N)
    assert all(np.isfinite(v).all() for v in ref.values())
    assert all(np.isfinite(v).all() for t in g.values() for v in t) and all(t[0].any() for t in g.values())
    assert (ref["Sq"] > 0).all() and (ref["Sp"] > 0).all() and (ref["Spx"] > 0).all()


def test_masked_references_are_finite_and_the_mask_is_the_existing_cases():
    name = "O" + GC.GROUP_CASE
    _, _, x, mask, _, x_full = OB.case(name)
    seen = (mask != 0).sum(1)
    assert seen[0] == 0 and seen[1] == mask.shape[1] and ((seen[2:] > 0) & (seen[2:] < mask.shape[1])).all()
    assert np.isnan(x[mask == 0]).all() and np.isfinite(x_full).all()
    ref, g = OB.reference(name, "off"), OB.grad_reference(name, "off")
    assert all(np.isfinite(v).all() for v in ref.values())
    assert all(np.isfinite(v).all() for t in g.values() for v in t)
    # no observed addend on the all-missing image alone (test_gpu_observed._check_terms asks exact zeros there)
    assert ((ref["Spx"] > 0).sum(0) == [0] + [GC.K] * (GC.N - 1)).all()


def test_nll_posterior_and_impute_references_are_finite_and_non_vacuous():
    import test_gpu_edges as TE
    import test_gpu_impute as TI
    import test_gpu_posterior as TP
    for k in (GC.K, 128):
        O, spec, params, x, eps = TE._oracle_case(TE.ARCH2, GC.N, k, 7000 + k)
        assert np.isfinite(O.log_px_per_image(params, spec, x, k, eps=eps, chunk=1000)).all()
    for n in (GC.N, 4):
        ref = TP._case(1, n, GC.K)[2]                              # (asserts min w~ and 1 < ESS < k itself)
        assert np.isfinite(ref["log_px"]).all() and np.isfinite(ref["probs"]).all()
    ref = TI._case(1, GC.N, GC.K)[4]                               # (asserts check_non_vacuous itself)
    assert np.isfinite(ref["log_px"]).all() and np.isfinite(ref["x_mean"]).all()
