"""The aggregate-posterior reference (tests/aggregate_ref.py) against a brute-force
evaluation, the ELBO-surgery identities, and the fairness of the GPU bars: the
same lines in float32 must sit well inside them (no GPU needed)."""
import math

import numpy as np
import pytest

import aggregate_ref as AR


def test_case_table_covers_every_pair_and_the_named_shapes():
    shapes = set(AR.SHAPES.values())
    for a, b, pick in ((AR.D1S, AR.MS, lambda c: (c[0], c[1])), (AR.D1S, AR.RS, lambda c: (c[0], c[2])),
                       (AR.MS, AR.RS, lambda c: (c[1], c[2]))):
        assert {pick(c) for c in shapes} == {(u, v) for u in a for v in b}
    assert {(1, 1, 1), (65, 65, 17), (200, 1000, 257)} <= shapes
    assert any(R == 1 and M == 1000 for _, M, R in shapes)


def test_reference_equals_brute_force():
    rng = np.random.default_rng(1)
    R, M, d, P = 5, 4, 3, 2
    h, mu = rng.standard_normal((R, d)), rng.standard_normal((M, d))
    s = np.exp(rng.standard_normal((M, d)))
    ref = AR.aggregate(h, mu, s, P)
    for r in range(R):
        t = [[-0.5 * ((h[r, j] - mu[m, j]) / s[m, j]) ** 2 - math.log(s[m, j]) - 0.5 * math.log(2 * math.pi)
              for j in range(d)] for m in range(M)]
        J = [sum(row) for row in t]
        assert ref["log_q_agg"][r] == pytest.approx(math.log(sum(math.exp(v) for v in J) / M), abs=1e-12)
        assert ref["log_q_own"][r] == pytest.approx(J[r % P], abs=1e-12)
        for j in range(d):
            assert ref["log_q_dim"][r, j] == pytest.approx(math.log(sum(math.exp(t[m][j]) for m in range(M)) / M), abs=1e-12)
            assert ref["log_q_own_dim"][r, j] == pytest.approx(t[r % P][j], abs=1e-12)
        m_star = int(np.argmax(J))
        z = (h[r] - mu[m_star]) / s[m_star]
        assert ref["S"][r] == pytest.approx((0.5 * z * z + np.abs(np.log(s[m_star])) + AR.HALF_LOG_2PI).sum(), rel=1e-12)


@pytest.mark.parametrize("name", ["d50_M63_R1", "d3_M65_R15", "small", "wide"])
def test_information_identity_and_mi_bound(name):
    h, mu, s, P = AR.inputs(name)
    ref = AR.reference(name)
    # L = 1: log q(h|x) is the own term, log p(h) the standard normal's
    lq, lp = ref["log_q_own"], -0.5 * (h * h).sum(-1) - h.shape[1] * AR.HALF_LOG_2PI
    kl, mi, mkl = AR.information(lq, lp, ref["log_q_own"], ref["log_q_agg"])
    assert mi + mkl == pytest.approx(kl, rel=1e-12, abs=1e-9)
    # each row's own term is one of the M terms of the aggregate: own - agg <= log M row by row
    assert (ref["log_q_own"] - ref["log_q_agg"]).max() <= np.log(mu.shape[0]) + 1e-12
    assert mi <= np.log(mu.shape[0]) + 1e-12
    if name == "small":
        assert mi == pytest.approx(np.log(mu.shape[0]), abs=1e-9)
        np.testing.assert_allclose(ref["log_q_agg"], ref["log_q_own"] - np.log(mu.shape[0]), rtol=0, atol=1e-9)


def test_m1_aggregate_is_the_own_term():
    ref = AR.reference("m1")
    np.testing.assert_allclose(ref["log_q_agg"], ref["log_q_own"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(ref["log_q_dim"], ref["log_q_own_dim"], rtol=0, atol=1e-12)


def test_poisoned_row_stays_alone():
    ref = AR.reference("poison")
    bad = ~np.isfinite(ref["log_q_agg"])
    assert bad.tolist() == [r == 5 for r in range(len(bad))]
    assert np.isfinite(np.delete(ref["log_q_dim"], 5, axis=0)).all() and not np.isfinite(ref["log_q_dim"][5]).any()


@pytest.mark.parametrize("name", sorted(AR.ALL))
def test_float32_lines_stay_within_a_quarter_of_the_bars(name):
    """Fairness: the prescribed float32 evaluation (difference form, 1 / s and log s
    formed once, column-order J, online logsumexp) against the float64 reference."""
    h, mu, s, P = AR.inputs(name)
    got = AR.aggregate(h, mu, s, P, dtype=np.float32)
    worst = AR.errors(got, AR.reference(name))
    assert set(worst) == set(AR.OUTPUTS)
    for n, (e_max, e_row) in worst.items():
        assert e_max <= 0.25 and e_row <= 0.25, (name, n, e_max, e_row)
