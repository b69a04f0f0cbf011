"""The numpy restatement of iwae_binarize's draw (binarize_ref.py) against
known answers, and the statistical bounds the GPU test relies on, evaluated
with the GPU test's seed (no GPU needed)."""
import numpy as np
import pytest

import binarize_ref as R

# Philox4x32-10 known answers (counter, key, output)
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    got = tuple(int(w) for w in R.philox4x32_10(ctr, key))
    assert got == want, [hex(g) for g in got]


def test_philox_is_vectorised_like_its_scalar_form():
    ctr = tuple(np.array([c[i] for c, _, _ in KAT], np.uint64) for i in range(4))
    for (_, key, want), row in zip(KAT, range(len(KAT))):
        got = R.philox4x32_10(ctr, key)
        assert tuple(int(g[row]) for g in got) == want


def test_uniform_mapping_reaches_one_from_ffffff80_on():
    u = R.uniform_from_u32(np.array([0xFFFFFFFF, 0xFFFFFF80, 0xFFFFFF7F, 0], np.uint32))
    assert u.dtype == np.float32
    assert u[0] == np.float32(1.0) and u[1] == np.float32(1.0)
    assert u[2] < np.float32(1.0)
    assert u[3] == np.float32(0.5 * 2.0 ** -32) and u[3] > 0


def test_pixel_rule_edges():
    one = np.float32(1.0)
    assert R.pixel_rule(one, one) == 1.0                       # x = 1 at u = 1.0: the x >= 1 clause
    assert R.pixel_rule(np.float32(0.999), np.float32(1.5)) == 1.0
    for x in (np.float32("nan"), np.float32(0.0), np.float32(-0.25)):
        assert R.pixel_rule(np.float32(0.0), x) == 0.0
        assert R.pixel_rule(np.float32(0.5), x) == 0.0
    assert R.pixel_rule(np.float32(0.3), np.float32(0.3)) == 0.0    # the tie u == x
    assert R.pixel_rule(np.float32(0.0), np.float32(1e-30)) == 1.0
    assert R.pixel_rule(np.float32(0.2), np.float32(0.3)) == 1.0


def test_counter_layout():
    """Row = output row, group = j / 4, value = j % 4, layer 19 in bits 20.. of the second word."""
    assert R.LAYER == 19
    seed, base = 0x123456789abcdef0, (7 << 32) | 5
    u = R.philox_uniforms(seed, base, 3, 10)
    assert u.shape == (3, 10)
    for r, j in ((0, 0), (2, 9), (1, 6)):
        w = R.philox4x32_10((r, (19 << 20) | (j // 4), 5, 7), (0x9abcdef0, 0x12345678))
        assert u[r, j] == R.uniform_from_u32(w[j % 4])
    assert ((u > 0) & (u <= 1)).all()


def test_gather_zero_rows_outside():
    x = np.arange(12, dtype=np.float32).reshape(3, 4)
    g = R.gather(x, [2, -1, 0, 3, 2])
    assert (g[0] == x[2]).all() and (g[4] == x[2]).all() and (g[2] == x[0]).all()
    assert (g[1] == 0).all() and (g[3] == 0).all()


def test_mean_bound_with_the_gpu_seed():
    x = np.full((64, 784), 0.3, np.float32)
    b = R.binarize(x, R.SEED, 0)
    assert set(np.unique(b)) == {0.0, 1.0}
    assert abs(float(b.mean(dtype=np.float64)) - 0.3) <= 5 * np.sqrt(0.21 / 50176)


def test_consecutive_positions_are_independent_with_the_gpu_seed():
    x = np.full((64, 784), 0.5, np.float32)
    a, b = R.binarize(x, R.SEED, 0), R.binarize(x, R.SEED, 1)
    assert abs(float((a == b).mean(dtype=np.float64)) - 0.5) <= 5 * 0.5 / np.sqrt(50176)


def test_binary_images_are_a_fixed_point():
    rng = np.random.default_rng(1)
    x = (rng.random((64, 784)) < 0.2).astype(np.float32)
    assert (R.binarize(x, R.SEED, 3) == x).all()
    # ... even where the uniform is exactly 1.0
    assert R.pixel_rule(np.ones_like(x), x).tolist() == x.tolist()
