"""Dynamic binarisation on the device (iwae_binarize, Flexible_Model.binarize,
fit(binarize=True), train_schedule(binarize=True)) against the numpy
restatement of tests/binarize_ref.py.  Every comparison is exact: the draw is
integer Philox, three float32 operations and two comparisons, all restated bit
for bit, so any difference is a kernel fault, not rounding and not chance (the
statistical bounds are checked on the restatement in test_binarize_ref.py with
the same seed)."""
import ctypes
import functools

import numpy as np
import pytest

import binarize_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
SPECIALS = (0.0, 1.0, 1.5, -0.25, float("nan"), 1e-30)


@functools.lru_cache(maxsize=None)
def _model(x_dim, seed=R.SEED):
    from iwae_replication_project_amd import Flexible_Model
    return Flexible_Model([8], [8], [4], [x_dim], dataset_bias=None, loss_function="IWAE", k=3, x_dim=x_dim, seed=seed)


def _count(m):
    return int(m._lib.iwae_debug_count(m._h, 22))


def _dev(m, a, dtype=None):
    import torch
    with torch.cuda.stream(m._stream):
        t = torch.as_tensor(a).to(device=m.device, dtype=dtype)
    m._stream.synchronize()
    return t


def _host(m, t):
    m._stream.synchronize()
    return t.cpu().numpy()


def _inputs(n, x_dim, seed):
    """Grey levels with the special values and ties u == x in them, and uniforms in [0, 1)."""
    rng = np.random.default_rng(seed)
    x = rng.random((n, x_dim)).astype(np.float32)
    u = rng.random((n, x_dim)).astype(np.float32)
    xf, uf = x.reshape(-1), u.reshape(-1)
    for i, v in enumerate(SPECIALS):
        xf[(3 + 11 * i) % xf.size] = v
    for i in range(4):
        uf[(5 + 13 * i) % uf.size] = xf[(5 + 13 * i) % xf.size]       # ties
    return x, u


# --------------------------------------------------------------- injected u
@pytest.mark.parametrize("x_dim", [784, 50, 7, 1])
@pytest.mark.parametrize("n", [1, 5, 257])
def test_injected_u_matches_the_rule_exactly(x_dim, n):
    import torch
    m = _model(x_dim)
    x, u = _inputs(n, x_dim, 1000 + 10 * x_dim + n)
    want = R.pixel_rule(u, x)
    if x.size > 40:
        assert 0 < want.mean() < 1
    xt, ut = _dev(m, x), _dev(m, u)
    c0 = _count(m)
    got = _host(m, m.binarize(xt, u=ut))                       # the facade's own buffer
    assert got.shape == (n, x_dim) and (got == want).all()
    ld0 = (x_dim + 3) // 4 * 4
    for ld in (ld0, ld0 + 8):
        with torch.cuda.stream(m._stream):
            big = torch.full((n + 1, ld), SENTINEL, device=m.device)
        out = m.binarize(xt, u=ut, out=big[:n, :x_dim])
        assert out.data_ptr() == big.data_ptr()
        b = _host(m, big)
        assert (b[:n, :x_dim] == want).all(), (x_dim, n, ld)
        assert (b[:n, x_dim:] == SENTINEL).all() and (b[n:] == SENTINEL).all()
        if n > 1:                                              # the raw call with this ld
            big.fill_(SENTINEL)
            from iwae_replication_project_amd import _lib
            m._call(m._lib.iwae_binarize(m._h, _lib.fptr(xt), n, None, n, _lib.fptr(ut), _lib.fptr(big), ld))
            b = _host(m, big)
            assert (b[:n, :x_dim] == want).all() and (b[:n, x_dim:] == SENTINEL).all() and (b[n:] == SENTINEL).all()
    assert _count(m) - c0 == (5 if n > 1 else 3)


def test_misaligned_x_takes_the_scalar_path_with_the_same_result():
    import torch
    n, x_dim = 5, 784
    m = _model(x_dim)
    x, u = _inputs(n, x_dim, 7)
    with torch.cuda.stream(m._stream):
        base = torch.zeros(n * x_dim + 1, device=m.device)
        xv = base[1:].view(n, x_dim)
        xv.copy_(torch.from_numpy(x))
    assert xv.data_ptr() % 16 == 4
    want = R.pixel_rule(u, x)
    assert (_host(m, m.binarize(xv, u=_dev(m, u))) == want).all()
    assert (_host(m, m.binarize(_dev(m, x), u=_dev(m, u))) == want).all()
    m.set_seed(R.SEED)                                         # and on device noise
    a = _host(m, m.binarize(xv))
    m.set_seed(R.SEED)
    b = _host(m, m.binarize(_dev(m, x)))
    assert (a == b).all() and (a == R.binarize(x, R.SEED, 0)).all()


def test_in_place():
    n, x_dim = 257, 784
    m = _model(x_dim)
    x, u = _inputs(n, x_dim, 8)
    xt = _dev(m, x)
    out = m.binarize(xt, u=_dev(m, u), out=xt)
    assert out.data_ptr() == xt.data_ptr()
    assert (_host(m, xt) == R.pixel_rule(u, x)).all()


# --------------------------------------------------------------------- perm
PERM = list(range(8, -1, -1)) + [3, -1, 9]                     # the reversal, a repeat, two indices outside


@pytest.mark.parametrize("x_dim", [50, 784])
def test_perm_gathers_output_rows(x_dim):
    import torch
    m = _model(x_dim)
    x, _ = _inputs(9, x_dim, 9)
    _, u = _inputs(12, x_dim, 10)
    xt = _dev(m, x)
    want = R.binarize(x, 0, 0, perm=PERM, u=u)
    assert (want[10] == 0).all() and (want[11] == 0).all() and want[:10].any()
    for perm in (PERM, np.array(PERM, np.int32), torch.tensor(PERM)):
        got = _host(m, m.binarize(xt, perm=perm, u=_dev(m, u)))
        assert got.shape == (12, x_dim) and (got == want).all()
    # device noise: the draws belong to the OUTPUT rows
    m.set_seed(R.SEED)
    got = _host(m, m.binarize(xt, perm=PERM))
    assert (got == R.binarize(x, R.SEED, 0, perm=PERM)).all()
    # the identity perm gives perm=None's bits
    m.set_seed(R.SEED)
    a = _host(m, m.binarize(xt))
    m.set_seed(R.SEED)
    b = _host(m, m.binarize(xt, perm=np.arange(9)))
    assert (a == b).all() and (a == R.binarize(x, R.SEED, 0)).all()
    with pytest.raises(ValueError):
        m.binarize(xt, perm=np.array([0.0, 1.0]))              # not integers
    with pytest.raises(ValueError):
        m.binarize(xt, perm=np.zeros((2, 2), np.int64))
    with pytest.raises(ValueError):
        m.binarize(xt, perm=PERM, u=np.zeros((9, x_dim), np.float32))   # u is per OUTPUT row
    with pytest.raises(ValueError):
        m.binarize(xt, out=torch.zeros(12, x_dim, device=m.device))


# ------------------------------------------------------------------- Philox
@pytest.mark.parametrize("n,x_dim", [(5, 50), (3, 784)])
def test_philox_stream_and_position(n, x_dim):
    m = _model(x_dim)
    rng = np.random.default_rng(11)
    x = rng.random((n, x_dim)).astype(np.float32)
    xt = _dev(m, x)
    m.set_seed(R.SEED)
    first, second = _host(m, m.binarize(xt)), _host(m, m.binarize(xt))
    assert (first == R.binarize(x, R.SEED, 0)).all()
    assert (second == R.binarize(x, R.SEED, 1)).all()
    assert (first != second).any()
    try:
        m.set_noise_stream(1)
        other = _host(m, m.binarize(xt))
        assert (other != first).any() and (other != R.binarize(x, R.SEED, 0)).any()
    finally:
        m.set_noise_stream(0)
    m.set_seed(R.SEED)
    assert (_host(m, m.binarize(xt)) == first).all()


def test_empty_call_launches_nothing_and_keeps_the_position():
    import torch
    from iwae_replication_project_amd import _lib
    x_dim = 50
    m = _model(x_dim)
    x = np.random.default_rng(12).random((5, x_dim)).astype(np.float32)
    xt = _dev(m, x)
    m.set_seed(R.SEED)
    c0 = _count(m)
    e = m.binarize(torch.zeros(0, x_dim))
    assert tuple(e.shape) == (0, x_dim) and e.device == m.device and e.dtype == torch.float32
    e = m.binarize(xt, perm=np.zeros(0, np.int64))
    assert tuple(e.shape) == (0, x_dim)
    buf = _dev(m, np.full((5, 52), SENTINEL, np.float32))
    assert m._lib.iwae_binarize(m._h, _lib.fptr(xt), 5, None, 0, None, _lib.fptr(buf), 52) == 0
    assert _count(m) == c0
    assert (_host(m, buf) == SENTINEL).all()
    assert (_host(m, m.binarize(xt)) == R.binarize(x, R.SEED, 0)).all()       # still base 0
    assert _count(m) == c0 + 1


# ---------------------------------------------- fixed point and statistics
def test_binary_images_come_back_bit_for_bit():
    m = _model(784)
    x = (np.random.default_rng(1).random((64, 784)) < 0.2).astype(np.float32)
    m.set_seed(R.SEED)
    xt = _dev(m, x)
    for _ in range(2):
        assert (_host(m, m.binarize(xt)) == x).all()


def test_statistics_with_the_restatements_seed():
    m = _model(784)
    m.set_seed(R.SEED)
    x3 = np.full((64, 784), 0.3, np.float32)
    b = _host(m, m.binarize(_dev(m, x3)))
    assert (b == R.binarize(x3, R.SEED, 0)).all()
    assert abs(float(b.mean(dtype=np.float64)) - 0.3) <= 5 * np.sqrt(0.21 / 50176)
    m.set_seed(R.SEED)
    x5 = _dev(m, np.full((64, 784), 0.5, np.float32))
    a, b = _host(m, m.binarize(x5)), _host(m, m.binarize(x5))
    assert abs(float((a == b).mean(dtype=np.float64)) - 0.5) <= 5 * 0.5 / np.sqrt(50176)


# ------------------------------------------------------------- side effects
def test_no_side_effects_and_bad_layouts():
    import torch
    from iwae_replication_project_amd import Adam, _lib
    from iwae_replication_project_amd._lib import IwaeError
    x_dim = 50
    m = _model(x_dim, seed=5)
    m.compile(optimizer=Adam(learning_rate=1e-3, epsilon=1e-4))
    x = np.random.default_rng(13).random((5, x_dim)).astype(np.float32)
    for _ in range(2):
        m.train_step((x > 0.5).astype(np.float32))             # weights moved, Adam state, a captured graph
    w0, (am0, av0, st0), g0, c0 = m.get_weights(), m.get_optimizer_state(), m.graph_captures(), _count(m)
    ws0 = m._lib.iwae_workspace_bytes(m._h)
    xt = _dev(m, x)
    m.binarize(xt)
    m.binarize(xt, perm=[4, 4, 0])
    m.binarize(xt, u=np.zeros((5, x_dim), np.float32))
    assert _count(m) == c0 + 3
    # layouts the library refuses: ld below / off a multiple of 4, a misaligned out
    with torch.cuda.stream(m._stream):
        tight = torch.zeros(5, 50, device=m.device)            # row stride 50
        wide = torch.zeros(5 * 54 + 1, device=m.device)
        off = wide[1:1 + 5 * 52].view(5, 52)[:, :50]           # stride 52, 4 bytes off
        odd = wide[:5 * 54].view(5, 54)[:, :50]                # stride 54
    for bad in (tight, off, odd):
        with pytest.raises(IwaeError):
            m.binarize(xt, out=bad)
    fn, xp, op = m._lib.iwae_binarize, _lib.fptr(xt), _lib.fptr(wide)
    perm = _dev(m, np.arange(5), torch.int64)
    pp = ctypes.cast(ctypes.c_void_p(perm.data_ptr()), ctypes.POINTER(ctypes.c_longlong))
    for rc in (fn(m._h, None, 5, None, 5, None, op, 52),        # NULL x
               fn(m._h, xp, 5, None, 5, None, None, 52),        # NULL out
               fn(m._h, xp, 5, None, -1, None, op, 52),         # negative n
               fn(m._h, xp, -1, pp, 5, None, op, 52),           # negative n_src
               fn(m._h, xp, 4, None, 5, None, op, 52),          # n > n_src without perm
               fn(m._h, xp, 5, None, 5, None, op, 48),          # ld < x_dim
               fn(m._h, xp, 5, None, 5, None, op, 54),          # ld % 4
               fn(m._h, xp, 5, None, 5, None, op, (1 << 22) + 4),
               fn(m._h, xp, 5, None, 5, None, _lib.fptr(off), 52)):   # alignment
        assert rc == -1
        assert m._lib.iwae_last_error(m._h)
    with torch.cuda.stream(m._stream):
        wide.fill_(SENTINEL)
    assert fn(m._h, xp, 4, pp, 5, None, op, 52) == 0           # with perm n may exceed n_src (row 4: zeros)
    m._stream.synchronize()
    assert _count(m) == c0 + 4
    assert (wide.view(-1)[:5 * 52].view(5, 52)[4, :50] == 0).all()
    w1, (am1, av1, st1) = m.get_weights(), m.get_optimizer_state()
    assert all((a == b).all() for a, b in zip(w0, w1))
    assert (am0 == am1).all() and (av0 == av1).all() and st0 == st1
    assert m.graph_captures() == g0 and m._lib.iwae_workspace_bytes(m._h) == ws0
    m.check_kernel_status()


# ---------------------------------------------------------------------- fit
def _pair(x_dim, seed=11):
    from iwae_replication_project_amd import Adam, Flexible_Model
    ms = []
    for _ in range(2):
        m = Flexible_Model([8], [8], [4], [x_dim], dataset_bias=None, loss_function="IWAE", k=3, x_dim=x_dim, seed=seed)
        m.compile(optimizer=Adam(learning_rate=1e-3, epsilon=1e-4))
        ms.append(m)
    return ms


def _manual_epoch(m, xd, perm, B, mask=None):
    """One epoch of fit(binarize=True), spelled out; returns the epoch's mean loss."""
    import torch
    N = xd.shape[0]
    xb = m.binarize(xd, perm)
    nfull = N // B
    with torch.cuda.stream(m._stream):
        ms = None if mask is None else (mask if perm is None else mask[perm.to(m.device)])
        losses = torch.zeros((N + B - 1) // B, device=m.device)
    if nfull:
        full = m.train_steps(xb[:nfull * B], B, sync=False, mask=None if ms is None else ms[:nfull * B])
        with torch.cuda.stream(m._stream):
            losses[:nfull] = full
    if N % B:
        out = m.train_step(xb[nfull * B:], sync=False, mask=None if ms is None else ms[nfull * B:])[m.loss_function]
        with torch.cuda.stream(m._stream):
            losses[nfull] = out[0]
    m._stream.synchronize()
    return float(losses.mean().item())


@pytest.mark.parametrize("shuffle,masked", [(True, False), (False, False), (True, True)])
def test_fit_binarize_equals_the_spelled_out_sequence(shuffle, masked):
    import torch
    x_dim, N, B = 50, 12, 5
    a, b = _pair(x_dim)
    rng = np.random.default_rng(14)
    x = rng.random((N, x_dim)).astype(np.float32)
    x[rng.random((N, x_dim)) < 0.5] = 0.0
    mask = (rng.random((N, x_dim)) < 0.7).astype(np.float32) if masked else None
    c0 = _count(a)
    hist = a.fit(x, epochs=2, batch_size=B, shuffle=shuffle, seed=3, mask=mask, binarize=True)["IWAE"]
    assert _count(a) - c0 == 2                                 # one launch per epoch
    xd = _dev(b, x)
    md = None if mask is None else _dev(b, mask)
    g = torch.Generator(device="cpu")
    g.manual_seed(3)
    want = []
    for _ in range(2):
        perm = torch.randperm(N, generator=g) if shuffle else None
        want.append(_manual_epoch(b, xd, perm, B, md))
    assert hist == want and all(np.isfinite(hist))
    assert all((p == q).all() for p, q in zip(a.get_weights(), b.get_weights()))
    # the binarisation is what the steps saw: plain fit on the grey levels differs
    c = _pair(x_dim)[0]
    plain = c.fit(x, epochs=2, batch_size=B, shuffle=shuffle, seed=3, mask=mask)["IWAE"]
    assert plain != hist


def test_train_schedule_binarize_equals_its_manual_loop():
    import torch
    from iwae_replication_project_amd import data
    x_dim, N, B = 50, 10, 4
    a, b = _pair(x_dim, seed=12)
    x = np.random.default_rng(15).random((N, x_dim)).astype(np.float32)
    c0 = _count(a)
    res = data.train_schedule(a, x, stages=2, batch_size=B, passes=lambda i: 1, binarize=True)
    assert res == [None, None] and _count(a) - c0 == 2
    xd = _dev(b, x)
    for i in (1, 2):
        b.optimizer.learning_rate = data.stage_learning_rate(i)
        b._push_adam()
        perm = torch.randperm(N, generator=torch.Generator(device="cpu"))    # fit's unseeded generator
        _manual_epoch(b, xd, perm, B)
    assert all((p == q).all() for p, q in zip(a.get_weights(), b.get_weights()))
    assert a.epoch == b.epoch == 6
