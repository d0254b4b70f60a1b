"""cov() / corr(): the covariance / Pearson correlation of every record with
one or several fixed signals along an axis, from one read of the array.

Runs on the CPU test executor as it is (tests/cpu_backend.py has neither entry
point: the methods' fallback), on a subclass of it with bm_comoment_state /
bm_comoment_combine in numpy (the orchestration the HIP backend takes) and,
marked gpu, on the HIP kernels.  The truth is float128; the tolerance is
comoment_cases.truth_and_bound's.
"""
import ctypes

import numpy as np
import pytest

import bolt_amd as bolt
import comoment_cases as S
from comoment_cases import METHODS


@pytest.fixture(scope="module", params=["cpu", "cpu-fused", pytest.param("gpu", marks=pytest.mark.gpu)])
def bctx(request):
    from bolt_amd import MI355XContext
    from bolt_amd.mi355x._ops import register_backend
    import cpu_backend
    if request.param == "gpu":
        import torch
        if not torch.cuda.is_available():
            pytest.skip("no GPU")
        yield MI355XContext(device="cuda:0")
        return
    if request.param == "cpu-fused":
        register_backend("cpu", S.fused_backend())
    else:
        cpu_backend.install()
    yield MI355XContext(device="cpu")
    cpu_backend.install()  # the plain executor again, for the modules that follow


def _backend(arr):
    from bolt_amd.mi355x._ops import backend_for
    return backend_for(arr._device)


# (dtype, shape, axis) in named groups, each the smallest shape that reaches its
# branch of bm_comoment.hip.  rows: vec = min(16 B / item, 8) halved until it
# divides R and the pitch; a row is cut into chunks of 2048 elements (the LDS
# image of a signal), more than one chunk goes through the workspace and the
# merge kernel; the main loop takes whole steps of 2 * 64 * vec elements, the
# rest one vector a lane; a wave walks O * chunks / 8192 rows (at most 8).
# columns: vec likewise from I; tcv = the power of two >= I / vec, at most 64
# (64: y[r] is a scalar load); 256 / tcv row phases; R in chunks when O * column
# tiles < 2048 and R >= 16 * phases.
SHAPES = [
    "rows",
    ("float32", (5, 300), 1),        # vec 4: 16-B loads, shorter than one main step (512)
    ("float32", (5, 301), 1),        # vec 1 (odd R): scalar loads, two main steps of 128 and a rest
    ("float64", (4, 130), 1),        # vec 2
    ("float16", (3, 64), 1),         # vec 8, shorter than one wave-wide step (64 x 8)
    ("float32", (1, 7), 1),          # one row, 7 of 64 lanes
    ("uint8", (7, 260), 1),          # vec 4 (260 % 8 != 0): 4-B loads
    ("uint16", (7, 264), 1),         # vec 8: 16-B loads
    ("int32", (7, 260), 1),          # vec 4
    ("int64", (7, 260), 1),          # vec 2
    ("bool", (40, 9), 1),            # through the uint8 kernels, vec 1
    "rows_thresholds",
    ("float32", (3, 512), 1),        # exactly one main step, no rest
    ("float32", (3, 516), 1),        # one main step and a rest of one vector
    ("float32", (3, 2044), 1),       # one chunk, staged whole
    ("float32", (3, 2048), 1),       # one chunk at its limit: the state stored by the rows kernel
    ("float32", (3, 2052), 1),       # two chunks (2048 + 4): workspace and merge kernel
    ("float32", (16403, 12), 1),     # a wave walks 2 rows; the last block's waves leave early
    ("float32", (2, 50000), 1),      # rows split into 25 chunks
    "columns",
    ("float32", (300, 7, 5), 0),     # I = 35: vec 1, tcv 64 (29 lanes idle), R in 9 chunks
    ("float32", (64, 8, 16), 0),     # I = 128: vec 4, tcv 32 (8 phases, per-lane y loads)
    ("float32", (6, 50, 10), 1),     # O = 6 > 1, vec 2, tcv 8 (32 phases)
    ("float64", (20000, 8), 0),      # vec 2, tcv 4 (64 phases), R in 39 chunks
    ("uint8", (300, 7, 5), 0),       # float64 out
    ("float32", (40, 600), 0),       # vec 4, tcv 64, 3 column tiles (the last of 22 vectors), R whole
    "permuted",
    ("float32", (6, 5, 7), (0, 2)),  # permuted to the front; the signal is (6, 7)
    "every_axis",
    ("float32", (200000,), None),    # one row in 98 chunks
    ("float32", (6, 5, 7), None),
    ("bool", (40, 9), None),
]


def _group(name):
    at = SHAPES.index(name) + 1
    out = []
    while at < len(SHAPES) and not isinstance(SHAPES[at], str):
        out.append(SHAPES[at])
        at += 1
    return out


# ------------------------------------------------------------------ 1. values
@pytest.mark.parametrize("group", [g for g in SHAPES if isinstance(g, str)])
def test_values(bctx, group):
    shapes = _group(group)
    assert shapes
    for dtype, shape, axis in shapes:
        x = S.rand(shape, dtype, seed=len(shape) + shape[0])
        S.check_both(bolt.array(x, bctx), x, axis, "%s %s axis %s" % (dtype, shape, axis))


def test_result_type_and_keepdims(bctx):
    x = S.rand((6, 5, 7), "float32", seed=1)
    b = bolt.array(x, bctx)
    from bolt_amd.local import BoltArrayLocal
    for name in METHODS:
        f = getattr(b, name)
        r = f(S.signals(x, 2)[0], axis=2)
        assert type(r) is BoltArrayLocal and r.shape == (6, 5) and r.dtype == np.float32
        assert f(S.signals(x, 2)[0], axis=2, keepdims=True).shape == (6, 5, 1)
        assert f(S.signals(x, (0, 2))[0], axis=(0, 2), keepdims=True).shape == (1, 5, 1)
        s = f(S.signals(x, None)[0])
        assert isinstance(s, np.float32) and not isinstance(s, np.ndarray)
        assert f(S.signals(x, None)[0], keepdims=True).shape == (1, 1, 1)
    for kaxes in ((0,), (0, 1)):
        bs = bolt.array(x, bctx, axis=kaxes)
        for axis in (2, 0, (1, 2), None):
            S.check_both(bs, x, axis, "split %d axis %s" % (bs.split, axis))
    # statistics dtype: float16 keeps its own, integers give float64
    for dtype in ("float16", "int32", "bool"):
        xd = S.rand((4, 9), dtype, seed=2)
        assert np.asarray(bolt.array(xd, bctx).corr(np.arange(9.0), axis=1)).dtype == S.out_dtype(dtype)


# --------------------------------------------------------- 2. several signals
@pytest.mark.parametrize("k", [3, 6])
def test_several_signals(bctx, k):
    """K = 3 (one batch, the 4-signal kernels with a plane of zeros) and K = 6
    (two batches): every plane has the bytes of its one-signal call."""
    for shape, axis, out in (((5, 300), 1, (5,)), ((300, 7, 5), 0, (7, 5))):
        x = S.rand(shape, "float32", seed=3)
        b = bolt.array(x, bctx)
        ys = S.signals(x, axis, seed=k, k=k)
        for name in METHODS:
            f = getattr(b, name)
            got = np.asarray(f(ys, axis=axis))
            assert got.shape == (k,) + out and got.dtype == np.float32
            for j in range(k):
                one = np.asarray(f(ys[j], axis=axis))
                assert got[j].tobytes() == one.tobytes(), (name, shape, j)
                S.check_values(got[j], x, ys[j], axis, name, "K=%d plane %d %s" % (k, j, shape))
            kd = np.asarray(f(ys, axis=axis, keepdims=True))
            want = (k,) + tuple(1 if i == axis else n for i, n in enumerate(shape))
            assert kd.shape == want and kd.tobytes() == got.tobytes()
        # one signal given as (1,) + the reduced extents keeps the leading axis
        assert np.asarray(b.cov(ys[:1], axis=axis)).shape == (1,) + out


# ----------------------------------------------- 3. offset and adversarial data
def test_offset_and_adversarial(bctx):
    for shape, axis in (((5, 300), 1), ((300, 7, 5), 0), ((6, 5, 7), (0, 2)), ((2, 5000), 1)):
        x = S.rand(shape, "float32", seed=11, offset=1e6)
        S.check_both(bolt.array(x, bctx), x, axis, "offset %s axis %s" % (shape, axis))
    # a record whose first element (the kernels' pivot) is an outlier
    for shape, axis in (((4, 3000), 1), ((3000, 6), 0)):
        x = S.rand(shape, "float32", seed=12)
        if axis == 1:
            x[:, 0] = 3e6
        else:
            x[0, :] = 3e6
        S.check_both(bolt.array(x, bctx), x, axis, "outlier first %s" % (shape,))
    # a ramp record against a ramp signal: r = 1, never above
    for dtype in ("float32", "float64"):
        ramp = np.arange(3000, dtype=np.float64)
        x = np.stack([2.5 * ramp + 7, -0.5 * ramp + 1e5, ramp * 1e-3]).astype(dtype)
        for arr, axis in ((x, 1), (np.ascontiguousarray(x.T), 0)):
            r = np.asarray(bolt.array(arr, bctx).corr(ramp, axis=axis))
            assert np.all(np.abs(r) <= 1.0), r
            S.check_values(r, arr, ramp, axis, "corr", "ramp %s axis %d" % (dtype, axis))
            S.check_values(np.asarray(bolt.array(arr, bctx).cov(ramp, axis=axis)), arr, ramp, axis, "cov", "ramp")
    # corr(-y) == -corr(y) within the bound
    x = S.rand((5, 300), "float32", seed=13)
    b = bolt.array(x, bctx)
    y = S.signals(x, 1)[1]
    pos, neg = np.asarray(b.corr(y, axis=1)), np.asarray(b.corr(-y, axis=1))
    _, bound = S.truth_and_bound(x, y, 1, "corr")
    assert np.all(np.abs(pos.astype(np.longdouble) + neg.astype(np.longdouble)) <= bound)
    # a signal far from zero: 1e4 + noise
    y4 = 1e4 + np.random.default_rng(5).standard_normal(300)
    for name in METHODS:
        S.check_values(np.asarray(getattr(b, name)(y4, axis=1)), x, y4, 1, name, "signal 1e4 + noise")


# ------------------------------------------------------- 4. degenerate records
def test_degenerate(bctx):
    x = S.rand((3, 64), "float32", seed=6)
    x[1] = 2.5
    y = S.signals(x, 1)[0]
    for arr, axis in ((x, 1), (np.ascontiguousarray(x.T), 0)):
        b = bolt.array(arr, bctx)
        c, r = np.asarray(b.cov(y, axis=axis)), np.asarray(b.corr(y, axis=axis))
        assert c[1] == 0.0 and np.isnan(r[1]) and np.isfinite(r[[0, 2]]).all() and np.isfinite(c[[0, 2]]).all()
        # a constant signal: cov 0, corr nan, for a value whose float64 mean is not exact too
        for const in (np.full(64, 0.1), np.ones(64, dtype=bool), np.full(64, 7, dtype=np.int16)):
            cc, rc = np.asarray(b.cov(const, axis=axis)), np.asarray(b.corr(const, axis=axis))
            assert np.all(cc == 0.0) and np.isnan(rc).all(), (const[0], cc, rc)
    # a nan spoils its own record only
    z = S.rand((3, 64), "float32", seed=8)
    z[1, 17] = np.nan
    for arr, axis in ((z, 1), (np.ascontiguousarray(z.T), 0)):
        b = bolt.array(arr, bctx)
        for name in METHODS:
            got = np.asarray(getattr(b, name)(np.stack([y, -y]), axis=axis))
            assert np.isnan(got[:, 1]).all() and np.isfinite(got[:, [0, 2]]).all()
            keep = np.delete(arr, 1, axis=1 - axis)
            S.check_values(np.delete(got[0], 1), keep, y, axis, name, "beside a nan")


def test_no_variance_no_correlation(bctx):
    """A state whose M2 is 0 beside a co-moment that rounding left nonzero (a
    nearly constant record): corr is nan, not a clamped +-inf; cov is C / n."""
    import torch
    from bolt_amd.mi355x import _lib, reduction
    from bolt_amd.mi355x._ops import backend_for, dtype_code
    dev = bolt.array(np.zeros(2, dtype=np.float32), bctx)._device
    be = backend_for(dev)
    st = np.array([[1.0, 1.0, 1.0], [0.0, 4.0, 0.0], [1e-20, 2.0, -1e-20]])  # mean, M2, C of three records
    for what, want in ((_lib.CO_CORR, [np.nan, 2.0 / np.sqrt(4.0 * 2.0), np.nan]), (_lib.CO_COV, [1.25e-21, 0.25, -1.25e-21])):
        states = torch.from_numpy(st.reshape(-1).copy().view(np.uint8)).to(dev)
        out = torch.zeros(3 * 8, dtype=torch.uint8, device=dev)
        reduction.comoment_combine(be, what, states, [8], [[0.5]], [[2.0]], 3, 1, out, np.dtype(np.float64),
                                   dtype_code(np.float64))
        got = out.cpu().numpy().view(np.float64)
        np.testing.assert_allclose(got, want, rtol=1e-15, equal_nan=True)


def test_empty_arrays(bctx):
    for dtype in ("float32", "uint8"):
        odt = S.out_dtype(dtype)
        for name in METHODS:
            # no records: nan; no outputs: an empty result
            r = np.asarray(getattr(bolt.array(np.zeros((4, 0), dtype=dtype), bctx), name)(np.zeros(0), axis=1))
            assert r.shape == (4,) and r.dtype == odt and np.isnan(r).all()
            r = np.asarray(getattr(bolt.array(np.zeros((4, 0), dtype=dtype), bctx), name)(np.zeros((2, 0)), axis=1))
            assert r.shape == (2, 4) and np.isnan(r).all()
            r = np.asarray(getattr(bolt.array(np.zeros((0, 5), dtype=dtype), bctx), name)(np.arange(5.0), axis=1))
            assert r.shape == (0,) and r.dtype == odt
            r = np.asarray(getattr(bolt.array(np.zeros((4, 0), dtype=dtype), bctx), name)(np.arange(4.0), axis=0))
            assert r.shape == (0,) and r.dtype == odt


# ----------------------------------------------------------------- 5. arguments
def test_bad_signals_raise_before_any_launch(bctx, monkeypatch):
    x = S.rand((4, 6, 5), "float32")
    b = bolt.array(x, bctx)
    be = _backend(b)

    def boom(*a, **k):
        raise AssertionError("a launch before the arguments were checked")
    for name in ("comoment_state", "comoment_combine", "reduce_state", "reduce", "reduce_rows", "permute",
                 "copy_strided"):
        if hasattr(be, name):
            monkeypatch.setattr(be, name, boom, raising=False)
    bad = [
        (np.zeros(5), 1),                        # wrong extent
        (np.zeros((6, 1)), 1),                   # wrong ndim / extents
        (np.zeros((2, 3, 6)), 1),                # too many axes
        (np.zeros((0, 6)), 1),                   # K = 0
        (np.zeros((5, 4)), (0, 2)),              # the reduced extents in the wrong order
        (np.zeros(6, dtype=np.complex64), 1),    # complex
        (np.array([None] * 6, dtype=object), 1),  # object
        (np.array([0, 1, np.nan, 3, 4, 5.0]), 1),  # non-finite
        (np.array([0, 1, np.inf, 3, 4, 5.0]), 1),
        (np.zeros(6), None),                     # every axis needs the whole shape
    ]
    for y, axis in bad:
        for name in METHODS:
            with pytest.raises(ValueError):
                getattr(b, name)(y, axis=axis)
    for badaxis in (3, (0, 5), -4):
        with pytest.raises(Exception) as want:
            b.mean(axis=badaxis)
        for name in METHODS:
            with pytest.raises(type(want.value)):
                getattr(b, name)(np.zeros(4), axis=badaxis)
    monkeypatch.undo()
    # lists, ints and bools are array-like and real
    for y in ([1, 2, 4, 8, 7, 1], np.array([1, 0, 0, 1, 1, 0], dtype=bool)):
        S.check_values(np.asarray(b.corr(y, axis=1)), x, np.asarray(y, dtype=np.float64), 1, "corr", "array-like")


# ----------------------------------------------------------- 6. row-padded input
def _nan_pad(s, rows, R):
    """Fill the pad of a row-padded array's buffer with nan."""
    from bolt_amd.mi355x.functional import view
    P = s.__dict__["_pitch"]
    view(s.__dict__["_pbuf"], (rows, P), s.dtype)[:, R:] = float("nan")


def test_row_padded(bctx):
    z = S.rand((500, 3, 4), "float32", seed=3)
    s = bolt.array(z, bctx).swap((0,), (0, 1))
    xs = np.ascontiguousarray(z.transpose(1, 2, 0))
    assert s.__dict__.get("_pitch") == 512 and "_data" not in s.__dict__
    _nan_pad(s, 12, 500)
    S.check_both(s, xs, 2, "padded axis 2")
    assert "_pbuf" in s.__dict__ and "_data" not in s.__dict__  # the rows were read in place
    ys = S.signals(xs, 2, k=3)
    got = np.asarray(s.corr(ys, axis=2))
    assert np.isfinite(got).all() and got.shape == (3, 3, 4)
    # columns over the padded rows: the pad columns' (nan) outputs are dropped
    for axis in (0, (0, 1)):
        S.check_both(s, xs, axis, "padded axis %s" % (axis,))
    if bctx.world_size == 1:
        assert "_data" not in s.__dict__
    # axes that are not one block are permuted out of the padded rows; every axis may compact, as sum() does
    for axis in ((0, 2), None):
        S.check_both(s, xs, axis, "padded axis %s" % (axis,))


def test_moment_states_untouched(bctx):
    x = S.rand((6, 5, 7), "float32", seed=2)
    b = bolt.array(x, bctx)
    b.mean(axis=2)
    kept = dict(b.__dict__.get("_kept", {}))
    before = set(b.__dict__)
    b.corr(S.signals(x, 2)[0], axis=2)
    b.cov(S.signals(x, 2), axis=2)
    assert dict(b.__dict__.get("_kept", {})).keys() == kept.keys() and set(b.__dict__) == before
    assert b.toarray().tobytes() == x.tobytes()


# --------------------------------------------------------------- 7. determinism
def test_deterministic(bctx):
    for shape, axis in (((5, 300), 1), ((2, 50000), 1), ((300, 7, 5), 0), ((6, 5, 7), (0, 2))):
        x = S.rand(shape, "float32", seed=9)
        b = bolt.array(x, bctx)
        ys = S.signals(x, axis)
        for name in METHODS:
            f = getattr(b, name)
            assert np.asarray(f(ys, axis=axis)).tobytes() == np.asarray(f(ys, axis=axis)).tobytes()


# ------------------------------------------------------- 8. stores stay inside
@pytest.mark.gpu
def test_state_and_workspace_guards():
    """bm_comoment_state writes its state and its workspace and nothing around
    them: guard regions before, between and after keep their bytes."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from bolt_amd.mi355x import _lib
    from bolt_amd.mi355x._ops import backend_for, dtype_code
    dev = torch.device("cuda:0")
    be = backend_for(dev)
    G = 4096
    rng = np.random.default_rng(0)
    # the last two sources start 8 B / 4 B past a 16-B boundary: narrower vectors
    # than the workspace query plans with, the same chunks and workspace
    # (float64 columns: vec 1, 32 row phases instead of vec 2, 64; 39 chunks both)
    for (O, R, I), K, dt, off in (((2, 50000, 1), 3, np.float32, 0), ((1, 300, 35), 2, np.float32, 0),
                                  ((5, 300, 1), 4, np.float32, 0), ((1, 40, 600), 1, np.float32, 0),
                                  ((1, 20000, 8), 1, np.float64, 8), ((2, 4100, 1), 2, np.float32, 4)):
        x = rng.standard_normal((O, R, I)).astype(dt)
        y = rng.standard_normal((K, R))
        n = ctypes.c_size_t(0)
        assert be.lib.bm_comoment_workspace_bytes(dtype_code(dt), O, R, I, K, ctypes.byref(n)) == 0
        sbytes, wbytes = (2 + K) * O * I * 8, n.value
        wpad = -(-wbytes // 256) * 256
        buf = torch.full((3 * G + sbytes + wpad,), 0xA5, dtype=torch.uint8, device=dev)
        state = buf[G:G + sbytes]
        ws = buf[2 * G + sbytes:2 * G + sbytes + wbytes]
        src = torch.empty(off + x.nbytes, dtype=torch.uint8, device=dev)[off:]
        src.copy_(torch.from_numpy(x.reshape(-1).view(np.uint8)))
        assert src.data_ptr() % 16 == off
        ym = [float(v) for v in y.mean(axis=1)]
        be.comoment_state(src, dtype_code(dt), O, R, I, R, torch.from_numpy(y.reshape(-1)).to(dev), ym,
                          [0.0] * K, state, workspace=ws if wbytes else None)
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        assert (host[:G] == 0xA5).all() and (host[G + sbytes:2 * G + sbytes] == 0xA5).all()
        assert (host[2 * G + sbytes + wbytes:] == 0xA5).all()
        st = host[G:G + sbytes].view(np.float64).reshape(2 + K, O * I)
        xd = x.astype(np.float64)
        d = xd - xd.mean(axis=1, keepdims=True)
        np.testing.assert_allclose(st[0], xd.mean(axis=1).reshape(-1), rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(st[1], (d * d).sum(axis=1).reshape(-1), rtol=1e-11)
        for k in range(K):
            want = (d * (y[k] - y[k].mean()).reshape(1, R, 1)).sum(axis=1).reshape(-1)
            np.testing.assert_allclose(st[2 + k], want, rtol=1e-9, atol=1e-9 * np.abs(d).max() * R ** 0.5)
