"""center() / zscore(): every record minus its mean [over its standard
deviation] along an axis, as a device array of the same shape.

Runs on the CPU test executor as it is (tests/cpu_backend.py has neither entry
point: the methods' fallback), on a subclass of it with bm_standardize_rows /
bm_standardize_apply in numpy (the orchestration the HIP backend takes: pitches,
rows not taken, float64 planes) and, marked gpu, on the HIP kernels.  The truth
is float128; the tolerance is standardize_cases.truth_and_bound's.
"""
import numpy as np
import pytest

import bolt_amd as bolt
import standardize_cases as S
from standardize_cases import METHODS


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


def _both(b, x, axis, tag):
    for name in METHODS:
        S.check_array(getattr(b, name)(axis=axis), b, x, axis, name == "zscore", tag)


# (dtype, shape, axis) in named groups, each the smallest shape that reaches its
# branch; the plan of each was worked out from bm_standardize.hip (rows: vec =
# widest of 16 B / item, at most 8 elements, dividing R and both pitches; a
# thread holds min(8 vec, 32) elements; wave per row up to 64 x that, block per
# row up to 256 x that with at least 256 rows, else not taken) and from
# plan_reduce (bm_reduce.hip) for the two-pass moments, as test_stats_fused names them
SHAPES = [
    "rows_wave",
    ("float32", (5, 300), 1),        # vec 4: 16-B loads and stores
    ("float32", (5, 301), 1),        # vec 1 (odd R): scalar loads and stores
    ("float64", (4, 130), 1),        # vec 2
    ("float16", (3, 64), 1),         # vec 8, shorter than one wave-wide step (64 x 8)
    ("float32", (1, 7), 1),          # one row, 7 of 64 lanes
    ("uint8", (7, 260), 1),          # vec 4 (260 % 8 != 0): 4-B loads, float64 out in two 16-B stores
    ("uint16", (7, 264), 1),         # vec 8: 16-B loads, four 16-B stores
    ("int32", (7, 260), 1),          # vec 4, item size 4 -> 8
    ("int64", (7, 260), 1),          # vec 2, item size kept
    ("bool", (40, 9), 1),            # through the uint8 kernels, vec 1
    "rows_thresholds",
    # float32, R % 4 == 0: vec 4, 32 elements a thread: wave <= 2048 < block <= 8192
    ("float32", (3, 2044), 1),       # wave
    ("float32", (3, 2048), 1),       # wave, at its limit
    ("float32", (3, 2052), 1),       # beyond a wave, 3 rows < 256: not taken -> two-pass
    # float32, odd R: vec 1, 8 elements a thread: wave <= 512 < block <= 2048
    ("float32", (3, 511), 1),        # wave, vec 1
    ("float32", (3, 513), 1),        # not taken (3 rows)
    ("float32", (256, 513), 1),      # block per row, vec 1, first length past the wave
    ("float32", (256, 2047), 1),     # block per row, vec 1, one below its limit
    ("float32", (256, 2049), 1),     # vec 1, past the block's 2048: not taken
    ("float32", (256, 2052), 1),     # block per row, vec 4, first length past the wave
    ("float32", (255, 2052), 1),     # one row short of a block each: not taken
    ("float32", (256, 8192), 1),     # block per row at its limit
    ("float32", (256, 8196), 1),     # past it: not taken
    ("float32", (2, 50000), 1),      # far past the on-chip limit: not taken, rows in 2 chunks each
    "columns",
    ("float32", (300, 7, 5), 0),     # I = 35: apply vec 1; moments in 9 chunks
    ("float32", (64, 8, 16), 0),     # I = 128: apply vec 4
    ("float32", (6, 50, 10), 1),     # O = 6 > 1, apply vec 2
    ("float64", (20000, 8), 0),      # apply vec 2, moments in 39 chunks
    ("uint8", (300, 7, 5), 0),       # exact integer moments, float64 out
    "permuted",
    ("float32", (6, 5, 7), (0, 2)),  # permuted to the front, applied, permuted back
    ("uint8", (300, 7, 5), (0, 2)),  # the permute back moves 8-byte items
    "every_axis",
    ("float32", (200000,), None),    # one row of 200000: not taken; moments in 195 chunks, apply rows vec 4
    ("bool", (40, 9), None),
    ("float32", (6, 5, 7), None),    # one row of 210: wave per row
]
_PLAN = {(3, 2044): "wave", (3, 2048): "wave", (3, 2052): None, (3, 511): "wave", (3, 513): None,
         (256, 513): "block", (256, 2047): "block", (256, 2049): None, (256, 2052): "block",
         (255, 2052): None, (256, 8192): "block", (256, 8196): None, (2, 50000): None}


def _group(name):
    at = SHAPES.index(name) + 1
    out = []
    while at < len(SHAPES) and not isinstance(SHAPES[at], str):
        out.append(SHAPES[at])
        at += 1
    return out


# ------------------------------------------------------------------ 1. values
@pytest.mark.parametrize("group", [g for g in SHAPES if isinstance(g, str)])
def test_values(bctx, group, monkeypatch):
    shapes = _group(group)
    assert shapes
    for dtype, shape, axis in shapes:
        x = S.rand(shape, dtype, seed=len(shape) + shape[0])
        b = bolt.array(x, bctx)
        be = _backend(b)
        taken = []
        if hasattr(be, "standardize_rows"):
            inner = be.standardize_rows
            monkeypatch.setattr(be, "standardize_rows", lambda *a, _f=inner: taken.append(_f(*a)) or taken[-1],
                                raising=False)
        _both(b, x, axis, "%s %s axis %s" % (dtype, shape, axis))
        if group == "rows_thresholds":
            # the thresholds named above are the kernels' (and the numpy executor's)
            assert S.rows_plan(4, *shape) == _PLAN[shape], shape
            if hasattr(be, "standardize_rows"):
                assert taken == [_PLAN[shape] is not None] * 2, (shape, taken)
        elif group == "rows_wave" and hasattr(be, "standardize_rows"):
            assert taken == [True, True], (shape, taken)
        monkeypatch.undo()


def test_offset_data(bctx):
    """float32 1e6 + N(0,1): the mean must not lose the deviations' digits."""
    for shape, axis in (((5, 300), 1), ((300, 7, 5), 0), ((6, 5, 7), (0, 2))):
        x = S.rand(shape, "float32", seed=11, offset=1e6)
        _both(bolt.array(x, bctx), x, axis, "offset %s axis %s" % (shape, axis))


def test_key_value_splits(bctx):
    x = S.rand((6, 5, 7), "float32", seed=2)
    for kaxes in ((0,), (0, 1)):
        b = bolt.array(x, bctx, axis=kaxes)
        assert b.split == len(kaxes)
        for axis in (2, 0, (1, 2), None):
            _both(b, x, axis, "split %d axis %s" % (b.split, axis))
    # the input keeps its records and whatever moment state it had
    b = bolt.array(x, bctx)
    b.mean(axis=2)
    kept = dict(b.__dict__.get("_kept", {}))
    r = b.zscore(axis=2)
    assert dict(b.__dict__.get("_kept", {})).keys() == kept.keys() and "_kept" not in r.__dict__
    assert b.toarray().tobytes() == x.tobytes()


# ---------------------------------------------------------- 2. row-padded input
def test_row_padded(bctx):
    z = S.rand((500, 3, 4), "float32", seed=3)
    s = bolt.array(z, bctx).swap((0,), (0, 1))
    xs = np.ascontiguousarray(z.transpose(1, 2, 0))
    assert s.__dict__.get("_pitch") == 512 and "_data" not in s.__dict__
    fused = hasattr(_backend(s), "standardize_rows")
    for name in METHODS:
        r = getattr(s, name)(axis=2)
        if fused:
            # the same item size: padded like the input, rows of 500 at 512
            assert "_pbuf" in r.__dict__ and r.__dict__["_pitch"] == 512 and "_data" not in r.__dict__
        S.check_array(r, s, xs, 2, name == "zscore", "padded axis 2")
        assert "_pbuf" in s.__dict__ and "_data" not in s.__dict__
    for axis in (0, (0, 2), None):
        _both(s, xs, axis, "padded axis %s" % (axis,))
        assert "_pbuf" in s.__dict__ and "_data" not in s.__dict__, axis
    # item size 1 -> 8: a dense float64 result, the padded rows still read in place
    u = S.rand((2000, 2, 2), "uint8", seed=4)
    su = bolt.array(u, bctx).swap((0,), (0, 1))
    assert "_pbuf" in su.__dict__
    us = np.ascontiguousarray(u.transpose(1, 2, 0))
    for name in METHODS:
        r = getattr(su, name)(axis=2)
        assert "_pbuf" not in r.__dict__ and r.dtype == np.float64
        S.check_array(r, su, us, 2, name == "zscore", "padded uint8 axis 2")
    assert "_pbuf" in su.__dict__ and "_data" not in su.__dict__


# ------------------------------------------------------ 3. one read, one write
_COUNTED = ("standardize_rows", "standardize_apply", "reduce", "reduce_rows", "reduce_moments", "reduce_state",
            "reduce_combine", "reduce_combine_moments", "permute", "copy_strided")


def _counting(monkeypatch, be):
    calls = dict.fromkeys(_COUNTED, 0)

    def proxy(name, fn):
        def call(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return call
    for name in _COUNTED:
        if hasattr(be, name):
            monkeypatch.setattr(be, name, proxy(name, getattr(be, name)), raising=False)
    return calls


def test_one_read_one_write(bctx, monkeypatch):
    x = S.rand((500, 3, 4), "float32", seed=5)
    dense = bolt.array(np.ascontiguousarray(x.transpose(1, 2, 0)), bctx)
    padded = bolt.array(x, bctx).swap((0,), (0, 1))
    assert "_pbuf" in padded.__dict__
    be = _backend(dense)
    fused = hasattr(be, "standardize_rows")
    for arr in (dense, padded):
        for name in METHODS:
            with monkeypatch.context() as mp:
                calls = _counting(mp, be)
                getattr(arr, name)(axis=2)
            if fused:
                # one launch reads the rows and writes the result
                assert calls.pop("standardize_rows") == 1
                assert not any(calls.values()), calls
            else:
                # the fallback: one state read, the apply in torch
                assert calls["reduce_state"] == 1 and calls["reduce"] == calls["reduce_rows"] == 0
                assert calls["permute"] == 0 and calls["copy_strided"] == (1 if arr is padded else 0)
    cols = bolt.array(x, bctx)
    for name in METHODS:
        with monkeypatch.context() as mp:
            calls = _counting(mp, be)
            getattr(cols, name)(axis=0)
        # one moments launch sequence, then one apply
        assert calls["reduce_moments"] + calls["reduce_state"] == 1
        assert calls["reduce"] == calls["reduce_rows"] == calls["permute"] == calls["copy_strided"] == 0
        assert calls["standardize_rows"] == 0 and calls["standardize_apply"] == (1 if fused else 0)


# ------------------------------------------------------- 4. degenerate records
def test_degenerate_records(bctx):
    x = S.rand((3, 64), "float32", seed=6)
    x[1] = 2.5
    b = bolt.array(x, bctx)
    c, z = b.center(axis=1).toarray(), b.zscore(axis=1).toarray()
    assert c.dtype == z.dtype == np.float32
    assert np.all(c[1] == 0.0) and np.isnan(z[1]).all()
    for row in (0, 2):
        S.check_values(c[row:row + 1], x[row:row + 1], 1, False, "row %d" % row)
        S.check_values(z[row:row + 1], x[row:row + 1], 1, True, "row %d" % row)
    # the same row as a column (the two-pass path)
    bt = bolt.array(np.ascontiguousarray(x.T), bctx)
    ct, zt = bt.center(axis=0).toarray(), bt.zscore(axis=0).toarray()
    assert np.all(ct[:, 1] == 0.0) and np.isnan(zt[:, 1]).all() and np.isfinite(zt[:, (0, 2)]).all()
    # a reduced axis of one element
    one = bolt.array(S.rand((4, 1), "float32", seed=7), bctx)
    assert np.all(one.center(axis=1).toarray() == 0.0) and one.center(axis=1).shape == (4, 1)
    assert np.isnan(one.zscore(axis=1).toarray()).all()
    # a nan spoils its own record only
    y = S.rand((3, 64), "float32", seed=8)
    y[1, 17] = np.nan
    by = bolt.array(y, bctx)
    for name in METHODS:
        got = getattr(by, name)(axis=1).toarray()
        assert np.isnan(got[1]).all()
        for row in (0, 2):
            S.check_values(got[row:row + 1], y[row:row + 1], 1, name == "zscore", "beside a nan, row %d" % row)
        gt = getattr(bolt.array(np.ascontiguousarray(y.T), bctx), name)(axis=0).toarray()
        assert np.isnan(gt[:, 1]).all() and np.isfinite(gt[:, (0, 2)]).all()


def test_empty_arrays(bctx):
    for shape, axis in (((0, 5), 1), ((4, 0), 1), ((4, 0), 0)):
        for dtype in ("float32", "uint8"):
            b = bolt.array(np.zeros(shape, dtype=dtype), bctx)
            for name in METHODS:
                r = getattr(b, name)(axis=axis)
                assert type(r) is type(b) and r.shape == shape and r.dtype == S.out_dtype(dtype)
                got = r.toarray()
                assert got.shape == shape and got.dtype == S.out_dtype(dtype)


# ----------------------------------------------------------------- 5. arguments
def test_bad_arguments(bctx):
    b = bolt.array(S.rand((4, 6), "float32"), bctx)
    for bad in (2, (0, 5), -3):
        with pytest.raises(Exception) as want:
            b.mean(axis=bad)
        for name in METHODS:
            with pytest.raises(type(want.value)):
                getattr(b, name)(axis=bad)
    c = bolt.array(np.ones((3, 4), dtype=np.complex64), bctx)
    for name in METHODS:
        with pytest.raises(NotImplementedError):
            getattr(c, name)(axis=0)
        with pytest.raises(TypeError):
            getattr(b, name)(axis=0, keepdims=True)  # the result has the array's shape


# --------------------------------------------------------------- 6. determinism
def test_deterministic(bctx):
    for shape, axis in (((5, 300), 1), ((256, 2052), 1), ((300, 7, 5), 0), ((6, 5, 7), (0, 2))):
        x = S.rand(shape, "float32", seed=9)
        b = bolt.array(x, bctx)
        for name in METHODS:
            assert getattr(b, name)(axis=axis).toarray().tobytes() == getattr(b, name)(axis=axis).toarray().tobytes()
        # zscore's numerator is center: center / std meets zscore's bound
        c = b.center(axis=axis).toarray().astype(np.longdouble)
        sd = np.sqrt(x.astype(np.longdouble).var(axis=axis, keepdims=True))
        z = b.zscore(axis=axis).toarray().astype(np.longdouble)
        _, bound = S.truth_and_bound(x, axis, True)
        assert np.all(np.abs(c / sd - z) <= 2 * bound), (shape, axis)
