"""normalize(): every record against its own baseline, (x - b) / (b + offset),
b the record's percentile or mean along an axis, as a device array of the same
shape.

Runs on the CPU test executor as it is (tests/cpu_backend.py has none of the
entry points: the methods' fallbacks), on a subclass of it with
bm_normalize_rows next to the standardize and quantile entry points in numpy
(the orchestration the HIP backend takes: pitches, rows not taken, float64
baseline planes) and, marked gpu, on the HIP kernels.  'percentile' is compared
bit for bit with the numpy restatement (normalize_cases.percentile_truth) on
every route; 'mean' against a longdouble truth within
normalize_cases.mean_truth_and_bound.

The three normalize test modules are named to be collected after every other
module, as test_zz_swap_moments is: no existing test changes its place in the
suite's order.
"""
import numpy as np
import pytest

import bolt_amd as bolt
import normalize_cases as N
import quantile_cases as Q
import test_standardize as TS


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
        register_backend("cpu", N.fused_backend())
    else:
        cpu_backend.install()
    yield MI355XContext(device="cpu")
    cpu_backend.install()  # the plain executor again, for the modules that follow


def _backend(arr):
    from bolt_amd.mi355x._ops import backend_for
    return backend_for(arr._device)


def _public(be):
    return [n for n in dir(be) if not n.startswith("_") and callable(getattr(be, n))]


def _counting(monkeypatch, be):
    """Every public method of the backend behind a counter -> {name: calls}."""
    calls = {}

    def proxy(name, fn):
        def call(*a, **k):
            calls[name] = calls.get(name, 0) + 1
            return fn(*a, **k)
        return call
    for name in _public(be):
        monkeypatch.setattr(be, name, proxy(name, getattr(be, name)), raising=False)
    return calls


# ------------------------------------------------------------------ 1. values
# test_standardize's shapes as they stand: the rows plan is the same
# (normalize_cases.rows_plan), and so are the layouts behind the other groups
@pytest.mark.parametrize("group", [g for g in TS.SHAPES if isinstance(g, str)])
def test_values(bctx, group, monkeypatch):
    shapes = TS._group(group)
    assert shapes
    for dtype, shape, axis in shapes:
        x = N.rand(shape, dtype, seed=len(shape) + shape[0])
        b = bolt.array(x, bctx)
        be = _backend(b)
        taken, plans = [], []
        if hasattr(be, "normalize_rows"):
            def rows(*a, _f=be.normalize_rows, _es=x.dtype.itemsize):
                # (src, code, O, R, src_pitch, baseline, rank, frac, offset, dst, out_code, dst_pitch)
                plans.append(N.rows_plan(_es, a[2], a[3], a[4], a[11]) is not None)
                taken.append(_f(*a))
                return taken[-1]
            monkeypatch.setattr(be, "normalize_rows", rows, raising=False)
        N.check_both(b, x, axis, "%s %s axis %s" % (dtype, shape, axis))
        assert taken == plans, (shape, taken, plans)   # every call the launch got, against the mirrored plan
        if group == "rows_thresholds":
            # the thresholds test_standardize names are this kernel's too (and the numpy executor's)
            assert N.rows_plan(4, *shape) == TS._PLAN[shape], shape
            if hasattr(be, "normalize_rows"):
                assert taken == [TS._PLAN[shape] is not None] * 2, (shape, taken)
        elif group == "rows_wave" and hasattr(be, "normalize_rows"):
            assert taken == [True, True], (shape, taken)
        monkeypatch.undo()


# pos = (perc / 100)(n - 1): whole for every perc here on 11 values, for 0 and 100 only on 12
_G_ZERO = {(11, 0): True, (11, 100): True, (11, 20): True, (11, 50): True,
           (12, 0): True, (12, 100): True, (12, 20): False, (12, 50): False}


def test_percentiles(bctx):
    """perc 0, 100, 20 and 50 over an odd and an even count, so that the
    baseline is one of the record's values (g == 0) and an interpolated one,
    as rows (one launch) and as columns (the baseline plane, then the apply)."""
    for n in (11, 12):
        for shape, axis in (((5, n), 1), ((n, 6), 0)):
            for dtype in ("float32", "uint8", "float16"):
                x = N.rand(shape, dtype, seed=n)
                b = bolt.array(x, bctx)
                for perc in (0, 100, 20, 50):
                    _, g = N.percentile_baseline(x, axis, perc)
                    assert (g == 0.0) == _G_ZERO[(n, perc)], (n, perc, g)
                    N.check_percentile(b.normalize(axis=axis, perc=perc), b, x, axis, perc, 0.1,
                                       "%s %s axis %d" % (dtype, shape, axis))
    # the defaults: the percentile baseline, perc 20, offset 0.1
    x = N.rand((5, 12), "float32", seed=1)
    b = bolt.array(x, bctx)
    assert b.normalize(axis=1).toarray().tobytes() == \
        b.normalize(axis=1, method="percentile", perc=20, offset=0.1).toarray().tobytes()
    N.check_percentile(b.normalize(axis=1), b, x, 1)
    # the float32 baseline is not rounded to float32: an interpolated one differs from percentile()'s result
    bl, g = N.percentile_baseline(x, 1, 20)
    assert g != 0.0 and np.any(bl.astype(np.float32).astype(np.float64) != bl)


def test_offsets_and_offset_data(bctx):
    """offset negative and 0; float32 1e6 + N(0,1), where the baseline must keep the deviations' digits."""
    x = N.rand((5, 300), "float32", seed=3)
    b = bolt.array(x, bctx)
    for offset in (-0.5, 0, 0.0, 2):
        N.check_both(b, x, 1, "offsets", offset=offset)
    for shape, axis in (((5, 300), 1), ((300, 7, 5), 0), ((6, 5, 7), (0, 2))):
        x = N.rand(shape, "float32", seed=11, offset=1e6)
        N.check_both(bolt.array(x, bctx), x, axis, "offset data %s axis %s" % (shape, axis))


def test_key_value_splits(bctx):
    x = N.rand((6, 5, 7), "float32", seed=2)
    for kaxes in ((0,), (0, 1)):
        b = bolt.array(x, bctx, axis=kaxes)
        assert b.split == len(kaxes)
        for axis in (2, 0, (1, 2), None):
            N.check_both(b, x, axis, "split %d axis %s" % (b.split, axis))
    # the input keeps its records and whatever moment state it had; the result has none
    b = bolt.array(x, bctx)
    b.mean(axis=2)
    kept = dict(b.__dict__.get("_kept", {}))
    for method in N.METHODS:
        r = b.normalize(axis=2, method=method)
        assert dict(b.__dict__.get("_kept", {})).keys() == kept.keys() and "_kept" not in r.__dict__
    assert b.toarray().tobytes() == x.tobytes()


# ---------------------------------------------------------- 2. special records
def test_special_records(bctx):
    # one value a record: x - b is 0 for either baseline
    x1 = N.rand((4, 1), "float32", seed=7)
    b1 = bolt.array(x1, bctx)
    for method in N.METHODS:
        r = b1.normalize(axis=1, method=method)
        assert r.shape == (4, 1) and np.all(r.toarray() == 0.0)
    N.check_percentile(b1.normalize(axis=1), b1, x1, 1)
    # a record of equal values, beside ordinary ones: zeros
    x = N.rand((3, 64), "float32", seed=6)
    x[1] = 2.5
    for arr, axis in ((x, 1), (np.ascontiguousarray(x.T), 0)):
        b = bolt.array(arr, bctx)
        N.check_both(b, arr, axis, "equal values axis %d" % axis)
        for method in N.METHODS:
            got = b.normalize(axis=axis, method=method).toarray()
            assert np.all((got[1] if axis == 1 else got[:, 1]) == 0.0)
    # a NaN spoils its own record only, on the rows and on the columns route
    y = N.rand((3, 64), "float32", seed=8)
    y[1, 17] = np.nan
    clean = np.ascontiguousarray(y[(0, 2), :])
    t, bound = N.mean_truth_and_bound(clean, 1, 0.1)
    for arr, axis in ((y, 1), (np.ascontiguousarray(y.T), 0)):
        b = bolt.array(arr, bctx)
        N.check_percentile(b.normalize(axis=axis), b, arr, axis, tag="beside a nan")   # (the truth has the NaN row)
        for method in N.METHODS:
            got = b.normalize(axis=axis, method=method).toarray()
            rows = got if axis == 1 else got.T
            assert np.isnan(rows[1]).all() and np.isfinite(rows[(0, 2), :]).all(), (method, axis)
        assert np.all(np.abs(rows[(0, 2), :].astype(np.longdouble) - t) <= bound), axis   # ('mean', the last method)
    # zeros of both signs: they order -0.0 before +0.0 and compare equal; the result is the restatement's
    z = N.rand((4, 40), "float32", seed=9)
    z[1, ::2], z[1, 1::2] = -0.0, 0.0
    z[2, :30], z[2, 30:] = -0.0, np.abs(z[2, 30:])
    bz = bolt.array(z, bctx)
    for perc in (0, 20, 50):
        N.check_percentile(bz.normalize(axis=1, perc=perc), bz, z, 1, perc)
    # an integer record whose baseline is -offset: b + offset == 0 gives inf and, where x == b, nan, as numpy
    u = np.arange(-3, 17, dtype=np.int32).reshape(1, 20).repeat(3, axis=0)
    u[1] += 5
    u[2] += 7
    bu = bolt.array(u, bctx)
    got = N.check_percentile(bu.normalize(axis=1, perc=0, offset=3), bu, u, 1, 0, 3)   # b = -3
    assert np.isnan(got[0, 0]) and np.isposinf(got[0, 1:]).all() and np.isfinite(got[1:]).all()
    got = bu.normalize(axis=1, method="mean", offset=-6.5).toarray()                      # the mean is 6.5
    assert np.isinf(got[0]).all() and np.isfinite(got[1:]).all()
    # float16 in, float16 out; int64 beyond 2^53 rounds on conversion, as the restatement does
    h = N.rand((3, 64), "float16", seed=10)
    N.check_both(bolt.array(h, bctx), h, 1, "float16")
    w = (np.int64(1) << 60) + np.arange(7 * 36, dtype=np.int64).reshape(7, 36) * 1001
    N.check_percentile(bolt.array(w, bctx).normalize(axis=1, perc=50), bolt.array(w, bctx), w, 1, 50)


def test_empty_arrays(bctx):
    for shape, axis in (((0, 5), 1), ((4, 0), 1), ((4, 0), 0)):
        for dtype in ("float32", "uint8"):
            b = bolt.array(np.zeros(shape, dtype=dtype), bctx)
            for method in N.METHODS:
                r = b.normalize(axis=axis, method=method)
                assert type(r) is type(b) and r.shape == shape and r.dtype == N.out_dtype(dtype)
                got = r.toarray()
                assert got.shape == shape and got.dtype == N.out_dtype(dtype)


# ---------------------------------------------------------- 3. row-padded input
def test_row_padded(bctx):
    z = N.rand((500, 3, 4), "float32", seed=3)
    s = bolt.array(z, bctx).swap((0,), (0, 1))
    xs = np.ascontiguousarray(z.transpose(1, 2, 0))
    assert s.__dict__.get("_pitch") == 512 and "_data" not in s.__dict__
    fused = hasattr(_backend(s), "normalize_rows")
    for method, check in (("percentile", N.check_percentile), ("mean", N.check_mean)):
        r = s.normalize(axis=2, method=method)
        if fused:
            # the same item size: padded like the input, rows of 500 at 512
            assert "_pbuf" in r.__dict__ and r.__dict__["_pitch"] == 512 and "_data" not in r.__dict__
        check(r, s, xs, 2, tag="padded axis 2")
        assert "_pbuf" in s.__dict__ and "_data" not in s.__dict__
    for axis in (0, (0, 2), None):
        N.check_both(s, xs, axis, "padded axis %s" % (axis,))
        assert "_pbuf" in s.__dict__ and "_data" not in s.__dict__, axis
    # item size 2 -> 8: a dense float64 result, the padded rows still read in place
    u = N.rand((1000, 2, 2), "uint16", seed=4)
    su = bolt.array(u, bctx).swap((0,), (0, 1))
    assert "_pbuf" in su.__dict__
    us = np.ascontiguousarray(u.transpose(1, 2, 0))
    for method, check in (("percentile", N.check_percentile), ("mean", N.check_mean)):
        r = su.normalize(axis=2, method=method)
        assert "_pbuf" not in r.__dict__ and r.dtype == np.float64
        check(r, su, us, 2, tag="padded uint16 axis 2")
    assert "_pbuf" in su.__dict__ and "_data" not in su.__dict__


# ------------------------------------------------------ 4. one read, one write
def test_routes(bctx, monkeypatch):
    """Rows the launch takes: that launch and nothing else.  Columns: the
    baseline plane stays on the device (one moments launch sequence, or one
    permute and the quantile rows), then one apply."""
    x = N.rand((500, 3, 4), "float32", seed=5)
    dense = bolt.array(np.ascontiguousarray(x.transpose(1, 2, 0)), bctx)
    padded = bolt.array(x, bctx).swap((0,), (0, 1))
    assert "_pbuf" in padded.__dict__
    be = _backend(dense)
    fused = hasattr(be, "normalize_rows")
    for arr in (dense, padded):
        for method in N.METHODS:
            with monkeypatch.context() as mp:
                calls = _counting(mp, be)
                arr.normalize(axis=2, method=method)
            if fused:
                assert calls == {"normalize_rows": 1}, calls
            else:
                assert "permute" not in calls and "standardize_rows" not in calls
    cols = bolt.array(x, bctx)
    for method in N.METHODS:
        with monkeypatch.context() as mp:
            calls = _counting(mp, be)
            cols.normalize(axis=0, method=method)
        assert calls.get("normalize_rows", 0) == 0 and calls.get("standardize_rows", 0) == 0
        assert calls.get("standardize_apply", 0) == (1 if fused else 0)
        if method == "mean":
            assert calls.get("reduce_moments", 0) + calls.get("reduce_state", 0) == 1 and "permute" not in calls
        else:
            assert calls.get("permute", 0) == 1   # the columns as rows, for the select
            if fused:
                assert calls.get("quantile_rows", 0) == 1


@pytest.mark.gpu
def test_one_launch_on_the_gpu(monkeypatch):
    """Over the last axis of a shape the kernel takes, normalize() is one call
    into the library -- bm_normalize_rows -- and neither the apply nor the
    quantile entry points."""
    import torch
    from bolt_amd import MI355XContext
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ctx = MI355XContext(device="cuda:0")
    x = N.rand((40, 2000), "float32", seed=12)
    b = bolt.array(x, ctx)
    be = _backend(b)
    assert N.rows_plan(4, 40, 2000) == "wave"
    for method in N.METHODS:
        with monkeypatch.context() as mp:
            calls = _counting(mp, be)
            r = b.normalize(axis=1, method=method)
        assert calls == {"normalize_rows": 1}, calls
        (N.check_percentile if method == "percentile" else N.check_mean)(r, b, x, 1, tag="one launch")


# ----------------------------------------------------------------- 5. arguments
def test_bad_arguments(bctx, monkeypatch):
    b = bolt.array(N.rand((4, 6), "float32"), bctx)
    be = _backend(b)

    def boom(*a, **k):
        raise AssertionError("a backend call before the arguments were checked")
    for name in _public(be):
        monkeypatch.setattr(be, name, boom, raising=False)
    for bad in ("median", "window", "window-exact", None, 20):
        with pytest.raises(ValueError):
            b.normalize(axis=1, method=bad)
    for bad in (-1, 100.5, float("nan"), float("inf"), "20", None, [20], (20, 30), 1j):
        with pytest.raises(ValueError):
            b.normalize(axis=1, perc=bad)
    for bad in (float("nan"), float("inf"), -float("inf"), "0.1", None, [0.1], 1j):
        for method in N.METHODS:
            with pytest.raises(ValueError):
                b.normalize(axis=1, method=method, offset=bad)
    # 'mean' does not look at perc
    monkeypatch.undo()
    b.normalize(axis=1, method="mean", perc=None)
    for name in _public(be):
        monkeypatch.setattr(be, name, boom, raising=False)
    for bad in (2, (0, 5), -3):
        with pytest.raises(Exception) as want:
            b.mean(axis=bad)
        for method in N.METHODS:
            with pytest.raises(type(want.value)):
                b.normalize(axis=bad, method=method)
    with pytest.raises(TypeError):
        b.normalize(axis=0, keepdims=True)  # the result has the array's shape
    monkeypatch.undo()
    c = bolt.array(np.ones((3, 4), dtype=np.complex64), bctx)
    for method in N.METHODS:
        with pytest.raises(NotImplementedError):
            c.normalize(axis=0, method=method)


# --------------------------------------------------------------- 6. determinism
def test_deterministic(bctx):
    for shape, axis in (((5, 300), 1), ((256, 2052), 1), ((300, 7, 5), 0), ((6, 5, 7), (0, 2))):
        x = N.rand(shape, "float32", seed=9)
        b = bolt.array(x, bctx)
        for method in N.METHODS:
            assert b.normalize(axis=axis, method=method).toarray().tobytes() == \
                b.normalize(axis=axis, method=method).toarray().tobytes()
    # the baseline is percentile()'s value where that is not rounded: float64 results
    u = N.rand((7, 260), "uint8", seed=9)
    bu = bolt.array(u, bctx)
    p = np.asarray(bu.percentile(20, axis=1))
    bl, _ = N.percentile_baseline(u, 1, 20)
    assert Q.same(p, bl.reshape(p.shape))
