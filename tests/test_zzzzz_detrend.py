"""detrend(): every record minus its least-squares polynomial of degree
``order`` along an axis (and its mean), as a device array of the same shape.

Runs on the CPU test executor as it is (tests/cpu_backend.py has none of the
entry points: the method's fallbacks), on a subclass of it with bm_detrend_rows
/ bm_detrend_apply next to the standardize and co-moment entry points in numpy
(the orchestration the HIP backend takes: pitches, rows not taken, float64
planes, the basis table) and, marked gpu, on the HIP kernels.  The truth is the
Gram-polynomial projection in longdouble; the tolerance is
detrend_cases.truth_and_bound's, the project's own for center().

The three detrend test modules are named to be collected after every other
module, as test_zzz_normalize is: no existing test changes its place in the
suite's order.
"""
import numpy as np
import pytest

import bolt_amd as bolt
import detrend_cases as D
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
        register_backend("cpu", D.fused_backend())
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


def _check(b, x, axis, order, tag=""):
    return D.check_array(b.detrend(axis=axis, order=order), b, x, axis, order, tag)


# ------------------------------------------------------------------ 1. values
# test_standardize's shapes as they stand: the rows plan is bm_standardize_rows'
# (detrend_cases.rows_plan), and so are the layouts behind the other groups.
# Orders 1 and 3 on every shape, 5 and 8 (two batches of co-moment signals on
# the two-pass routes) on the first shape of each group.
@pytest.mark.parametrize("group", [g for g in TS.SHAPES if isinstance(g, str)])
def test_values(bctx, group, monkeypatch):
    shapes = TS._group(group)
    assert shapes
    for at, (dtype, shape, axis) in enumerate(shapes):
        x = D.rand(shape, dtype, seed=len(shape) + shape[0])
        b = bolt.array(x, bctx)
        be = _backend(b)
        orders = (1, 3, 5, 8) if at == 0 else (1, 3)
        taken, plans = [], []
        if hasattr(be, "detrend_rows"):
            def rows(*a, _f=be.detrend_rows, _es=x.dtype.itemsize):
                # (src, code, O, R, src_pitch, order, dst, out_code, dst_pitch)
                plans.append(D.rows_plan(_es, a[2], a[3], a[4], a[8]) is not None)
                taken.append(_f(*a))
                return taken[-1]
            monkeypatch.setattr(be, "detrend_rows", rows, raising=False)
        for order in orders:
            _check(b, x, axis, order, "%s %s axis %s" % (dtype, shape, axis))
        assert taken == plans, (shape, taken, plans)   # every call the launch got, against the mirrored plan
        if group == "rows_thresholds":
            # the thresholds test_standardize names are this kernel's too (and the numpy executor's)
            assert D.rows_plan(4, *shape) == TS._PLAN[shape], shape
            if hasattr(be, "detrend_rows"):
                assert taken == [TS._PLAN[shape] is not None] * len(orders), (shape, taken)
        elif group == "rows_wave" and hasattr(be, "detrend_rows"):
            assert taken == [True] * len(orders), (shape, taken)
        monkeypatch.undo()


def test_truth_against_polyfit():
    """The truth (Gram projection, longdouble) against numpy's own polyfit
    residual over the abscissa scaled to [-1, 1]: within 1e-9 max|x|."""
    for shape in ((4, 7), (3, 64), (2, 2000)):
        x = D.rand(shape, "float64", seed=shape[1])
        for order in (1, 3, 5):
            t, _ = D.truth_and_bound(x, 1, order)
            want = D.polyfit_residual(x, order)
            err = float(np.abs(t - want).max())
            print("%s order %d: |truth - polyfit| = %.3g" % (shape, order, err))
            assert err <= 1e-9 * np.abs(x).max(), (shape, order, err)


# ---------------------------------------------------------- 2. exact polynomials
def _poly(n, coefs):
    r = np.arange(n, dtype=np.float64)
    return sum(c * r ** k for k, c in enumerate(coefs))


def test_exact_polynomials(bctx):
    """A float64 record that is a polynomial of degree <= order with small
    integer coefficients detrends to the bound's floor; one degree higher
    leaves the truth's residual.  As rows (one launch) and as columns."""
    n = 24
    rng = np.random.default_rng(5)
    for order in (1, 3, 5):
        rows = np.stack([_poly(n, rng.integers(-3, 4, size=deg + 1)) for deg in range(order + 1)] +
                        [_poly(n, list(rng.integers(-3, 4, size=order + 1)) + [2])])
        assert rows.dtype == np.float64
        for arr, axis in ((rows, 1), (np.ascontiguousarray(rows.T), 0)):
            b = bolt.array(arr, bctx)
            got = _check(b, arr, axis, order, "polynomials axis %d" % axis)
            got = got if axis == 1 else got.T
            floor = 1e-12 * np.abs(rows).max(axis=1, keepdims=True)
            assert np.all(np.abs(got[:-1]) <= 2 * floor[:-1] + 1e-300), (order, axis)
            t, _ = D.truth_and_bound(arr, axis, order)
            t = t if axis == 1 else t.T
            assert np.abs(t[-1]).max() > 1.0 and np.abs(got[-1]).max() > 1.0   # degree order + 1 stays
    # order = n - 1 interpolates: the residual is rounding noise
    for n in range(2, 10):
        x = D.rand((4, n), "float64", seed=n)
        for arr, axis in ((x, 1), (np.ascontiguousarray(x.T), 0)):
            got = _check(bolt.array(arr, bctx), arr, axis, n - 1, "interpolating n %d axis %d" % (n, axis))
            assert np.all(np.abs(got) <= 2e-12 * np.abs(x).max()), (n, axis)


def test_offset_data(bctx):
    """float32 1e6 + 0.01 r + N(0,1): the deviations are projected, not the
    values, so the offset costs no digits."""
    rng = np.random.default_rng(11)
    for shape, axis in (((5, 300), 1), ((300, 7, 5), 0), ((6, 5, 7), (0, 2))):
        ax = D.axes_of(np.empty(shape), axis)
        pos = np.arange(int(np.prod([shape[a] for a in ax]))).reshape([shape[a] for a in ax])
        pos = np.expand_dims(pos, [i for i in range(len(shape)) if i not in ax])
        x = (1e6 + 0.01 * pos + rng.standard_normal(shape)).astype(np.float32)
        b = bolt.array(x, bctx)
        for order in (1, 3):
            _check(b, x, axis, order, "offset %s axis %s" % (shape, axis))


def test_key_value_splits(bctx):
    x = D.rand((6, 5, 7), "float32", seed=2)
    for kaxes in ((0,), (0, 1)):
        b = bolt.array(x, bctx, axis=kaxes)
        assert b.split == len(kaxes)
        for axis in (2, 0, (1, 2), None):
            _check(b, x, axis, 2, "split %d axis %s" % (b.split, axis))


def test_no_state_left(bctx):
    """The input keeps its records and whatever moment state it had; the result has none."""
    x = D.rand((6, 5, 7), "float32", seed=2)
    b = bolt.array(x, bctx)
    b.mean(axis=2)
    kept = dict(b.__dict__.get("_kept", {}))
    before = set(b.__dict__)
    for axis, order in ((2, 1), (0, 3), ((0, 2), 5), (2, 0)):
        r = b.detrend(axis=axis, order=order)
        assert "_kept" not in r.__dict__
    assert dict(b.__dict__.get("_kept", {})).keys() == kept.keys() and set(b.__dict__) == before
    assert b.toarray().tobytes() == x.tobytes()


# ---------------------------------------------------------- 3. row-padded input
def test_row_padded(bctx, monkeypatch):
    z = D.rand((500, 3, 4), "float32", seed=3)
    s = bolt.array(z, bctx).swap((0,), (0, 1))
    xs = np.ascontiguousarray(z.transpose(1, 2, 0))
    assert s.__dict__.get("_pitch") == 512 and "_data" not in s.__dict__
    be = _backend(s)
    fused = hasattr(be, "detrend_rows")
    for order in (1, 3):
        with monkeypatch.context() as mp:
            calls = _counting(mp, be)
            r = s.detrend(axis=2, order=order)
        if fused:
            # the same item size: padded like the input, rows of 500 at 512; the source is never compacted
            assert "_pbuf" in r.__dict__ and r.__dict__["_pitch"] == 512 and "_data" not in r.__dict__
            assert calls == {"detrend_rows": 1}, calls
        D.check_array(r, s, xs, 2, order, "padded axis 2")
        assert "_pbuf" in s.__dict__ and "_data" not in s.__dict__
    for axis in (0, (0, 2), None):
        _check(s, xs, axis, 2, "padded axis %s" % (axis,))   # (axis 0 has 3 values a record)
        assert "_pbuf" in s.__dict__ and "_data" not in s.__dict__, axis
    # item size 1 -> 8: a dense float64 result, the padded rows still read in place
    u = D.rand((2000, 2, 2), "uint8", seed=4)
    su = bolt.array(u, bctx).swap((0,), (0, 1))
    assert "_pbuf" in su.__dict__
    us = np.ascontiguousarray(u.transpose(1, 2, 0))
    for order in (1, 3):
        r = su.detrend(axis=2, order=order)
        assert "_pbuf" not in r.__dict__ and r.dtype == np.float64
        D.check_array(r, su, us, 2, order, "padded uint8 axis 2")
    assert "_pbuf" in su.__dict__ and "_data" not in su.__dict__


# ------------------------------------------------------ 4. one read, one write
def test_launch_counts(bctx, monkeypatch):
    x = D.rand((500, 3, 4), "float32", seed=5)
    dense = bolt.array(np.ascontiguousarray(x.transpose(1, 2, 0)), bctx)
    padded = bolt.array(x, bctx).swap((0,), (0, 1))
    assert "_pbuf" in padded.__dict__
    be = _backend(dense)
    fused = hasattr(be, "detrend_rows")
    for arr in (dense, padded):
        with monkeypatch.context() as mp:
            calls = _counting(mp, be)
            arr.detrend(axis=2, order=3)
        if fused:
            assert calls == {"detrend_rows": 1}, calls   # one launch reads the rows and writes the result
        else:
            assert "permute" not in calls and "copy_strided" not in calls
    cols = bolt.array(x, bctx)
    for order, reads in ((3, 1), (5, 2)):
        with monkeypatch.context() as mp:
            calls = _counting(mp, be)
            cols.detrend(axis=0, order=order)
        assert "permute" not in calls and "copy_strided" not in calls and "detrend_rows" not in calls, calls
        if fused:
            assert calls == {"comoment_state": reads, "detrend_apply": 1}, calls


@pytest.mark.gpu
def test_one_launch_on_the_gpu(monkeypatch):
    """Over the last axis of a shape the kernel takes, detrend() is one call
    into the library -- bm_detrend_rows -- at every order."""
    import torch
    from bolt_amd import MI355XContext
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ctx = MI355XContext(device="cuda:0")
    x = D.rand((40, 2000), "float32", seed=12)
    b = bolt.array(x, ctx)
    be = _backend(b)
    assert D.rows_plan(4, 40, 2000) == "wave"
    for order in (1, 4, 8):
        with monkeypatch.context() as mp:
            calls = _counting(mp, be)
            r = b.detrend(axis=1, order=order)
        assert calls == {"detrend_rows": 1}, calls
        D.check_array(r, b, x, 1, order, "one launch")


# ------------------------------------------------------------- 5. order 0
def test_order_zero_is_center(bctx, monkeypatch):
    for shape, axis in (((5, 300), 1), ((300, 7, 5), 0), ((6, 5, 7), None)):
        x = D.rand(shape, "float32", seed=1)
        b = bolt.array(x, bctx)
        assert b.detrend(axis=axis, order=0).toarray().tobytes() == b.center(axis=axis).toarray().tobytes()
    seen = []
    monkeypatch.setattr(type(b), "center", lambda self, axis=None: seen.append(axis) or "centred")
    assert b.detrend(axis=1, order=0) == "centred" and seen == [1]   # through the same call


# ------------------------------------------------------- 6. degenerate records
def test_degenerate_records(bctx):
    x = D.rand((3, 64), "float32", seed=6)
    x[1] = 2.5
    for arr, axis in ((x, 1), (np.ascontiguousarray(x.T), 0)):
        b = bolt.array(arr, bctx)
        for order in (1, 3):
            got = _check(b, arr, axis, order, "constant record axis %d" % axis)
            got = got if axis == 1 else got.T
            assert got.dtype == np.float32 and np.all(got[1] == 0.0)
    # a nan and an infinity spoil their own records only, as rows and as columns
    y = D.rand((5, 64), "float32", seed=8)
    y[1, 17] = np.nan
    y[3, 40] = np.inf
    clean = np.ascontiguousarray(y[(0, 2, 4), :])
    for order in (1, 3):
        t, bound = D.truth_and_bound(clean, 1, order)
        for arr, axis in ((y, 1), (np.ascontiguousarray(y.T), 0)):
            got = bolt.array(arr, bctx).detrend(axis=axis, order=order).toarray()
            rows = got if axis == 1 else got.T
            assert np.isnan(rows[1]).all() and np.isnan(rows[3]).all(), (order, axis)
            assert np.all(np.abs(rows[(0, 2, 4), :].astype(np.longdouble) - t) <= bound), (order, axis)
    # a reduced axis of one element: the mean is all there is to remove
    one = bolt.array(D.rand((3, 1), "float32", seed=7), bctx)
    r = one.detrend(axis=1, order=0)
    assert r.shape == (3, 1) and np.all(r.toarray() == 0.0)
    with pytest.raises(ValueError):
        one.detrend(axis=1, order=1)


def test_empty_arrays(bctx):
    for shape, axis in (((0, 5), 1), ((4, 0), 1), ((4, 0), 0)):
        for dtype in ("float32", "uint8"):
            b = bolt.array(np.zeros(shape, dtype=dtype), bctx)
            for order in (0, 1, 8):
                r = b.detrend(axis=axis, order=order)
                assert type(r) is type(b) and r.shape == shape and r.dtype == D.out_dtype(dtype)
                got = r.toarray()
                assert got.shape == shape and got.dtype == D.out_dtype(dtype)


# ----------------------------------------------------------------- 7. arguments
def test_bad_arguments(bctx, monkeypatch):
    b = bolt.array(D.rand((4, 6), "float32"), bctx)
    be = _backend(b)

    def boom(*a, **k):
        raise AssertionError("a backend call before the arguments were checked")
    for name in _public(be):
        monkeypatch.setattr(be, name, boom, raising=False)
    for bad in (True, False, np.True_, 1.0, 1.5, "1", None, [1], (1,), 1j, float("nan")):
        with pytest.raises(ValueError):
            b.detrend(axis=1, order=bad)
    for bad in (-1, 9, 100):
        with pytest.raises(ValueError):
            b.detrend(axis=1, order=bad)
    # order >= n: 6 values over axis 1, 4 over axis 0, 24 over both
    for axis, bad in ((1, 6), (1, 8), (0, 4), (0, 5)):
        with pytest.raises(ValueError):
            b.detrend(axis=axis, order=bad)
    for bad in (2, (0, 5), -3):
        with pytest.raises(Exception) as want:
            b.mean(axis=bad)
        with pytest.raises(type(want.value)):
            b.detrend(axis=bad)
    with pytest.raises(TypeError):
        b.detrend(axis=0, keepdims=True)  # the result has the array's shape
    monkeypatch.undo()
    D.check_array(b.detrend(axis=1, order=np.int64(5)), b, b.toarray(), 1, 5, "numpy integer order")
    D.check_array(b.detrend(order=8), b, b.toarray(), None, 8, "every axis, order 8 of 24 values")
    c = bolt.array(np.ones((3, 4), dtype=np.complex64), bctx)
    with pytest.raises(NotImplementedError):
        c.detrend(axis=0)


# --------------------------------------------------------------- 8. determinism
def test_deterministic(bctx):
    for shape, axis in (((5, 300), 1), ((256, 2052), 1), ((300, 7, 5), 0), ((6, 5, 7), (0, 2))):
        x = D.rand(shape, "float32", seed=9)
        b = bolt.array(x, bctx)
        for order in (1, 5):
            assert b.detrend(axis=axis, order=order).toarray().tobytes() == \
                b.detrend(axis=axis, order=order).toarray().tobytes()
