"""stats(): mean, var and std over an axis from one read of the array.

Runs on the CPU test executor (host logic; tests/cpu_backend.py has no fused
entry points, so it takes stats()' one-state fallback) and, marked gpu, on
the HIP kernels (bm_reduce_moments / bm_reduce_combine_moments).  The rules:
var and std carry the bits of b.var / b.std; the mean is the Welford mean of
the variance's state and meets golden_cases.stat_close against b.mean and the
float128 truth; count is the number of records per output; one reduction
launch sequence reads the array, after at most one _align permute.
"""
import ctypes
import math

import numpy as np
import pytest

import bolt_amd as bolt
import golden_cases as G

FIELDS = ("mean", "var", "std")
_OTHER = {"mean": "std", "var": "mean", "std": "var"}
_MOMENT_CASES = [c for c in G.cases("stat") if c["name"] in FIELDS]


@pytest.fixture(scope="module", params=["cpu", pytest.param("gpu", marks=pytest.mark.gpu)])
def bctx(request):
    """conftest's bctx (the CPU test executor, or the HIP kernels marked gpu) at
    module scope: these tests run together, in this file's place in the suite,
    not regrouped with every other module's by the session-wide parameter."""
    from bolt_amd import MI355XContext
    if request.param == "gpu":
        import torch
        if not torch.cuda.is_available():
            pytest.skip("no GPU")
        return MI355XContext(device="cuda:0")
    import cpu_backend
    cpu_backend.install()
    return MI355XContext(device="cpu")


def _bits(a):
    a = np.asarray(a)
    return (type(a), a.dtype, a.shape, a.tobytes())


def _same(got, want):
    """Same result type, dtype, shape and bytes."""
    return type(got) is type(want) and _bits(got)[1:] == _bits(want)[1:]


# ------------------------------------------------------------ 1. golden parity
@pytest.mark.parametrize("name", FIELDS)
def test_golden_parity(name, bctx):
    """test_golden_api.test_stat's assertions on the field of a two-name stats()
    call, for every golden "stat" case of the statistic (the case id is in the
    assertion message of a failure)."""
    cases = [c for c in _MOMENT_CASES if c["name"] == name]
    assert len(cases) > 100
    for case in cases:
        try:
            _golden_case(case, bctx)
        except BaseException as e:
            raise AssertionError("golden case %s: %r" % (G.case_id(case), e)) from e


def _golden_case(case, bctx):
    x = G.make_input(case["input"])
    b = bolt.array(x, bctx, axis=G.tup(case["axis"]), npartitions=case["npartitions"])
    ax = G.tup(case["reduce_axis"])
    name = case["name"]
    names = (name, _OTHER[name])
    if "raises" in case:
        with pytest.raises(Exception) as e:
            b.stats(axis=ax, keepdims=case["keepdims"], names=names)
        assert type(e.value).__name__ == case["raises"]
        return
    st = b.stats(axis=ax, keepdims=case["keepdims"], names=names)
    got = getattr(st, name)
    want = G.arr(case, "out")
    assert type(got).__name__ == case["result_type"]
    assert str(np.asarray(got).dtype) == case["result_dtype"]
    assert np.asarray(got).shape == want.shape
    truth = G.truth_stat(x, name, ax)
    assert G.stat_close(got, want, truth, want.dtype, x, name)
    assert getattr(st, _OTHER[name]) is not None
    assert all(getattr(st, f) is None for f in FIELDS if f not in names)


# ------------------------------------------- 2. consistency with the methods
def _rand(shape, dtype, seed=0):
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype)
    if dt == np.bool_:
        return rng.integers(0, 2, size=shape).astype(bool)
    if dt.kind in "iu":
        info = np.iinfo(dt)
        lo, hi = max(info.min, -(1 << 40)), min(info.max, 1 << 40)
        return rng.integers(lo, hi, size=shape, dtype=np.int64).astype(dt)
    return (10 + 3 * rng.standard_normal(shape)).astype(dt)


# (dtype, shape, axis), in named groups (one test each): the smallest shapes that reach each branch of
# plan_reduce / comb_blk (bolt_amd/csrc/bm_reduce.hip); the plan of each was
# worked out from that code and is named here
SHAPES = [
    # rows kernel (I == 1), one chunk per row
    "rows",
    ("float32", (5, 300), 1),        # vec 4 (300 % 4 == 0), R < 1024: one chunk
    ("float32", (5, 301), 1),        # vec 1 (odd R): scalar loads and the scalar tail
    ("float64", (4, 130), 1),        # vec 2
    ("float16", (3, 64), 1),         # vec 8, chunk shorter than one wave-wide step
    # rows kernel, R split into chunks -> workspace partials + combine
    ("float32", (6, 5000), 1),       # 4 chunks of 1252, 6 outputs: k_red_combine with pivots
    ("float32", (200000,), None),    # 195 chunks, 1 output: k_red_combine_blk with pivots
    # column kernel (I > 1)
    "columns",
    ("float32", (300, 7, 5), 0),     # I = 35: vec 1, one 64-lane tile, 4 row phases; 9 chunks -> combine_blk
    ("float32", (64, 8, 16), 0),     # I = 128: vec 4, 32-lane tile, 8 row phases merged in LDS, one chunk
    ("float32", (6, 50, 10), 1),     # O = 6 > 1, vec 2, 32 row phases, one chunk
    ("float64", (20000, 8), 0),      # R in 39 chunks, 8 outputs: combine_blk
    ("float32", (4000, 2048), 0),    # 125 chunks of 32 rows, 2048 outputs > 1024: k_red_combine
    "layouts",
    # planes of 5.6 MB: together past the 8 MiB zero-copy limit, each alone within it (a host buffer per plane)
    ("float64", (3, 700000), 0),
    # reduced axes not one block: permuted to the front once
    ("float32", (6, 5, 7), (0, 2)),
    # exact integer sums (1- and 2-byte integers, bool): k_red_cols_int / k_red_rows_int
    "integers",
    ("uint8", (300, 7, 5), 0),       # column sums, 9 chunks: integer partials, combine_blk int_sums
    ("uint8", (300, 7, 5), (0, 2)),  # permuted, then rows of 1500
    ("int16", (6, 5000), 1),         # rows, 2 chunks (vec 8): integer partials, k_red_combine int_sums
    ("bool", (40, 9), 0),            # bool through the uint8 kernels
    ("bool", (40, 9), None),
    # 4- and 8-byte integers take the float64 Welford path
    ("int32", (50, 12), 0),
    ("int32", (50, 12), 1),
    ("int64", (50, 12), 0),
    ("int64", (50, 12), 1),
]


def _check_fields(b, x, axis, keepdims=False, names=FIELDS):
    st = b.stats(axis=axis, keepdims=keepdims, names=names)
    want = set(names)
    ax = tuple(range(x.ndim)) if axis is None else (tuple(axis) if isinstance(axis, (list, tuple)) else (axis,))
    assert isinstance(st.count, int) and st.count == int(np.prod([x.shape[a] for a in ax]))
    for f in FIELDS:
        if f not in want:
            assert getattr(st, f) is None
    if "var" in want:
        assert _same(st.var, b.var(axis=axis, keepdims=keepdims))
    if "std" in want:
        assert _same(st.std, b.std(axis=axis, keepdims=keepdims))
    if "mean" in want:
        ref = b.mean(axis=axis, keepdims=keepdims)
        assert type(st.mean) is type(ref)
        assert np.asarray(st.mean).dtype == np.asarray(ref).dtype
        assert np.asarray(st.mean).shape == np.asarray(ref).shape
        truth = G.truth_stat(x, "mean", list(ax))
        assert G.stat_close(st.mean, ref, truth, np.asarray(ref).dtype, x, "mean")
    return st


def _group(name):
    """The SHAPES entries that follow the group's name, up to the next name."""
    at = SHAPES.index(name) + 1
    out = []
    while at < len(SHAPES) and not isinstance(SHAPES[at], str):
        out.append(SHAPES[at])
        at += 1
    return out


@pytest.mark.parametrize("group", [g for g in SHAPES if isinstance(g, str)])
def test_matches_methods(bctx, group):
    shapes = _group(group)
    assert shapes
    for dtype, shape, axis in shapes:
        x = _rand(shape, dtype, seed=len(shape) + shape[0])
        b = bolt.array(x, bctx)
        try:
            _check_fields(b, x, axis)
            _check_fields(b, x, axis, names=("mean", "std"))
        except AssertionError as e:
            raise AssertionError("%s %s axis %s: %s" % (dtype, shape, axis, e)) from e


def test_single_name_delegates(bctx):
    x = _rand((6, 50, 10), "float32")
    b = bolt.array(x, bctx)
    for f, alias in (("std", "stdev"), ("var", "variance"), ("mean", "mean")):
        for names in (f, (f,), [alias], (f, alias)):
            st = b.stats(axis=1, names=names)
            assert _same(getattr(st, f), getattr(b, f)(axis=1))
            assert st.count == 50
            assert all(getattr(st, g) is None for g in FIELDS if g != f)


def test_axis_and_keepdims_forms(bctx):
    x = _rand((6, 5, 7), "float64")
    b = bolt.array(x, bctx, axis=(0, 1))
    for axis in (0, (0,), [0], (0, 1), [1, 2], (0, 2), (0, 1, 2), None, 2):
        for keepdims in (False, True):
            _check_fields(b, x, axis, keepdims=keepdims)
    st = b.stats(names=("variance", "stdev", "mean"))
    assert st.count == 210 and isinstance(st.var, np.float64)
    # a unit axis that the reference's _align squeezes (plan.swap_shape)
    x1 = _rand((4, 1, 5), "float32")
    _check_fields(bolt.array(x1, bctx), x1, 2)
    _check_fields(bolt.array(x1, bctx), x1, 0)


def test_bad_arguments(bctx):
    x = _rand((4, 6), "float32")
    b = bolt.array(x, bctx)
    for names in ((), [], "median", ("mean", "max"), ("mean", None), (["mean"],), "sum"):
        with pytest.raises(ValueError):
            b.stats(axis=0, names=names)
    for bad in (2, (0, 5), -3):
        with pytest.raises(Exception) as want:
            b.mean(axis=bad)
        with pytest.raises(type(want.value)):
            b.stats(axis=bad, names=("mean", "var"))
    c = bolt.array(np.ones((3, 4), dtype=np.complex64), bctx)
    with pytest.raises(Exception) as want:
        c.mean(axis=0)
    with pytest.raises(type(want.value)):
        c.stats(axis=0)


def test_zero_records(bctx):
    b = bolt.array(np.zeros((0, 3), dtype=np.float32), bctx)
    st = b.stats(axis=0)
    assert st.count == 0
    assert _same(st.mean, b.mean(axis=0)) and st.mean == 0.0
    assert _same(st.var, b.var(axis=0)) and math.isnan(st.var) and math.isnan(st.std)
    st = b.stats(axis=0, keepdims=True, names=("mean", "var"))
    assert _same(st.mean, b.mean(axis=0, keepdims=True)) and st.std is None


# row-padded swap results: rows of >= 1536 B that are no multiple of 128 B
PADDED = [((500, 3, 4), 512),     # rows of 500 float32 at a pitch of 512: one chunk per row
          ((5000, 2, 3), 5056)]   # rows of 5000 at 5056: 6 rows, each in 4 chunks


@pytest.mark.parametrize("shape,pitch", PADDED, ids=["r500", "r5000"])
def test_row_padded_read_in_place(bctx, shape, pitch):
    x = _rand(shape, "float32", seed=3)
    s = bolt.array(x, bctx).swap((0,), (0, 1))
    xs = np.ascontiguousarray(x.transpose(1, 2, 0))
    assert "_pbuf" in s.__dict__ and s.__dict__["_pitch"] == pitch
    for axis in (2, 0, (0, 1), (0, 2), None):
        for names in (FIELDS, ("mean", "std")):
            s.stats(axis=axis, names=names)
            # read in place: still padded, no dense copy was materialised
            assert "_pbuf" in s.__dict__ and "_data" not in s.__dict__, axis
    for axis in (2, 0, (0, 1), (0, 2), None):
        _check_fields(s, xs, axis)
        _check_fields(s, xs, axis, keepdims=True, names=("var", "mean"))


@pytest.mark.parametrize("kind", ["offset", "outlier"])
def test_ill_conditioned_float64(bctx, kind):
    """test_gpu_numerics' rows: a +1e6 offset, or an outlier leading every row;
    every field against the float128 truth at rtol 1e-12 (var / std pure
    relative, the mean with stat_close's floor of rtol * max|x|)."""
    rng = np.random.default_rng(7)
    x = rng.standard_normal((64, 10000))
    if kind == "outlier":
        x[:, 0] = 100.0
    else:
        x += 1e6
    b = bolt.array(x, bctx)
    st = b.stats(axis=1)
    v = x.astype(np.longdouble)
    tvar = v.var(axis=1)
    for got, truth in ((st.var, tvar), (st.std, np.sqrt(tvar))):
        err = np.abs(np.asarray(got, dtype=np.longdouble) - truth) / np.abs(truth)
        print(kind, "max relative error", float(err.max()))
        assert float(err.max()) <= 1e-12
    tmean = v.mean(axis=1)
    merr = np.abs(np.asarray(st.mean, dtype=np.longdouble) - tmean)
    print(kind, "mean max abs error", float(merr.max()))
    assert np.all(merr <= 1e-12 * np.abs(tmean) + 1e-12 * float(np.abs(x).max()))
    assert _same(st.var, b.var(axis=1)) and _same(st.std, b.std(axis=1))


# ----------------------------------------------------------------- 3. one read
_COUNTED = ("reduce", "reduce_rows", "reduce_moments", "reduce_state", "reduce_combine",
            "reduce_combine_moments", "permute", "copy_strided")


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


def test_one_read(bctx, monkeypatch):
    for layout in ("dense", "permuted", "padded_rows", "padded_cols", "padded_perm", "padded_all"):
        with monkeypatch.context() as mp:
            _one_read(bctx, mp, layout)


def _one_read(bctx, monkeypatch, layout):
    from bolt_amd.mi355x._ops import backend_for
    x = _rand((500, 3, 4), "float32", seed=5)
    b = bolt.array(x, bctx)
    if layout == "dense":
        arr, axis = b, 0
    elif layout == "permuted":
        arr, axis = b, (0, 2)
    else:
        arr = b.swap((0,), (0, 1))
        assert "_pbuf" in arr.__dict__
        axis = {"padded_rows": 2, "padded_cols": 0, "padded_perm": (0, 2), "padded_all": None}[layout]
    be = backend_for(arr._device)
    calls = _counting(monkeypatch, be)
    st = arr.stats(axis=axis, names=("mean", "std"))
    assert st.mean is not None and st.std is not None and st.var is None
    assert calls["reduce"] == 0 and calls["reduce_rows"] == 0
    assert calls["reduce_moments"] + calls["reduce_state"] == 1
    assert calls["permute"] + calls["copy_strided"] <= 1
    if layout in ("permuted", "padded_perm"):
        assert calls["permute"] + calls["copy_strided"] == 1
    # for contrast: the two methods read the array twice
    for name in calls:
        calls[name] = 0
    arr.mean(axis=axis)
    arr.std(axis=axis)
    assert calls["reduce"] + calls["reduce_rows"] + calls["reduce_state"] == 2
    assert calls["reduce_moments"] == 0


# ------------------------------------------------------------------ 4. C ABI
def test_abi_argument_errors():
    """The new entry points refuse bad arguments before touching a device (no GPU needed)."""
    from bolt_amd.mi355x import _lib
    lib = _lib.load()
    F32, F64, I32 = _lib.BM_F32, _lib.BM_F64, _lib.BM_I32
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)  # never dereferenced: every call below fails its checks
    f = lib.bm_reduce_moments
    assert f(p, F32, 2, 8, 1, 8, None, None, None, F32, None, 0, None) == -1
    assert b"no output" in lib.bm_last_error()
    assert f(None, F32, 2, 8, 1, 8, p, p, p, F32, None, 0, None) == -1
    assert b"null pointer" in lib.bm_last_error()
    assert f(p, F32, 2, 8, 1, 8, p, None, p, I32, None, 0, None) == -1
    assert b"not a float dtype" in lib.bm_last_error()
    assert f(p, F32, 2, 8, 1, 7, p, None, None, F32, None, 0, None) == -1
    assert b"row_pitch" in lib.bm_last_error()
    assert f(p, F32, 2, 8, 4, 16, p, None, None, F32, None, 0, None) == -1  # a pitch with I > 1
    assert b"row_pitch" in lib.bm_last_error()
    for O, R, I in ((0, 8, 1), (2, 0, 1), (2, 8, 0)):
        assert f(p, F32, O, R, I, R, p, p, p, F32, None, 0, None) == -1
        assert b"empty reduction" in lib.bm_last_error()
    assert f(p, 99, 2, 8, 1, 8, p, p, p, F32, None, 0, None) == -1
    # a chunked plan without its workspace: BM_E_WS, still before any launch
    assert f(p, F32, 1, 200000, 1, 200000, p, p, p, F32, None, 0, None) == _lib.BM_E_WS
    assert b"workspace too small" in lib.bm_last_error()
    g = lib.bm_reduce_combine_moments
    counts = _lib.i64_array([4, 4])
    assert g(F32, p, counts, 2, 8, None, None, None, F64, None) == -1
    assert b"bad arguments" in lib.bm_last_error()
    assert g(F32, None, counts, 2, 8, p, p, p, F64, None) == -1
    assert g(F32, p, None, 2, 8, p, p, p, F64, None) == -1
    assert g(F32, p, counts, 2, 8, p, p, p, I32, None) == -1
    assert b"not a float dtype" in lib.bm_last_error()
    assert g(F32, p, counts, 2, 0, p, p, p, F64, None) == -1
    for nparts in (0, -1, _lib.MAX_COMBINE_PARTS + 1):
        assert g(F32, p, counts, nparts, 8, p, p, p, F64, None) == -1
        assert b"bad arguments" in lib.bm_last_error()
    assert g(99, p, counts, 2, 8, p, p, p, F64, None) == -1
