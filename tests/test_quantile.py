"""quantile() / percentile() / median(): exact order statistics of every record
along an axis.

Runs on the CPU test executor as it is (tests/cpu_backend.py has neither entry
point: the methods' torch.sort fallback), on a subclass of it with
bm_quantile_rows / bm_quantile_select in numpy (the orchestration the HIP
backend takes) and, marked gpu, on the HIP kernels.  'lower' / 'higher' are
compared with numpy.quantile itself, 'linear' with the restated formula
(quantile_cases.truth), all bit for bit (zeros by ==); float64 results also
with numpy's own 'linear' inside 4 spacings.
"""
import ctypes

import numpy as np
import pytest

import bolt_amd as bolt
import quantile_cases as S
from quantile_cases import METHODS, QG


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
# branch of bm_quantile.hip.  rows: vec = min(16 B / item, 8) halved until it
# divides R and the pitch; a thread holds min(8 vec, 32) elements; one wave per
# row up to 64 times that (2048 elements of 4 bytes or narrower at their widest
# vector, 1024 of 8 bytes), one block per row up to 256 times that and only
# with 256 rows or more; everything else streams: rows in slices of at least
# 4096 elements over as many blocks as give the batch 2048.
SHAPES = [
    "wave",
    ("float32", (5, 300), 1),        # vec 4: 16-B loads, 75 of 64 x 8 slots
    ("float32", (5, 301), 1),        # vec 1 (odd R): scalar loads, 8 elements a lane
    ("float32", (1, 7), 1),          # one row, 7 of 64 lanes
    ("float32", (4, 1), 1),          # one value: every rank is 0
    ("float32", (4, 2), 1),          # the pair
    "wave_limit",
    ("float32", (3, 2048), 1),       # every slot of the wave full
    ("float64", (4, 130), 1),        # vec 2, 64-bit keys
    ("float64", (3, 1024), 1),       # the 8-byte wave limit
    "block",
    ("float32", (256, 2052), 1),     # the first size past the wave, just enough rows
    ("float32", (256, 8192), 1),     # every slot of the block full
    ("float64", (256, 1028), 1),
    "streaming",
    ("float32", (3, 2052), 1),       # too few rows for a block each: one slice a row
    ("float32", (256, 8196), 1),     # past the block's registers: 2 slices a row
    ("float32", (2, 50000), 1),      # 12 slices a row
    ("float32", (200000,), None),    # one row over 48 blocks
    "grid_tail",
    ("float32", (16403, 12), 1),     # the last block's waves leave early
    "dtypes_wave",
    ("float16", (7, 264), 1),        # vec 8, 16-bit keys
    ("uint8", (7, 260), 1),          # vec 4 (260 % 8 != 0), 8-bit keys: 8 iterations
    ("uint16", (7, 264), 1),
    ("int32", (7, 260), 1),
    ("int64", (7, 260), 1),
    ("bool", (40, 9), 1),            # through the uint8 kernels, vec 1
    "dtypes_streaming",
    ("float16", (2, 9000), 1),       # two passes
    ("float64", (2, 9000), 1),       # eight passes
    ("uint8", (2, 9000), 1),         # one pass, 8-B loads
    ("uint16", (2, 9000), 1),
    ("int32", (2, 9000), 1),
    ("int64", (2, 9000), 1),
    ("bool", (2, 9000), 1),
    "permuted",
    ("float32", (300, 7, 5), 0),     # columns: permuted to (7, 5, 300)
    ("float32", (6, 50, 10), 1),     # a middle axis
    ("float32", (6, 5, 7), (0, 2)),  # reduced axes that are not one block
    ("float32", (6, 5, 7), None),    # every axis: one row in place
]


def _group(name):
    at = SHAPES.index(name) + 1
    out = []
    while at < len(SHAPES) and not isinstance(SHAPES[at], str):
        out.append(SHAPES[at])
        at += 1
    return out


# ------------------------------------------------------------------ 1. shapes
@pytest.mark.parametrize("group", [g for g in SHAPES if isinstance(g, str)])
def test_shapes(bctx, group):
    shapes = _group(group)
    assert shapes
    for dtype, shape, axis in shapes:
        x = S.rand(shape, dtype, seed=len(shape) + shape[0])
        S.check_all(bolt.array(x, bctx), x, axis, "%s %s axis %s" % (dtype, shape, axis))


def test_plan_reaches_both_paths():
    """The fused executor takes the kernels' plan: the shapes above reach the
    rows path and the streaming path where their comments say."""
    from bolt_amd import MI355XContext
    from bolt_amd.mi355x._ops import register_backend
    import cpu_backend
    be = S.fused_backend()
    register_backend("cpu", be)
    try:
        ctx = MI355XContext(device="cpu")
        for group, want in (("wave", "rows"), ("wave_limit", "rows"), ("block", "rows"), ("streaming", "select"),
                            ("dtypes_wave", "rows"), ("dtypes_streaming", "select"), ("permuted", "rows")):
            for dtype, shape, axis in _group(group):
                be.calls = {"rows": 0, "select": 0}
                bolt.array(np.zeros(shape, dtype=dtype), ctx).median(axis=axis)
                assert be.calls == {"rows": int(want == "rows"), "select": int(want == "select")}, (shape, be.calls)
    finally:
        cpu_backend.install()


# ------------------------------------------------------------------ 2. values
def _value_cases(dtype, shape):
    """(name, array) pairs of ``shape`` (rows along the last axis)."""
    rng = np.random.default_rng(shape[-1])
    dt = np.dtype(dtype)
    out = []
    if dt.kind == "f":
        base = rng.standard_normal(shape)
        out.append(("all equal", np.full(shape, 2.5)))
        out.append(("ties", np.round(2 * base) / 2))
        out.append(("negative", -1 - np.abs(base)))
        out.append(("mixed sign", base))
        inf = base.copy()
        inf[0, :3] = np.inf
        inf[1, :2] = -np.inf
        inf[2, 0], inf[2, 1] = np.inf, -np.inf
        out.append(("inf", inf))
        nan = base.copy()
        nan[1, shape[1] // 2] = np.nan
        nan[3, 0] = -np.nan
        nan[3, -1] = np.nan
        out.append(("nan", nan))
        out.append(("zeros", rng.choice(np.array([-0.0, 0.0, -1.0, 1.0]), size=shape)))
    else:
        info = np.iinfo(dt)
        v = rng.integers(info.min, info.max, size=shape, dtype=np.int64 if dt.kind == "i" else np.uint64,
                         endpoint=True)
        v[0, 1], v[0, -1] = info.min, info.max
        v[1, :] = info.max
        v[2, :] = info.min
        out.append(("extremes", v))
        out.append(("ties", rng.integers(0, 4, size=shape)))
    return [(name, np.ascontiguousarray(a.astype(dt))) for name, a in out]


@pytest.mark.parametrize("dtype", ["float32", "float64", "float16", "int32", "int64", "uint8", "uint16", "uint64"])
def test_values(bctx, dtype):
    for shape in ((6, 300), (4, 9000)):   # the wave path and the streaming path
        for name, x in _value_cases(dtype, shape):
            b = bolt.array(x, bctx)
            S.check_all(b, x, 1, "%s %s %s" % (name, dtype, shape), qs=(0.0, 1.0, 0.5, QG))
            if name == "nan":
                # the rows with a NaN are NaN for every q and method, the others untouched
                for method in METHODS:
                    got = np.asarray(b.quantile((0.0, 0.5, 1.0), axis=1, method=method))
                    assert np.isnan(got[:, [1, 3]]).all() and np.isfinite(got[:, [0, 2]]).all(), (shape, method)


# ----------------------------------------------------------------------- 3. q
@pytest.mark.parametrize("k", [3, 5])
def test_sequences(bctx, k):
    """A sequence of 3 (one batch) and of 5 ('linear': two batches): plane k
    has the bytes of the scalar call with q[k]."""
    qs = [QG, 0.5, 0.9, 0.0, 0.77][:k]
    for dtype, shape, axis, out in (("float32", (5, 300), 1, (5,)), ("float32", (300, 7, 5), 0, (7, 5)),
                                    ("uint16", (3, 9000), 1, (3,))):
        x = S.rand(shape, dtype, seed=3)
        b = bolt.array(x, bctx)
        for method in METHODS:
            got = np.asarray(b.quantile(qs, axis=axis, method=method))
            assert got.shape == (k,) + out
            for j in range(k):
                one = S.check(b, x, qs[j], axis, method, "K=%d plane %d %s" % (k, j, shape))
                assert got[j].tobytes() == one.tobytes() and got.dtype == one.dtype, (method, shape, j)
            kd = np.asarray(b.quantile(qs, axis=axis, method=method, keepdims=True))
            want = (k,) + tuple(1 if i == axis else n for i, n in enumerate(shape))
            assert kd.shape == want and kd.tobytes() == got.tobytes()
            # tuples and arrays are sequences too; one q given as a sequence keeps the leading axis
            assert np.asarray(b.quantile(np.array(qs), axis=axis, method=method)).tobytes() == got.tobytes()
            assert np.asarray(b.quantile(tuple(qs[:1]), axis=axis, method=method)).shape == (1,) + out


def test_percentile_median_and_result_type(bctx):
    from bolt_amd.local import BoltArrayLocal
    x = S.rand((6, 5, 7), "float32", seed=1)
    b = bolt.array(x, bctx)
    for axis in (2, 0, (0, 2), None):
        for method in METHODS:
            p = np.asarray(b.percentile(25, axis=axis, method=method))
            assert p.tobytes() == np.asarray(b.quantile(0.25, axis=axis, method=method)).tobytes()
            p = np.asarray(b.percentile((10, 50, 90), axis=axis, method=method))
            assert p.tobytes() == np.asarray(b.quantile((0.1, 0.5, 0.9), axis=axis, method=method)).tobytes()
        m = np.asarray(b.median(axis=axis))
        assert m.tobytes() == np.asarray(b.quantile(0.5, axis=axis)).tobytes()
        S.check(b, x, 0.5, axis, "linear", "median axis %s" % (axis,))
    r = b.median(axis=2)
    assert type(r) is BoltArrayLocal and r.shape == (6, 5) and r.dtype == np.float32
    assert b.median(axis=2, keepdims=True).shape == (6, 5, 1)
    assert b.quantile(0.3, axis=(0, 2), keepdims=True).shape == (1, 5, 1)
    assert b.quantile((0.3, 0.6), axis=(0, 2), keepdims=True).shape == (2, 1, 5, 1)
    s = b.median()
    assert isinstance(s, np.float32) and not isinstance(s, np.ndarray)
    assert b.median(keepdims=True).shape == (1, 1, 1)
    for kaxes in ((0,), (0, 1)):
        bs = bolt.array(x, bctx, axis=kaxes)
        for axis in (2, 0, (1, 2), None):
            S.check_all(bs, x, axis, "split %d axis %s" % (bs.split, axis), qs=(0.5, QG))
    # result dtypes: 'linear' the statistics dtype, 'lower' / 'higher' the array's own
    for dtype in ("float16", "int32", "bool", "uint8"):
        xd = S.rand((4, 9), dtype, seed=2)
        bd = bolt.array(xd, bctx)
        assert np.asarray(bd.median(axis=1)).dtype == S.out_dtype(dtype)
        assert np.asarray(bd.quantile(0.3, axis=1, method="lower")).dtype == np.dtype(dtype)
        assert np.asarray(bd.quantile(0.3, axis=1, method="higher")).dtype == np.dtype(dtype)


# ------------------------------------------------------------------ 4. errors
def test_bad_arguments_raise_before_any_launch(bctx, monkeypatch):
    x = S.rand((4, 6, 5), "float32")
    b = bolt.array(x, bctx)
    empty = bolt.array(np.zeros((4, 0), dtype=np.float32), bctx)
    be = _backend(b)

    def boom(*a, **k):
        raise AssertionError("a launch before the arguments were checked")
    for name in ("quantile_rows", "quantile_select", "reduce_state", "reduce", "reduce_rows", "permute",
                 "copy_strided"):
        if hasattr(be, name):
            monkeypatch.setattr(be, name, boom, raising=False)
    for q in (-0.1, 1.1, np.nan, np.inf, [0.5, 1.5], [[0.5, 0.6]], np.zeros((2, 2)), [], "0.5", 0.5j, None):
        for method in METHODS:
            with pytest.raises(ValueError):
                b.quantile(q, axis=1, method=method)
    for q in (-1, 100.5, np.nan, [50, 101]):
        with pytest.raises(ValueError):
            b.percentile(q, axis=1)
    for method in ("nearest", "midpoint", None, 3):
        with pytest.raises(ValueError):
            b.quantile(0.5, axis=1, method=method)
        with pytest.raises(ValueError):
            b.percentile(50, axis=1, method=method)
    for method in ("lower", "higher"):
        with pytest.raises(ValueError):
            empty.quantile(0.5, axis=1, method=method)
    # no records: 'linear' gives nan, and launches nothing
    r = np.asarray(empty.quantile(0.5, axis=1))
    assert r.shape == (4,) and r.dtype == np.float32 and np.isnan(r).all()
    r = np.asarray(empty.quantile((0.1, 0.5), axis=1))
    assert r.shape == (2, 4) and np.isnan(r).all()
    assert np.isnan(empty.median())
    for badaxis in (3, (0, 5), -4):
        with pytest.raises(Exception) as want:
            b.mean(axis=badaxis)
        with pytest.raises(type(want.value)):
            b.median(axis=badaxis)
    monkeypatch.undo()
    # no outputs: an empty result
    r = np.asarray(bolt.array(np.zeros((0, 5), dtype=np.float32), bctx).median(axis=1))
    assert r.shape == (0,) and r.dtype == np.float32
    r = np.asarray(empty.quantile(0.5, axis=0, method="lower"))
    assert r.shape == (0,) and r.dtype == np.float32
    # ints and bools are real
    S.check(b, x, 1, 1, "linear", "q = int 1")
    assert np.asarray(b.quantile(True, axis=1, method="lower")).tobytes() == \
        np.asarray(b.quantile(1.0, axis=1, method="lower")).tobytes()


# ----------------------------------------------------------- 5. row-padded input
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
    S.check_all(s, xs, 2, "padded axis 2")
    assert "_pbuf" in s.__dict__ and "_data" not in s.__dict__  # the rows were read in place
    # other axes are permuted out of the padded rows: the pad is not read, the array stays padded
    for axis in (0, (0, 1), (0, 2), None):
        S.check_all(s, xs, axis, "padded axis %s" % (axis,), qs=(0.5, QG))
    assert "_pbuf" in s.__dict__ and "_data" not in s.__dict__


def test_moment_states_untouched(bctx):
    x = S.rand((6, 5, 7), "float32", seed=2)
    b = bolt.array(x, bctx)
    b.mean(axis=2)
    kept = dict(b.__dict__.get("_kept", {}))
    before = set(b.__dict__)
    b.median(axis=2)
    b.quantile((0.1, 0.9), axis=0, method="lower")
    assert dict(b.__dict__.get("_kept", {})).keys() == kept.keys() and set(b.__dict__) == before
    assert b.toarray().tobytes() == x.tobytes()


# ------------------------------------------------------- 6. stores stay inside
@pytest.mark.gpu
def test_planes_and_workspace_guards():
    """bm_quantile_rows / bm_quantile_select write their planes and their
    workspace and nothing around them: guard regions before, between and after
    keep their bytes."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from bolt_amd.mi355x._ops import backend_for, dtype_code
    dev = torch.device("cuda:0")
    be = backend_for(dev)
    G = 4096
    rng = np.random.default_rng(0)
    # the last source starts 4 B past a 16-B boundary: scalar loads
    for (O, R), dt, ranks, frac, off in (((5, 300), np.float32, [0, 149, 299], [0.0, 0.5, 0.0], 0),
                                          ((300, 2052), np.float32, [7, 2050], [0.25, 0.75], 0),
                                          ((3, 9000), np.float32, [0, 4499, 8999, 17], [0.0, 0.5, 0.0, 0.125], 0),
                                          ((2100, 8196), np.uint8, [5, 8194], [0.5, 0.5], 0),
                                          ((2, 50000), np.float64, [49998] * 4, [0.5] * 4, 0),
                                          ((3, 4100), np.float32, [1, 4098], [0.0, 0.5], 4)):
        x = rng.integers(0, 256, size=(O, R)).astype(dt) if dt is np.uint8 else \
            (rng.standard_normal((O, R)) * 50).astype(dt)
        code, odt = dtype_code(dt), S.out_dtype(dt)
        nranks = len(ranks) + sum(1 for g in frac if g)
        n = ctypes.c_size_t(0)
        assert be.lib.bm_quantile_workspace_bytes(code, O, R, nranks, ctypes.byref(n)) == 0
        obytes, wbytes = len(ranks) * O * odt.itemsize, n.value
        opad, wpad = -(-obytes // 256) * 256, -(-wbytes // 256) * 256
        buf = torch.full((3 * G + opad + wpad,), 0xA5, dtype=torch.uint8, device=dev)
        out = buf[G:G + obytes]
        ws = buf[2 * G + opad:2 * G + opad + wbytes]
        src = torch.empty(off + x.nbytes, dtype=torch.uint8, device=dev)[off:]
        src.copy_(torch.from_numpy(x.reshape(-1).view(np.uint8)))
        assert src.data_ptr() % 16 == off
        if not be.quantile_rows(src, code, O, R, R, ranks, frac, out, dtype_code(odt)):
            be.quantile_select(src, code, O, R, R, ranks, frac, out, dtype_code(odt), workspace=ws)
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        assert (host[:G] == 0xA5).all() and (host[G + obytes:2 * G + opad] == 0xA5).all(), (O, R)
        assert (host[2 * G + opad + wbytes:] == 0xA5).all(), (O, R)
        got = host[G:G + obytes].view(odt).reshape(len(ranks), O)
        srt = np.sort(x, axis=1).astype(np.float64)
        for k, (r, g) in enumerate(zip(ranks, frac)):
            want = srt[:, r] + ((srt[:, r + 1] - srt[:, r]) * g if g else 0.0)
            assert np.array_equal(got[k], want.astype(odt)), (O, R, k)
