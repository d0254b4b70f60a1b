"""The swap's moments kernel after its instruction diet (bm_copy.hip k_transpose
with F: the unmasked path of whole tiles, the pivot chosen on the element
word, row pairs as plain values) and the finish queued ahead (array.FINISH_AHEAD:
the first mean() of a state the swap left also launches std's finish, and the
other way round).

Everything runs on the GPU, thresholds lowered as test_zz_swap_moments.py's
fuse_small does.  Shapes (N, p, q) are swapped to (p, q, N): La = p * q result
rows of R = N values.  The tile each picks (bm_copy.hip pick_tile, TA x TB with
TB along the result's rows) is checked through the workspace size, which is
24 * rows bytes per b-tile:

float32 (256, 2, 64)  64x256  R exactly one tile: unmasked path only
        (260, 2, 64)  64x64   R = 4 TB + 4: full tiles, one live vector in the last
        (40, 8, 16)   64x64   R < TB: the masked path only
        (442, 2, 64)  64x64   padded rows, R % 4 = 2: element-wise tail store
        (758, 2, 64)  64x256  padded rows, R % 4 = 2: two unmasked tiles and a
                              masked one with element masks
        (760, 2, 60)  64x256  120 rows: the second a-tile has rows past La, so
                              its full-width tiles take the masked path
        (760, 2, 36)  32x256  72 rows: rows past La in a kernel without the
                              unmasked path
float64 (256, 2, 16)  32x256  R exactly one tile
        (258, 2, 32)  64x32   R = 8 TB + 2: one live vector in the last tile
        (66, 2, 32)   64x32   R = 2 TB + 2
        (24, 8, 16)   64x32   R < TB
        (221, 2, 32)  64x32   padded rows, odd R
        (1001, 2, 16) 32x256  padded rows, odd R: unmasked tiles and element masks
        (1000, 2, 27) 32x256  54 rows: the second a-tile has rows past La
        (260, 5, 14)  16x128  70 rows: rows past La in the last a-tile
R = TB + 4 itself picks no moments tile (float32 rows of 68 go to 128x32 tiles),
so the single live vector rides behind more than one full tile.  No case makes
a block walk more than one tile: the grid cap is 2^22 tiles.
"""
import numpy as np
import pytest

import bolt_amd as bolt
import bolt_amd.mi355x.array as A
import golden_cases as G
from bolt_amd.mi355x import _lib

pytestmark = pytest.mark.gpu

NAMES = ("mean", "var", "std")


@pytest.fixture(scope="module")
def gctx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return bolt.MI355XContext(device="cuda:0")


@pytest.fixture
def fuse_small(monkeypatch):
    monkeypatch.setattr(A, "FUSE_SWAP_MOMENTS", True)
    monkeypatch.setattr(A, "_FUSE_SWAP_MIN_BYTES", 0)


def _count_combines(mp, be):
    calls = {"reduce": 0, "reduce_rows": 0, "reduce_combine": 0}

    def proxy(name, fn):
        def call(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return call
    for name in calls:
        mp.setattr(be, name, proxy(name, getattr(be, name)), raising=False)
    return calls


def _truth(rows, name):
    with np.errstate(all="ignore"):
        return getattr(np.asarray(rows, dtype=np.longdouble), name)(axis=-1)


def _fused_state(arr):
    e = (arr.__dict__.get("_kept") or {}).get((arr.ndim - 1,))
    return e if e is not None and e.serves_mean else None


def _swap(gctx, x):
    return bolt.array(x, gctx).swap((0,), (0, 1))


def _btiles(s):
    """b-tiles of the swap that made ``s``: its workspace holds 24 B per row and b-tile."""
    be = s._backend
    rows, R = int(np.prod(s.shape[:-1])), s.shape[-1]
    pitch = s.__dict__.get("_pitch", R)
    es = s.dtype.itemsize
    from bolt_amd.mi355x._ops import dtype_code
    nws = be.copy_moments_plan([rows, R], [1, rows], [pitch, 1], es, dtype_code(s.dtype), R, pitch, rows)[3]
    assert nws % (24 * rows) == 0
    return nws // (24 * rows)


# (dtype, shape, state-size divisor, padded rows, b-tiles = ceil(R / TB))
SHAPES = [
    ("float32", (256, 2, 64), 64, False, 1),
    ("float32", (260, 2, 64), 64, False, 5),
    ("float32", (40, 8, 16), 1, False, 1),
    ("float32", (442, 2, 64), 64, True, 7),
    ("float32", (758, 2, 64), 64, True, 3),
    ("float32", (760, 2, 60), 64, True, 3),
    ("float32", (760, 2, 36), 64, True, 3),
    ("float64", (256, 2, 16), 64, False, 1),
    ("float64", (258, 2, 32), 64, False, 9),
    ("float64", (66, 2, 32), 1, False, 3),
    ("float64", (24, 8, 16), 1, False, 1),
    ("float64", (221, 2, 32), 64, True, 7),
    ("float64", (1001, 2, 16), 64, True, 4),
    ("float64", (1000, 2, 27), 64, True, 4),
    ("float64", (260, 5, 14), 64, False, 3),
]


@pytest.mark.parametrize("dtype,shape,div,padded,ntb", SHAPES,
                         ids=["%s-%s" % (d, "x".join(map(str, s))) for d, s, _, _, _ in SHAPES])
def test_shapes(gctx, fuse_small, monkeypatch, dtype, shape, div, padded, ntb):
    monkeypatch.setattr(A, "_FUSE_SWAP_STATE_DIV", div)
    rng = np.random.default_rng(shape[0] + shape[2])
    x = (10 + 3 * rng.standard_normal(shape)).astype(dtype)
    want = np.ascontiguousarray(x.transpose(1, 2, 0))
    s = _swap(gctx, x)
    assert _fused_state(s) is not None, "the swap did not fuse"
    assert ("_pbuf" in s.__dict__) == padded
    assert _btiles(s) == ntb
    got = {n: getattr(s, n)(axis=2) for n in NAMES}
    for n in NAMES:
        t = _truth(want, n)
        assert got[n].shape == want.shape[:2]
        assert G.stat_close(got[n], t.astype(got[n].dtype), t, got[n].dtype, x, n), (n, dtype, shape)
    assert s.toarray().tobytes() == want.tobytes()


def _data_rows(kind, dtype, nrows, R, TB):
    rng = np.random.default_rng(7)
    if kind == "normal":
        return (10 + 3 * rng.standard_normal((nrows, R))).astype(dtype)
    if kind == "offset":
        return (1e6 + rng.standard_normal((nrows, R))).astype(dtype)
    if kind == "constant":
        return np.repeat((1234.5 + np.arange(nrows))[:, None], R, axis=1).astype(dtype)
    rows = (10 + 3 * rng.standard_normal((nrows, R))).astype(dtype)
    rows[3, 0] = np.nan
    rows[5, 0] = np.inf
    rows[5, TB] = np.inf
    return rows


# full tiles and one live vector: float32 260 in 64-wide tiles, float64 258 in 32-wide ones
@pytest.mark.parametrize("kind", ["normal", "offset", "constant", "nonfinite"])
@pytest.mark.parametrize("dtype,R,q,TB,ntb", [("float32", 260, 64, 64, 5), ("float64", 258, 32, 32, 9)])
def test_data(gctx, fuse_small, dtype, R, q, TB, ntb, kind):
    rows = _data_rows(kind, dtype, 2 * q, R, TB)
    x = np.ascontiguousarray(rows.T).reshape(R, 2, q)
    s = _swap(gctx, x)
    assert _fused_state(s) is not None and _btiles(s) == ntb
    got = {n: getattr(s, n)(axis=2).reshape(2 * q) for n in NAMES}
    assert s.toarray().tobytes() == rows.tobytes()
    with np.errstate(all="ignore"):
        if kind == "constant":
            assert np.all(got["var"] == 0.0) and np.all(got["std"] == 0.0)
            assert np.array_equal(got["mean"], rows[:, 0])
            return
        fin = np.ones(2 * q, dtype=bool)
        if kind == "nonfinite":
            fin[[3, 5]] = False
            # numpy's own mean of the rows with a NaN / two infinities: NaN, inf
            ref = rows[~fin].astype(np.float64).mean(axis=-1)
            assert np.array_equal(got["mean"][~fin], ref.astype(got["mean"].dtype), equal_nan=True), got["mean"][~fin]
        for n in NAMES:
            t = _truth(rows[fin], n)
            assert G.stat_close(got[n][fin], t.astype(got[n].dtype), t, got[n].dtype, rows[fin], n), (n, dtype, kind)


@pytest.mark.parametrize("dtype,R,q,TB,ntb", [("float32", 260, 64, 64, 5), ("float64", 258, 32, 32, 9)])
def test_nonfinite_rows_var_std(gctx, fuse_small, dtype, R, q, TB, ntb):
    """numpy's var / std of a row with a NaN at column 0, and of a row with +inf
    at columns 0 and TB: NaN.  The tile states keep the M2 they always had (0
    where the tile's sums give NaN); the merged state's M2 is NaN where the
    row's mean is not finite (bm_reduce.hip m2_out), as the rows kernels' is, so
    every path of the library agrees with numpy on such rows."""
    rows = _data_rows("nonfinite", dtype, 2 * q, R, TB)
    x = np.ascontiguousarray(rows.T).reshape(R, 2, q)
    s = _swap(gctx, x)
    assert _fused_state(s) is not None and _btiles(s) == ntb
    with np.errstate(all="ignore"):
        for n in ("var", "std"):
            got = getattr(s, n)(axis=2).reshape(2 * q)[[3, 5]]
            ref = getattr(rows[[3, 5]].astype(np.float64), n)(axis=-1)
            print(n, dtype, "got", got, "numpy", ref)
            assert np.array_equal(got, ref.astype(got.dtype), equal_nan=True), (n, got, ref)


# ------------------------------------------------------- the finish queued ahead
def _x760(seed):
    rng = np.random.default_rng(seed)
    return (10 + 3 * rng.standard_normal((760, 2, 64))).astype("float32")


def _calls_of(calls, fn):
    before = calls["reduce_combine"]
    out = fn()
    return out, calls["reduce_combine"] - before


@pytest.mark.parametrize("first,second", [("mean", "std"), ("std", "mean")])
def test_pair_is_finished_by_the_first_call(gctx, fuse_small, monkeypatch, first, second):
    monkeypatch.setattr(A, "FINISH_AHEAD", True)
    x = _x760(21)
    s = _swap(gctx, x)
    assert _fused_state(s) is not None
    calls = _count_combines(monkeypatch, s._backend)
    a, na = _calls_of(calls, lambda: getattr(s, first)(axis=2))
    b, nb = _calls_of(calls, lambda: getattr(s, second)(axis=2))
    assert (na, nb) == (2, 0)
    # the plane is handed out once: a further call launches its own finish
    b2, nb2 = _calls_of(calls, lambda: getattr(s, second)(axis=2))
    a2, na2 = _calls_of(calls, lambda: getattr(s, first)(axis=2))
    assert (nb2, na2) == (1, 1)
    assert b2.tobytes() == b.tobytes() and a2.tobytes() == a.tobytes()
    assert calls["reduce"] == 0 and calls["reduce_rows"] == 0
    want = np.ascontiguousarray(x.transpose(1, 2, 0))
    for n, v in ((first, a), (second, b)):
        t = _truth(want, n)
        assert G.stat_close(v, t.astype(v.dtype), t, v.dtype, x, n)
    # the same bytes with the switch off
    monkeypatch.setattr(A, "FINISH_AHEAD", False)
    p = _swap(gctx, x)
    assert getattr(p, first)(axis=2).tobytes() == a.tobytes()
    assert getattr(p, second)(axis=2).tobytes() == b.tobytes()


def test_var_queues_nothing(gctx, fuse_small, monkeypatch):
    monkeypatch.setattr(A, "FINISH_AHEAD", True)
    s = _swap(gctx, _x760(22))
    calls = _count_combines(monkeypatch, s._backend)
    assert _calls_of(calls, lambda: s.var(axis=2))[1] == 1
    assert not _fused_state(s).ahead
    assert _calls_of(calls, lambda: s.std(axis=2))[1] == 2    # std first: mean's finish rides along
    assert _calls_of(calls, lambda: s.var(axis=2))[1] == 1
    assert _calls_of(calls, lambda: s.mean(axis=2))[1] == 0


def test_unpersist_drops_the_queued_plane(gctx, fuse_small, monkeypatch):
    monkeypatch.setattr(A, "FINISH_AHEAD", True)
    x = _x760(23)
    s = _swap(gctx, x)
    calls = _count_combines(monkeypatch, s._backend)
    m = s.mean(axis=2)
    assert calls["reduce_combine"] == 2 and _lib.STAT_STD in _fused_state(s).ahead
    s.unpersist()
    assert "_kept" not in s.__dict__
    sd = s.std(axis=2)                      # reads the rows: nothing is left to serve it
    assert calls["reduce_combine"] == 2 and calls["reduce_rows"] + calls["reduce"] == 1
    want = np.ascontiguousarray(x.transpose(1, 2, 0))
    for n, v in (("mean", m), ("std", sd)):
        t = _truth(want, n)
        assert G.stat_close(v, t.astype(v.dtype), t, v.dtype, x, n)


def test_switch_off_counts_as_before(gctx, fuse_small, monkeypatch):
    monkeypatch.setattr(A, "FINISH_AHEAD", False)
    s = _swap(gctx, _x760(24))
    calls = _count_combines(monkeypatch, s._backend)
    for n in ("mean", "std", "std", "var", "mean"):
        assert _calls_of(calls, lambda: getattr(s, n)(axis=2))[1] == 1, n
    assert not _fused_state(s).ahead
