"""The swap's moments kernel with its store phase as one block (bm_copy.hip
k_transpose with F, the two kernels whose LDS tile holds a CU to two blocks:
float32 64x256 and float64 32x256).  There a row pair's (s1, s2, pivot) wait in
registers and reach the LDS staging once, after the tile's last pair, in the
whole-tile path and in the masked one.  A result staged under the wrong pair,
row or segment is what these tests look for, so every row has a mean and a std
of its own: row r holds 10 r + (1 + r % 7) N(0, 1).

Everything runs on the GPU, thresholds lowered as test_zz_swap_moments_diet.py's
fuse_small does.  Shapes (N, p, q) are swapped to (p, q, N): La = p * q result
rows of R = N values.  The b-tile count, read from the workspace size (24 B per
row and b-tile), tells which kernel ran:

float32 (512, 2, 64)   2  128 rows = two a-tiles of two whole 64x256 tiles:
                          the unmasked path only, all 8 pairs of every lane live
        (720, 2, 64)   3  two whole tiles, then 208 = 52 whole vectors (the
                          last tile of rows of 2000): masked path, lane-uniform
        (726, 2, 60)   3  120 rows: rows past La in the second a-tile; the
                          ragged tile's last live vector holds 2 elements
        (3330, 2, 60) 14  120 rows; the ragged tile is 2 elements in all
float64 (512, 2, 16)   2  32 rows, whole 32x256 tiles only
        (961, 2, 27)   4  54 rows, odd R, rows past La

A ragged tile of 2 elements behind two whole ones, (514, 2, 60), does not fuse:
rows of 514 float32 are neither 16-byte aligned nor padded (the padding would
exceed 1/16 of the row).  (726, 2, 60) is the shortest padded R = 2 mod 4 that
still picks 64x256 in 3 b-tiles; R = 3330 is the shortest whose ragged tile is
2 elements and for which pick_tile prefers 64x256 to 64x64.  float64 rows of
771 go to 64x32 tiles; 961 is the shortest odd R in 4 b-tiles of 32x256.
"""
import functools

import numpy as np
import pytest

import bolt_amd as bolt
import bolt_amd.mi355x.array as A
import golden_cases as G

pytestmark = pytest.mark.gpu

NAMES = ("mean", "var", "std")

# (dtype, shape, b-tiles)
F32_WHOLE = ("float32", (512, 2, 64), 2)
F32_C2_TAIL = ("float32", (720, 2, 64), 3)
F64_WHOLE = ("float64", (512, 2, 16), 2)
SHAPES = [
    F32_WHOLE,
    F32_C2_TAIL,
    ("float32", (726, 2, 60), 3),
    ("float32", (3330, 2, 60), 14),
    F64_WHOLE,
    ("float64", (961, 2, 27), 4),
]
_ids = lambda cases: ["%s-%s" % (c[0], "x".join(map(str, c[1]))) for c in cases]  # noqa: E731


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


def _fused_state(arr):
    e = (arr.__dict__.get("_kept") or {}).get((arr.ndim - 1,))
    return e if e is not None and e.serves_mean else None


def _btiles(s):
    """b-tiles of the swap that made ``s``: its workspace holds 24 B per row and b-tile."""
    from bolt_amd.mi355x._ops import dtype_code
    rows, R = int(np.prod(s.shape[:-1])), s.shape[-1]
    pitch = s.__dict__.get("_pitch", R)
    nws = s._backend.copy_moments_plan([rows, R], [1, rows], [pitch, 1], s.dtype.itemsize, dtype_code(s.dtype), R,
                                       pitch, rows)[3]
    assert nws % (24 * rows) == 0
    return nws // (24 * rows)


@functools.lru_cache(maxsize=None)
def _rows(dtype, shape, kind):
    """The result rows (La, R) of one case, read-only: every row its own mean and std."""
    N, p, q = shape
    La = p * q
    rng = np.random.default_rng(N + q)
    r = np.arange(La)[:, None]
    rows = (10.0 * r + (1 + r % 7) * rng.standard_normal((La, N))).astype(dtype)
    if kind == "pivots":  # every one in the first column of a tile: the pivot of its row there
        rows[[3, 40], 0] = np.nan
        rows[[5, 77], 256] = np.inf
        rows[9, 256] = -np.inf
    elif kind == "constant":
        rows[0, :] = 1234.5
        rows[La - 1 if La < 64 else 63, :] = -77.25
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def _truth(dtype, shape, kind):
    with np.errstate(all="ignore"):
        rows = np.asarray(_rows(dtype, shape, kind), dtype=np.longdouble)
        return {n: getattr(rows, n)(axis=-1) for n in NAMES}


def _swap(gctx, dtype, shape, kind, ntb):
    """The fused swap of one case, the kernel checked through the b-tile count."""
    N, p, q = shape
    rows = _rows(dtype, shape, kind)
    s = bolt.array(np.ascontiguousarray(rows.T).reshape(N, p, q), gctx).swap((0,), (0, 1))
    assert _fused_state(s) is not None, "the swap did not fuse"
    assert _btiles(s) == ntb
    return s


def _stats(s):
    return {n: getattr(s, n)(axis=2).reshape(-1) for n in NAMES}


def _close(got, dtype, shape, kind, sel, n):
    t = _truth(dtype, shape, kind)[n][sel]
    return G.stat_close(got[n][sel], t.astype(got[n].dtype), t, got[n].dtype, _rows(dtype, shape, kind)[sel], n)


@pytest.mark.parametrize("dtype,shape,ntb", SHAPES, ids=_ids(SHAPES))
def test_distinct_rows(gctx, fuse_small, dtype, shape, ntb):
    s = _swap(gctx, dtype, shape, "normal", ntb)
    got = _stats(s)
    rows = _rows(dtype, shape, "normal")
    for n in NAMES:
        assert got[n].shape == (rows.shape[0],)
        assert _close(got, dtype, shape, "normal", slice(None), n), (n, dtype, shape)
    # x.transpose(1, 2, 0) of the (N, p, q) input, made contiguous, is the rows themselves
    assert s.toarray().tobytes() == rows.tobytes()


def test_pivots_per_pair(gctx, fuse_small):
    dtype, shape, ntb = F32_WHOLE
    s = _swap(gctx, dtype, shape, "pivots", ntb)
    got = _stats(s)
    rows = _rows(dtype, shape, "pivots")
    bad = np.zeros(rows.shape[0], dtype=bool)
    bad[[3, 40, 5, 77, 9]] = True
    with np.errstate(all="ignore"):
        ref = rows[bad].astype(np.float64).mean(axis=-1).astype(got["mean"].dtype)
    assert np.array_equal(got["mean"][bad], ref, equal_nan=True), got["mean"][bad]
    for n in ("var", "std"):
        assert np.all(np.isnan(got[n][bad])), (n, got[n][bad])
    for n in NAMES:
        assert _close(got, dtype, shape, "pivots", ~bad, n), n
    assert s.toarray().tobytes() == rows.tobytes()


CONSTANT = [F32_WHOLE, F32_C2_TAIL, F64_WHOLE]


@pytest.mark.parametrize("dtype,shape,ntb", CONSTANT, ids=_ids(CONSTANT))
def test_constant_rows(gctx, fuse_small, dtype, shape, ntb):
    got = _stats(_swap(gctx, dtype, shape, "constant", ntb))
    rows = _rows(dtype, shape, "constant")
    const = [0, rows.shape[0] - 1 if rows.shape[0] < 64 else 63]
    assert np.all(got["var"][const] == 0.0) and np.all(got["std"][const] == 0.0), (got["var"][const], got["std"][const])
    assert np.array_equal(got["mean"][const], rows[const, 0])
    rest = np.ones(rows.shape[0], dtype=bool)
    rest[const] = False
    for n in NAMES:
        assert _close(got, dtype, shape, "constant", rest, n), n


SWITCH = [F32_WHOLE + ("pivots",), F32_C2_TAIL + ("normal",), F64_WHOLE + ("normal",)]


@pytest.mark.parametrize("dtype,shape,ntb,kind", SWITCH, ids=_ids(SWITCH))
def test_agrees_with_the_switch_off_path(gctx, fuse_small, monkeypatch, dtype, shape, ntb, kind):
    fused = _stats(_swap(gctx, dtype, shape, kind, ntb))
    monkeypatch.setattr(A, "FUSE_SWAP_MOMENTS", False)
    N, p, q = shape
    rows = _rows(dtype, shape, kind)
    s = bolt.array(np.ascontiguousarray(rows.T).reshape(N, p, q), gctx).swap((0,), (0, 1))
    assert _fused_state(s) is None
    plain = _stats(s)
    fin = np.isfinite(rows.astype(np.float64)).all(axis=-1)
    for n in NAMES:
        assert np.array_equal(np.isnan(plain[n]), np.isnan(fused[n])), n
        assert _close(plain, dtype, shape, kind, fin, n), ("plain", n)
        assert _close(fused, dtype, shape, kind, fin, n), ("fused", n)
