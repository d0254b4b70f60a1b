"""swap() leaves the moment state of the result's rows (array.FUSE_SWAP_MOMENTS,
bm_copy_strided_moments): the transpose kernel that moves the records also
emits (mean, M2) of every tile row, and mean / var / std over the last axis of
the result are finished from the merged state without a reduction launch.

Everything here runs on the GPU (the CPU test executor has no such capability
and keeps the plain path).  _FUSE_SWAP_MIN_BYTES (the 256 MiB Infinity Cache)
is lowered to 0; the state-size rule (16 B per row at most 1/64 of the bytes)
stays at its real value except for the one shape with 40-element rows.  The
module keeps one context for all its tests and runs after the others.

Tile shapes (bm_copy.hip pick_tile) of the swaps below, TA x TB with TB along
the result's rows: float32 (600, 4, 36) 32x64 (ten b-tiles, a tail of 24 and a
tail a-tile), (760, 2, 64) 64x256 (C2's tile: three b-tiles, a tail of 248),
(760, 4, 36) 32x256 (tail a-tile), (256, 2, 64) 64x256 (one full b-tile),
(40, 8, 16) 64x64 (one partial b-tile, four rows per wave); float64
(520, 3, 32) 32x64, (1000, 2, 16) 32x256 (two waves per tile row); the
numerics rows float32 16x256 and float64 16x128, the C ABI cases float32 64x128
and float64 64x32: every moments tile the library has is run here.  Rows of
760 float32 and 520 / 1000 float64 are stored at a padded pitch, the others
dense.
"""
import ctypes

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


def _counting(mp, be):
    calls = {"reduce": 0, "reduce_rows": 0, "reduce_combine": 0, "copy_strided": 0}

    def proxy(name, fn):
        def call(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return call
    for name in calls:
        mp.setattr(be, name, proxy(name, getattr(be, name)), raising=False)
    return calls


def _x(shape, dtype, seed=0):
    rng = np.random.default_rng(seed)
    return (10 + 3 * rng.standard_normal(shape)).astype(dtype)


def _truth(rows, name):
    r = np.asarray(rows, dtype=np.longdouble)
    v = getattr(r, name)(axis=-1)
    return v


def _fused_state(arr):
    e = (arr.__dict__.get("_kept") or {}).get((arr.ndim - 1,))
    return e if e is not None and e.serves_mean else None


# (dtype, shape, padded rows expected, state-size divisor)
SHAPES = [
    ("float32", (600, 4, 36), False, 64),
    ("float32", (760, 2, 64), True, 64),
    ("float32", (760, 4, 36), True, 64),
    ("float32", (256, 2, 64), False, 64),
    ("float32", (40, 8, 16), False, 1),
    ("float64", (520, 3, 32), True, 64),
    ("float64", (1000, 2, 16), True, 64),
]


@pytest.mark.parametrize("dtype,shape,padded,div", SHAPES, ids=["%s-%s" % (d, "x".join(map(str, s)))
                                                              for d, s, _, _ in SHAPES])
def test_swap_leaves_the_state(gctx, fuse_small, monkeypatch, dtype, shape, padded, div):
    import torch
    monkeypatch.setattr(A, "_FUSE_SWAP_STATE_DIV", div)
    x = _x(shape, dtype, seed=len(shape) + shape[0])
    want = torch.from_numpy(x).permute(1, 2, 0).contiguous().numpy()
    base = bolt.array(x, gctx)
    calls = _counting(monkeypatch, base._backend)
    s = base.swap((0,), (0, 1))
    assert calls["copy_strided"] == 1
    assert ("_pbuf" in s.__dict__) == padded
    assert _fused_state(s) is not None, "the swap did not fuse"
    got = {n: getattr(s, n)(axis=2) for n in NAMES}
    assert calls["reduce"] == 0 and calls["reduce_rows"] == 0 and calls["reduce_combine"] == 3
    for n in NAMES:
        t = _truth(want, n)
        assert got[n].shape == want.shape[:2]
        assert G.stat_close(got[n], t.astype(got[n].dtype), t, got[n].dtype, x, n), (n, dtype, shape)
    # the records, bit for bit (a padded result is compacted here: the state stays)
    assert s.toarray().tobytes() == want.tobytes()
    assert _fused_state(s) is not None


def test_unaligned_rows_do_not_fuse(gctx, fuse_small, monkeypatch):
    """Source rows of 65 float32 (260 B) are not 16-B aligned: the element-wise
    tiles run, nothing is kept and every result is the switch-off path's."""
    x = _x((300, 5, 13), "float32", seed=5)
    s = bolt.array(x, gctx).swap((0,), (0, 1))
    assert not s.__dict__.get("_kept")
    got = [getattr(s, n)(axis=2) for n in NAMES]
    monkeypatch.setattr(A, "FUSE_SWAP_MOMENTS", False)
    p = bolt.array(x, gctx).swap((0,), (0, 1))
    assert s.toarray().tobytes() == p.toarray().tobytes() == np.ascontiguousarray(x.transpose(1, 2, 0)).tobytes()
    for g, n in zip(got, NAMES):
        assert g.tobytes() == getattr(p, n)(axis=2).tobytes()


R_NUM = 520  # float32 / float64 rows of 520: three 256-wide or nine 64-wide b-tiles


def _numeric_rows(dtype):
    rng = np.random.default_rng(11)
    rows = rng.standard_normal((16, R_NUM))
    rows[0:4] += 1e6                       # offset data
    rows[4, 0] += 100.0                    # one outlier, at the pivot's position
    rows[5] = 1234.5                       # constant rows
    rows[6] = 1e6 + 0.5
    rows = rows.astype(dtype)
    rows[7, 300] = np.nan
    rows[8, 10] = np.inf                   # in the first b-tile
    rows[9, R_NUM - 1] = np.inf            # in the last one
    # infinities at a tile's first column, where the tile takes its pivot:
    # 256 and 512 start a b-tile of every width (64, 128, 256)
    rows[10, 256] = np.inf
    rows[11, 512] = -np.inf
    rows[13, 256] = np.inf                 # inf - inf over the row: NaN
    rows[13, 512] = -np.inf
    return rows


_NONFINITE = (7, 8, 9, 10, 11, 13)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_numerics_rows(gctx, fuse_small, monkeypatch, dtype):
    rows = _numeric_rows(dtype)
    x = np.ascontiguousarray(rows.T).reshape(R_NUM, 2, 8)
    s = bolt.array(x, gctx).swap((0,), (0, 1))
    assert _fused_state(s) is not None
    got = {n: getattr(s, n)(axis=2).reshape(16) for n in NAMES}
    monkeypatch.setattr(A, "FUSE_SWAP_MOMENTS", False)
    p = bolt.array(x, gctx).swap((0,), (0, 1))
    assert not p.__dict__.get("_kept")
    off = {n: getattr(p, n)(axis=2).reshape(16) for n in NAMES}
    fin = np.array([r not in _NONFINITE for r in range(16)])
    with np.errstate(all="ignore"):
        for n in NAMES:
            t = _truth(rows[fin], n)
            print(n, dtype, "max rel err", float(np.max(np.abs(got[n][fin] - t) / np.maximum(np.abs(t), 1e-300))))
            assert G.stat_close(got[n][fin], t.astype(got[n].dtype), t, got[n].dtype, rows[fin], n), (n, dtype)
            # NaN exactly where the switch-off path gives NaN
            assert np.array_equal(np.isnan(got[n]), np.isnan(off[n])), (n, got[n][7:14], off[n][7:14])
        assert got["std"][5] == 0.0 and got["std"][6] == 0.0 and got["var"][5] == 0.0 and got["var"][6] == 0.0
        assert got["mean"][5] == rows[5, 0] and got["mean"][6] == rows[6, 0]
        assert np.isnan(got["mean"][7]) and got["mean"][8] == np.inf and got["mean"][9] == np.inf
        assert got["mean"][10] == np.inf and got["mean"][11] == -np.inf
        assert np.isnan(got["mean"][13])
        # the means of the non-finite rows are the switch-off path's
        assert np.array_equal(got["mean"][list(_NONFINITE)], off["mean"][list(_NONFINITE)], equal_nan=True)
        if dtype == "float64":
            keep = np.array([r for r in range(16) if fin[r] and r not in (5, 6)])
            t = _truth(rows[keep], "var")
            assert np.all(np.abs(got["var"][keep] - t) <= 1e-12 * np.abs(t))


# ------------------------------------------------------------------ the C ABI
def _abi_case(gctx, dtype="float32", La=128, R=600, pitch=608):
    import torch
    from bolt_amd.mi355x._ops import backend_for, dtype_code
    dev = torch.device("cuda:0")
    be = backend_for(dev)
    x = _x((R, La), dtype, seed=3)                     # source: R rows of La; result: La rows of R
    es = x.dtype.itemsize
    src = torch.from_numpy(x.view(np.uint8).reshape(-1)).to(dev)
    dst = torch.full((La * pitch * es,), 0xAB, dtype=torch.uint8, device=dev)
    shape, sstr, dstr = _lib.i64_array([La, R]), _lib.i64_array([1, La]), _lib.i64_array([pitch, 1])
    code = dtype_code(x.dtype)
    return be, dev, x, es, src, dst, (shape, sstr, dstr), code


def _call(be, src, dst, arrs, es, code, R, pitch, rows, ws, nws, state, nstate):
    fused = ctypes.c_int(-7)
    rc = be.lib.bm_copy_strided_moments(src.data_ptr(), dst.data_ptr(), 2, arrs[0], arrs[1], arrs[2], es, code,
                                        R, pitch, rows, ws.data_ptr() if ws is not None else None, nws,
                                        state.data_ptr() if state is not None else None, nstate,
                                        ctypes.byref(fused), be._stream(src))
    return rc, fused.value


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_abi_state_matches_reduce_state(gctx, dtype):
    import torch
    La, R, pitch = 128, 600, 608
    be, dev, x, es, src, dst, arrs, code = _abi_case(gctx, dtype, La, R, pitch)
    n = ctypes.c_size_t(0)
    assert be.lib.bm_copy_strided_moments_workspace_bytes(2, arrs[0], arrs[1], arrs[2], es, code, R, pitch, La,
                                                          ctypes.byref(n)) == 0
    assert n.value > 0 and n.value % (24 * La) == 0     # three float64 planes per b-tile
    ws = torch.empty(n.value, dtype=torch.uint8, device=dev)
    nstate = be.state_bytes(_lib.STAT_VAR, code, La)
    assert nstate == 16 * La
    state = torch.zeros(nstate, dtype=torch.uint8, device=dev)
    rc, fused = _call(be, src, dst, arrs, es, code, R, pitch, La, ws, n.value, state, nstate)
    assert (rc, fused) == (0, 1), be.lib.bm_last_error()
    out = dst.cpu().numpy().view(x.dtype).reshape(La, pitch)
    assert out[:, :R].tobytes() == np.ascontiguousarray(x.T).tobytes()
    assert np.all(out[:, R:].view(np.uint8) == 0xAB)      # the pad is not written
    dense = torch.from_numpy(np.ascontiguousarray(x.T).view(np.uint8).reshape(-1)).to(dev)
    ref = torch.zeros(nstate, dtype=torch.uint8, device=dev)
    be.reduce_state(_lib.STAT_VAR, dense, code, La, R, 1, ref)
    a = state.cpu().numpy().view(np.float64).reshape(2, La)
    b = ref.cpu().numpy().view(np.float64).reshape(2, La)
    tm, tv = _truth(x.T, "mean"), _truth(x.T, "var")
    assert G.stat_close(a[0], b[0], tm, np.float64, x, "mean")
    assert G.stat_close(a[1] / R, b[1] / R, tv, np.float64, x, "var")
    # a workspace one byte short is refused, nothing fused
    rc, fused = _call(be, src, dst, arrs, es, code, R, pitch, La, ws, n.value - 1, state, nstate)
    assert (rc, fused) == (_lib.BM_E_WS, 0)


def test_abi_bad_arguments_launch_nothing(gctx):
    import torch
    La, R, pitch = 128, 600, 608
    be, dev, x, es, src, dst, arrs, code = _abi_case(gctx, "float32", La, R, pitch)
    ws = torch.empty(24 * La * 16, dtype=torch.uint8, device=dev)
    nstate = 16 * La
    state = torch.full((nstate,), 0xCD, dtype=torch.uint8, device=dev)
    bad = [
        dict(state=None),                         # null state
        dict(nstate=nstate - 8),                  # state too small
        dict(R=R + 1),                            # R does not match the copy
        dict(pitch=R - 1),                        # pitch below R
        dict(code=_lib.BM_I32),                   # not a float dtype
    ]
    for kw in bad:
        a = dict(R=R, pitch=pitch, state=state, nstate=nstate, code=code)
        a.update(kw)
        rc, fused = _call(be, src, dst, arrs, es, a["code"], a["R"], a["pitch"], La, ws, ws.numel(), a["state"],
                          a["nstate"])
        assert rc == _lib.BM_E_ARG and fused in (0, -7), kw
        assert b"bm_copy_strided_moments" in be.lib.bm_last_error()
    torch.cuda.synchronize()
    assert bool((dst == 0xAB).all()) and bool((state == 0xCD).all())


# -------------------------------------------------------- switches, lifetime
def test_switch_and_threshold(gctx, monkeypatch):
    x = _x((760, 2, 64), "float32", seed=9)
    want = np.ascontiguousarray(x.transpose(1, 2, 0))
    # the default threshold: a small swap asks for nothing
    monkeypatch.setattr(A, "FUSE_SWAP_MOMENTS", True)
    base = bolt.array(x, gctx)
    calls = _counting(monkeypatch, base._backend)
    d = base.swap((0,), (0, 1))
    assert "_kept" not in d.__dict__
    ref = [getattr(d, n)(axis=2) for n in NAMES]
    assert calls["reduce_rows"] >= 1
    # the switch off, threshold lowered: the same
    monkeypatch.setattr(A, "_FUSE_SWAP_MIN_BYTES", 0)
    monkeypatch.setattr(A, "FUSE_SWAP_MOMENTS", False)
    o = bolt.array(x, gctx).swap((0,), (0, 1))
    assert "_kept" not in o.__dict__
    assert [getattr(o, n)(axis=2).tobytes() for n in NAMES] == [r.tobytes() for r in ref]
    assert o.toarray().tobytes() == d.toarray().tobytes() == want.tobytes()


def test_lifetime(gctx, fuse_small, monkeypatch):
    x = _x((760, 2, 64), "float32", seed=10)
    s = bolt.array(x, gctx).swap((0,), (0, 1))
    e = _fused_state(s)
    assert e is not None
    m = s.mean(axis=2)
    # a further swap of the result carries nothing over: rows of 64 float32 are
    # below the state-size rule, so the back-swap keeps no state at all and its
    # statistic reads its own rows
    back = s.swap((0, 1), (0,))
    assert not back.__dict__.get("_kept")
    assert back.toarray().tobytes() == x.tobytes()
    bm = back.mean(axis=2)
    tb = _truth(x, "mean")
    assert G.stat_close(bm, tb.astype(bm.dtype), tb, bm.dtype, x, "mean")
    # swapping again fuses a state of its own, right for its own rows
    again = back.swap((0,), (0, 1))
    e3 = _fused_state(again)
    assert e3 is not None and e3[0] is not e[0]
    sd = again.std(axis=2)
    ts = _truth(np.ascontiguousarray(x.transpose(1, 2, 0)), "std")
    assert G.stat_close(sd, ts.astype(sd.dtype), ts, sd.dtype, x, "std")
    # derived arrays are new objects and start empty
    for derived in (s[:, :32], s.astype("float64"), s.clip(0, 20)):
        assert derived is not s and not derived.__dict__.get("_kept")
    assert _fused_state(s) is e
    # unpersist() drops it; the statistic then reads the rows
    s.unpersist()
    assert "_kept" not in s.__dict__
    calls = _counting(monkeypatch, s._backend)
    m2 = s.mean(axis=2)
    assert calls["reduce_rows"] + calls["reduce"] == 1
    t = _truth(np.ascontiguousarray(x.transpose(1, 2, 0)), "mean")
    assert G.stat_close(m, t.astype(m.dtype), t, m.dtype, x, "mean")
    assert G.stat_close(m2, t.astype(m2.dtype), t, m2.dtype, x, "mean")
