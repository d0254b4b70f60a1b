"""bm_quantile_rows / bm_quantile_select refuse bad arguments before any
launch, and bm_quantile_workspace_bytes sizes the streaming path's scratch:
every call here fails its checks (or has nothing to do), so no device is
touched and the pointers, host addresses, are never dereferenced."""
import ctypes

import pytest

from bolt_amd.mi355x import _lib


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def p():
    buf = ctypes.create_string_buffer(4096)
    yield ctypes.addressof(buf)
    del buf


F16, F32, F64, U8, I32, I64 = _lib.BM_F16, _lib.BM_F32, _lib.BM_F64, _lib.BM_U8, _lib.BM_I32, _lib.BM_I64


def _calls(lib, p):
    """Both entry points behind one signature: f(src, dtype, O, R, pitch, ranks, frac, out, out_dtype)."""
    taken = ctypes.c_int(7)

    def rows(src, dt, O, R, pitch, ranks, frac, out, odt):
        r = None if ranks is None else _lib.i64_array(ranks)
        g = None if frac is None else _lib.f64_array(frac)
        n = len(ranks if ranks is not None else frac)
        return lib.bm_quantile_rows(src, dt, O, R, pitch, r, g, n, out, odt, ctypes.byref(taken), None)

    def select(src, dt, O, R, pitch, ranks, frac, out, odt):
        r = None if ranks is None else _lib.i64_array(ranks)
        g = None if frac is None else _lib.f64_array(frac)
        n = len(ranks if ranks is not None else frac)
        return lib.bm_quantile_select(src, dt, O, R, pitch, r, g, n, out, odt, p, 4096, None)

    return (rows, select), taken


def test_argument_errors(lib, p):
    fs, taken = _calls(lib, p)
    E = _lib.BM_E_ARG
    for f in fs:
        for src, ranks, frac, out in ((None, [1], [0.0], p), (p, None, [0.0], p), (p, [1], None, p), (p, [1], [0.0], None)):
            assert f(src, F32, 2, 8, 8, ranks, frac, out, F32) == E
            assert b"null pointer" in lib.bm_last_error()
        assert f(p, 99, 2, 8, 8, [1], [0.0], p, F64) == E
        assert b"bad dtype" in lib.bm_last_error()
        # the output dtype is the input's own or its statistics dtype, nothing else
        for din, dout in ((F32, F64), (F32, F16), (F16, F32), (F64, F32), (U8, F32), (I32, F32), (I64, I32), (F32, 99)):
            assert f(p, din, 2, 8, 8, [1], [0.0], p, dout) == E, (din, dout)
            assert b"out_dtype" in lib.bm_last_error()
        # an interpolated quantile of integers needs float64
        assert f(p, I32, 2, 8, 8, [1], [0.5], p, I32) == E
        assert b"statistics dtype" in lib.bm_last_error()
        for O, R in ((-1, 8), (2, -1)):
            assert f(p, F32, O, R, 8, [0], [0.0], p, F32) == E
            assert b"negative extent" in lib.bm_last_error()
        assert f(p, F32, 2, 8, 7, [1], [0.0], p, F32) == E   # pitch < R
        assert b"pitch" in lib.bm_last_error()
        # a rank that is not below R; with frac != 0 the next rank counts too
        for ranks, frac in (([8], [0.0]), ([-1], [0.0]), ([7], [0.5]), ([0, 9], [0.0, 0.0])):
            assert f(p, F32, 2, 8, 8, ranks, frac, p, F32) == E, (ranks, frac)
            assert b"rank" in lib.bm_last_error()
        for frac in (-0.5, 1.0, float("nan")):
            assert f(p, F32, 2, 8, 8, [1], [frac], p, F32) == E
            assert b"frac" in lib.bm_last_error()
        # more than BM_QUANTILE_MAX_RANKS ranks: nine quantiles, or five that take two each
        assert f(p, F32, 2, 80, 80, list(range(9)), [0.0] * 9, p, F32) == E
        assert b"quantiles" in lib.bm_last_error()
        assert f(p, F32, 2, 80, 80, list(range(5)), [0.5] * 5, p, F32) == E
        assert b"ranks" in lib.bm_last_error()
        assert f(p, F32, 2, 8, 8, [], [], p, F32) == E
    assert taken.value == 7  # a refused call leaves it alone
    # nothing to write: a no-op, not an error
    for f in fs:
        assert f(p, F32, 0, 8, 8, [1], [0.5], p, F32) == 0
        assert f(p, U8, 0, 8, 8, [1], [0.0], p, U8) == 0
        assert f(p, F32, 2, 0, 0, [0], [0.0], p, F32) == E   # no rank is below R = 0
    assert taken.value == 1
    # rows the registers do not hold: *taken = 0, nothing launched
    rows = fs[0]
    for O, R in ((2, 50000), (255, 2052), (300, 8196)):
        taken.value = 7
        assert rows(p, F32, O, R, R, [1], [0.5], p, F32) == 0 and taken.value == 0
    taken.value = 7
    assert rows(p, F64, 3, 1028, 1028, [1], [0.5], p, F64) == 0 and taken.value == 0
    # a workspace that is missing or too small
    r, g = _lib.i64_array([1]), _lib.f64_array([0.5])
    assert lib.bm_quantile_select(p, F32, 2, 50000, 50000, r, g, 1, p, F32, None, 0, None) == _lib.BM_E_WS
    assert lib.bm_quantile_select(p, F32, 2, 50000, 50000, r, g, 1, p, F32, p, 16, None) == _lib.BM_E_WS
    assert b"workspace" in lib.bm_last_error()


def test_workspace_query(lib):
    def ws(dt, O, R, nranks):
        n = ctypes.c_size_t(0)
        assert lib.bm_quantile_workspace_bytes(dt, O, R, nranks, ctypes.byref(n)) == 0
        return n.value
    assert ws(F32, 0, 9000, 2) == 0 and ws(F32, 3, 0, 2) == 0
    # it grows with the rows and with the ranks, and holds a 64-bit 256-bin histogram per row and rank
    sizes = [[ws(F32, O, 9000, S) for S in range(1, _lib.QUANTILE_MAX_RANKS + 1)] for O in (1, 2, 3, 100)]
    for row in sizes:
        assert all(a < b for a, b in zip(row, row[1:]))
    for a, b in zip(sizes, sizes[1:]):
        assert all(x < y for x, y in zip(a, b))
    assert ws(F32, 3, 9000, 2) >= 3 * 2 * 256 * 8
    assert ws(U8, 3, 9000, 2) == ws(F64, 3, 9000, 2)
    n = ctypes.c_size_t(0)
    E = _lib.BM_E_ARG
    assert lib.bm_quantile_workspace_bytes(F32, 3, 9000, 2, None) == E
    assert lib.bm_quantile_workspace_bytes(99, 3, 9000, 2, ctypes.byref(n)) == E
    assert lib.bm_quantile_workspace_bytes(F32, -3, 9000, 2, ctypes.byref(n)) == E
    for S in (0, _lib.QUANTILE_MAX_RANKS + 1):
        assert lib.bm_quantile_workspace_bytes(F32, 3, 9000, S, ctypes.byref(n)) == E
        assert b"ranks" in lib.bm_last_error()
