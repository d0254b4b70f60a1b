"""bm_comoment_workspace_bytes / bm_comoment_state / bm_comoment_combine refuse
bad arguments before any launch: every call here fails its checks (or has
nothing to do), so no device is touched and the pointers, host addresses, are
never dereferenced."""
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


F16, F32, F64, U8, I64 = _lib.BM_F16, _lib.BM_F32, _lib.BM_F64, _lib.BM_U8, _lib.BM_I64
D4 = _lib.f64_array([0.0] * 4)


def test_state_argument_errors(lib, p):
    f = lib.bm_comoment_state
    for src, y, ym, st in ((None, p, D4, p), (p, None, D4, p), (p, p, None, p), (p, p, D4, None)):
        assert f(src, F32, 2, 8, 1, 8, y, ym, D4, 1, st, None, 0, None) == _lib.BM_E_ARG
        assert b"null pointer" in lib.bm_last_error()
    assert f(p, 99, 2, 8, 1, 8, p, D4, D4, 1, p, None, 0, None) == _lib.BM_E_ARG
    assert b"bad dtype" in lib.bm_last_error()
    for O, R, I in ((-1, 8, 1), (2, -8, 1), (2, 8, -1)):
        assert f(p, F32, O, R, I, 8, p, D4, D4, 1, p, None, 0, None) == _lib.BM_E_ARG
        assert b"negative extent" in lib.bm_last_error()
    assert f(p, F32, 2, 8, 1, 7, p, D4, D4, 1, p, None, 0, None) == _lib.BM_E_ARG    # pitch < R
    assert b"pitch" in lib.bm_last_error()
    assert f(p, F32, 2, 8, 4, 16, p, D4, D4, 1, p, None, 0, None) == _lib.BM_E_ARG   # a pitch with I > 1
    assert b"pitch" in lib.bm_last_error()
    for K in (0, -1, _lib.COMOMENT_MAX_SIGNALS + 1):
        assert f(p, F32, 2, 8, 1, 8, p, D4, D4, K, p, None, 0, None) == _lib.BM_E_ARG
        assert b"signals" in lib.bm_last_error()
    # nothing to store: a no-op, not an error (yresid may be NULL)
    for O, R, I in ((0, 8, 1), (2, 0, 1), (2, 8, 0)):
        assert f(p, F32, O, R, I, R, p, D4, None, 2, p, None, 0, None) == 0
    # a chunked reduction without its workspace
    assert f(p, F32, 2, 50000, 1, 50000, p, D4, D4, 1, p, None, 0, None) == _lib.BM_E_WS
    assert b"workspace" in lib.bm_last_error()


def test_combine_argument_errors(lib, p):
    g = lib.bm_comoment_combine
    cnt = _lib.i64_array([8])
    for st, c, ym, yq, out in ((None, cnt, D4, D4, p), (p, None, D4, D4, p), (p, cnt, None, D4, p),
                               (p, cnt, D4, None, p), (p, cnt, D4, D4, None)):
        assert g(_lib.CO_CORR, st, c, ym, yq, 1, 4, 1, out, F32, None) == _lib.BM_E_ARG
        assert b"null pointer" in lib.bm_last_error()
    for what in (-1, 2):
        assert g(what, p, cnt, D4, D4, 1, 4, 1, p, F32, None) == _lib.BM_E_ARG
        assert b"what" in lib.bm_last_error()
    for dout in (U8, I64, 99, -1):   # not a statistics dtype
        assert g(_lib.CO_COV, p, cnt, D4, D4, 1, 4, 1, p, dout, None) == _lib.BM_E_ARG
        assert b"out_dtype" in lib.bm_last_error()
    for K in (0, _lib.COMOMENT_MAX_SIGNALS + 1):
        assert g(_lib.CO_COV, p, cnt, D4, D4, 1, 4, K, p, F32, None) == _lib.BM_E_ARG
        assert b"signals" in lib.bm_last_error()
    many = _lib.i64_array([1] * 300)
    big = _lib.f64_array([0.0] * 1200)
    for nparts in (0, -1, _lib.COMOMENT_MAX_PARTS + 1):
        assert g(_lib.CO_COV, p, many, big, big, nparts, 4, 1, p, F32, None) == _lib.BM_E_ARG
        assert b"parts" in lib.bm_last_error()
    assert g(_lib.CO_COV, p, many, big, big, 100, 4, 4, p, F32, None) == _lib.BM_E_ARG   # 400 part signals
    assert g(_lib.CO_COV, p, cnt, D4, D4, 1, -4, 1, p, F32, None) == _lib.BM_E_ARG
    assert b"negative extent" in lib.bm_last_error()
    assert g(_lib.CO_COV, p, _lib.i64_array([-8]), D4, D4, 1, 4, 1, p, F32, None) == _lib.BM_E_ARG
    assert b"negative count" in lib.bm_last_error()
    for dout in (F16, F32, F64):
        assert g(_lib.CO_CORR, p, cnt, D4, D4, 1, 0, 1, p, dout, None) == 0   # nothing to store


def test_workspace_bytes(lib):
    w = lib.bm_comoment_workspace_bytes
    n = ctypes.c_size_t(7)
    assert w(F32, 2, 8, 1, 1, None) == _lib.BM_E_ARG
    assert w(99, 2, 8, 1, 1, ctypes.byref(n)) == _lib.BM_E_ARG
    assert w(F32, -2, 8, 1, 1, ctypes.byref(n)) == _lib.BM_E_ARG
    assert w(F32, 2, 8, 1, 5, ctypes.byref(n)) == _lib.BM_E_ARG and n.value == 7
    for O, R, I in ((0, 8, 1), (2, 0, 1), (2, 8, 0)):
        assert w(F32, O, R, I, 1, ctypes.byref(n)) == 0 and n.value == 0
    # monotone in K, on an unchunked and on chunked layouts (rows and columns)
    for dt, O, R, I in ((F32, 5, 300, 1), (F32, 2, 50000, 1), (F32, 1, 300, 35), (F64, 1, 20000, 8), (U8, 1, 10 ** 6, 1)):
        sizes = []
        for K in range(1, _lib.COMOMENT_MAX_SIGNALS + 1):
            assert w(dt, O, R, I, K, ctypes.byref(n)) == 0
            sizes.append(n.value)
        assert sizes == sorted(sizes), (O, R, I, sizes)
        assert (sizes[0] == 0) == (sizes[-1] == 0)
    assert w(F64, 1, 20000, 8, 1, ctypes.byref(n)) == 0 and n.value == 39 * 4 * 8 * 8  # 39 chunks, whatever the pointer
    assert w(F32, 5, 300, 1, 4, ctypes.byref(n)) == 0 and n.value == 0          # one chunk: no workspace
    assert w(F32, 2, 50000, 1, 1, ctypes.byref(n)) == 0 and n.value == 25 * 4 * 2 * 8  # 25 chunks of [P, S1, S2, Sxy]
