"""bm_standardize_rows / bm_standardize_apply refuse bad arguments before any
launch: every call here fails its checks (or has nothing to do), so no device
is touched and the pointers, host addresses, are never dereferenced."""
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


def test_rows_argument_errors(lib, p):
    f = lib.bm_standardize_rows
    taken = ctypes.c_int(7)
    t = ctypes.byref(taken)
    for src, dst, tk in ((None, p, t), (p, None, t), (p, p, None)):
        assert f(src, F32, 2, 8, 8, dst, F32, 8, 1, tk, None) == _lib.BM_E_ARG
        assert b"null pointer" in lib.bm_last_error()
    assert f(p, F32, 2, 8, 7, p, F32, 8, 1, t, None) == _lib.BM_E_ARG   # src_pitch < R
    assert b"pitch" in lib.bm_last_error()
    assert f(p, F32, 2, 8, 8, p, F32, 7, 1, t, None) == _lib.BM_E_ARG   # dst_pitch < R
    assert b"pitch" in lib.bm_last_error()
    # the output dtype is the input's statistics dtype, nothing else
    for din, dout in ((F32, F64), (F32, F16), (F16, F32), (F64, F32), (U8, F32), (U8, U8), (I32, F32), (I64, I64),
                      (F32, 99)):
        assert f(p, din, 2, 8, 8, p, dout, 8, 1, t, None) == _lib.BM_E_ARG, (din, dout)
        assert b"out_dtype" in lib.bm_last_error()
    assert f(p, 99, 2, 8, 8, p, F64, 8, 1, t, None) == _lib.BM_E_ARG
    assert b"bad dtype" in lib.bm_last_error()
    for scale in (-1, 2):
        assert f(p, F32, 2, 8, 8, p, F32, 8, scale, t, None) == _lib.BM_E_ARG
        assert b"scale" in lib.bm_last_error()
    for O, R in ((-1, 8), (2, -1)):
        assert f(p, F32, O, R, 8, p, F32, 8, 1, t, None) == _lib.BM_E_ARG
        assert b"negative extent" in lib.bm_last_error()
    assert taken.value == 7  # a refused call leaves it alone
    # nothing to write: a no-op, not an error
    assert f(p, F32, 0, 8, 8, p, F32, 8, 1, t, None) == 0 and taken.value == 1
    assert f(p, U8, 0, 8, 8, p, F64, 8, 0, t, None) == 0
    assert f(p, F32, 2, 0, 0, p, F32, 0, 1, t, None) == 0
    # rows the kernels do not hold: *taken = 0, nothing launched
    taken.value = 7
    assert f(p, F32, 2, 50000, 50000, p, F32, 50000, 1, t, None) == 0 and taken.value == 0
    taken.value = 7
    assert f(p, F32, 255, 2052, 2052, p, F32, 2052, 1, t, None) == 0 and taken.value == 0


def test_apply_argument_errors(lib, p):
    g = lib.bm_standardize_apply
    for src, mean, dst in ((None, p, p), (p, None, p), (p, p, None)):
        assert g(src, F32, 2, 8, 1, 8, mean, p, dst, F32, 8, None) == _lib.BM_E_ARG
        assert b"null pointer" in lib.bm_last_error()
    assert g(p, F32, 2, 8, 1, 7, p, p, p, F32, 8, None) == _lib.BM_E_ARG   # src_pitch < R
    assert b"pitches" in lib.bm_last_error()
    assert g(p, F32, 2, 8, 1, 8, p, p, p, F32, 7, None) == _lib.BM_E_ARG   # dst_pitch < R
    assert g(p, F32, 2, 8, 4, 16, p, p, p, F32, 8, None) == _lib.BM_E_ARG  # a pitch with I > 1
    assert g(p, F32, 2, 8, 4, 8, p, p, p, F32, 16, None) == _lib.BM_E_ARG
    assert b"pitches" in lib.bm_last_error()
    for din, dout in ((F32, F64), (U8, F32), (F64, F32), (I64, I64), (F16, F32)):
        assert g(p, din, 2, 8, 1, 8, p, None, p, dout, 8, None) == _lib.BM_E_ARG
        assert b"out_dtype" in lib.bm_last_error()
    assert g(p, 99, 2, 8, 1, 8, p, p, p, F64, 8, None) == _lib.BM_E_ARG
    for O, R, I in ((-1, 8, 1), (2, -8, 1), (2, 8, -1)):
        assert g(p, F32, O, R, I, 8, p, p, p, F32, 8, None) == _lib.BM_E_ARG
        assert b"negative extent" in lib.bm_last_error()
    for O, R, I in ((0, 8, 1), (2, 0, 1), (2, 8, 0)):
        assert g(p, F32, O, R, I, R, p, None, p, F32, R, None) == 0
