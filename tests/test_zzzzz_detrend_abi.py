"""bm_detrend_rows / bm_detrend_apply refuse bad arguments before any launch:
every call here fails its checks (or has nothing to do, or is not taken), so no
device is touched and the pointers, host addresses, are never dereferenced.
(Named to be collected after every other module: see test_zzzzz_detrend.)"""
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
E = _lib.BM_E_ARG
_BAD_OUT = ((F32, F64), (F32, F16), (F16, F32), (F64, F32), (U8, F32), (U8, U8), (I32, F32), (I64, I64), (F32, 99))


def test_constants():
    assert _lib.DETREND_MAX_ORDER == 8 == 2 * _lib.COMOMENT_MAX_SIGNALS   # BM_DETREND_MAX_ORDER


def test_rows_argument_errors(lib, p):
    f = lib.bm_detrend_rows
    taken = ctypes.c_int(7)
    t = ctypes.byref(taken)
    # (src, in_dtype, O, R, src_pitch, order, dst, out_dtype, dst_pitch, taken, stream)
    for src, dst, tk in ((None, p, t), (p, None, t), (p, p, None)):
        assert f(src, F32, 2, 8, 8, 1, dst, F32, 8, tk, None) == E
        assert b"null pointer" in lib.bm_last_error()
    assert f(p, 99, 2, 8, 8, 1, p, F64, 8, t, None) == E
    assert b"bad dtype" in lib.bm_last_error()
    # the output dtype is the input's statistics dtype, nothing else
    for din, dout in _BAD_OUT:
        assert f(p, din, 2, 8, 8, 1, p, dout, 8, t, None) == E, (din, dout)
        assert b"out_dtype" in lib.bm_last_error()
    for O, R in ((-1, 8), (2, -1)):
        assert f(p, F32, O, R, 8, 1, p, F32, 8, t, None) == E
        assert b"negative extent" in lib.bm_last_error()
    assert f(p, F32, 2, 8, 7, 1, p, F32, 8, t, None) == E   # src_pitch < R
    assert b"pitch" in lib.bm_last_error()
    assert f(p, F32, 2, 8, 8, 1, p, F32, 7, t, None) == E   # dst_pitch < R
    assert b"pitch" in lib.bm_last_error()
    for order in (0, -1, 9, 100):
        assert f(p, F32, 2, 2000, 2000, order, p, F32, 2000, t, None) == E, order
        assert b"outside 1..8" in lib.bm_last_error()
    for R, order in ((8, 8), (3, 5), (1, 1), (2, 2)):
        assert f(p, F32, 2, R, R, order, p, F32, R, t, None) == E, (R, order)
        assert b"order < R" in lib.bm_last_error()
    assert taken.value == 7  # a refused call leaves it alone


def test_rows_noop_and_not_taken(lib, p):
    f = lib.bm_detrend_rows
    taken = ctypes.c_int(7)
    t = ctypes.byref(taken)
    # nothing to write: a no-op, not an error
    assert f(p, F32, 0, 8, 8, 3, p, F32, 8, t, None) == 0 and taken.value == 1
    taken.value = 7
    assert f(p, U8, 0, 8, 8, 1, p, F64, 8, t, None) == 0 and taken.value == 1
    taken.value = 7
    assert f(p, F32, 2, 0, 0, 1, p, F32, 0, t, None) == 0 and taken.value == 1
    # rows the kernels do not hold: *taken = 0, nothing launched
    for order in (1, 8):
        taken.value = 7
        assert f(p, F32, 2, 50000, 50000, order, p, F32, 50000, t, None) == 0 and taken.value == 0
        taken.value = 7
        assert f(p, F32, 255, 2052, 2052, order, p, F32, 2052, t, None) == 0 and taken.value == 0
        taken.value = 7
        assert f(p, F32, 256, 8196, 8196, order, p, F32, 8196, t, None) == 0 and taken.value == 0
    # the vector must divide dst_pitch too: R = 2048 at a dst pitch of 2049 runs scalar, 8 elements a thread,
    # and 3 rows of 2048 are then neither a wave's (512) nor enough for a block each
    taken.value = 7
    assert f(p, F32, 3, 2048, 2048, 2, p, F32, 2049, t, None) == 0 and taken.value == 0


def test_apply_argument_errors(lib, p):
    f = lib.bm_detrend_apply
    # (src, in_dtype, O, R, I, src_pitch, mean, coef, basis, order, dst, out_dtype, dst_pitch, stream)
    for at in (0, 6, 7, 8, 10):
        a = [p, F32, 2, 8, 1, 8, p, p, p, 1, p, F32, 8, None]
        a[at] = None
        assert f(*a) == E, at
        assert b"null pointer" in lib.bm_last_error()
    assert f(p, 99, 2, 8, 1, 8, p, p, p, 1, p, F64, 8, None) == E
    assert b"bad dtype" in lib.bm_last_error()
    for din, dout in _BAD_OUT:
        assert f(p, din, 2, 8, 1, 8, p, p, p, 1, p, dout, 8, None) == E, (din, dout)
        assert b"out_dtype" in lib.bm_last_error()
    for O, R, I in ((-1, 8, 1), (2, -1, 1), (2, 8, -1)):
        assert f(p, F32, O, R, I, 8, p, p, p, 1, p, F32, 8, None) == E
        assert b"negative extent" in lib.bm_last_error()
    # pitches: >= R, and R itself unless I == 1
    for I, sp, dp in ((1, 7, 8), (1, 8, 7), (4, 9, 8), (4, 8, 9)):
        assert f(p, F32, 2, 8, I, sp, p, p, p, 1, p, F32, dp, None) == E, (I, sp, dp)
        assert b"pitches" in lib.bm_last_error()
    for order in (0, -1, 9):
        assert f(p, F32, 2, 2000, 1, 2000, p, p, p, order, p, F32, 2000, None) == E, order
        assert b"outside 1..8" in lib.bm_last_error()
    # (order >= R is the rows entry point's refusal only: R here may be one rank's slab of a longer record,
    # and the basis table is the caller's)
    # nothing to write: a no-op, not an error
    for O, R, I in ((0, 8, 1), (2, 0, 1), (2, 8, 0), (0, 8, 4)):
        sp = R
        assert f(p, F32, O, R, I, sp, p, p, p, 1, p, F32, sp, None) == 0, (O, R, I)
