"""bm_normalize_rows refuses bad arguments before any launch: every call here
fails its checks (or has nothing to do, or is not taken), so no device is
touched and the pointers, host addresses, are never dereferenced.  (Named to
be collected after every other module: see test_zzz_normalize.)"""
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
MEAN, RANK = _lib.NORM_MEAN, _lib.NORM_RANK
E = _lib.BM_E_ARG


def test_constants():
    assert (MEAN, RANK) == (0, 1)   # BM_NORM_MEAN, BM_NORM_RANK of include/bolt_mi355x.h


def test_argument_errors(lib, p):
    f = lib.bm_normalize_rows
    taken = ctypes.c_int(7)
    t = ctypes.byref(taken)
    for base in (MEAN, RANK):
        for src, dst, tk in ((None, p, t), (p, None, t), (p, p, None)):
            assert f(src, F32, 2, 8, 8, base, 1, 0.0, 0.1, dst, F32, 8, tk, None) == E
            assert b"null pointer" in lib.bm_last_error()
        assert f(p, 99, 2, 8, 8, base, 1, 0.0, 0.1, p, F64, 8, t, None) == E
        assert b"bad dtype" in lib.bm_last_error()
        # the output dtype is the input's statistics dtype, nothing else
        for din, dout in ((F32, F64), (F32, F16), (F16, F32), (F64, F32), (U8, F32), (U8, U8), (I32, F32),
                          (I64, I64), (F32, 99)):
            assert f(p, din, 2, 8, 8, base, 1, 0.0, 0.1, p, dout, 8, t, None) == E, (din, dout)
            assert b"out_dtype" in lib.bm_last_error()
        for O, R in ((-1, 8), (2, -1)):
            assert f(p, F32, O, R, 8, base, 0, 0.0, 0.1, p, F32, 8, t, None) == E
            assert b"negative extent" in lib.bm_last_error()
        assert f(p, F32, 2, 8, 7, base, 1, 0.0, 0.1, p, F32, 8, t, None) == E   # src_pitch < R
        assert b"pitch" in lib.bm_last_error()
        assert f(p, F32, 2, 8, 8, base, 1, 0.0, 0.1, p, F32, 7, t, None) == E   # dst_pitch < R
        assert b"pitch" in lib.bm_last_error()
        for offset in (float("nan"), float("inf"), -float("inf")):
            assert f(p, F32, 2, 8, 8, base, 1, 0.0, offset, p, F32, 8, t, None) == E
            assert b"offset" in lib.bm_last_error()
    for base in (-1, 2):
        assert f(p, F32, 2, 8, 8, base, 1, 0.0, 0.1, p, F32, 8, t, None) == E
        assert b"baseline" in lib.bm_last_error()
    # a rank that is not below R; with frac != 0 the next rank counts too
    for rank, frac in ((8, 0.0), (-1, 0.0), (7, 0.5)):
        assert f(p, F32, 2, 8, 8, RANK, rank, frac, 0.1, p, F32, 8, t, None) == E, (rank, frac)
        assert b"rank" in lib.bm_last_error()
    for frac in (-0.5, 1.0, float("nan")):
        assert f(p, F32, 2, 8, 8, RANK, 1, frac, 0.1, p, F32, 8, t, None) == E
        assert b"frac" in lib.bm_last_error()
    assert taken.value == 7  # a refused call leaves it alone


def test_noop_and_not_taken(lib, p):
    f = lib.bm_normalize_rows
    taken = ctypes.c_int(7)
    t = ctypes.byref(taken)
    for base in (MEAN, RANK):
        # nothing to write: a no-op, not an error
        taken.value = 7
        assert f(p, F32, 0, 8, 8, base, 1, 0.5, 0.1, p, F32, 8, t, None) == 0 and taken.value == 1
        taken.value = 7
        assert f(p, U8, 0, 8, 8, base, 0, 0.0, 0.1, p, F64, 8, t, None) == 0 and taken.value == 1
        taken.value = 7
        assert f(p, F32, 2, 0, 0, base, 0, 0.0, 0.1, p, F32, 0, t, None) == 0 and taken.value == 1
        # rows the kernels do not hold: *taken = 0, nothing launched
        taken.value = 7
        assert f(p, F32, 2, 50000, 50000, base, 9999, 0.5, 0.1, p, F32, 50000, t, None) == 0 and taken.value == 0
        taken.value = 7
        assert f(p, F32, 255, 2052, 2052, base, 410, 0.2, 0.1, p, F32, 2052, t, None) == 0 and taken.value == 0
    # the mean baseline ignores rank and frac
    taken.value = 7
    assert f(p, F32, 2, 50000, 50000, MEAN, -5, 7.0, 0.1, p, F32, 50000, t, None) == 0 and taken.value == 0
    # the vector must divide dst_pitch too: R = 2048 at a dst pitch of 2049 runs scalar, 8 elements a thread,
    # and 3 rows of 2048 are then neither a wave's (512) nor enough for a block each
    taken.value = 7
    assert f(p, F32, 3, 2048, 2048, RANK, 409, 0.4, 0.1, p, F32, 2049, t, None) == 0 and taken.value == 0
