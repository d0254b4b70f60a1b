"""Shared by the center() / zscore() tests: the float128 truth and the
tolerance, the plan of bm_standardize_rows worked out from the kernel code
(bolt_amd/csrc/bm_standardize.hip), and a numpy executor with the two entry
points, so the orchestration the HIP backend takes runs on the CPU.
"""
import numpy as np

import cpu_backend as C

METHODS = ("center", "zscore")


def axes_of(x, axis):
    if axis is None:
        return tuple(range(x.ndim))
    return tuple(axis) if isinstance(axis, (tuple, list)) else (axis,)


def out_dtype(dtype):
    """The dtype of record - 0.0: float16 / float32 stay, everything else float64."""
    dt = np.dtype(dtype)
    return dt if dt in (np.dtype(np.float16), np.dtype(np.float32)) else np.dtype(np.float64)


def truth_and_bound(x, axis, scale):
    """(truth, bound) in longdouble:
    |got - truth| <= 2 eps(out) |truth| + 1e-12 max|x_record| / std_record + smallest_subnormal(out),
    std_record = 1 for center.  1e-12 is the project's float64 parity rtol
    (golden_cases.stat_close) on the float64 intermediate in the statistic's own
    units, 2 eps its allowance for the final rounding, the subnormal term the
    rounding floor of the output format."""
    ax = axes_of(x, axis)
    v = x.astype(np.longdouble)
    c = v - v.mean(axis=ax, keepdims=True)
    sd = np.sqrt(v.var(axis=ax, keepdims=True))
    big = np.abs(v).max(axis=ax, keepdims=True)
    fi = np.finfo(out_dtype(x.dtype))
    with np.errstate(all="ignore"):
        t = c / sd if scale else c
        floor = 1e-12 * big / (sd if scale else 1.0)
    return t, 2 * np.longdouble(fi.eps) * np.abs(t) + floor + np.longdouble(fi.smallest_subnormal)


def check_values(got, x, axis, scale, tag=""):
    """``got`` (ndarray) against the truth; prints the worst error / bound ratio before asserting."""
    t, bound = truth_and_bound(x, axis, scale)
    assert got.dtype == out_dtype(x.dtype), (tag, got.dtype)
    assert got.shape == x.shape, (tag, got.shape)
    assert np.isfinite(t).all(), tag  # no record of zero variance outside the dedicated test
    err = np.abs(got.astype(np.longdouble) - t)
    ratio = float((err / bound).max()) if err.size else 0.0
    print("%s %s: max error / bound = %.3g" % (tag, "zscore" if scale else "center", ratio))
    assert np.all(err <= bound), (tag, ratio)


def check_array(r, b, x, axis, scale, tag=""):
    """The result array ``r`` of ``b.center / zscore(axis)``: type, shape, split, dtype, context, values."""
    assert type(r) is type(b), tag
    assert r.shape == b.shape == x.shape and r.split == b.split, (tag, r.shape, r.split)
    assert r.dtype == out_dtype(x.dtype), (tag, r.dtype)
    assert r.context is b.context and r._npartitions == b._npartitions, tag
    check_values(r.toarray(), x, axis, scale, tag)


def rand(shape, dtype, seed=0, offset=None):
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype)
    if offset is not None:
        return (offset + rng.standard_normal(shape)).astype(dt)
    if dt == np.bool_:
        return rng.integers(0, 2, size=shape).astype(bool)
    if dt.kind in "iu":
        info = np.iinfo(dt)
        lo, hi = max(info.min, -(1 << 40)), min(info.max, 1 << 40)
        return rng.integers(lo, hi, size=shape, dtype=np.int64).astype(dt)
    return (10 + 3 * rng.standard_normal(shape)).astype(dt)


# ---- the plan of bm_standardize_rows (bm_standardize.hip: pick_vec, lane_vecs,
# kBlockMinRows), for buffers aligned to 16 B as every allocation here is
MAX_VEC = 8
BLOCK_MIN_ROWS = 256


def rows_vec(es, R, sp, dp):
    vec = min(16 // es, MAX_VEC)
    while vec > 1 and not (R % vec == 0 and sp % vec == 0 and dp % vec == 0):
        vec >>= 1
    return vec


def rows_plan(es, O, R, sp=None, dp=None):
    """'wave' (one wave per row), 'block' (one block per row) or None (not taken)."""
    vec = rows_vec(es, R, R if sp is None else sp, R if dp is None else dp)
    held = min(8 * vec, 32)  # elements a thread holds
    if R <= 64 * held:
        return "wave"
    if R <= 256 * held and O >= BLOCK_MIN_ROWS:
        return "block"
    return None


def fused_backend():
    """CpuBackend plus bm_standardize_rows / bm_standardize_apply (include/bolt_mi355x.h) in numpy float64."""

    class FusedCpuBackend(C.CpuBackend):
        def _out(self, y, dst, out_code, O, R, pitch):
            odt = np.dtype(C._CODES[out_code])
            d = dst.numpy().view(odt)
            if pitch is None:
                d[...] = y.astype(odt).reshape(-1)
            else:
                d[:O * pitch].reshape(O, pitch)[:, :R] = y.astype(odt)

        def standardize_rows(self, src, code, O, R, src_pitch, dst, out_code, dst_pitch, scale):
            dt = np.dtype(C._CODES[code])
            assert src_pitch >= R and dst_pitch >= R and np.dtype(C._CODES[out_code]) == out_dtype(dt)
            if O == 0 or R == 0:
                return True
            if rows_plan(dt.itemsize, O, R, src_pitch, dst_pitch) is None:
                return False
            x = src.numpy().view(dt)[:O * src_pitch].reshape(O, src_pitch)[:, :R].astype(np.float64)
            with np.errstate(all="ignore"):
                y = x - x.mean(axis=1, keepdims=True)
                if scale:
                    y = y / np.sqrt(np.square(y).mean(axis=1, keepdims=True))
            self._out(y, dst, out_code, O, R, dst_pitch)
            return True

        def standardize_apply(self, src, code, O, R, I, src_pitch, mean, std, dst, out_code, dst_pitch):
            dt = np.dtype(C._CODES[code])
            assert src_pitch >= R and dst_pitch >= R and (I == 1 or src_pitch == dst_pitch == R)
            assert np.dtype(C._CODES[out_code]) == out_dtype(dt)
            if O == 0 or R == 0 or I == 0:
                return
            a = src.numpy().view(dt)
            if I == 1:
                x = a[:O * src_pitch].reshape(O, src_pitch)[:, :R].reshape(O, R, 1)
            else:
                x = a.reshape(O, R, I)
            m = mean.numpy().view(np.float64).reshape(O, 1, I)
            with np.errstate(all="ignore"):
                y = x.astype(np.float64) - m
                if std is not None:
                    y = y / std.numpy().view(np.float64).reshape(O, 1, I)
            self._out(y.reshape(O, R * I), dst, out_code, O, R * I, dst_pitch if I == 1 else None)

    return FusedCpuBackend()
