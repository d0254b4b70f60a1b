"""Rows that hold a NaN or an infinity, for test_zzzz_nonfinite_moments.py and
test_zzzzzz_nonfinite_comoment.py: the arrays, and the truth of their mean /
var / std, cov / corr and detrend.

The contract is numpy's: the mean of such a row is what a sum over it gives
(+inf, -inf, or NaN for inf - inf or a NaN), its var and std are NaN.  The
truth is stated here by classification -- which non-finite values the row
holds -- so that it does not depend on any order of summation;
test_truth_is_numpys holds the classification to numpy's own float64 mean /
var / std on every array of this module, which makes numpy the reference.

"Diagonal" arrays mark row i of a finite base at column i, so one launch tries
every position of the reduced axis -- pivot, main loop, tail, chunk starts,
last element -- without the test knowing the kernel's plan.  Where one long
row is reduced a diagonal is impossible; the dense patterns stand in.  Where
an array has fewer rows than positions, marked_columns lists the positions
that matter: both ends, the middle, and both sides of every chunk boundary.

cov(), corr() and detrend() of such a record are NaN -- detrend() on every
element of it -- as numpy's own float64 formulas give (x - mean(x) holds
inf - inf, or the NaN); Truth.bad is that classification, and
test_zzzzzz_nonfinite_comoment.py's test_truth_is_numpys holds it to numpy.
The records beside them are held to the methods' own truths and bounds
(comoment_cases, detrend_cases), computed on Truth.xfine.
"""
import functools

import numpy as np

NAMES = ("mean", "var", "std")
INF = np.inf

# what marks row i of a diagonal: (value, column offset as a function of (i, n))
VARIANTS = {
    "pinf": ((INF, lambda i, n: i),),
    "ninf": ((-INF, lambda i, n: i),),
    "nan": ((np.nan, lambda i, n: i),),
    "pinf_pinf": ((INF, lambda i, n: i), (INF, lambda i, n: (i + 257) % n)),     # truth +inf
    "pinf_ninf": ((INF, lambda i, n: i), (-INF, lambda i, n: (i + n // 2) % n)),  # truth NaN
}


@functools.lru_cache(maxsize=2)
def _base(nrows, n, dtype, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((nrows, n))
    x *= 3.0
    x += 10.0
    x = x.astype(dtype)
    x.setflags(write=False)
    return x


def base(nrows, n, dtype, seed=0):
    """(nrows, n) of 10 + 3 N(0, 1) in ``dtype``, read-only and shared."""
    return _base(int(nrows), int(n), np.dtype(dtype).name, int(seed))


CHUNK = 2048  # bm_comoment.hip's kRowsChunk: the elements of a row one wave sums


def marked_columns(n, chunk=CHUNK):
    """The positions of a record of ``n`` values a shape with few rows marks:
    0, 1, the last, the middle, and both sides of every multiple of ``chunk``
    below n."""
    cols = {0, 1, n - 1, n // 2}
    for m in range(chunk, n, chunk):
        cols |= {m - 1, m}
    return sorted(c for c in cols if 0 <= c < n)


def diagonal(n, dtype, variant, nrows=None, seed=0, cols=None):
    """(nrows, n): row i < n marked at column i by ``variant``, the rows from
    n on (nrows defaults to n + 2) left finite.  ``cols``: row i marked at
    column cols[i] instead, the rows from len(cols) on left finite."""
    nrows = n + 2 if nrows is None else nrows
    x = base(nrows, n, dtype, seed).copy()
    if cols is None:
        c = np.arange(min(n, nrows))
    else:
        c = np.asarray(cols, dtype=np.int64)
        assert len(c) <= nrows and c.min() >= 0 and c.max() < n
    i = np.arange(len(c))
    for value, col in VARIANTS[variant]:
        x[i, col(c, n)] = value
    return x


def finite_twin(x):
    """``x`` with its non-finite values replaced by 10 (the base's centre): what the signals are drawn from."""
    return np.where(np.isfinite(x), x, 10).astype(x.dtype)


def records(x, axis):
    """``x`` as (outputs, n): the kept axes flattened in their order, the
    reduced ones (``axis``: an int, a tuple or None) in ascending order."""
    x = np.asarray(x)
    ax = tuple(range(x.ndim)) if axis is None else tuple(sorted(a % x.ndim for a in np.atleast_1d(axis).tolist()))
    kept = [i for i in range(x.ndim) if i not in ax]
    return x.transpose(kept + list(ax)).reshape(int(np.prod([x.shape[i] for i in kept], dtype=np.int64)), -1)


# one long row: (name, sign-free description); every chunk's first element is
# infinite in "even", "odd" or "all" whatever the chunk length
_DENSE_ONE_SIGN = ("even", "odd", "all", "first", "middle", "last")
DENSE = tuple("%s_%s" % (s, p) for s in ("pinf", "ninf") for p in _DENSE_ONE_SIGN) + ("pinf_first_ninf_last",)


def dense(n, dtype, pattern, seed=0):
    """One row of ``n`` values with the dense ``pattern`` of infinities."""
    x = base(1, n, dtype, seed)[0].copy()
    if pattern == "pinf_first_ninf_last":
        x[0], x[n - 1] = INF, -INF
        return x
    sign, where = pattern.split("_")
    v = INF if sign == "pinf" else -INF
    if where == "even":
        x[0::2] = v
    elif where == "odd":
        x[1::2] = v
    elif where == "all":
        x[:] = v
    else:
        x[{"first": 0, "middle": n // 2, "last": n - 1}[where]] = v
    return x


def dense_rows(n, dtype, patterns, nrows, seed=0):
    """(nrows, n): one dense pattern per row, the rest of the rows finite."""
    x = base(nrows, n, dtype, seed).copy()
    for r, p in enumerate(patterns):
        x[r] = dense(n, dtype, p, seed)
    return x


class Truth(object):
    """mean / var / std of ``x`` over ``axis`` (an int, a tuple or None), the
    outputs flattened in the order of the kept axes.  ``bad``: the outputs
    whose values are not all finite; mean / var / std: float64, exact there
    (the classification); ``fine``: longdouble truths of the other outputs
    (golden_cases.stat_close's), ``xfine`` their values."""

    def __init__(self, x, axis):
        x = np.asarray(x)
        ax = tuple(range(x.ndim)) if axis is None else tuple(sorted(np.atleast_1d(axis).tolist()))
        kept = [i for i in range(x.ndim) if i not in ax]
        rows = records(x, ax)
        nan =np.isnan(rows).any(axis=1)
        pinf = (rows == INF).any(axis=1)
        ninf = (rows == -INF).any(axis=1)
        self.bad = nan | pinf | ninf
        self.xfine = rows[~self.bad]
        v = self.xfine.astype(np.longdouble)
        self.fine = {"mean": v.mean(axis=1), "var": v.var(axis=1), "std": np.sqrt(v.var(axis=1))}
        mean = np.full(rows.shape[0], np.nan)
        mean[~self.bad] = self.fine["mean"].astype(np.float64)
        mean[pinf & ~ninf & ~nan] = INF
        mean[ninf & ~pinf & ~nan] = -INF
        self.mean = mean
        self.var = np.full(rows.shape[0], np.nan)
        self.var[~self.bad] = self.fine["var"].astype(np.float64)
        self.std = np.full(rows.shape[0], np.nan)
        self.std[~self.bad] = self.fine["std"].astype(np.float64)
        self.rows = rows
        self.kept_shape = tuple(x.shape[i] for i in kept)


# --------------------------------------------------------------- the cases --
# Diagonal cases: (id, layout, dtype, n, chunked).  The reduced axis is n long;
# ``chunked`` is what the library's plan must say of it (asserted on the GPU
# with bm_reduce_workspace_bytes, never restated here).
#   rows: (n + 2, n) over the last axis.
#   cols: the transpose, (n, n + 4), over axis 0 -- four finite columns, not
#         two, so that the row length keeps n's divisibility by the 16-B vector.
#   chunked None: rows of 520 run as one chunk from an aligned pointer, but
#         bm_reduce_workspace_bytes also reserves for the scalar plan of an
#         unaligned one, which splits them in two; that these launches are not
#         chunked is shown by the state they keep (test_kept_states: a chunked
#         plan keeps none).
ROWS = [
    ("rows-f16-520", "rows", "float16", 520, None),      # one chunk: main loop and tail
    ("rows-f32-520", "rows", "float32", 520, None),
    ("rows-f64-520", "rows", "float64", 520, None),
    ("rows-f32-131", "rows", "float32", 131, False),     # the scalar plan (vec 1), one chunk
    ("rows-f32-521", "rows", "float32", 521, True),      # the scalar plan, two chunks
    ("rows-f32-2052", "rows", "float32", 2052, True),    # 2 to 4 chunks: k_red_combine
    ("rows-f64-2052", "rows", "float64", 2052, True),
    ("rows-f16-4104", "rows", "float16", 4104, True),
]
COLS = [
    ("cols-f16-60", "cols", "float16", 60, False),
    ("cols-f32-60", "cols", "float32", 60, False),
    ("cols-f64-60", "cols", "float64", 60, False),
    ("cols-f32-300", "cols", "float32", 300, True),
    ("cols-f64-300", "cols", "float64", 300, True),
    ("cols-f32-301", "cols", "float32", 301, True),      # the scalar plan, chunked
]
DIAGONALS = ROWS + COLS
DENSE_N = 20000   # one output from many chunks: k_red_combine_blk


def layout(case, variant):
    """-> (array, axis, (O, R, I) of the launch) of a diagonal case."""
    _, kind, dtype, n, _ = case
    if kind == "rows":
        return diagonal(n, dtype, variant), 1, (n + 2, n, 1)
    x = np.ascontiguousarray(diagonal(n, dtype, variant, nrows=n + 4).T)
    return x, 0, (1, n, n + 4)


def permuted(variant):
    """(6, 50, 10) float32 over the middle axis: the diagonal over the 50 in
    the first 50 of the 60 outputs, the other ten finite."""
    rows = diagonal(50, "float32", variant, nrows=60)
    return np.ascontiguousarray(rows.reshape(6, 10, 50).transpose(0, 2, 1)), 1


MARKED_ROWS = (40, 2052)   # fewer rows than positions: marked_columns


def marked(variant, dtype="float32"):
    """MARKED_ROWS: row i marked at marked_columns(2052)[i], the other rows finite -> (array, axis)."""
    nrows, n = MARKED_ROWS
    return diagonal(n, dtype, variant, nrows=nrows, cols=marked_columns(n)), 1


def swapped(n, a, b, dtype, variant):
    """(n, a, b) with a * b == n whose swap to (a, b, n) has the diagonal over
    n as its rows."""
    assert a * b == n
    rows = diagonal(n, dtype, variant, nrows=n)
    return np.ascontiguousarray(rows.reshape(a, b, n).transpose(2, 0, 1))


def dense_pair(dtype="float64"):
    """The 13 dense patterns as the rows of two (8, DENSE_N) arrays (the
    second also keeps three finite rows)."""
    return (dense_rows(DENSE_N, dtype, DENSE[:8], 8), dense_rows(DENSE_N, dtype, DENSE[8:], 8))


def every_array():
    """(tag, array, axis) of every array this module builds for the tests."""
    for variant in VARIANTS:
        for case in DIAGONALS:
            x, axis, _ = layout(case, variant)
            yield "%s-%s" % (case[0], variant), x, axis
        x, axis = permuted(variant)
        yield "permuted-%s" % variant, x, axis
        for dtype in ("float32", "float64"):
            s = np.ascontiguousarray(swapped(520, 8, 65, dtype, variant).transpose(1, 2, 0))
            yield "swap-%s-%s" % (dtype, variant), s, 2
        s = np.ascontiguousarray(swapped(500, 20, 25, "float32", variant).transpose(1, 2, 0))
        for axis in (2, 0, None):
            yield "padded-%s-%s" % (axis, variant), s, axis
        x, axis = marked(variant)
        yield "marked-%s" % variant, x, axis
    for dtype in ("float32", "float64"):
        for p in DENSE:
            yield "dense-%s-%s" % (dtype, p), dense(DENSE_N, dtype, p), None
    for k, x in enumerate(dense_pair()):
        yield "dense-rows-%d" % k, x, 1
