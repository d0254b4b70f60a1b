"""Rows that hold a NaN or an infinity, on every moments path, against numpy.

The library's contract for such a row is numpy's: the mean is what a sum over
the row gives (+inf, -inf, or NaN for inf - inf or a NaN), var and std are NaN
-- whatever the layout, the chunking or the rank count, and wherever in the row
the value sits.  nonfinite_cases.py builds "diagonal" arrays that try every
position of the reduced axis in one launch, and states the truth by
classification; test_truth_is_numpys holds that to numpy itself.

Every check on a non-finite row is exact (np.array_equal with equal_nan, the
truth rounded to the result's dtype); the finite rows each array keeps are held
to golden_cases.stat_close, as in test_zz_swap_moments.py, so a remedy that
disturbs finite rows fails here too.  Runs on the CPU test executor and, marked
gpu, on the HIP kernels; the two-rank cases run over gloo on the CPU executor.

Shapes are the smallest that reach each branch of bm_reduce.hip's plan; whether
a shape is chunked is asked of the library (bm_reduce_workspace_bytes), not
restated.  stats()' mean is another arithmetic than mean()'s (the Welford mean
of the variance's state), so on finite rows it is held to stat_close and on
non-finite rows to the bytes of mean(); var and std are the methods' bytes
everywhere.

The module's name sorts it after every other one, as test_zz_swap_moments.py
and test_zzz_normalize.py do: the tests before it keep their places in a run.
"""
import ctypes
import os
import socket
import traceback

import numpy as np
import pytest

import bolt_amd as bolt
import bolt_amd.mi355x.array as A
import cpu_backend
import golden_cases as G
import nonfinite_cases as N
from bolt_amd.mi355x import _lib
from nonfinite_cases import NAMES, VARIANTS

VARIANT_IDS = list(VARIANTS)


@pytest.fixture(scope="module", params=["cpu", pytest.param("gpu", marks=pytest.mark.gpu)])
def nctx(request):
    from bolt_amd import MI355XContext
    from bolt_amd.mi355x._ops import register_backend
    from test_stats_moments_kept import KeepingCpuBackend
    if request.param == "gpu":
        import torch
        if not torch.cuda.is_available():
            pytest.skip("no GPU")
        yield MI355XContext(device="cuda:0")
        return
    # the CPU executor with bm_reduce_keep's contract: the plain one where nothing is kept
    register_backend("cpu", KeepingCpuBackend())
    yield MI355XContext(device="cpu")
    cpu_backend.install()  # the plain executor again, for the modules that follow


@pytest.fixture(scope="module")
def gctx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return bolt.MI355XContext(device="cuda:0")


def _on_gpu(ctx):
    return str(ctx.device).startswith("cuda")


def _flat(v):
    return np.asarray(v).reshape(-1)


def _exact(got, want):
    return np.array_equal(got, want, equal_nan=True)


def _moments(b, axis):
    """mean / var / std by their methods, by stats() of all three and by stats() of each name alone."""
    methods = {n: getattr(b, n)(axis=axis) for n in NAMES}
    st = b.stats(axis=axis, names=NAMES)
    singles = {n: getattr(b.stats(axis=axis, names=(n,)), n) for n in NAMES}
    return methods, {n: getattr(st, n) for n in NAMES}, singles


def _check_truth(vals, t, tag):
    """{name: result} against the Truth ``t``: exact on its non-finite outputs, stat_close on the others."""
    for n in NAMES:
        g = _flat(vals[n])
        assert g.shape == t.bad.shape, (tag, n, g.shape)
        with np.errstate(over="ignore"):
            want = getattr(t, n).astype(g.dtype)
        assert _exact(g[t.bad], want[t.bad]), (tag, n, "non-finite rows", np.flatnonzero(
            ~((g == want) | (np.isnan(g) & np.isnan(want))) & t.bad)[:8].tolist())
        fine = t.fine[n]
        assert G.stat_close(g[~t.bad], fine.astype(g.dtype), fine, g.dtype, t.xfine, n), (tag, n, "finite rows")


def _check(b, x, axis, tag):
    t = N.Truth(x, axis)
    methods, fused, singles = _moments(b, axis)
    _check_truth(methods, t, tag + ("methods",))
    _check_truth(fused, t, tag + ("stats",))
    for n in NAMES:
        m, f, s = _flat(methods[n]), _flat(fused[n]), _flat(singles[n])
        assert m.dtype == f.dtype == s.dtype, (tag, n)
        assert _exact(s, m), (tag, n, "stats of one name is the method")
        if n == "mean":
            assert _exact(f[t.bad], m[t.bad]), (tag, n, "stats against the method, non-finite rows")
        else:
            assert _exact(f, m), (tag, n, "stats against the method")
    return t


def _assert_plan(ctx, dtype, O, R, I, chunked, tag):
    """What the library's plan says of [O][R][I] (HIP only): chunked plans need a workspace."""
    if not _on_gpu(ctx) or chunked is None:
        return
    from bolt_amd.mi355x._ops import backend_for, dtype_code
    import torch
    lib = backend_for(torch.device("cuda:0")).lib
    n = ctypes.c_size_t(0)
    for stat in (_lib.STAT_MEAN, _lib.STAT_VAR):
        assert lib.bm_reduce_workspace_bytes(stat, dtype_code(np.dtype(dtype)), O, R, I, ctypes.byref(n)) == 0
        assert (n.value > 0) == chunked, (tag, "chunked" if chunked else "unchunked", n.value)


# ------------------------------------------------- the truth is numpy's (CPU)
def test_truth_is_numpys():
    """The classification restates numpy: on every array of nonfinite_cases its
    mean / var / std equal numpy's float64 ones -- exactly on the non-finite
    outputs; on the finite ones within 1e-12 relative (numpy's pairwise float64
    sums of at most 20000 values of one sign carry a few eps; the truth is
    longdouble)."""
    seen = 0
    for tag, x, axis in N.every_array():
        t = N.Truth(x, axis)
        ax = None if axis is None else axis
        xf = x.astype(np.float64)
        with np.errstate(all="ignore"):
            ref = {"mean": xf.mean(axis=ax), "var": xf.var(axis=ax), "std": xf.std(axis=ax)}
        assert t.bad.any() or tag.startswith("dense"), tag
        for n in NAMES:
            r = _flat(ref[n])
            got = getattr(t, n)
            assert _exact(got[t.bad], r[t.bad]), (tag, n)
            assert np.allclose(got[~t.bad], r[~t.bad], rtol=1e-12, atol=0.0), (tag, n)
        seen += 1
    assert seen > 100


# ---------------------------------------------------------------- diagonals
# Rows of 2052 and 4104 values are there for the HIP plan alone, which splits
# them into chunks; the CPU executor has no chunks, and its longdouble passes
# over 17 million values take a minute a case: those shapes run on the GPU only.
LONG_ROWS = [c for c in N.ROWS if c[3] > 2000]
DIAGONALS = [c for c in N.DIAGONALS if c not in LONG_ROWS]


def _diagonal(ctx, case, variant):
    x, axis, (O, R, I) = N.layout(case, variant)
    _assert_plan(ctx, case[2], O, R, I, case[4], case[0])
    t = _check(bolt.array(x, ctx), x, axis, (case[0], variant))
    assert int(t.bad.sum()) == case[3]


@pytest.mark.parametrize("variant", VARIANT_IDS)
@pytest.mark.parametrize("case", DIAGONALS, ids=[c[0] for c in DIAGONALS])
def test_diagonal(nctx, case, variant):
    _diagonal(nctx, case, variant)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANT_IDS)
@pytest.mark.parametrize("case", LONG_ROWS, ids=[c[0] for c in LONG_ROWS])
def test_diagonal_chunked_rows(gctx, case, variant):
    _diagonal(gctx, case, variant)


@pytest.mark.parametrize("variant", VARIANT_IDS)
def test_permuted_middle_axis(nctx, variant):
    x, axis = N.permuted(variant)
    t = _check(bolt.array(x, nctx), x, axis, ("permuted", variant))
    assert int(t.bad.sum()) == 50


@pytest.mark.parametrize("variant", VARIANT_IDS)
def test_row_padded_in_place(nctx, variant):
    """Rows of 500 float32 at a pitch of 512, read in place: over the rows,
    over the padded rows' columns, and over every axis."""
    x = N.swapped(500, 20, 25, "float32", variant)
    s = bolt.array(x, nctx).swap((0,), (0, 1))
    assert s.__dict__.get("_pitch") == 512
    xs = np.ascontiguousarray(x.transpose(1, 2, 0))
    for axis in (2, 0, None):
        _check(s, xs, axis, ("padded", axis, variant))
    assert s.toarray().tobytes() == xs.tobytes()


# ------------------------------------------------------- one long row: dense
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_dense_one_output(nctx, dtype):
    _assert_plan(nctx, dtype, 1, N.DENSE_N, 1, True, "dense")
    for p in N.DENSE:
        x = N.dense(N.DENSE_N, dtype, p)
        t = _check(bolt.array(x, nctx), x, None, ("dense", dtype, p))
        assert t.bad.all()
        want = np.nan if p == "pinf_first_ninf_last" else (np.inf if p.startswith("pinf") else -np.inf)
        assert _exact(t.mean, np.array([want]))


def test_dense_few_outputs(nctx):
    _assert_plan(nctx, "float64", 8, N.DENSE_N, 1, True, "dense rows")
    for k, x in enumerate(N.dense_pair()):
        t = _check(bolt.array(x, nctx), x, 1, ("dense rows", k))
        assert int(t.bad.sum()) == (8, 5)[k]


# ------------------------------------------------------- kept moment states
KEPT = [c for c in N.DIAGONALS if c[0] in ("rows-f16-520", "rows-f32-520", "rows-f64-520", "cols-f32-60", "cols-f64-60")]


@pytest.mark.parametrize("order", [("mean", "std", "var"), ("std", "mean")], ids=["mean-std-var", "std-mean"])
@pytest.mark.parametrize("variant", VARIANT_IDS)
@pytest.mark.parametrize("case", KEPT, ids=[c[0] for c in KEPT])
def test_kept_states(nctx, monkeypatch, case, variant, order):
    """mean / var / std with their moment states kept, in both orders: the
    truth, and the bytes of the calls with KEEP_MOMENTS off.  (The state-size
    rule is lifted for the columns, whose 60 values per output are below it.)"""
    x, axis, _ = N.layout(case, variant)
    t = N.Truth(x, axis)
    monkeypatch.setattr(A, "KEEP_MOMENTS", False)
    b = bolt.array(x, nctx)
    plain = {n: _flat(getattr(b, n)(axis=axis)) for n in order}
    assert not b.__dict__.get("_kept")
    monkeypatch.setattr(A, "KEEP_MOMENTS", True)
    monkeypatch.setattr(A, "_KEEP_MIN_BYTES", 0)
    monkeypatch.setattr(A, "_KEEP_COLS", True)
    if case[1] == "cols":
        monkeypatch.setattr(A, "_KEEP_STATE_DIV", 1)
    b = bolt.array(x, nctx)
    kept = {n: _flat(getattr(b, n)(axis=axis)) for n in order}
    assert b.__dict__.get("_kept"), "no state was kept"
    for n in order:
        with np.errstate(over="ignore"):
            want = getattr(t, n).astype(kept[n].dtype)
        assert _exact(kept[n][t.bad], want[t.bad]), (case[0], variant, order, n, "truth")
        assert _exact(kept[n], plain[n]), (case[0], variant, order, n, "KEEP_MOMENTS off")


# -------------------------------------------------- the swap's fused state
# (520, 8, 65) is the diagonal over R = 520 as the swap's rows; (520, 65, 8) the
# same rows through a narrower source (other tiles of bm_copy.hip's plan).
@pytest.mark.parametrize("variant", VARIANT_IDS)
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("ab", [(8, 65), (65, 8)], ids=["8x65", "65x8"])
def test_swap_state(nctx, monkeypatch, ab, dtype, variant):
    x = N.swapped(520, ab[0], ab[1], dtype, variant)
    xs = np.ascontiguousarray(x.transpose(1, 2, 0))
    monkeypatch.setattr(A, "KEEP_MOMENTS", False)
    monkeypatch.setattr(A, "FUSE_SWAP_MOMENTS", False)
    p = bolt.array(x, nctx).swap((0,), (0, 1))
    plain = {n: _flat(getattr(p, n)(axis=2)) for n in NAMES}
    assert not p.__dict__.get("_kept")
    monkeypatch.setattr(A, "FUSE_SWAP_MOMENTS", True)
    monkeypatch.setattr(A, "_FUSE_SWAP_MIN_BYTES", 0)
    s = bolt.array(x, nctx).swap((0,), (0, 1))
    if _on_gpu(nctx):
        e = (s.__dict__.get("_kept") or {}).get((2,))
        assert e is not None and e.serves_mean, "the swap did not fuse"
    t = _check(s, xs, 2, ("swap", ab, dtype, variant))
    assert t.bad.all()
    for n in NAMES:
        assert _exact(_flat(getattr(s, n)(axis=2))[t.bad], plain[n][t.bad]), (ab, dtype, variant, n)
    assert s.toarray().tobytes() == xs.tobytes()


# ------------------------------------------- center / zscore / normalize
# rows of 520: a wave per row; of 2052 float32: past the wave's registers, a
# block per row (the HIP plan's, so on the GPU only, as LONG_ROWS); axis 0 of
# the columns layout: the apply route
STANDARDIZE = [c for c in N.DIAGONALS if c[0] in ("rows-f32-520", "rows-f64-520", "cols-f32-60")]
STANDARDIZE_LONG = [c for c in N.DIAGONALS if c[0] == "rows-f32-2052"]


def _standardize_truth(x, axis, t, what):
    """numpy's float64 formula with the mean of the classification, rounded once."""
    xf = x.astype(np.float64)
    shape = [1 if i == axis else d for i, d in enumerate(x.shape)]
    with np.errstate(all="ignore"):
        m = t.mean.reshape(shape)
        d = xf - m
        if what == "zscore":
            d = d / t.std.reshape(shape)
        elif what == "normalize":
            d = d / (m + 0.1)
        return d.astype(x.dtype)


def _standardize(nctx, case, variant):
    """center is -inf, +inf or NaN per element as x - mean gives, zscore and
    normalize(method='mean') NaN throughout, on every element of the non-finite
    rows; the finite rows keep the bytes they have when no row is marked (the
    same shape, so the same kernels)."""
    x, axis, _ = N.layout(case, variant)
    n = case[3]
    clean = N.base(*((n + 2, n) if case[1] == "rows" else (n + 4, n)), case[2])
    clean = clean if case[1] == "rows" else np.ascontiguousarray(clean.T)
    t = N.Truth(x, axis)
    bad = t.bad if axis == 1 else None
    b, c = bolt.array(x, nctx), bolt.array(clean, nctx)
    calls = {"center": lambda a: a.center(axis=axis), "zscore": lambda a: a.zscore(axis=axis),
             "normalize": lambda a: a.normalize(axis=axis, method="mean", offset=0.1)}
    for what, call in calls.items():
        got = call(b).toarray()
        want = _standardize_truth(x, axis, t, what)
        ref = call(c).toarray()
        assert got.dtype == want.dtype and got.shape == want.shape
        if axis == 1:
            g_bad, w_bad, g_fine, r_fine = got[bad], want[bad], got[~bad], ref[~bad]
        else:
            g_bad, w_bad, g_fine, r_fine = got[:, t.bad], want[:, t.bad], got[:, ~t.bad], ref[:, ~t.bad]
        assert _exact(g_bad, w_bad), (case[0], variant, what)
        if what != "center":
            assert np.isnan(g_bad).all(), (case[0], variant, what)
        assert g_fine.tobytes() == r_fine.tobytes(), (case[0], variant, what, "finite rows")


@pytest.mark.parametrize("variant", VARIANT_IDS)
@pytest.mark.parametrize("case", STANDARDIZE, ids=[c[0] for c in STANDARDIZE])
def test_standardize(nctx, case, variant):
    _standardize(nctx, case, variant)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANT_IDS)
@pytest.mark.parametrize("case", STANDARDIZE_LONG, ids=[c[0] for c in STANDARDIZE_LONG])
def test_standardize_block_per_row(gctx, case, variant):
    _standardize(gctx, case, variant)


# ------------------------------------------------------ two ranks over gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _two_rank_array():
    """(64, 33) float64, sharded over axis 0 (32 rows a rank); columns 0-7 hold
    infinities in rank 0's slab, in rank 1's, in both, and of both signs."""
    x = N.base(64, 33, "float64", seed=3).copy()
    x[5, 0] = np.inf                      # rank 0's slab
    x[40, 1] = np.inf                     # rank 1's
    x[5, 2] = x[40, 2] = np.inf           # both
    x[5, 3], x[40, 3] = np.inf, -np.inf   # +inf on rank 0, -inf on rank 1: NaN
    x[0, 4] = np.inf                      # each slab's first row
    x[32, 5] = np.inf
    x[63, 6] = -np.inf
    x[31, 7] = np.nan
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("nparts", [2, 4, 16], ids=["2-ranks", "4-ranks", "16-ranks"])
def test_rank_merge_kernels(gctx, nparts):
    """The ranks' merge on the HIP kernels, as array._reduced runs it over a
    sharded axis: bm_reduce_state of every slab of the two-rank array, then
    bm_reduce_combine / bm_reduce_combine_moments with the slabs' counts (a
    thread per output for a few parts, a block per output from eight on)."""
    import torch
    from bolt_amd.mi355x import functional as F
    from bolt_amd.mi355x._ops import dtype_code
    x = _two_rank_array()
    t = N.Truth(x, 0)
    dev = torch.device("cuda:0")
    be = bolt.array(x, gctx)._backend
    code = dtype_code(x.dtype)
    rows, nout = x.shape[0] // nparts, x.shape[1]
    xd = torch.from_numpy(x).to(dev)
    got = {}
    for name, stat in zip(NAMES, (_lib.STAT_MEAN, _lib.STAT_VAR, _lib.STAT_STD)):
        sb = be.state_bytes(stat, code, nout)
        states = torch.empty(nparts * sb, dtype=torch.uint8, device=dev)
        for p in range(nparts):
            be.reduce_state(stat, F.as_bytes(xd[p * rows:(p + 1) * rows].contiguous()), code, 1, rows, nout,
                            states[p * sb:(p + 1) * sb])
        out = torch.empty(nout * 8, dtype=torch.uint8, device=dev)
        be.reduce_combine(stat, code, states, [rows] * nparts, nout, out, code)
        got[name] = out.cpu().numpy().view(np.float64)
        if stat == _lib.STAT_VAR:
            outs = [torch.empty(nout * 8, dtype=torch.uint8, device=dev) for _ in NAMES]
            be.reduce_combine_moments(code, states, [rows] * nparts, nout, tuple(outs), code)
            fused = {n: o.cpu().numpy().view(np.float64) for n, o in zip(NAMES, outs)}
    _check_truth(got, t, ("rank merge", nparts, "methods"))
    _check_truth(fused, t, ("rank merge", nparts, "moments"))
    for n in NAMES:
        assert _exact(fused[n][t.bad], got[n][t.bad]), (nparts, n)


def _gloo_body(rank, world):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [here, os.path.dirname(here)]
    from bolt_amd import MI355XContext
    import cpu_backend as C
    C.install()
    ctx = MI355XContext(device="cpu")
    assert ctx.world_size == world and ctx.rank == rank
    x = _two_rank_array()
    b = bolt.array(x, ctx)
    t = _check(b, x, 0, ("gloo", rank))
    assert int(t.bad.sum()) == 8
    assert _exact(t.mean[:8], np.array([np.inf, np.inf, np.inf, np.nan, np.inf, np.inf, -np.inf, np.nan]))


def _gloo_worker(rank, world, port, errq):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    try:
        dist.init_process_group("gloo", rank=rank, world_size=world)
        _gloo_body(rank, world)
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        errq.put((rank, traceback.format_exc()))
        raise


def test_two_ranks_gloo():
    import torch.multiprocessing as mp
    world = 2
    ctx = mp.get_context("spawn")
    errq = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gloo_worker, args=(r, world, port, errq)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=240)
    errs = []
    while not errq.empty():
        errs.append(errq.get())
    for p in procs:
        if p.is_alive():
            p.kill()
    assert not errs, "\n".join("rank %d:\n%s" % e for e in errs)
    assert all(p.exitcode == 0 for p in procs)
