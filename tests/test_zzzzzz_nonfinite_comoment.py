"""Records that hold a NaN or an infinity, on every path of cov(), corr() and
detrend(), against numpy.

The contract is numpy's: x - mean(x) of such a record holds inf - inf (or the
NaN), so its cov and corr are NaN and its detrend is NaN on every element --
whatever the layout, the chunking or the rank count, and wherever in the record
the value sits; the co-moment state's mean plane is what a sum over the record
gives (+inf, -inf, or NaN for inf - inf or a NaN).  nonfinite_cases.py builds
"diagonal" arrays that try every position of the reduced axis in one launch and
states the truth by classification; test_truth_is_numpys holds that to numpy's
own float64 formulas on every array of that module.

Every check on a non-finite record is exact (NaN, or the mean of the
classification); the finite records each array keeps are held to the methods'
own truths and bounds, computed on those records alone
(comoment_cases.truth_and_bound, detrend_cases.truth_and_bound: no tolerance is
introduced here), so a remedy that disturbs finite records fails here too.  The
signals are comoment_cases.signals of the array with its marks taken out
(nonfinite_cases.finite_twin): finite, the second one correlated with the first
record.

Runs on the CPU test executor as it is (the methods' fallbacks), on
detrend_cases.fused_backend (the orchestration the HIP backend takes) and,
marked gpu, on the HIP kernels; the two-rank cases run over gloo on the fused
executor.  Both CPU executors form x - mean(x) as numpy does and are NaN by
construction: they check the orchestration, the HIP run checks the kernels'
arithmetic.  Shapes are the smallest that reach each branch of bm_comoment.hip's
and bm_detrend.hip's plans; whether a shape is chunked is asked of the library
(bm_comoment_workspace_bytes), whether the rows kernel took a launch of
bm_detrend_rows, never restated.  (Rows of more than 2048 values are there for
the HIP plans -- chunks, a block per row; the CPU executors, which have
neither, run them too, a second or two a case.)

The module's name sorts it after test_zzzzz_detrend*.py, as
test_zzzz_nonfinite_moments.py sorts after its subjects.
"""
import ctypes
import os
import socket
import traceback

import numpy as np
import pytest

import bolt_amd as bolt
import comoment_cases as CM
import cpu_backend
import detrend_cases as D
import nonfinite_cases as N
from comoment_cases import METHODS
from nonfinite_cases import VARIANTS

VARIANT_IDS = list(VARIANTS)


def _make_ctx(param):
    from bolt_amd import MI355XContext
    from bolt_amd.mi355x._ops import register_backend
    if param == "gpu":
        import torch
        if not torch.cuda.is_available():
            pytest.skip("no GPU")
        return MI355XContext(device="cuda:0")
    if param == "cpu-fused":
        register_backend("cpu", D.fused_backend())
    else:
        cpu_backend.install()
    return MI355XContext(device="cpu")


@pytest.fixture(scope="module", params=["cpu", "cpu-fused", pytest.param("gpu", marks=pytest.mark.gpu)])
def bctx(request):
    yield _make_ctx(request.param)
    cpu_backend.install()  # the plain executor again, for the modules that follow


def _on_gpu(ctx):
    return str(ctx.device).startswith("cuda")


def _backend(arr):
    from bolt_amd.mi355x._ops import backend_for
    return backend_for(arr._device)


def _case(cid):
    return [c for c in N.DIAGONALS if c[0] == cid][0]


def _signals(x, axis, k=None):
    return CM.signals(N.finite_twin(x), axis, k=k)


def _assert_chunked(ctx, dtype, O, R, I, chunked, tag):
    """What the library's plan says of [O][R][I] (HIP only): a chunked plan needs a workspace."""
    if not _on_gpu(ctx):
        return
    from bolt_amd.mi355x._ops import backend_for, dtype_code
    import torch
    lib = backend_for(torch.device("cuda:0")).lib
    n = ctypes.c_size_t(0)
    for K in (1, 2, 4):
        assert lib.bm_comoment_workspace_bytes(dtype_code(np.dtype(dtype)), O, R, I, K, ctypes.byref(n)) == 0
        assert (n.value > 0) == chunked, (tag, "chunked" if chunked else "unchunked", K, n.value)


def _check_plane(got, t, y, name, tag):
    """One signal's cov / corr plane against the Truth ``t``: NaN on its
    non-finite records, comoment_cases' truth and bound on the others."""
    g = np.asarray(got).reshape(-1)
    assert g.shape == t.bad.shape, (tag, name, g.shape)
    assert g.dtype == CM.out_dtype(t.rows.dtype), (tag, name, g.dtype)
    wrong = np.flatnonzero(t.bad & ~np.isnan(g))
    assert wrong.size == 0, (tag, name, "non-finite records", wrong.size, wrong[:8].tolist(), g[wrong[:8]].tolist())
    if (~t.bad).any():
        CM.check_values(g[~t.bad], t.xfine, np.asarray(y).reshape(-1), 1, name, "%s finite records" % (tag,))


def _each(names, check):
    """``check(name)`` for every name, then one assertion of all that failed: a
    wrong cov does not hide corr, nor one order or dense pattern the next."""
    failed = []
    for name in names:
        try:
            check(name)
        except AssertionError as e:
            failed.append(e.args[0] if e.args else name)
    assert not failed, failed


def _check_comoment(b, x, axis, tag):
    """cov and corr of ``b`` with the first signal alone and with both at once."""
    t = N.Truth(x, axis)
    ys = _signals(x, axis)

    def check(name):
        f = getattr(b, name)
        one, two = np.asarray(f(ys[0], axis=axis)), np.asarray(f(ys, axis=axis))
        _check_plane(one, t, ys[0], name, tag + ("K=1",))
        _check_plane(two[1], t, ys[1], name, tag + ("K=2",))
        assert two[0].tobytes() == one.tobytes(), (tag, name, "plane 0 of two signals is the one-signal call")
    _each(METHODS, check)
    return t


# ------------------------------------------------- the truth is numpy's (CPU)
def test_truth_is_numpys():
    """The classification restates numpy: on every array of nonfinite_cases,
    numpy's own float64 mean((x - mean(x)) (y - mean(y))) over the records is
    NaN exactly on the classified ones and finite elsewhere, and x - mean(x)
    minus its float64 least-squares line (order 1: slope sum(d t) / sum(t t)
    over the centred positions t) is NaN throughout exactly on those records
    and finite throughout elsewhere."""
    seen = 0
    for tag, x, axis in N.every_array():
        t = N.Truth(x, axis)
        assert t.bad.any() or tag.startswith("dense"), tag
        rows = t.rows.astype(np.float64)
        n = rows.shape[1]
        y = np.random.default_rng(seen).standard_normal(n)
        pos = np.arange(n, dtype=np.float64) - (n - 1) / 2.0
        with np.errstate(all="ignore"):
            d = rows - rows.mean(axis=1, keepdims=True)
            cov = (d * (y - y.mean())).mean(axis=1)
            res = d - ((d * pos).sum(axis=1, keepdims=True) / (pos * pos).sum()) * pos
        assert np.array_equal(np.isnan(cov), t.bad), tag
        assert np.isfinite(cov[~t.bad]).all(), tag
        assert np.array_equal(np.isnan(res).all(axis=1), t.bad), tag
        assert np.isnan(res[t.bad]).all() and np.isfinite(res[~t.bad]).all(), tag
        seen += 1
    assert seen > 100


def test_marked_columns():
    """0, 1, the last, the middle and both sides of every multiple of the chunk below n."""
    assert N.marked_columns(2052) == [0, 1, 1026, 2047, 2048, 2051]
    assert N.marked_columns(4104) == [0, 1, 2047, 2048, 2052, 4095, 4096, 4103]
    assert N.marked_columns(2048) == [0, 1, 1024, 2047]
    x, axis = N.marked("pinf")
    assert x.shape == N.MARKED_ROWS and axis == 1
    assert np.argwhere(np.isinf(x)).tolist() == [[i, c] for i, c in enumerate(N.marked_columns(2052))]
    assert N.diagonal(7, "float32", "nan").tobytes() == N.diagonal(7, "float32", "nan", cols=range(7)).tobytes()


# ------------------------------------------------------- cov / corr: diagonals
# (id, chunked): what bm_comoment_workspace_bytes must say of the case.
#   rows (n + 2, n) over the last axis: float32 520 -- vec 4, one main step and
#   a rest; 131 -- vec 1; float64 520 -- vec 2; float16 520 -- vec 8; 2052 -- two
#   chunks, workspace and k_co_merge; float16 4104 -- three chunks.
#   columns (n, n + 4) over axis 0: 60 -- unchunked, tcv < 64, several row
#   phases; 300 -- tcv 64, R in chunks; 301 -- the scalar plan, chunked.
CO_ROWS = [("rows-f32-520", False), ("rows-f32-131", False), ("rows-f64-520", False), ("rows-f16-520", False),
           ("rows-f32-2052", True), ("rows-f64-2052", True), ("rows-f16-4104", True)]
CO_COLS = [("cols-f16-60", False), ("cols-f32-60", False), ("cols-f64-60", False), ("cols-f32-300", True),
           ("cols-f32-301", True)]


def _diagonal(ctx, cid, chunked, variant):
    case = _case(cid)
    x, axis, (O, R, I) = N.layout(case, variant)
    _assert_chunked(ctx, case[2], O, R, I, chunked, cid)
    t = _check_comoment(bolt.array(x, ctx), x, axis, (cid, variant))
    assert int(t.bad.sum()) == case[3]


@pytest.mark.parametrize("variant", VARIANT_IDS)
@pytest.mark.parametrize("cid,chunked", CO_ROWS + CO_COLS, ids=[c[0] for c in CO_ROWS + CO_COLS])
def test_comoment_diagonal(bctx, cid, chunked, variant):
    _diagonal(bctx, cid, chunked, variant)


@pytest.mark.parametrize("variant", VARIANT_IDS)
def test_comoment_permuted_middle_axis(bctx, variant):
    """(6, 50, 10) over the middle axis: the columns kernel with O > 1."""
    x, axis = N.permuted(variant)
    t = _check_comoment(bolt.array(x, bctx), x, axis, ("permuted", variant))
    assert int(t.bad.sum()) == 50


@pytest.mark.parametrize("k", [3, 6])
def test_comoment_several_signals(bctx, k):
    """K = 3 (the four-signal kernels with a plane of zeros) and K = 6 (two
    batches): every plane still has the bytes of its one-signal call, NaNs
    included (the kernels' NaNs are those of the same operations whatever K is:
    no payload needs canonicalising)."""
    for cid in ("rows-f32-520", "cols-f32-300"):
        x, axis, _ = N.layout(_case(cid), "pinf")
        t = N.Truth(x, axis)
        b = bolt.array(x, bctx)
        ys = _signals(x, axis, k=k)
        def check(name):
            f = getattr(b, name)
            got = np.asarray(f(ys, axis=axis))
            assert got.shape == (k,) + t.bad.shape
            for j in range(k):
                one = np.asarray(f(ys[j], axis=axis))
                assert got[j].tobytes() == one.tobytes(), (cid, name, k, j)
                _check_plane(got[j], t, ys[j], name, (cid, "K=%d plane %d" % (k, j)))
        _each(METHODS, check)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_comoment_dense_one_output(bctx, dtype):
    """Every axis of one long row: one output from ten chunks."""
    _assert_chunked(bctx, dtype, 1, N.DENSE_N, 1, True, "dense")

    def check(p):
        x = N.dense(N.DENSE_N, dtype, p)
        b = bolt.array(x, bctx)
        ys = _signals(x, None)
        got = {name: [np.asarray(getattr(b, name)(y, axis=None)) for y in (ys[0], ys)] for name in METHODS}
        for name in METHODS:
            for g in got[name]:
                assert g.dtype == np.dtype(dtype) and np.isnan(g).all(), (dtype, p, name, g.tolist())
    _each(N.DENSE, check)


# ------------------------------------------------------------ the state itself
STATE_CASES = ["rows-f32-520", "rows-f32-2052", "cols-f32-300"]


def _state(b, axis, ys):
    """reduction.comoment_state of ``b`` over ``axis`` as array._comoment_batch calls it -> (2 + K, outputs) float64."""
    from bolt_amd.mi355x import reduction
    from bolt_amd.mi355x.dist import _empty
    plan, _, _ = reduction.plan_for(b, (axis,), reduction.COMOMENT)
    src = reduction.source(b, plan, moments=False)
    assert src.drop is None
    K = ys.shape[0]
    yk = ys.reshape(K, -1)
    ymean, yresid, _ = reduction.signal_centre(yk)
    state = _empty((2 + K) * src.nlaunch * 8, src.buf.device)
    with np.errstate(all="ignore"):
        reduction.comoment_state(_backend(b), src, b.dtype, plan.code, yk, ymean, yresid, state)
    return state.cpu().numpy().view(np.float64).reshape(2 + K, src.nlaunch).copy()


def _check_state(st, t, ys, tag):
    """The (mean, M2, C_k) planes ``st``: on the non-finite records the mean of
    the classification exactly and NaN M2 and C_k; on the others
    test_stat_comoment.py::test_state_and_workspace_guards' check."""
    bad = t.bad
    assert np.array_equal(st[0][bad], t.mean[bad], equal_nan=True), (tag, "mean plane", np.flatnonzero(
        bad & ~((st[0] == t.mean) | (np.isnan(st[0]) & np.isnan(t.mean))))[:8].tolist())
    assert np.isnan(st[1][bad]).all(), (tag, "M2 plane")
    for k in range(len(ys)):
        wrong = np.flatnonzero(bad & ~np.isnan(st[2 + k]))
        assert wrong.size == 0, (tag, "co-moment plane", k, wrong.size, wrong[:8].tolist())
    xd = t.xfine.astype(np.float64)
    d = xd - xd.mean(axis=1, keepdims=True)
    np.testing.assert_allclose(st[0][~bad], xd.mean(axis=1), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(st[1][~bad], (d * d).sum(axis=1), rtol=1e-11)
    for k, y in enumerate(ys):
        y = y.reshape(-1)
        want = (d * (y - y.mean())).sum(axis=1)
        np.testing.assert_allclose(st[2 + k][~bad], want, rtol=1e-9, atol=1e-9 * np.abs(d).max() * d.shape[1] ** 0.5)


@pytest.mark.parametrize("variant", VARIANT_IDS)
@pytest.mark.parametrize("cid", STATE_CASES)
def test_state_planes(bctx, cid, variant):
    x, axis, _ = N.layout(_case(cid), variant)
    t = N.Truth(x, axis)
    ys = _signals(x, axis)
    _check_state(_state(bolt.array(x, bctx), axis, ys), t, ys, (cid, variant))


# --------------------------------------------------------------------- detrend
def _check_detrend(got, x, axis, order, t, tag):
    """NaN on every element of the non-finite records, detrend_cases' truth and bound on the others."""
    assert got.dtype == D.out_dtype(x.dtype) and got.shape == x.shape, (tag, got.dtype, got.shape)
    g = N.records(got, axis)
    wrong = np.flatnonzero(~np.isnan(g[t.bad]).all(axis=1))
    assert wrong.size == 0, (tag, order, "non-finite records with an output that is not NaN", wrong.size,
                             np.flatnonzero(t.bad)[wrong[:8]].tolist())
    truth, bound = D.truth_and_bound(t.xfine, 1, order)
    err = np.abs(g[~t.bad].astype(np.longdouble) - truth)
    assert np.all(err <= bound), (tag, order, "finite records", float((err / bound).max()))


def _detrend(ctx, monkeypatch, x, axis, orders, taken_want, tag):
    """detrend at ``orders``; ``taken_want``: what every bm_detrend_rows launch
    must answer (None: it must not be asked)."""
    t = N.Truth(x, axis)
    b = bolt.array(x, ctx)
    be = _backend(b)
    taken = []
    if hasattr(be, "detrend_rows"):
        def rows(*a, _f=be.detrend_rows):
            taken.append(_f(*a))
            return taken[-1]
        monkeypatch.setattr(be, "detrend_rows", rows, raising=False)
    _each(orders, lambda order: _check_detrend(b.detrend(axis=axis, order=order).toarray(), x, axis, order, t, tag))
    if hasattr(be, "detrend_rows"):
        assert taken == ([] if taken_want is None else [taken_want] * len(orders)), (tag, taken)
    return t


ORDERS = (1, 2, 5)   # 5: two batches of co-moment signals on the state + apply routes
# a wave per row; rows of 2052 float32: past a wave's registers, and 2054 of
# them, at least the 256 the plan asks for: a block per row
DETREND_ROWS = ["rows-f32-520", "rows-f64-520", "rows-f16-520", "rows-f32-131", "rows-f32-2052"]
DETREND_COLS = ["cols-f32-60", "cols-f32-300", "cols-f32-301", "cols-f64-60"]


@pytest.mark.parametrize("variant", VARIANT_IDS)
@pytest.mark.parametrize("cid", DETREND_ROWS)
def test_detrend_rows_kernel(bctx, monkeypatch, cid, variant):
    x, axis, _ = N.layout(_case(cid), variant)
    orders = ORDERS + ((8,) if cid == "rows-f32-520" else ())
    _detrend(bctx, monkeypatch, x, axis, orders, True, (cid, variant))


@pytest.mark.parametrize("variant", VARIANT_IDS)
def test_detrend_rows_not_taken(bctx, monkeypatch, variant):
    """(40, 2052) float32: too long for a wave, too few rows for a block each:
    bm_detrend_rows declines, the chunked co-moment state and the apply run."""
    x, axis = N.marked(variant)
    _assert_chunked(bctx, "float32", x.shape[0], x.shape[1], 1, True, "marked")
    t = _detrend(bctx, monkeypatch, x, axis, ORDERS, False, ("marked", variant))
    assert int(t.bad.sum()) == len(N.marked_columns(x.shape[1]))


@pytest.mark.parametrize("variant", VARIANT_IDS)
@pytest.mark.parametrize("cid", DETREND_COLS)
def test_detrend_columns(bctx, monkeypatch, cid, variant):
    x, axis, _ = N.layout(_case(cid), variant)
    orders = ORDERS + ((8,) if cid == "cols-f32-60" else ())
    _detrend(bctx, monkeypatch, x, axis, orders, None, (cid, variant))


@pytest.mark.parametrize("variant", VARIANT_IDS)
def test_detrend_permuted_middle_axis(bctx, monkeypatch, variant):
    x, axis = N.permuted(variant)
    t = _detrend(bctx, monkeypatch, x, axis, ORDERS, None, ("permuted", variant))
    assert int(t.bad.sum()) == 50


# ----------------------------------------------------------------- rank merges
# the reduced axis cut into slabs of unequal length: a marked record's infinity
# lies in the first, a middle or the last slab depending on its row
SLABS = {"rows-f32-2052": ((0, 1030, 2052), (0, 600, 1500, 2052)), "cols-f32-300": ((0, 100, 300), (0, 70, 180, 300))}


@pytest.mark.parametrize("variant", VARIANT_IDS)
@pytest.mark.parametrize("nparts", [2, 3])
@pytest.mark.parametrize("cid", sorted(SLABS))
def test_slab_merge(bctx, cid, nparts, variant):
    """The ranks' merge as array._comoment_batch runs it over a sharded axis:
    reduction.comoment_state of every slab with its slice of the signals, then
    reduction.comoment_combine with the slabs' counts, as cov and as corr."""
    import torch
    from bolt_amd.mi355x import _lib, functional as F, reduction
    from bolt_amd.mi355x._ops import backend_for, dtype_code
    from bolt_amd.mi355x.dist import _empty
    case = _case(cid)
    x, axis, (O, R, I) = N.layout(case, variant)
    t = N.Truth(x, axis)
    ys = _signals(x, axis)
    K, nout = len(ys), O * I
    dev = bolt.array(np.zeros(2, dtype=np.float32), bctx)._device
    be = backend_for(dev)
    code = dtype_code(x.dtype)
    cuts = SLABS[cid][nparts - 2]
    bounds = list(zip(cuts[:-1], cuts[1:]))
    parts = [reduction.signal_centre(np.ascontiguousarray(ys[:, lo:hi])) for lo, hi in bounds]
    states = []
    for (lo, hi), part in zip(bounds, parts):
        slab = np.ascontiguousarray(x[:, lo:hi] if axis == 1 else x[lo:hi])
        buf = F.as_bytes(torch.from_numpy(slab).to(dev))
        state = _empty((2 + K) * nout * 8, dev)
        with np.errstate(all="ignore"):
            reduction.comoment_state(be, (buf, O, hi - lo, I, hi - lo), x.dtype, code,
                                     np.ascontiguousarray(ys[:, lo:hi]), part[0], part[1], state)
        states.append(state)
    states = torch.cat(states)
    counts = [hi - lo for lo, hi in bounds]
    def check(name):
        out = _empty(K * nout * x.dtype.itemsize, dev)
        with np.errstate(all="ignore"):
            reduction.comoment_combine(be, {"cov": _lib.CO_COV, "corr": _lib.CO_CORR}[name], states, counts,
                                       [p[0] for p in parts], [reduction.signal_m2(p[2], p[1]) for p in parts],
                                       nout, K, out, x.dtype, code)
        got = F.view(out, (K, nout), x.dtype).cpu().numpy()
        for j in range(K):
            _check_plane(got[j], t, ys[j], name, (cid, nparts, variant, "signal %d" % j))
    _each(METHODS, check)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gloo_body(rank, world):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [here, os.path.dirname(here)]
    from bolt_amd import MI355XContext
    from bolt_amd.mi355x._ops import register_backend
    be = D.fused_backend()
    calls = {"comoment_state": 0, "comoment_combine": 0, "detrend_apply": 0}
    for name in calls:
        def counted(*a, _f=getattr(be, name), _n=name, **k):
            calls[_n] += 1
            return _f(*a, **k)
        setattr(be, name, counted)
    register_backend("cpu", be)
    ctx = MI355XContext(device="cpu")
    assert ctx.world_size == world and ctx.rank == rank
    for variant in VARIANTS:
        # (60, 64) sharded over axis 0, 30 rows a rank, and axis 0 reduced: the
        # mark of column i lies in rank 0's slab for i < 30, in rank 1's from 30
        # on; pinf_ninf's two marks of a column lie in different slabs
        x, axis, _ = N.layout(_case("cols-f32-60"), variant)
        b = bolt.array(x, ctx)
        t = _check_comoment(b, x, axis, ("gloo", rank, variant))
        assert int(t.bad.sum()) == 60
        for order in (1, 5):
            _check_detrend(b.detrend(axis=axis, order=order).toarray(), x, axis, order, t, ("gloo", rank, variant))
    assert all(calls.values()), calls


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
    """cov, corr and detrend at orders 1 and 5 with the sharded axis reduced:
    one state per rank, gathered; combine_moments for the mean, the merged
    covariances times n for the coefficients."""
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
