"""mean / var / std keep the moment state of their one read (array.KEEP_MOMENTS,
bm_reduce_keep): a later var / std over the same axes is finished from the
state without reading the array, and every result keeps its bits.

The C-ABI tests run on the GPU.  The method tests run on the HIP kernels
(marked gpu) and on a test-local subclass of the CPU executor that implements
the ``state=`` keyword with reduce + reduce_state, so the caching logic runs
without a GPU; tests/cpu_backend.py itself has no such capability and pins the
unchanged path.  _KEEP_MIN_BYTES (the 256 MiB Infinity Cache) is lowered to 0
where a small array has to keep its state; the state-size rule (16 B per
output at most 1/64 of the bytes read) stays at its real value, so the kept
layouts reduce at least 256 float32 per output.  Column layouts are narrow
(I <= 16): plan_reduce gives them many row phases and no chunks, so the HIP
kernels keep them too (a chunked plan reports kept = 0, covered below).
"""
import ctypes
import itertools
import os

import numpy as np
import pytest

import bolt_amd as bolt
import bolt_amd.mi355x.array as A
import cpu_backend
from bolt_amd.mi355x import _lib

MEAN, VAR, STD = _lib.STAT_MEAN, _lib.STAT_VAR, _lib.STAT_STD
NAMES = ("mean", "var", "std")
_READS = ("reduce", "reduce_rows", "reduce_state", "permute", "copy_strided")
_COUNTED = _READS + ("reduce_combine",)


class KeepingCpuBackend(cpu_backend.CpuBackend):
    """The CPU executor with bm_reduce_keep's contract: the plain launch, then
    the STAT_VAR state of the same values (dense rows for a padded layout)."""
    keeps_moments = True

    def reduce(self, stat, src, code, O, R, I, out, out_code, state=None):
        cpu_backend.CpuBackend.reduce(self, stat, src, code, O, R, I, out, out_code)
        if state is None:
            return None
        with np.errstate(all="ignore"):
            cpu_backend.CpuBackend.reduce_state(self, VAR, src, code, O, R, I, state)
        return True

    def reduce_rows(self, stat, src, code, O, R, pitch, out, out_code, state=None):
        cpu_backend.CpuBackend.reduce_rows(self, stat, src, code, O, R, pitch, out, out_code)
        if state is None:
            return None
        import torch
        es = np.dtype(cpu_backend._CODES[code]).itemsize
        rows = src.numpy()[:O * pitch * es].reshape(O, pitch * es)[:, :R * es]
        cpu_backend.CpuBackend.reduce_state(self, VAR, torch.from_numpy(np.ascontiguousarray(rows).reshape(-1)),
                                            code, O, R, 1, state)
        return True


@pytest.fixture(scope="module", params=["cpu", pytest.param("gpu", marks=pytest.mark.gpu)])
def kctx(request):
    """A context whose backend keeps moments: the HIP kernels, or the keeping CPU executor."""
    from bolt_amd import MI355XContext
    from bolt_amd.mi355x._ops import register_backend
    if request.param == "gpu":
        import torch
        if not torch.cuda.is_available():
            pytest.skip("no GPU")
        yield MI355XContext(device="cuda:0")
        return
    register_backend("cpu", KeepingCpuBackend())
    yield MI355XContext(device="cpu")
    cpu_backend.install()  # the other modules' executor


@pytest.fixture
def keep_small(monkeypatch):
    """Keep the state of arrays smaller than the Infinity Cache too, and of
    column reductions (off by default for their measured store cost, DESIGN.md
    section 3: the branches stay tested; test_columns_keep_nothing_by_default
    pins the default)."""
    monkeypatch.setattr(A, "KEEP_MOMENTS", True)
    monkeypatch.setattr(A, "_KEEP_MIN_BYTES", 0)
    monkeypatch.setattr(A, "_KEEP_COLS", True)


def _small_pitch(mp):
    """test_row_pitch.small_pitch: pad every transposed row that is no multiple of 16 B, to 64 B."""
    mp.setattr(A, "_PITCH_MIN_ROW", 1)
    mp.setattr(A, "_PITCH_LINE", 16)
    mp.setattr(A, "_PITCH_ALIGN", 64)
    mp.setattr(A, "_PITCH_PAD_DIV", 0)
    mp.setattr(A, "_PITCH_PLANS", {})


def _counting(mp, be):
    """test_stats_fused._counting, also recording each call's name and whether it carried ``state=``."""
    calls = dict.fromkeys(_COUNTED, 0)
    log = []

    def proxy(name, fn):
        def call(*a, **k):
            calls[name] += 1
            log.append((name, k.get("state") is not None))
            return fn(*a, **k)
        return call
    for name in _COUNTED:
        if hasattr(be, name):
            mp.setattr(be, name, proxy(name, getattr(be, name)), raising=False)
    return calls, log


def _reads(calls):
    return sum(calls[n] for n in _READS)


def _x(shape, dtype="float32", seed=0):
    rng = np.random.default_rng(seed)
    if np.dtype(dtype).kind in "iu":
        return rng.integers(0, 1000, size=shape).astype(dtype)
    return (10 + 3 * rng.standard_normal(shape)).astype(dtype)


# layout -> (array, axis): every one reduces >= 256 float32 per output (the
# state-size rule) in an unchunked plan
LAYOUTS = ("padded_rows", "padded_cols", "permuted", "dense_rows", "dense_cols")


def _layout(ctx, layout, mp, dtype="float32", seed=1):
    if layout == "padded_rows":   # a swap result: rows of 500 (2000 B) at a pitch of 512, read in place
        s = bolt.array(_x((500, 3, 4), dtype, seed), ctx).swap((0,), (0, 1))
        assert s.__dict__.get("_pitch") == 512
        return s, 2
    if layout == "padded_cols":   # rows of 5 at a pitch of 16: columns over the padded rows, pad outputs dropped
        _small_pitch(mp)
        s = bolt.array(_x((5, 300, 1), dtype, seed), ctx).swap((0,), (0, 1))
        assert s.__dict__.get("_pitch") == 16 and s.shape == (300, 1, 5)
        return s, 0
    if layout == "permuted":      # reduced axes not one block: permuted to the front, then 300 x 5 columns
        return bolt.array(_x((10, 5, 30), dtype, seed), ctx), (0, 2)
    if layout == "dense_rows":
        return bolt.array(_x((9, 512), dtype, seed), ctx), 1
    return bolt.array(_x((300, 8), dtype, seed), ctx), 0


def _bits(a):
    a = np.asarray(a)
    return (a.dtype, a.shape, a.tobytes())


# ------------------------------------------------------- 2. methods, every order
@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_order_same_bits(kctx, keep_small, monkeypatch, layout):
    """The six orders of (mean, var, std), each on a fresh array: the results
    with KEEP_MOMENTS on are those with it off, byte for byte."""
    for order in itertools.permutations(NAMES):
        got = {}
        for on in (False, True):
            with monkeypatch.context() as mp:
                mp.setattr(A, "KEEP_MOMENTS", on)
                arr, axis = _layout(kctx, layout, mp)
                got[on] = [_bits(getattr(arr, name)(axis=axis)) for name in order]
                got[on].append(_bits(getattr(arr, order[0])(axis=axis, keepdims=True)))
                assert bool(arr.__dict__.get("_kept")) == on, (layout, order, on)
        assert got[True] == got[False], (layout, order)


# ---------------------------------------------------------- 3. no second read
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("first", NAMES)
def test_no_second_read(kctx, keep_small, monkeypatch, layout, first):
    """After the first of mean / var / std a following var and std read
    nothing: zero reduce / reduce_rows / reduce_state / permute / copy_strided
    calls and one reduce_combine each."""
    from bolt_amd.mi355x._ops import backend_for
    arr, axis = _layout(kctx, layout, monkeypatch)
    calls, log = _counting(monkeypatch, backend_for(arr._device))

    def launch():
        return [e for e in log if e[0] in ("reduce", "reduce_rows")][-1]
    getattr(arr, first)(axis=axis)
    assert calls["reduce"] + calls["reduce_rows"] == 1 and calls["reduce_combine"] == 0
    assert launch()[1], "the first call's launch carries state="
    assert arr.__dict__.get("_kept"), layout
    for name in ("var", "std"):
        for k in calls:
            calls[k] = 0
        getattr(arr, name)(axis=axis)
        assert _reads(calls) == 0 and calls["reduce_combine"] == 1, (layout, first, name, calls)
    # a mean after the state is kept is the plain launch again: its bits are not the state's mean
    for k in calls:
        calls[k] = 0
    arr.mean(axis=axis)
    assert calls["reduce"] + calls["reduce_rows"] == 1 and calls["reduce_combine"] == 0
    assert calls["reduce_state"] == 0 and not launch()[1]


def test_mean_after_std_reads_once(kctx, keep_small, monkeypatch):
    from bolt_amd.mi355x._ops import backend_for
    arr, axis = _layout(kctx, "padded_rows", monkeypatch)
    arr.std(axis=axis)
    calls, _ = _counting(monkeypatch, backend_for(arr._device))
    arr.mean(axis=axis)
    assert calls["reduce"] + calls["reduce_rows"] == 1 and _reads(calls) == 1 and calls["reduce_combine"] == 0


def test_other_axes_and_arrays_start_empty(kctx, keep_small, monkeypatch):
    """The state belongs to (array, axes): other axes and derived arrays read."""
    from bolt_amd.mi355x._ops import backend_for
    arr, _ = _layout(kctx, "dense_rows", monkeypatch)
    arr.mean(axis=1)
    assert list(arr.__dict__["_kept"]) == [(1,)]
    calls, _ = _counting(monkeypatch, backend_for(arr._device))
    arr.std(axis=0)   # 9 float32 per output: nothing kept either
    assert calls["reduce"] + calls["reduce_rows"] == 1 and list(arr.__dict__["_kept"]) == [(1,)]
    t = arr.swap((0,), (0,))
    assert not t.__dict__.get("_kept")
    r = arr.reshape(9, 512)
    assert r is arr or not r.__dict__.get("_kept")


# ------------------------------------------- 4. nothing kept when it must not be
def _two_reads(arr, axis, monkeypatch):
    """mean(); std() -> the log of backend calls, asserted to be two plain reads."""
    from bolt_amd.mi355x._ops import backend_for
    with monkeypatch.context() as mp:
        calls, log = _counting(mp, backend_for(arr._device))
        m, s = arr.mean(axis=axis), arr.std(axis=axis)
    assert calls["reduce"] + calls["reduce_rows"] == 2 and calls["reduce_combine"] == 0, calls
    assert not any(st for _, st in log), "no launch carries state="
    assert not arr.__dict__.get("_kept")
    return log, (_bits(m), _bits(s))


def _same_as_off(make, axis, monkeypatch):
    log, res = _two_reads(make(), axis, monkeypatch)
    with monkeypatch.context() as mp:
        mp.setattr(A, "KEEP_MOMENTS", False)
        log_off, res_off = _two_reads(make(), axis, mp)
    assert log == log_off and res == res_off


def test_small_array_at_real_thresholds(kctx, monkeypatch):
    monkeypatch.setattr(A, "KEEP_MOMENTS", True)
    assert A._KEEP_MIN_BYTES == 256 << 20
    _same_as_off(lambda: bolt.array(_x((9, 512)), kctx), 1, monkeypatch)
    _same_as_off(lambda: bolt.array(_x((500, 3, 4)), kctx).swap((0,), (0, 1)), 2, monkeypatch)


def test_state_larger_than_a_64th_of_the_read(kctx, keep_small, monkeypatch):
    # 8 float32 per output: 16 B of state against 32 B read
    _same_as_off(lambda: bolt.array(_x((600, 8)), kctx), 1, monkeypatch)
    # 255 float32 per output: 16 * 64 = 1024 > 1020 B
    _same_as_off(lambda: bolt.array(_x((7, 255)), kctx), 1, monkeypatch)
    arr = bolt.array(_x((7, 256)), kctx)   # 1024 B per output: kept
    arr.mean(axis=1)
    assert arr.__dict__.get("_kept")


@pytest.mark.parametrize("layout", ("padded_cols", "permuted", "dense_cols"))
def test_columns_keep_nothing_by_default(kctx, keep_small, monkeypatch, layout):
    """Column reductions (I > 1) keep no state unless _KEEP_COLS is lifted."""
    monkeypatch.setattr(A, "_KEEP_COLS", False)
    for first in ("mean", "std"):
        with monkeypatch.context() as mp:
            arr, axis = _layout(kctx, layout, mp)
            getattr(arr, first)(axis=axis)
            assert not arr.__dict__.get("_kept")
            _two_reads(arr, axis, mp)


def test_integer_input_keeps_nothing(kctx, keep_small, monkeypatch):
    _same_as_off(lambda: bolt.array(_x((9, 512), "uint16"), kctx), 1, monkeypatch)


def test_switch_off(kctx, keep_small, monkeypatch):
    monkeypatch.setattr(A, "KEEP_MOMENTS", False)
    _two_reads(bolt.array(_x((9, 512)), kctx), 1, monkeypatch)


def test_switch_reads_the_environment():
    import subprocess
    import sys
    code = "import bolt_amd.mi355x.array as A; print(A.KEEP_MOMENTS)"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for val, want in (("0", "False"), ("1", "True"), (None, "True")):
        env = dict(os.environ, PYTHONPATH=root)
        env.pop("BOLT_AMD_KEEP_MOMENTS", None)
        if val is not None:
            env["BOLT_AMD_KEEP_MOMENTS"] = val
        out = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, check=True).stdout
        assert out.decode().strip() == want


def test_plain_cpu_backend_keeps_nothing(keep_small, monkeypatch):
    """tests/cpu_backend.py does not know the capability: today's path, call for call."""
    from bolt_amd import MI355XContext
    from bolt_amd.mi355x._ops import backend_for, register_backend
    plain = cpu_backend.CpuBackend()
    assert not hasattr(plain, "keeps_moments")
    monkeypatch.setitem(__import__("bolt_amd.mi355x._ops", fromlist=["_BACKENDS"])._BACKENDS, "cpu", plain)
    ctx = MI355XContext(device="cpu")
    for layout in LAYOUTS:
        with monkeypatch.context() as mp:
            arr, axis = _layout(ctx, layout, mp)
            assert backend_for(arr._device) is plain
            calls, log = _counting(mp, plain)
            arr.mean(axis=axis)
            arr.std(axis=axis)
            assert calls["reduce"] + calls["reduce_rows"] == 2 and calls["reduce_combine"] == 0
            assert not any(st for _, st in log) and not arr.__dict__.get("_kept")
    del register_backend


def test_unpersist_releases_and_compact_keeps(kctx, keep_small, monkeypatch):
    from bolt_amd.mi355x._ops import backend_for
    arr, axis = _layout(kctx, "padded_rows", monkeypatch)
    want = _bits(arr.std(axis=axis))
    assert arr.__dict__.get("_kept")
    be = backend_for(arr._device)
    # _compact moves bytes, not values; the keys are logical axes
    arr._compact()
    assert "_pbuf" not in arr.__dict__ and arr.__dict__.get("_kept")
    calls, _ = _counting(monkeypatch, be)
    assert _bits(arr.std(axis=axis)) == want
    assert _reads(calls) == 0 and calls["reduce_combine"] == 1
    arr.unpersist()
    assert not arr.__dict__.get("_kept")
    for k in calls:
        calls[k] = 0
    assert _bits(arr.std(axis=axis)) == want   # (dense rows now: the same plan over the same values)
    assert calls["reduce"] + calls["reduce_rows"] == 1 and calls["reduce_combine"] == 0


def _two_ranks_body(rank, world):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [here, os.path.dirname(here)]
    from bolt_amd import MI355XContext
    from bolt_amd.mi355x._ops import register_backend
    be = KeepingCpuBackend()
    register_backend("cpu", be)
    A.KEEP_MOMENTS, A._KEEP_MIN_BYTES = True, 0
    ctx = MI355XContext(device="cpu")
    assert ctx.world_size == world
    log = []
    for name in ("reduce", "reduce_rows", "reduce_state", "reduce_combine"):
        def call(*a, _f=getattr(be, name), _n=name, **k):
            log.append((_n, k.get("state") is not None))
            return _f(*a, **k)
        setattr(be, name, call)
    want = _x((8, 600), seed=3)
    for axis, reads in ((1, ["reduce", "reduce"]), (0, ["reduce_state", "reduce_combine"] * 2)):
        del log[:]
        arr = bolt.array(want, ctx)
        m, s = arr.mean(axis=axis), arr.std(axis=axis)
        assert [n for n, _ in log] == reads, (rank, axis, log)
        assert not any(st for _, st in log) and not arr.__dict__.get("_kept"), (rank, axis)
        assert np.allclose(m, want.mean(axis=axis), rtol=1e-5) and np.allclose(s, want.std(axis=axis), rtol=1e-4)


def _two_ranks_worker(rank, world, port, errq):
    import traceback
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    try:
        dist.init_process_group("gloo", rank=rank, world_size=world)
        _two_ranks_body(rank, world)
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        errq.put((rank, traceback.format_exc()))
        raise


def test_two_ranks_keep_nothing():
    """A 2-rank gloo context (keeping CPU executor): every call is today's."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    errq = ctx.Queue()
    procs = [ctx.Process(target=_two_ranks_worker, args=(r, 2, port, errq)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=300)
    errs = []
    while not errq.empty():
        errs.append(errq.get())
    for p in procs:
        if p.is_alive():
            p.kill()
    assert not errs, "\n".join("rank %d:\n%s" % e for e in errs)
    assert all(p.exitcode == 0 for p in procs)


# ------------------------------------------------------------------ 1. C ABI
# data of one reduction of n values, by kind
KINDS = ("normal", "offset", "outlier", "constant", "nan", "inf")


def _fill(kind, n, rng):
    v = rng.standard_normal(n)
    if kind == "offset":
        v += 1e6
    elif kind == "outlier":
        v[n // 2] = 1e8
    elif kind == "constant":
        v[:] = 3.25
    elif kind == "nan":
        v[n // 3] = np.nan
    elif kind == "inf":
        v[n - 1] = np.inf
    return v


def _dev(a, off=0):
    """Host array -> device bytes; ``off`` bytes past a 16-B boundary."""
    import torch
    from bolt_amd.mi355x.transfer import to_device
    raw = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    if off:
        raw = np.concatenate([np.zeros(off, np.uint8), raw])
    t = to_device(raw, torch.device("cuda:0"))
    assert t.data_ptr() % 16 == 0
    return t[off:]


def _check_keep(be, dtype, src, dense, O, R, I, pitch, tag):
    """bm_reduce_keep against the plain launches on the same buffer, its state
    against bm_reduce_state(BM_STAT_VAR) of the dense values, and the one-part
    bm_reduce_combine of the state against bm_reduce(VAR / STD).  -> kept."""
    import torch
    from bolt_amd.mi355x._ops import dtype_code
    code = dtype_code(np.dtype(dtype))
    odt = np.dtype(np.float64) if np.dtype(dtype).itemsize == 8 or np.dtype(dtype).kind != "f" else np.dtype(dtype)
    ocode = dtype_code(odt)
    nout = O * I

    def buf(nbytes, fill):
        return torch.full((nbytes,), fill, dtype=torch.uint8, device="cuda:0")

    plain, outs, states, kept, fin = {}, {}, {}, {}, {}
    ref_state = buf(16 * nout, 0)
    with np.errstate(all="ignore"):
        be.reduce_state(VAR, dense, code, O, R, I, ref_state)
        for stat in (MEAN, VAR, STD):
            plain[stat], outs[stat] = buf(nout * odt.itemsize, 0), buf(nout * odt.itemsize, 0)
            states[stat] = buf(16 * nout, 0xA5)
            if I == 1:
                be.reduce_rows(stat, src, code, O, R, pitch, plain[stat], ocode)
                kept[stat] = be.reduce_rows(stat, src, code, O, R, pitch, outs[stat], ocode, state=states[stat])
            else:
                be.reduce(stat, src, code, O, R, I, plain[stat], ocode)
                kept[stat] = be.reduce(stat, src, code, O, R, I, outs[stat], ocode, state=states[stat])
            if kept[stat]:
                for fs in (VAR, STD):
                    fin[stat, fs] = buf(nout * odt.itemsize, 0)
                    be.reduce_combine(fs, code, states[stat], [R], nout, fin[stat, fs], ocode)
    torch.cuda.synchronize()
    host = lambda t: t.cpu().numpy().tobytes()
    assert len(set(kept.values())) == 1, (tag, kept)
    for stat in (MEAN, VAR, STD):
        assert host(outs[stat]) == host(plain[stat]), (tag, "out", stat)
        if kept[stat]:
            assert host(states[stat]) == host(ref_state), (tag, "state", stat)
            for fs in (VAR, STD):
                assert host(fin[stat, fs]) == host(plain[fs]), (tag, "combine", stat, fs)
        else:
            assert host(states[stat]) == b"\xa5" * (16 * nout), (tag, "state untouched", stat)
    return kept[MEAN]


ROWS_R = (1, 3, 511, 512, 513, 1029, 2000)
ROWS_O = (1, 9, 37)   # 37: 10 blocks of 4 rows, enough for rows_block's 8-XCD remap
COLS_R = (1, 7, 8, 9, 20, 33, 63, 100)   # 20: the 4-row loop; 63: two 8-row batches in some phases, unchunked
COLS_I = (2, 3, 256, 257, 1000)
COLS_O = (1, 3)
FLOATS = ("float16", "float32", "float64")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", FLOATS)
def test_gpu_keep_rows_abi(gpu_ctx, dtype):
    """Rows kernel: dense rows and rows at a pitch > R (whole 16-B vectors, so
    the dense copy's plan is the padded rows'), every data kind in every shape
    (rows of an array cycle through the kinds; one-row arrays take each)."""
    import torch
    from bolt_amd.mi355x._ops import backend_for
    be = backend_for(torch.device("cuda:0"))
    rng = np.random.default_rng(11)
    es = np.dtype(dtype).itemsize
    nkept = 0
    for R, O in itertools.product(ROWS_R, ROWS_O):
        for k0 in (range(len(KINDS)) if O == 1 else (0,)):
            with np.errstate(all="ignore"):
                x = np.stack([_fill(KINDS[(o + k0) % len(KINDS)], R, rng) for o in range(O)]).astype(dtype)
            pitch = -(-R * es // 64) * 64 // es + 16
            xp = np.full((O, pitch), 7, dtype=dtype)
            xp[:, :R] = x
            dense = _dev(x)
            tag = (dtype, O, R, KINDS[k0])
            # one chunk per row unless R holds two chunks of four wave-wide vectors (plan_reduce)
            vec = 16 // es
            while vec > 1 and R % vec:
                vec >>= 1
            k = _check_keep(be, dtype, dense, dense, O, R, 1, R, tag + ("dense",))
            assert k == (R < 2 * 4 * 64 * vec), tag
            assert _check_keep(be, dtype, _dev(xp), dense, O, R, 1, pitch, tag + ("padded",)) == k, tag
            nkept += k
    assert nkept
    # a pointer 4 bytes off 16-B alignment (one element for float64): the scalar
    # plan (2-element vectors for float16); rows of 500 stay one chunk
    with np.errstate(all="ignore"):
        x = np.stack([_fill(KINDS[o % len(KINDS)], 500, rng) for o in range(9)]).astype(dtype)
    off = _dev(x, off=max(4, es))
    assert off.data_ptr() % 16 == max(4, es)
    assert _check_keep(be, dtype, off, off, 9, 500, 1, 500, (dtype, "offset pointer"))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", FLOATS)
def test_gpu_keep_cols_abi(gpu_ctx, dtype):
    """Columns kernel: column j of an array holds data kind j % 6."""
    import torch
    from bolt_amd.mi355x._ops import backend_for
    be = backend_for(torch.device("cuda:0"))
    rng = np.random.default_rng(12)
    nkept = 0
    for R, I, O in itertools.product(COLS_R, COLS_I, COLS_O):
        with np.errstate(all="ignore"):
            x = np.stack([np.stack([_fill(KINDS[(j + o) % len(KINDS)], R, rng) for j in range(I)], axis=1)
                          for o in range(O)]).astype(dtype)
        assert x.shape == (O, R, I)
        src = _dev(x)
        k = _check_keep(be, dtype, src, src, O, R, I, R, (dtype, O, R, I))
        # at least four row phases of eight rows each before R is split into chunks (plan_reduce)
        assert k or R >= 64, (dtype, O, R, I)
        nkept += k
    assert nkept


@pytest.mark.gpu
def test_gpu_keep_unkept_plans(gpu_ctx):
    """Integer inputs and chunked plans run the plain launches: kept = 0, out as bm_reduce writes it."""
    import torch
    from bolt_amd.mi355x._ops import backend_for
    be = backend_for(torch.device("cuda:0"))
    x = _x((9, 513), "int16", seed=4)
    src = _dev(x)
    assert _check_keep(be, "int16", src, src, 9, 513, 1, 513, "int16 rows") is False
    x = _x((40, 12), "int16", seed=5)
    src = _dev(x)
    assert _check_keep(be, "int16", src, src, 1, 40, 12, 40, "int16 cols") is False
    # few outputs, long R: plan_reduce splits R over blocks
    n = ctypes.c_size_t(0)
    O, R = 1, 1 << 22
    assert be.lib.bm_reduce_workspace_bytes(VAR, _lib.BM_F32, O, R, 1, ctypes.byref(n)) == 0 and n.value > 0
    src = _dev(_x((O, R), seed=6))
    assert _check_keep(be, "float32", src, src, O, R, 1, R, "chunked rows") is False
    O, R, I = 1, 4000, 2048
    assert be.lib.bm_reduce_workspace_bytes(VAR, _lib.BM_F32, O, R, I, ctypes.byref(n)) == 0 and n.value > 0
    src = _dev(_x((O, R, I), seed=7))
    assert _check_keep(be, "float32", src, src, O, R, I, R, "chunked cols") is False


# --------------------------------------------------------- 5. argument errors
def test_keep_argument_errors():
    """bm_reduce_keep refuses bad arguments before touching a device (no GPU needed)."""
    lib = _lib.load()
    F32, F64, I32 = _lib.BM_F32, _lib.BM_F64, _lib.BM_I32
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)  # never dereferenced: every call below fails its checks
    kept = ctypes.c_int(7)
    k = ctypes.byref(kept)
    f = lib.bm_reduce_keep
    for args in ((MEAN, None, F32, 2, 8, 1, 8, p, F32, p, k),
                 (MEAN, p, F32, 2, 8, 1, 8, None, F32, p, k),
                 (VAR, p, F32, 2, 8, 1, 8, p, F32, None, k),
                 (STD, p, F32, 2, 8, 1, 8, p, F32, p, None)):
        assert f(*args, None, 0, None) == _lib.BM_E_ARG
        assert b"null pointer" in lib.bm_last_error()
    for stat in (_lib.STAT_SUM, _lib.STAT_MAX, _lib.STAT_FMIN, -1, 99):
        assert f(stat, p, F32, 2, 8, 1, 8, p, F32, p, k, None, 0, None) == _lib.BM_E_ARG
    assert b"stat" in lib.bm_last_error()
    assert f(MEAN, p, F32, 2, 8, 1, 8, p, I32, p, k, None, 0, None) == _lib.BM_E_ARG
    assert b"not a float dtype" in lib.bm_last_error()
    assert f(MEAN, p, F32, 2, 8, 1, 7, p, F32, p, k, None, 0, None) == _lib.BM_E_ARG
    assert b"row_pitch" in lib.bm_last_error()
    assert f(VAR, p, F32, 2, 8, 4, 16, p, F64, p, k, None, 0, None) == _lib.BM_E_ARG  # a pitch with I > 1
    assert b"row_pitch" in lib.bm_last_error()
    for O, R, I in ((0, 8, 1), (2, 0, 1), (2, 8, 0)):
        assert f(STD, p, F32, O, R, I, R, p, F32, p, k, None, 0, None) == _lib.BM_E_ARG
        assert b"empty reduction" in lib.bm_last_error()
    assert f(MEAN, p, 99, 2, 8, 1, 8, p, F32, p, k, None, 0, None) == _lib.BM_E_ARG
    assert kept.value == 7, "kept is written only once the arguments pass"
    # a chunked plan without its workspace: BM_E_WS before any launch, nothing kept
    assert f(VAR, p, F32, 1, 200000, 1, 200000, p, F32, p, k, None, 0, None) == _lib.BM_E_WS
    assert b"workspace too small" in lib.bm_last_error() and kept.value == 0
