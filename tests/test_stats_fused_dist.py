"""stats() across ranks on CPU: worlds 2 and 3 over gloo with the numpy test
executor, in the pattern of test_dist_gloo.py.  Over the sharded axis (one
STAT_VAR state per rank, one gather, one merge), over a kept-shard axis (per-rank
planes, one gather), over every axis, on a row-padded swap result and with a
leading extent smaller than the world (a rank with an empty slab).  Run once
on the executor as it is (no fused entry points: stats()' one-state fallback)
and once on a subclass that implements reduce_moments /
reduce_combine_moments, which takes the orchestration the HIP backend takes.
"""
import os
import socket
import traceback

import numpy as np
import pytest
import torch.multiprocessing as mp

FIELDS = ("mean", "var", "std")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _fused_backend():
    import cpu_backend as C

    class FusedCpuBackend(C.CpuBackend):
        """CpuBackend plus the two fused entry points (include/bolt_mi355x.h)."""

        def __init__(self):
            self.calls = {"reduce_moments": 0, "reduce_combine_moments": 0}

        def reduce_moments(self, src, code, O, R, I, pitch, outs, out_code):
            assert pitch >= R and (I == 1 or pitch == R) and any(o is not None for o in outs)
            self.calls["reduce_moments"] += 1
            a = src.numpy().view(C._CODES[code])
            if I == 1:
                x = a[:O * pitch].reshape(O, pitch)[:, :R].reshape(O, R, 1)
            else:
                x = a.reshape(O, R, I)
            with np.errstate(all="ignore"):
                planes = self._planes(C.STAT_VAR, code, x)
                for stat, o in zip((C.STAT_MEAN, C.STAT_VAR, C.STAT_STD), outs):
                    if o is not None:
                        self._finish(stat, code, planes, float(R), o, out_code)

        def reduce_combine_moments(self, code, states, counts, nout, outs, out_code):
            assert any(o is not None for o in outs)
            self.calls["reduce_combine_moments"] += 1
            om, ov, osd = outs
            if om is not None:
                means = states.view(len(counts), 2, nout * 8)[:, 0, :].contiguous().view(-1)
                self.reduce_combine(C.STAT_MEAN, code, means, counts, nout, om, out_code)
            if ov is not None:
                self.reduce_combine(C.STAT_VAR, code, states, counts, nout, ov, out_code)
            if osd is not None:
                self.reduce_combine(C.STAT_STD, code, states, counts, nout, osd, out_code)

    return FusedCpuBackend()


def _same(got, want):
    got_a, want_a = np.asarray(got), np.asarray(want)
    return (type(got) is type(want) and got_a.dtype == want_a.dtype and got_a.shape == want_a.shape
            and got_a.tobytes() == want_a.tobytes())


def _body(rank, world, fused):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [here, os.path.dirname(here)]
    import bolt_amd as bolt
    from bolt_amd import MI355XContext
    from bolt_amd.mi355x._ops import register_backend
    import cpu_backend
    import golden_cases as G
    be = None
    if fused:
        be = _fused_backend()
        register_backend("cpu", be)
    else:
        cpu_backend.install()
    ctx = MI355XContext(device="cpu")
    assert ctx.world_size == world and ctx.rank == rank

    def check(b, x, axis, keepdims=False, names=FIELDS):
        st = b.stats(axis=axis, keepdims=keepdims, names=names)
        ax = tuple(range(x.ndim)) if axis is None else (tuple(axis) if isinstance(axis, tuple) else (axis,))
        tag = (x.shape, str(x.dtype), axis, names)
        assert st.count == int(np.prod([x.shape[a] for a in ax])), tag
        for f in FIELDS:
            assert (getattr(st, f) is None) == (f not in names), tag
        if "var" in names:
            assert _same(st.var, b.var(axis=axis, keepdims=keepdims)), tag
        if "std" in names:
            assert _same(st.std, b.std(axis=axis, keepdims=keepdims)), tag
        if "mean" in names:
            ref = b.mean(axis=axis, keepdims=keepdims)
            assert type(st.mean) is type(ref) and np.asarray(st.mean).shape == np.asarray(ref).shape, tag
            assert np.asarray(st.mean).dtype == np.asarray(ref).dtype, tag
            truth = G.truth_stat(x, "mean", list(ax))
            assert G.stat_close(st.mean, ref, truth, np.asarray(ref).dtype, x, "mean"), tag

    rng = np.random.default_rng(0)
    x = (1000 + 50 * rng.standard_normal((7, 6, 5))).astype(np.float32)
    b = bolt.array(x, ctx)
    for axis in (0, (0, 2), (0, 1, 2), None):   # the sharded axis is reduced: states, one gather, one merge
        check(b, x, axis)
        check(b, x, axis, keepdims=True, names=("mean", "std"))
    for axis in (1, 2, (1, 2)):                 # the sharded axis is kept: per-rank planes, one gather
        check(b, x, axis)
        check(b, x, axis, names=("var", "mean"))
    # a leading extent smaller than the world: the last rank's slab is empty
    y = rng.standard_normal((world - 1, 6, 5))
    by = bolt.array(y, ctx)
    lo, hi = ctx.local_bounds(world - 1)
    assert (hi == lo) == (rank == world - 1)
    for axis in (0, 1, (0, 2), None):
        check(by, y, axis)
    # exact small integers
    u = rng.integers(0, 65536, size=(9, 4, 3)).astype(np.uint16)
    bu = bolt.array(u, ctx)
    for axis in (0, 2, None):
        check(bu, u, axis)
    # a row-padded swap result (rows of 500 float32 at a pitch of 512)
    z = (10 + rng.standard_normal((500, 3, 4))).astype(np.float32)
    s = bolt.array(z, ctx).swap((0,), (0, 1))
    zs = np.ascontiguousarray(z.transpose(1, 2, 0))
    for axis in (2, 0, (0, 2), None):
        check(s, zs, axis)
    # one name alone is the method itself
    assert _same(b.stats(axis=0, names="std").std, b.std(axis=0))
    if be is not None and rank == 0:
        assert be.calls["reduce_moments"] > 0 and be.calls["reduce_combine_moments"] > 0, be.calls


def _worker(rank, world, port, errq, fused):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    try:
        dist.init_process_group("gloo", rank=rank, world_size=world)
        _body(rank, world, fused)
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        errq.put((rank, traceback.format_exc()))
        raise


@pytest.mark.parametrize("fused", [False, True], ids=["fallback", "fused"])
@pytest.mark.parametrize("world", [2, 3])
def test_stats_multirank_gloo(world, fused):
    ctx = mp.get_context("spawn")
    errq = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, errq, fused)) for r in range(world)]
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
    assert all(p.exitcode == 0 for p in procs)  # every rank returned
