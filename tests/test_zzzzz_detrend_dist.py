"""detrend() across ranks on CPU: worlds 2 and 3 over gloo with the numpy test
executor, in the pattern of test_standardize_dist.py.  Over the sharded axis
(one co-moment state per rank and batch over its slice of the basis, one
gather, the co-moments and the mean merged in rank order, then this rank's
slab with its slice of the basis), over kept-shard axes (each rank its own
records), over every axis, with a leading extent smaller than the world (a
rank with an empty slab still takes part in every collective) and on a
row-padded swap result.  Run on the executor as it is (the method's fallbacks)
and on the subclass with the entry points (detrend_cases.fused_backend: the
HIP backend's orchestration).  (Named to be collected after every other
module: see test_zzzzz_detrend.)
"""
import os
import socket
import traceback

import numpy as np
import pytest
import torch.multiprocessing as mp


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _body(rank, world, fused):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [here, os.path.dirname(here)]
    import bolt_amd as bolt
    from bolt_amd import MI355XContext
    from bolt_amd.mi355x._ops import register_backend
    import cpu_backend
    import detrend_cases as D
    calls = {"detrend_rows": 0, "detrend_apply": 0, "comoment_state": 0, "comoment_combine": 0}
    if fused:
        be = D.fused_backend()
        for name in calls:
            def counted(*a, _f=getattr(be, name), _n=name, **k):
                calls[_n] += 1
                return _f(*a, **k)
            setattr(be, name, counted)
        register_backend("cpu", be)
    else:
        cpu_backend.install()
    ctx = MI355XContext(device="cpu")
    assert ctx.world_size == world and ctx.rank == rank

    def check(b, x, axis, orders=(1, 3)):
        for order in orders:
            r = b.detrend(axis=axis, order=order)  # every rank holds its slab; toarray gathers them all
            D.check_array(r, b, x, axis, order, "world %d rank %d %s %s axis %s"
                          % (world, rank, x.dtype, x.shape, axis))

    rng = np.random.default_rng(0)
    x = (1000 + 50 * rng.standard_normal((7, 6, 5))).astype(np.float32)
    b = bolt.array(x, ctx)
    for axis in (0, (0, 2), None, 1, 2, (1, 2)):
        check(b, x, axis)
    check(b, x, (0, 2), orders=(5, 8))   # two batches of signals over the sharded axis
    # order 0 is center(), across ranks too
    assert b.detrend(axis=0, order=0).toarray().tobytes() == b.center(axis=0).toarray().tobytes()
    # a leading extent smaller than the world: the last rank's slab is empty
    y = rng.standard_normal((world - 1, 6, 5))
    by = bolt.array(y, ctx)
    lo, hi = ctx.local_bounds(world - 1)
    assert (hi == lo) == (rank == world - 1)
    for axis in ((0, 1), 1, None):
        check(by, y, axis)
    if world == 3:
        check(by, y, 0, orders=(1,))   # two values a record
    else:
        with pytest.raises(ValueError):   # one value a record: on every rank, before any collective
            by.detrend(axis=0, order=1)
    u = rng.integers(0, 65536, size=(9, 4, 3)).astype(np.uint16)
    bu = bolt.array(u, ctx)
    for axis in (0, 2, None):
        check(bu, u, axis, orders=(1, 2))
    # a row-padded swap result (rows of 500 float32 at a pitch of 512)
    z = (10 + rng.standard_normal((500, 3, 4))).astype(np.float32)
    s = bolt.array(z, ctx).swap((0,), (0, 1))
    zs = np.ascontiguousarray(z.transpose(1, 2, 0))
    for axis in (2, 0, None):
        check(s, zs, axis, orders=(1, 2))
    if fused:
        assert all(v > 0 for v in calls.values()), calls


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
def test_detrend_multirank_gloo(world, fused):
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
