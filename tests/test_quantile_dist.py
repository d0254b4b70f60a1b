"""quantile() / percentile() / median() across ranks on CPU: worlds 2 and 3
over gloo with the numpy test executor, in the pattern of
test_stat_comoment_dist.py.  The sharded axis kept (each rank its own records,
the outputs gathered), the sharded axis reduced with others kept (one exchange
brings the kept axes to the front, then as before), a leading extent smaller
than the world (a rank with an empty slab still takes part in every
collective), a row-padded swap result, and every axis reduced, which raises
NotImplementedError.  Run on the executor as it is (the methods' fallback) and
on the subclass with the entry points (quantile_cases.fused_backend: the HIP
backend's orchestration).  Every rank must hold the same bytes.
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
    import torch
    import torch.distributed as dist
    import bolt_amd as bolt
    from bolt_amd import MI355XContext
    from bolt_amd.mi355x._ops import register_backend
    import cpu_backend
    import quantile_cases as S
    be = None
    if fused:
        be = S.fused_backend()
        be.calls = {"rows": 0, "select": 0}
        register_backend("cpu", be)
    else:
        cpu_backend.install()
    ctx = MI355XContext(device="cpu")
    assert ctx.world_size == world and ctx.rank == rank

    def same_everywhere(got, tag):
        mine = torch.from_numpy(np.frombuffer(np.ascontiguousarray(got).tobytes(), dtype=np.uint8).copy())
        if mine.numel() == 0:
            return
        every = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(every, mine)
        assert all(torch.equal(e, mine) for e in every), tag

    def check(b, x, axis):
        tag = "world %d rank %d %s %s axis %s" % (world, rank, x.dtype, x.shape, axis)
        qs = (0.0, S.QG, 0.5, 0.9, 1.0)   # 'linear': two batches
        for method in S.METHODS:
            got = np.asarray(b.quantile(qs, axis=axis, method=method))
            for j, q in enumerate(qs):
                one = S.check(b, x, q, axis, method, tag)
                assert one.tobytes() == got[j].tobytes(), tag
            same_everywhere(got, tag)

    rng = np.random.default_rng(0)
    x = (1000 + 50 * rng.standard_normal((7, 6, 5))).astype(np.float32)
    b = bolt.array(x, ctx)
    for axis in (1, 2, (1, 2), 0, (0, 2), (0, 1)):
        check(b, x, axis)
    for bb in (b, bolt.array(x[:, 0, 0].copy(), ctx)):
        for method in S.METHODS:
            with pytest.raises(NotImplementedError):
                bb.quantile(0.5, method=method)
        with pytest.raises(NotImplementedError):
            bb.median(axis=None)
    # a leading extent smaller than the world: the last rank's slab is empty
    y = rng.standard_normal((world - 1, 6, 5))
    by = bolt.array(y, ctx)
    lo, hi = ctx.local_bounds(world - 1)
    assert (hi == lo) == (rank == world - 1)
    for axis in (1, 2, 0, (0, 1)):
        check(by, y, axis)
    u = rng.integers(0, 65536, size=(9, 4, 3)).astype(np.uint16)
    bu = bolt.array(u, ctx)
    for axis in (2, 0, (0, 2)):
        check(bu, u, axis)
    # a row-padded swap result (rows of 500 float32 at a pitch of 512)
    z = (10 + rng.standard_normal((500, 3, 4))).astype(np.float32)
    s = bolt.array(z, ctx).swap((0,), (0, 1))
    zs = np.ascontiguousarray(z.transpose(1, 2, 0))
    for axis in (2, 0, (0, 2)):
        check(s, zs, axis)
    if fused:
        assert be.calls["rows"] > 0, be.calls


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
def test_quantile_multirank_gloo(world, fused):
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
