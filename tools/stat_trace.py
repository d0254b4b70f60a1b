"""Launch trace of the statistics, for comparing two revisions call by call.

    python tools/stat_trace.py [--device cpu|cuda:0] [--world N] [--full] > trace.txt
    timeout -k 10 300 python tools/stat_trace.py --device cuda:0 --time

Every public method of the backend (all but host_writable, whose calls depend
on which page-locked block the host allocator hands out) and
dist.all_gather_bytes is wrapped; for a fixed table of cases one line is
printed per call: the method, its scalar arguments, the byte sizes (never the
addresses) of its tensor arguments, ``pin`` for a tensor in page-locked host
memory, ``state=`` / ``moments=`` where given, and what it returned.  Run at
two revisions, the outputs must not differ: the same launches in the same
order with the same arguments, the same choice of host or device destination,
the same collectives with the same sizes on every rank.  --full prints those
lines; without it each (layout, dtype, axis) is one line that gives, per
method sequence, the number of calls and the first 8 hex digits of the SHA-1
of its --full lines (a difference is then read from two --full outputs).

The table: the layouts of tests/test_stats_moments_kept.py (_layout) in float32,
float64, int16 and uint8, the swaps of tests/test_zz_swap_moments.py (SHAPES)
in their own dtype and in int16, with the thresholds lowered as those tests
lower them; the axes last, first, middle, (0, 2) and None; the sequences
(mean, std, var), (std, mean), stats(), stats(names=('mean', 'std')), center,
zscore, (sum, max), each run, then run again after unpersist().  On the CPU the
executor is the keeping one of tests/test_stats_moments_kept.py plus the
standardize entry points of tests/standardize_cases.py, then the plain one
(the fallbacks; float32 and int16 only); --world N runs the layouts over gloo, one process per rank,
with an array whose last rank holds no records, and prints every rank's trace.

--time: the wall time per call of mean / stats / center over the last axis of
a resident (64, 8, 40) float32 array, the median of --calls calls of each, in
microseconds, each call ending in a device synchronise (the host path
dominates at this size).
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

DTYPES = ("float32", "float64", "int16", "uint8")
LAYOUTS = ("padded_rows", "padded_cols", "permuted", "dense_rows", "dense_cols")
SWAPS = [("float32", (600, 4, 36), 64), ("float32", (760, 2, 64), 64), ("float32", (760, 4, 36), 64),
         ("float32", (256, 2, 64), 64), ("float32", (40, 8, 16), 1), ("float64", (520, 3, 32), 64),
         ("float64", (1000, 2, 16), 64)]
SEQUENCES = [
    ("mean,std,var", lambda a, ax: [a.mean(axis=ax), a.std(axis=ax), a.var(axis=ax)]),
    ("std,mean", lambda a, ax: [a.std(axis=ax), a.mean(axis=ax)]),
    ("stats", lambda a, ax: [a.stats(axis=ax)]),
    ("stats(mean,std)", lambda a, ax: [a.stats(axis=ax, names=("mean", "std"))]),
    ("center", lambda a, ax: [a.center(axis=ax)]),
    ("zscore", lambda a, ax: [a.zscore(axis=ax)]),
    ("sum,max", lambda a, ax: [a.sum(axis=ax), a.max(axis=ax)]),
]
_SWITCHES = ("KEEP_MOMENTS", "_KEEP_MIN_BYTES", "_KEEP_COLS", "FUSE_SWAP_MOMENTS", "_FUSE_SWAP_MIN_BYTES",
             "_FUSE_SWAP_STATE_DIV", "_PITCH_MIN_ROW", "_PITCH_LINE", "_PITCH_ALIGN", "_PITCH_PAD_DIV",
             "_PITCH_PLANS")


def _show(v):
    import ctypes
    import torch
    if isinstance(v, torch.Tensor):
        return "%s[%d]" % ("pin" if v.is_pinned() else "u8", v.numel() * v.element_size())
    if isinstance(v, np.ndarray):
        return "nd%s" % (v.shape,)
    if isinstance(v, (list, tuple)):
        return "(" + ",".join(_show(e) for e in v) + ")"
    if isinstance(v, ctypes.Array):
        return "c[%d]" % len(v)
    if isinstance(v, (bool, int, float, str, type(None), np.integer, np.floating)):
        return str(v)
    return type(v).__name__


def _wrap(name, fn, log):
    def call(*a, **k):
        r = fn(*a, **k)
        log.append("  %s %s%s%s" % (name, " ".join(_show(v) for v in a),
                                    "".join(" %s=%s" % (n, _show(v)) for n, v in sorted(k.items())),
                                    "" if r is None else " -> " + _show(r)))
        return r
    return call


def trace_backend(be, log):
    for name in dir(be):
        if name.startswith("_") or name == "host_writable" or not callable(getattr(be, name)):
            continue
        setattr(be, name, _wrap(name, getattr(be, name), log))


def trace_gather(log):
    """dist.all_gather_bytes, under every name the package's modules hold it by."""
    from bolt_amd.mi355x import dist
    plain = dist.all_gather_bytes

    def gather(ctx, buf, sizes):
        log.append("  all_gather_bytes %s %s" % (_show(buf), _show(list(sizes))))
        return plain(ctx, buf, sizes)
    for mod in list(sys.modules.values()):
        if getattr(mod, "__name__", "").startswith("bolt_amd.") and getattr(mod, "all_gather_bytes", None) is plain:
            mod.all_gather_bytes = gather


def _x(shape, dtype, seed=1):
    rng = np.random.default_rng(seed)
    if np.dtype(dtype).kind in "iu":
        return rng.integers(0, 100, size=shape).astype(dtype)
    return (10 + 3 * rng.standard_normal(shape)).astype(dtype)


def _small_pitch(A):
    A._PITCH_MIN_ROW, A._PITCH_LINE, A._PITCH_ALIGN, A._PITCH_PAD_DIV, A._PITCH_PLANS = 1, 16, 64, 0, {}


def make(bolt, A, ctx, layout, dtype):
    """A fresh array of ``layout`` (a name of LAYOUTS, a shape to swap, or
    'empty_slab') -- its swap is part of the trace."""
    if layout == "padded_rows":
        return bolt.array(_x((500, 3, 4), dtype), ctx).swap((0,), (0, 1))
    if layout == "padded_cols":
        _small_pitch(A)
        return bolt.array(_x((5, 300, 1), dtype), ctx).swap((0,), (0, 1))
    if layout == "permuted":
        return bolt.array(_x((10, 5, 30), dtype), ctx)
    if layout == "dense_rows":
        return bolt.array(_x((9, 512), dtype), ctx)
    if layout == "dense_cols":
        return bolt.array(_x((300, 8), dtype), ctx)
    if layout == "empty_slab":   # a leading extent below the world: the last rank holds no records
        return bolt.array(_x((ctx.world_size - 1, 6, 5), dtype), ctx)
    return bolt.array(_x(layout, dtype), ctx).swap((0,), (0, 1))


def axes_of(ndim):
    out = [("last", ndim - 1), ("first", 0)]
    if ndim >= 3:
        out += [("middle", 1), ("(0,2)", (0, 2))]
    return out + [("None", None)]


def run_table(device, log, emit, world=1, dtypes=DTYPES):
    import bolt_amd as bolt
    import bolt_amd.mi355x.array as A
    from bolt_amd.mi355x._ops import backend_for
    ctx = bolt.MI355XContext(device=device)
    trace_backend(backend_for(ctx.device), log)
    trace_gather(log)
    saved = dict((n, getattr(A, n)) for n in _SWITCHES)
    table = [(l, d, 64) for l in LAYOUTS for d in dtypes]
    if world > 1:
        table += [("empty_slab", d, 64) for d in ("float32", "int16")]
    else:
        table += [(s, d, div) for d0, s, div in SWAPS for d in (d0, "int16")]
    for layout, dtype, div in table:
        ndim = 2 if layout in ("dense_rows", "dense_cols") else 3
        for aname, axis in axes_of(ndim):
            for sname, seq in SEQUENCES:
                A.KEEP_MOMENTS, A._KEEP_MIN_BYTES, A._KEEP_COLS = True, 0, True
                A.FUSE_SWAP_MOMENTS, A._FUSE_SWAP_MIN_BYTES, A._FUSE_SWAP_STATE_DIV = True, 0, div
                try:
                    emit("%s %s axis=%s %s" % (layout, dtype, aname, sname))
                    arr = make(bolt, A, ctx, layout, dtype)
                    emit("  kept after make: %s" % sorted(arr.__dict__.get("_kept") or ()))
                    for again in (False, True):
                        if again:
                            arr.unpersist()
                            emit("  unpersist")
                        seq(arr, axis)
                        emit("  kept: %s" % sorted(arr.__dict__.get("_kept") or ()))
                finally:
                    for n, v in saved.items():
                        setattr(A, n, v)


def digest(lines):
    """The --full output condensed: per (layout, dtype, axis) one line of
    ``sequence calls:hash`` entries; executor / rank markers pass through."""
    import hashlib
    out, cases = [], []

    def flush():
        rows = {}
        for head, body in cases:
            prefix, seq = head.rsplit(" ", 1)
            calls = sum(1 for l in body if not l.startswith(("  kept", "  unpersist")))
            rows.setdefault(prefix, []).append("%s %d:%s" % (seq, calls,
                                                             hashlib.sha1("\n".join(body).encode()).hexdigest()[:8]))
        out.extend("%s | %s" % (prefix, " | ".join(v)) for prefix, v in rows.items())
        del cases[:]
    for l in lines:
        if l.startswith("  "):
            cases[-1][1].append(l)
        elif l.startswith(("== ", "-- ")) or l == "end":
            flush()
            out.append(l)
        else:
            cases.append((l, []))
    flush()
    return out


def _cpu_backend(keeping):
    import cpu_backend
    if not keeping:
        return cpu_backend.CpuBackend()
    import standardize_cases as S
    from test_stats_moments_kept import KeepingCpuBackend
    fused = type(S.fused_backend())
    return type("TraceCpuBackend", (KeepingCpuBackend, fused), {})()


def _rank(rank, world, port, keeping, q):
    import torch.distributed as dist
    from bolt_amd.mi355x._ops import register_backend
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    register_backend("cpu", _cpu_backend(keeping))
    log = []
    try:
        run_table("cpu", log, log.append, world, DTYPES if keeping else DTYPES[::2])
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        import traceback
        log.append(traceback.format_exc())
        q.put((rank, log))
        raise
    q.put((rank, log))


def trace(a):
    out = []
    if not a.device.startswith("cpu"):
        run_table(a.device, out, out.append)
        out.append("end")
    else:
        from bolt_amd.mi355x._ops import register_backend
        for keeping in (True, False):
            out.append("== executor: %s, world %d" % ("keeping + standardize" if keeping else "plain", a.world))
            if a.world == 1:
                register_backend("cpu", _cpu_backend(keeping))
                run_table("cpu", out, out.append, 1, DTYPES if keeping else DTYPES[::2])
                continue
            import socket
            import torch.multiprocessing as mp
            s = socket.socket()
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
            s.close()
            mpc = mp.get_context("spawn")
            q = mpc.Queue()
            procs = [mpc.Process(target=_rank, args=(r, a.world, port, keeping, q)) for r in range(a.world)]
            for p in procs:
                p.start()
            logs = dict(q.get(timeout=600) for _ in procs)
            for p in procs:
                p.join(timeout=60)
            for r in range(a.world):
                out.append("-- rank %d" % r)
                out.extend(l for block in logs[r] for l in block.split("\n"))
    print("\n".join(out if a.full else digest(out)), flush=True)


def timed(a):
    import bolt_amd as bolt
    if a.device.startswith("cpu"):
        from bolt_amd.mi355x._ops import register_backend
        register_backend("cpu", _cpu_backend(True))
    ctx = bolt.MI355XContext(device=a.device)
    arr = bolt.array(_x((64, 8, 40), "float32"), ctx)
    sync = (lambda: None) if a.device.startswith("cpu") else __import__("torch").cuda.synchronize
    for name in ("mean", "stats", "center"):
        f = getattr(arr, name)
        for _ in range(200):
            f(axis=2)
        sync()
        ts = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            f(axis=2)
            sync()   # mean / stats return host results; center's launch is waited for here
            ts.append(time.perf_counter() - t0)
        print("%s(axis=2) median %.2f us per call over %d calls" % (name, 1e6 * float(np.median(ts)), a.calls),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", default="cpu")
    ap.add_argument("--world", type=int, default=1, help="ranks over gloo (cpu only)")
    ap.add_argument("--full", action="store_true", help="one line per call, not one digest line per case")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--calls", type=int, default=4000)
    a = ap.parse_args()
    return timed(a) if a.time else trace(a)


if __name__ == "__main__":
    sys.exit(main())
