"""Interleaved A/B timing of swap() with and without the fused row moments.

    timeout -k 10 600 python tools/swap_moments_ab.py [--shape 2000,512,512] [--rounds 9] [--warmup 2]

The source array is made once in HBM; every timed sequence swaps a fresh array
object over that one buffer, in rounds that alternate the switch:
  A  array.FUSE_SWAP_MOMENTS = False  -- the plain transpose; mean() reads the result, std() is
                                         finished from the state mean() kept (the parent's path)
  B  array.FUSE_SWAP_MOMENTS = True   -- the transpose leaves the rows' state; mean() and std()
                                         are finished from it
Sequences: swap((0,), (0, 1)) alone, and swap; mean(axis=-1); std(axis=-1).
Each is timed with a host clock (the sequence ends with a stream synchronise)
and, in rounds of their own, with hipEvents around the swap's one copy_strided
call (the transpose, plus B's merge kernel).  Prints medians, min-max spreads
and interquartile ranges, the largest difference between A's and B's
statistics, and the two criteria of DESIGN.md: the step's gain against the
larger interquartile range of the two variants (a single slow call of the host
clock -- a page fault, another process -- widens min-max beyond the whole gain
and says nothing about the other rounds), and the swap's own cost against a
third of what the first statistic saves.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SEQS = (("swap", ()), ("swap;mean;std", ("mean", "std")))


def summary(ts):
    a = np.asarray(ts)
    return float(np.median(a)), float(a.min()), float(a.max())


def iqr(ts):
    q1, q3 = np.percentile(np.asarray(ts), [25, 75])
    return float(q3 - q1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="2000,512,512")
    ap.add_argument("--dtype", default="float32", choices=("float32", "float64"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--min-bytes", type=int, default=None, help="array._FUSE_SWAP_MIN_BYTES for this run")
    a = ap.parse_args()
    assert a.rounds >= 7, "at least 7 rounds per variant"
    import torch
    import bolt_amd as bolt
    import bolt_amd.mi355x.array as A
    from bolt_amd.mi355x._ops import backend_for
    if a.min_bytes is not None:
        A._FUSE_SWAP_MIN_BYTES = a.min_bytes
    shape = tuple(int(s) for s in a.shape.split(","))
    dt = np.dtype(a.dtype)
    dev = torch.device("cuda:0")
    ctx = bolt.MI355XContext(device="cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    t = torch.randn(shape, generator=g, device=dev, dtype=getattr(torch, a.dtype)).mul_(50.0).add_(1000.0)
    base = bolt.ConstructMI355X.fromshards(t, shape, context=ctx, split=1, dtype=dt)
    del t
    nbytes = int(np.prod(shape)) * dt.itemsize
    print("%s %s swap((0,), (0, 1)), %.3f GB" % (a.dtype, shape, nbytes / 1e9), flush=True)

    def fresh():
        return base._derive(base._data, base._shape, base._split)

    def run(names, on):
        A.FUSE_SWAP_MOMENTS = on
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s = fresh().swap((0,), (0, 1))
        res = [getattr(s, n)(axis=s.ndim - 1) for n in names]
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        entry = (s.__dict__.get("_kept") or {}).get((s.ndim - 1,))
        return ms, res, entry is not None and entry.serves_mean

    worst = 0.0
    fusedB = None
    for _ in range(a.warmup):
        for tag, names in SEQS:
            ra, rb = run(names, False), run(names, True)
            assert not ra[2]
            fusedB = rb[2]
            for x, y in zip(ra[1], rb[1]):
                x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
                worst = max(worst, float(np.max(np.abs(x - y) / np.maximum(np.abs(x), 1e-300))))
    print("B fused: %s; largest relative difference of mean / std between A and B: %.3g" % (fusedB, worst),
          flush=True)

    host = {}
    for _ in range(a.rounds):
        for on in (False, True):
            for tag, names in SEQS:
                host.setdefault((on, tag), []).append(run(names, on)[0])

    be = backend_for(dev)
    spans = []
    plain = be.copy_strided

    def timed(*args, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = plain(*args, **kw)
        e1.record()
        spans.append((e0, e1))
        return r
    be.copy_strided = timed
    evs = {}
    try:
        for _ in range(a.rounds):
            for on in (False, True):
                del spans[:]
                run((), on)
                assert len(spans) == 1, "the swap is one copy_strided call"
                evs.setdefault(on, []).append(spans[0][0].elapsed_time(spans[0][1]))
    finally:
        del be.copy_strided
        A.FUSE_SWAP_MOMENTS = True

    for tag, _ in SEQS:
        for on in (False, True):
            med, lo, hi = summary(host[on, tag])
            print("host   %s %-14s median %8.3f ms  min %8.3f  max %8.3f  spread %6.3f  iqr %6.3f"
                  % ("B fuse" if on else "A off ", tag, med, lo, hi, hi - lo, iqr(host[on, tag])), flush=True)
    for on in (False, True):
        med, lo, hi = summary(evs[on])
        print("events %s copy_strided   median %8.3f ms  min %8.3f  max %8.3f  spread %6.3f  %7.1f GB/s"
              % ("B fuse" if on else "A off ", med, lo, hi, hi - lo, 2 * nbytes / 1e6 / med), flush=True)
    sa = summary(host[False, "swap;mean;std"])[0]
    sb = summary(host[True, "swap;mean;std"])[0]
    spread = max(iqr(host[False, "swap;mean;std"]), iqr(host[True, "swap;mean;std"]))
    ea, eb = summary(evs[False])[0], summary(evs[True])[0]
    print("step: swap; mean; std A - B = %.3f ms (%.1f%% of A), larger interquartile range %.3f ms -> %s"
          % (sa - sb, 100.0 * (sa - sb) / sa, spread, "B faster" if sa - sb > spread else "no gain"), flush=True)
    saved = (sa - sb) + (eb - ea)   # what the statistics save: the step's gain plus what the swap lost
    print("swap alone: B - A = %+.3f ms by events; the statistics save %.3f ms; a third of that %.3f ms -> %s"
          % (eb - ea, saved, saved / 3.0, "on by default" if eb - ea < saved / 3.0 else "behind the switch"),
          flush=True)


if __name__ == "__main__":
    sys.exit(main())
