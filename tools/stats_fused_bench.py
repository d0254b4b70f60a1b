"""Interleaved A/B timing of stats() against the two calls it replaces.

    timeout -k 10 600 python tools/stats_fused_bench.py --shape c2_rows [--rounds 9] [--warmup 3]

One process per shape (run each under its own `timeout`); after a warm-up the
two variants run in interleaved rounds on the same array:
  A  s.mean(axis); s.std(axis)               -- two reads (the baseline, unchanged code)
  B  s.stats(axis, names=('mean', 'std'))    -- one read
Each variant is timed with a host clock around the calls (the host results
they return imply the stream synchronise).  In further rounds every bm_reduce*
launch is bracketed by hipEvents: the mean, std and fused launch sequences on
their own.  Prints medians, min-max spread and GB/s of the array's bytes per
read, and the criterion: B's median below A's by more than A's own
round-to-round spread.  A last probe times the fused launch itself storing
one plane or two, into page-locked host memory or HBM: where its time over
std alone goes.

Shapes: c2_rows  float32 (512, 512, 2000) after swap, axis 2 (row-padded rows)
        c2_cols  the same data unswapped, (2000, 512, 512), axis 0 (columns)
        c4_cols  uint16 (2000, 1024, 1024), axis 0 (exact-integer columns)
        small_*  the same layouts at 1/64 of the size (a quick check of the tool)
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {
    "c2_rows": (np.float32, (2000, 512, 512), True, 2),
    "c2_cols": (np.float32, (2000, 512, 512), False, 0),
    "c4_cols": (np.uint16, (2000, 1024, 1024), False, 0),
    "small_rows": (np.float32, (2000, 64, 64), True, 2),
    "small_cols": (np.float32, (2000, 64, 64), False, 0),
    "small_int": (np.uint16, (2000, 128, 128), False, 0),
}


def make(name, ctx):
    import bolt_amd as bolt
    dtype, shape, swap, axis = SHAPES[name]
    rng = np.random.default_rng(1)
    if np.dtype(dtype).kind == "f":
        x = rng.random(shape, dtype=np.float32)
        x *= 100.0
        x += 1000.0
    else:
        x = rng.integers(0, 65536, size=shape, dtype=np.uint16)
    b = bolt.array(x, ctx, axis=(0,))
    nbytes = x.nbytes
    del x
    if swap:
        b = b.swap((0,), (0, 1))
    return b, axis, nbytes


def summary(ts):
    a = np.asarray(ts)
    return float(np.median(a)), float(a.min()), float(a.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", required=True, choices=sorted(SHAPES))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    assert a.rounds >= 7, "at least 7 rounds per variant"
    import torch
    import bolt_amd as bolt
    from bolt_amd.mi355x._ops import backend_for
    ctx = bolt.MI355XContext(device="cuda:0")
    s, axis, nbytes = make(a.shape, ctx)
    torch.cuda.synchronize()
    print("%s: %s %s axis %s, %s, %.3f GB" % (a.shape, s.dtype, s.shape, axis,
          "row-padded" if "_pbuf" in s.__dict__ else "dense", nbytes / 1e9), flush=True)

    def var_a():
        return s.mean(axis=axis), s.std(axis=axis)

    def var_b():
        st = s.stats(axis=axis, names=("mean", "std"))
        return st.mean, st.std

    for _ in range(a.warmup):
        ra, rb = var_a(), var_b()
    # the same statistics: std bit for bit, the mean within the parity rule's 1e-6 of the data's scale
    assert np.asarray(ra[1]).tobytes() == np.asarray(rb[1]).tobytes(), "std differs"
    scale = 1e-6 * (1100.0 if s.dtype.kind == "f" else 65535.0)
    assert float(np.max(np.abs(np.asarray(ra[0], np.float64) - np.asarray(rb[0], np.float64)))) <= scale

    host = {"A": [], "B": []}
    for _ in range(a.rounds):
        for tag, fn in (("A", var_a), ("B", var_b)):
            t0 = time.perf_counter()
            fn()
            host[tag].append((time.perf_counter() - t0) * 1e3)

    # hipEvents around every reduction launch sequence (separate rounds: the
    # event records stay out of the host-clock figures above)
    be = backend_for(s._device)
    spans = []
    last = {}

    def timed(name):
        fn = getattr(be, name)

        def call(*args, **kw):
            last[name] = args
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn(*args, **kw)
            e1.record()
            spans.append((name, e0, e1))
            return r
        return call
    saved = {}
    for name in ("reduce", "reduce_rows", "reduce_moments", "reduce_state"):
        saved[name] = getattr(be, name)
        setattr(be, name, timed(name))
    dev = {"mean": [], "std": [], "fused": []}
    try:
        for _ in range(a.rounds):
            for key, fn in (("mean", lambda: s.mean(axis=axis)), ("std", lambda: s.std(axis=axis)), ("fused", var_b)):
                del spans[:]
                fn()
                torch.cuda.synchronize()
                assert len(spans) == 1, [n for n, _, _ in spans]
                dev[key].append(spans[0][1].elapsed_time(spans[0][2]))
    finally:
        for name, fn in saved.items():
            setattr(be, name, fn)

    gb = nbytes / 1e6  # bytes / ms / 1e6 = GB/s
    for tag, reads, what in (("A", 2, "mean(); std()"), ("B", 1, "stats(mean, std)")):
        med, lo, hi = summary(host[tag])
        print("host   %s %-18s median %8.3f ms  min %8.3f  max %8.3f  spread %6.3f  %7.1f GB/s per read (%d read%s)"
              % (tag, what, med, lo, hi, hi - lo, reads * gb / med, reads, "s" if reads > 1 else ""), flush=True)
    for key in ("mean", "std", "fused"):
        med, lo, hi = summary(dev[key])
        print("events %-20s median %8.3f ms  min %8.3f  max %8.3f  spread %6.3f  %7.1f GB/s"
              % (key, med, lo, hi, hi - lo, gb / med), flush=True)
    ma, la, ha = summary(host["A"])
    mb = summary(host["B"])[0]
    print("criterion: A - B = %.3f ms (%.1f%% of A), A's spread %.3f ms -> %s"
          % (ma - mb, 100.0 * (ma - mb) / ma, ha - la, "B faster" if ma - mb > ha - la else "NOT MET"), flush=True)
    ms, ls, hs = summary(dev["std"])
    mf = summary(dev["fused"])[0]
    print("fused launch vs std alone: %+.3f ms (%+.1f%%), std's spread %.3f ms -> %s"
          % (mf - ms, 100.0 * (mf - ms) / ms, hs - ls, "within spread" if mf - ms <= hs - ls else "slower"),
          flush=True)

    # where the fused launch's time goes: the same bm_reduce_moments launch
    # storing one plane or two, into page-locked host memory or into HBM
    from bolt_amd.mi355x.transfer import host_result
    src, code, O, R, I, pitch, outs, ocode = last["reduce_moments"]
    nb = [o for o in outs if o is not None][0].numel()
    hbm = [torch.empty(nb, dtype=torch.uint8, device=src.device) for _ in range(2)]
    pinned = [host_result(be, nb, src.device) for _ in range(2)]
    variants = [("std -> HBM", (None, None, hbm[1])), ("mean + std -> HBM", (hbm[0], None, hbm[1]))]
    if all(h is not None for h in pinned):
        variants += [("std -> host", (None, None, pinned[1])), ("mean + std -> host", (pinned[0], None, pinned[1]))]
    probe = dict((v[0], []) for v in variants)
    for r in range(a.warmup + a.rounds):
        for tag, o3 in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            be.reduce_moments(src, code, O, R, I, pitch, o3, ocode)
            e1.record()
            e1.synchronize()
            if r >= a.warmup:
                probe[tag].append(e0.elapsed_time(e1))
    for tag, _ in variants:
        med, lo, hi = summary(probe[tag])
        print("probe  %-20s median %8.3f ms  min %8.3f  max %8.3f  spread %6.3f  (planes of %.2f MB)"
              % (tag, med, lo, hi, hi - lo, nb / 1e6), flush=True)


if __name__ == "__main__":
    sys.exit(main())
