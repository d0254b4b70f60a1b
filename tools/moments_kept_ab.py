"""Interleaved A/B timing of mean / std with the moment state kept or not.

    timeout -k 10 600 python tools/moments_kept_ab.py --layout c2_rows [--rounds 9] [--warmup 2]

One process per layout (run each under its own `timeout`).  The array is made
once in HBM; every timed sequence runs on a fresh array object over the same
buffer (no state held), in rounds that alternate the switch:
  A  array.KEEP_MOMENTS = False   -- every call reads the array (the parent's path)
  B  array.KEEP_MOMENTS = True    -- the first call keeps the state, a later std is finished from it
Sequences: mean() alone, std() alone, mean(); std().  Each is timed with a
host clock around the calls (the host results they return imply the stream
synchronise) and, in rounds of their own, with hipEvents around every
reduce / reduce_rows / reduce_combine launch (summed per sequence).  Prints
medians and min-max spreads, whether a state was kept, and two criteria:
  dual   B's mean() launch (M_MEAN and M_MOM accumulations of one read) against
         the slower of A's mean() and std() launches, within A's spread;
  pair   A - B of mean(); std() against A's spread.
The results of A and B are compared byte for byte first.

Layouts: c2_rows      float32 (512, 512, 2000) after swap, axis 2 (rows of 2000 at a pitch of 2048)
         c2_cols      the same data unswapped, (2000, 512, 512), axis 0 (columns; R split into chunks)
         target_cols  float32 (1024, 256, 256, 32), axis 0: the 64 GiB target's column reduction at 1/8 of its rows
         (column layouts keep nothing unless --keep-cols lifts array._KEEP_COLS)
         small_*      the same layouts at a fraction of the size (a quick check of the tool; see --min-bytes)
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LAYOUTS = {
    "c2_rows": ((2000, 512, 512), True, 2),
    "c2_cols": ((2000, 512, 512), False, 0),
    "target_cols": ((1024, 256, 256, 32), False, 0),
    "small_rows": ((2000, 64, 64), True, 2),
    "small_cols": ((1024, 256, 64, 32), False, 0),
}
SEQS = (("mean", ("mean",)), ("std", ("std",)), ("mean;std", ("mean", "std")))


def summary(ts):
    a = np.asarray(ts)
    return float(np.median(a)), float(a.min()), float(a.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layout", required=True, choices=sorted(LAYOUTS))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--keep-cols", action="store_true",
                    help="let a column layout keep the state too (array._KEEP_COLS): the measurement behind "
                         "the rule that it does not")
    ap.add_argument("--min-bytes", type=int, default=None,
                    help="array._KEEP_MIN_BYTES for this run (the small_* layouts are below the real 256 MiB)")
    a = ap.parse_args()
    assert a.rounds >= 7, "at least 7 rounds per variant"
    import torch
    import bolt_amd as bolt
    import bolt_amd.mi355x.array as A
    from bolt_amd.mi355x._ops import backend_for
    if a.min_bytes is not None:
        A._KEEP_MIN_BYTES = a.min_bytes
    A._KEEP_COLS = a.keep_cols
    shape, swap, axis = LAYOUTS[a.layout]
    dev = torch.device("cuda:0")
    ctx = bolt.MI355XContext(device="cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    t = torch.randn(shape, generator=g, device=dev, dtype=torch.float32).mul_(50.0).add_(1000.0)
    base = bolt.ConstructMI355X.fromshards(t, shape, context=ctx, split=1, dtype=np.float32)
    del t
    if swap:
        base = base.swap((0,), (0, 1))
    nbytes = int(np.prod(shape)) * 4
    torch.cuda.synchronize()
    padded = "_pbuf" in base.__dict__
    print("%s%s: float32 %s axis %s, %s, %.3f GB" % (a.layout, " --keep-cols" if a.keep_cols else "", base.shape, axis,
                                                   "row-padded" if padded else "dense", nbytes / 1e9), flush=True)

    def fresh():
        """A new array object over base's buffer: no state held."""
        d = base.__dict__
        if padded:
            return base._derive_padded(d["_pbuf"], d["_pitch"], base._shape, base._split)
        return base._derive(d["_data"], base._shape, base._split)

    def run(names, on):
        A.KEEP_MOMENTS = on
        s = fresh()
        t0 = time.perf_counter()
        res = [getattr(s, n)(axis=axis) for n in names]
        ms = (time.perf_counter() - t0) * 1e3
        return ms, res, bool(s.__dict__.get("_kept"))

    kept = {}
    for _ in range(a.warmup):
        for tag, names in SEQS:
            ra, rb = run(names, False), run(names, True)
            kept[tag] = rb[2]
            assert not ra[2]
            for x, y in zip(ra[1], rb[1]):
                assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), "results differ between A and B"
    print("state kept with the switch on: %s; results of A and B byte-identical"
          % ", ".join("%s %s" % (tag, kept[tag]) for tag, _ in SEQS), flush=True)

    host = {}
    for _ in range(a.rounds):
        for on in (False, True):
            for tag, names in SEQS:
                host.setdefault((on, tag), []).append(run(names, on)[0])

    # hipEvents around every reduction launch (separate rounds: the event
    # records stay out of the host-clock figures above)
    be = backend_for(dev)
    spans = []

    def timed(name):
        fn = getattr(be, name)

        def call(*args, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn(*args, **kw)
            e1.record()
            spans.append((name, e0, e1))
            return r
        return call
    saved = {}
    for name in ("reduce", "reduce_rows", "reduce_combine"):
        saved[name] = getattr(be, name)
        setattr(be, name, timed(name))
    evs, parts = {}, {}
    try:
        for _ in range(a.rounds):
            for on in (False, True):
                for tag, names in SEQS:
                    del spans[:]
                    run(names, on)
                    torch.cuda.synchronize()
                    each = [(n, e0.elapsed_time(e1)) for n, e0, e1 in spans]
                    evs.setdefault((on, tag), []).append(sum(ms for _, ms in each))
                    parts.setdefault((on, tag), []).append(each)
    finally:
        for name, fn in saved.items():
            setattr(be, name, fn)
        A.KEEP_MOMENTS = True

    gb = nbytes / 1e6  # bytes / ms / 1e6 = GB/s
    for what, table in (("host  ", host), ("events", evs)):
        for tag, _ in SEQS:
            for on in (False, True):
                med, lo, hi = summary(table[on, tag])
                print("%s %s %-9s median %8.3f ms  min %8.3f  max %8.3f  spread %6.3f  %7.1f GB/s of the array per ms"
                      % (what, "B keep" if on else "A off ", tag, med, lo, hi, hi - lo, gb / med), flush=True)
    # the launches of B's mean(); std(), one line each (medians over the rounds)
    seq = parts[True, "mean;std"]
    for i in range(len(seq[0])):
        print("events B mean;std launch %d %-15s median %8.3f ms"
              % (i, seq[0][i][0], float(np.median([r[i][1] for r in seq]))), flush=True)
    am, al, ah = summary(evs[False, "mean"])
    sm, sl, sh = summary(evs[False, "std"])
    bm = summary(evs[True, "mean"])[0]
    bs = summary(evs[True, "std"])[0]
    ref, spread = max(am, sm), max(ah - al, sh - sl)
    print("dual: B mean() launch %.3f ms against the slower of A's mean() %.3f / std() %.3f: %+.3f ms (%+.1f%%), "
          "A's spread %.3f ms -> %s" % (bm, am, sm, bm - ref, 100.0 * (bm - ref) / ref, spread,
                                         "mean() keeps nothing on this layout (the plain launch)" if not kept["mean"] else
                                         "within spread" if bm - ref <= spread else "slower"), flush=True)
    print("      B std() launch (stores the state it finalises) %.3f ms against A's %.3f: %+.3f ms"
          % (bs, sm, bs - sm), flush=True)
    pa, pl, ph = summary(host[False, "mean;std"])
    pb = summary(host[True, "mean;std"])[0]
    print("pair: mean(); std() A - B = %.3f ms (%.1f%% of A), A's spread %.3f ms -> %s"
          % (pa - pb, 100.0 * (pa - pb) / pa, ph - pl, "B faster" if pa - pb > ph - pl else "no gain"), flush=True)


if __name__ == "__main__":
    sys.exit(main())
