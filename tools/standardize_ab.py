"""Interleaved timing of zscore() against the map() it replaces and against a copy.

    timeout -k 10 600 python tools/standardize_ab.py --layout c2_rows [--rounds 9] [--warmup 2]

One process per layout (run each under its own `timeout`).  The array is made
once in HBM; every timed call runs on a fresh array object over the same buffer,
in rounds that take the variants in turn, each between two hipEvents on torch's
stream (every variant only queues launches; the events are read after a
synchronise at the end of the round):
  A  s.zscore(axis)
  B  s.map(lambda v: (v - v.mean()) / v.std(), axis=keys), the only way to do it
     on the device before zscore (rows layouts only: the reduced axis must be
     the record).  Records reach the function as torch tensors, whose std() is
     the sample one (ddof = 1): B's values are A's times sqrt((R - 1) / R), which
     the comparison below allows for; the cost is the same.
  C  the floor: bm_copy_strided of the array's bytes (pad included) from the
     input's buffer to a result buffer -- one read and one write; on the column
     layouts, whose zscore takes a moments read first, plus one mean reduction
     launch over the same layout (C+read).
Before timing, A is checked against the float128 truth on a sample of records
with the tests' tolerance (|err| <= 2 eps |truth| + 1e-12 max|x| / std +
smallest subnormal), and B against A.  Prints medians with min-max, A / C, the
bytes A moves per second against the 8 TB/s peak, and whether A beats B by
more than the larger of their spreads.

Layouts: c2_rows     float32 (512, 512, 2000) after swap, axis 2 (rows of 2000 at a pitch of 2048)
         c2_cols     the same data unswapped, (2000, 512, 512), axis 0 (columns: moments, then apply)
         small_*     the same at a fraction of the size (a quick check of the tool)
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LAYOUTS = {
    "c2_rows": ((2000, 512, 512), True, 2),
    "c2_cols": ((2000, 512, 512), False, 0),
    "small_rows": ((2000, 64, 64), True, 2),
    "small_cols": ((2000, 64, 64), False, 0),
}
PEAK = 8e12  # HBM bytes / s


def summary(ts):
    a = np.asarray(ts)
    return float(np.median(a)), float(a.min()), float(a.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layout", required=True, choices=sorted(LAYOUTS))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    assert a.rounds >= 9 and a.warmup >= 2, "at least 2 warm-ups and 9 rounds"
    import torch
    import bolt_amd as bolt
    from bolt_amd.mi355x import _lib
    from bolt_amd.mi355x._ops import backend_for, dtype_code
    from bolt_amd.mi355x.dist import _empty
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
    torch.cuda.synchronize()
    d = base.__dict__
    padded = "_pbuf" in d
    buf = d["_pbuf"] if padded else d["_data"]
    nbytes = int(np.prod(shape)) * 4
    print("%s: float32 %s axis %s, %s, %.3f GB (%.3f GB with the pad)"
          % (a.layout, base.shape, axis, "row-padded at %d" % d["_pitch"] if padded else "dense", nbytes / 1e9,
             buf.numel() / 1e9), flush=True)
    be = backend_for(dev)
    keys = tuple(range(base.split))

    def fresh():
        """A new array object over base's buffer (B compacts a padded one: that is part of its cost)."""
        if padded:
            return base._derive_padded(d["_pbuf"], d["_pitch"], base._shape, base._split)
        return base._derive(d["_data"], base._shape, base._split)

    def run_a():
        return fresh().zscore(axis=axis)

    def run_b():
        return fresh().map(lambda v: (v - v.mean()) / v.std(), axis=keys)

    dst = _empty(buf.numel(), dev)
    R, I = shape[0], int(np.prod(shape[1:]))
    mean_out = _empty(I * 4, dev)
    code = dtype_code(np.float32)

    def run_c():
        n = buf.numel() // 4
        be.copy_strided(buf, 0, dst, 0, [n], [1], [1], 4)
        if not swap:
            be.reduce(_lib.STAT_MEAN, buf, code, 1, R, I, mean_out, code)

    variants = [("A zscore", run_a), ("C copy" if swap else "C+read", run_c)]
    if swap:
        variants.insert(1, ("B map", run_b))

    # ---- checks before timing
    ra = run_a()
    rows = int(np.prod(base.shape[:-1])) if swap else None
    if swap:
        idx = torch.as_tensor(np.linspace(0, rows - 1, 64).astype(np.int64), device=dev)

        def records(arr):
            """(records, R): a strided view of padded rows, or the dense rows."""
            return arr._elements() if "_pbuf" in arr.__dict__ else arr._elements((rows, arr.shape[-1]))
        x = records(base)[idx].cpu().numpy()
        got = records(ra)[idx].cpu().numpy()
        ax = 1
    else:
        x = base._elements((R, I))[:, :64].cpu().numpy()
        got = ra._elements((R, I))[:, :64].cpu().numpy()
        ax = 0
    v = x.astype(np.longdouble)
    sd = np.sqrt(v.var(axis=ax, keepdims=True))
    truth = (v - v.mean(axis=ax, keepdims=True)) / sd
    fi = np.finfo(np.float32)
    bound = 2 * fi.eps * np.abs(truth) + 1e-12 * np.abs(v).max(axis=ax, keepdims=True) / sd + fi.smallest_subnormal
    err = np.abs(got.astype(np.longdouble) - truth)
    print("A against the float128 truth on 64 records: max error / bound = %.3g" % float((err / bound).max()), flush=True)
    assert np.all(err <= bound), "zscore misses the tolerance"
    if swap:
        rb = run_b()
        n = base.shape[-1]
        gb = records(rb)[idx].cpu().numpy().astype(np.float64) * np.sqrt((n - 1.0) / n)
        off = float(np.abs(gb - got).max())
        # (B's arithmetic is float32 throughout, on data offset by 20 standard
        # deviations: it is the looser of the two, so this is a check that both
        # do the same operation, not of A's accuracy)
        print("B (sample std, rescaled to the population one) against A: max |B - A| = %.3g" % off, flush=True)
        assert off <= 1e-2, "map() and zscore() disagree"
        del rb
    del ra
    torch.cuda.synchronize()

    times = dict((tag, []) for tag, _ in variants)
    for k in range(a.warmup + a.rounds):
        spans = []
        for tag, fn in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            del out
            spans.append((tag, e0, e1))
        torch.cuda.synchronize()
        if k >= a.warmup:
            for tag, e0, e1 in spans:
                times[tag].append(e0.elapsed_time(e1))

    stats = {}
    for tag, _ in variants:
        med, lo, hi = stats[tag] = summary(times[tag])
        print("%-9s median %8.3f ms  min %8.3f  max %8.3f  spread %6.3f" % (tag, med, lo, hi, hi - lo), flush=True)
    am, al, ah = stats["A zscore"]
    ctag = "C copy" if swap else "C+read"
    cm = stats[ctag][0]
    moved = (2 if swap else 3) * nbytes  # bytes A has to move: one read and one write, or two reads and one write
    print("A / %s = %.3f;  A moves %.3f GB in %.3f ms: %.2f TB/s = %.3f of 8 TB/s  (C: %.3f of 8 TB/s)"
          % (ctag, am / cm, moved / 1e9, am, moved / am / 1e9, moved / (am * 1e-3) / PEAK,
             moved / (cm * 1e-3) / PEAK), flush=True)
    if swap:
        bm, bl, bh = stats["B map"]
        spread = max(ah - al, bh - bl)
        print("B - A = %.3f ms (A is %.1fx faster), larger spread %.3f ms -> %s"
              % (bm - am, bm / am, spread, "A faster" if bm - am > spread else "no gain"), flush=True)


if __name__ == "__main__":
    sys.exit(main())
