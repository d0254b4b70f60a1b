"""Interleaved timing of detrend() against zscore(), against a copy, and against
its own two-pass path.

    timeout -k 10 600 python tools/detrend_ab.py --layout c2_rows [--rounds 9] [--warmup 2]

One process per layout (run each under its own `timeout`).  The array is made
once in HBM; every timed call runs on a fresh array object over the same buffer,
in rounds that take the variants in turn, each between two hipEvents on torch's
stream (every variant only queues launches; the events are read after a
synchronise at the end of the round):
  Dk  s.detrend(axis, order=k): on the rows layouts one bm_detrend_rows launch
  Fk  the same with the rows launch refused (rows not taken: forced here by a
      backend whose detrend_rows launches nothing and answers False), so the
      two-pass path runs: bm_comoment_state per batch of four basis rows, then
      bm_detrend_apply (rows layouts only)
  Z   s.zscore(axis): the same traffic with the least arithmetic
  C   the floor: bm_copy_strided of the array's bytes (pad included) from the
      input's buffer to a result buffer -- one read and one write; on the
      column layouts plus one mean reduction launch over the same layout
      (C+read)
Before timing, every D and F variant is checked against the longdouble truth
on a sample of records with the tests' tolerance (|err| <= 2 eps |truth| +
1e-12 max|x| + smallest subnormal; tests/detrend_cases.py).  Prints medians
with min-max, every D's ratio to Z and to C, and per order whether D beats F
by more than the larger of their spreads.

Layouts: c2_rows     float32 (512, 512, 2000) after swap, axis 2 (rows of 2000 at a pitch of 2048), orders 1 3 5 8
         c2_cols     the same data unswapped, (2000, 512, 512), axis 0 (columns: co-moments, then apply), order 1
         small_*     the same at a fraction of the size (a quick check of the tool)
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

LAYOUTS = {
    "c2_rows": ((2000, 512, 512), True, 2, (1, 3, 5, 8)),
    "c2_cols": ((2000, 512, 512), False, 0, (1,)),
    "small_rows": ((2000, 64, 64), True, 2, (1, 3, 5, 8)),
    "small_cols": ((2000, 64, 64), False, 0, (1,)),
}


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
    import detrend_cases as D
    from bolt_amd.mi355x import _lib
    from bolt_amd.mi355x._ops import backend_for, dtype_code
    from bolt_amd.mi355x.dist import _empty
    shape, swap, axis, orders = LAYOUTS[a.layout]
    dev = torch.device("cuda:0")
    ctx = bolt.MI355XContext(device="cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    t = torch.randn(shape, generator=g, device=dev, dtype=torch.float32).mul_(50.0).add_(1000.0)
    # a slow drift along the record, so that there is a trend to remove
    t.add_(torch.linspace(0.0, 300.0, shape[0], device=dev).reshape(-1, 1, 1))
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
    rows_launch = be.detrend_rows

    def fresh():
        """A new array object over base's buffer."""
        if padded:
            return base._derive_padded(d["_pbuf"], d["_pitch"], base._shape, base._split)
        return base._derive(d["_data"], base._shape, base._split)

    def run_d(order):
        return lambda: fresh().detrend(axis=axis, order=order)

    def run_f(order):
        def run():
            be.detrend_rows = lambda *args: False   # not taken, nothing launched
            try:
                return fresh().detrend(axis=axis, order=order)
            finally:
                be.detrend_rows = rows_launch
        return run

    def run_z():
        return fresh().zscore(axis=axis)

    dst = _empty(buf.numel(), dev)
    R, I = shape[0], int(np.prod(shape[1:]))
    mean_out = _empty(I * 4, dev)
    code = dtype_code(np.float32)

    def run_c():
        n = buf.numel() // 4
        be.copy_strided(buf, 0, dst, 0, [n], [1], [1], 4)
        if not swap:
            be.reduce(_lib.STAT_MEAN, buf, code, 1, R, I, mean_out, code)

    ctag = "C copy" if swap else "C+read"
    variants = [("D%d" % k, run_d(k)) for k in orders] + [("Z zscore", run_z), (ctag, run_c)]
    if swap:
        variants += [("F%d" % k, run_f(k)) for k in orders]

    # ---- checks before timing
    nrows = int(np.prod(base.shape[:-1])) if swap else None
    if swap:
        idx = torch.as_tensor(np.linspace(0, nrows - 1, 64).astype(np.int64), device=dev)

        def records(arr):
            """(records, R): a strided view of padded rows, or the dense rows."""
            return arr._elements() if "_pbuf" in arr.__dict__ else arr._elements((nrows, arr.shape[-1]))
        sample = lambda arr: records(arr)[idx].cpu().numpy()   # noqa: E731
        ax = 1
    else:
        sample = lambda arr: arr._elements((R, I))[:, :64].cpu().numpy()   # noqa: E731
        ax = 0
    x = sample(base)
    for tag, fn in variants:
        if tag[0] not in "DF":
            continue
        order = int(tag[1:])
        truth, bound = D.truth_and_bound(x, ax, order)
        r = fn()
        err = np.abs(sample(r).astype(np.longdouble) - truth)
        del r
        print("%s against the longdouble truth on 64 records: max error / bound = %.3g"
              % (tag, float((err / bound).max())), flush=True)
        assert np.all(err <= bound), "%s misses the tolerance" % tag
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
    zm, cm = stats["Z zscore"][0], stats[ctag][0]
    for k in orders:
        dm, dl, dh = stats["D%d" % k]
        line = "order %d: D / Z = %.3f, D / %s = %.3f" % (k, dm / zm, ctag, dm / cm)
        if swap:
            fm, fl, fh = stats["F%d" % k]
            spread = max(dh - dl, fh - fl)
            line += ";  F - D = %.3f ms (D is %.2fx faster), larger spread %.3f ms -> %s" \
                % (fm - dm, fm / dm, spread, "rows kernel faster" if fm - dm > spread else "no gain")
        print(line, flush=True)


if __name__ == "__main__":
    sys.exit(main())
