"""Interleaved timing of median() / percentile() against the map() they replace
and against std(), the one-read floor.

    timeout -k 10 900 python tools/quantile_ab.py [--size c2|small] [--rounds 9] [--warmup 2] [--placements 3] [--no-map]

Two builds of the library are compared by running it once per build, in turn,
with BOLT_AMD_LIB naming the build and --no-map (B does not depend on it).

One process.  C2's array, float32 (2000, 512, 512), is made in HBM and swapped
to (512, 512, 2000): rows of 2000 at a pitch of 2048 elements.  Every timed call
runs on a fresh array object over the same buffers, in rounds that take the
variants in turn, each between two hipEvents on torch's stream (every call ends
with the synchronise of its host result, so a span is the call's time on the
device and the host).  The whole is repeated over several placements: the
arrays are made anew behind a spacer of another size, so that they lie
elsewhere in HBM.
  A   s.median(axis=2): the rows kernel, one rank pair a row
  A3  s.percentile((10, 50, 90), axis=2): three quantiles of one read
  C   the floor: s.std(axis=2) over the same buffer with moment states off
      (BOLT_AMD_KEEP_MOMENTS=0, BOLT_AMD_FUSE_SWAP_MOMENTS=0, set here), so it
      reads the array once
  B   s.map(lambda v: v.quantile(0.5)) over the records: what users had before
      (torch sorts every record); timed in every round only when one call
      takes under 2 s, else once per placement
  D   x.median(axis=0) of the unswapped (2000, 512, 512): the permuted route
Before timing, A is checked bit for bit against numpy on a sample of records,
A3's middle plane against A, and B against A.  Prints, per placement and over
all, medians with min-max, the ratios to C and B / A.
"""
import argparse
import os
import sys
import time

os.environ["BOLT_AMD_KEEP_MOMENTS"] = "0"
os.environ["BOLT_AMD_FUSE_SWAP_MOMENTS"] = "0"

import numpy as np  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = {"c2": (2000, 512, 512), "small": (2000, 64, 64)}
SPACERS = (0, 3 << 20, 517 << 20, 1031 << 20)  # bytes held in front of each placement's arrays


def summary(ts):
    a = np.asarray(ts)
    return float(np.median(a)), float(a.min()), float(a.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="c2", choices=sorted(SIZES))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--placements", type=int, default=3)
    ap.add_argument("--no-map", action="store_true", help="leave B out (A/B runs of two library builds)")
    a = ap.parse_args()
    assert a.rounds >= 5 and a.warmup >= 2 and 1 <= a.placements <= len(SPACERS)
    import torch
    import bolt_amd as bolt
    shape = SIZES[a.size]
    dev = torch.device("cuda:0")
    ctx = bolt.MI355XContext(device="cuda:0")
    nbytes = int(np.prod(shape)) * 4
    R, nout = shape[0], int(np.prod(shape[1:]))
    order = ("A median", "A3 pct", "C std", "B map", "D cols")
    total = dict((tag, []) for tag in order)

    for pl in range(a.placements):
        spacer = torch.empty(SPACERS[pl], dtype=torch.uint8, device=dev) if SPACERS[pl] else None
        g = torch.Generator(device=dev)
        g.manual_seed(1)
        t = torch.randn(shape, generator=g, device=dev, dtype=torch.float32).mul_(50.0).add_(1000.0)
        cols = bolt.ConstructMI355X.fromshards(t, shape, context=ctx, split=1, dtype=np.float32)
        del t
        base = cols.swap((0,), (0, 1))
        torch.cuda.synchronize()
        d, dc = base.__dict__, cols.__dict__
        padded = "_pbuf" in d
        keys = tuple(range(base.split))
        print("placement %d (spacer %d MiB): float32 %s axis 2, %s, %.3f GB; columns %s axis 0"
              % (pl, SPACERS[pl] >> 20, base.shape, "row-padded at %d" % d["_pitch"] if padded else "dense",
                 nbytes / 1e9, cols.shape), flush=True)

        def fresh():
            """A new array object over base's buffer (B compacts a padded one: that is part of its cost)."""
            if padded:
                return base._derive_padded(d["_pbuf"], d["_pitch"], base._shape, base._split)
            return base._derive(d["_data"], base._shape, base._split)

        def run_a():
            return fresh().median(axis=2)

        def run_a3():
            return fresh().percentile((10, 50, 90), axis=2)

        def run_c():
            return fresh().std(axis=2)

        def run_b():
            return fresh().map(lambda v: v.quantile(0.5), axis=keys)

        def run_d():
            return cols._derive(dc["_data"], cols._shape, cols._split).median(axis=0)

        # ---- checks before timing
        ra, ra3, rd = np.asarray(run_a()), np.asarray(run_a3()), np.asarray(run_d())
        assert ra3.shape == (3,) + ra.shape and ra3[1].tobytes() == ra.tobytes(), "plane 1 of A3 is not A"
        assert rd.tobytes() == ra.tobytes(), "the permuted route disagrees with the rows"
        idx = np.linspace(0, nout - 1, 64).astype(np.int64)
        rows = base._elements() if padded else base._elements((nout, R))
        x = rows[torch.as_tensor(idx, device=dev)].cpu().numpy()[:, :R]
        srt = np.sort(x, axis=1).astype(np.float64)
        pos = 0.5 * (R - 1)
        fl = int(np.floor(pos))
        want = (srt[:, fl] + (srt[:, fl + 1] - srt[:, fl]) * (pos - fl) if pos != fl else srt[:, fl]).astype(np.float32)
        assert np.array_equal(ra.reshape(-1)[idx], want), "median() is not numpy's on the sampled records"
        b_once, b_rounds = float("nan"), False
        if not a.no_map:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rb = run_b()
            torch.cuda.synchronize()
            b_once = (time.perf_counter() - t0) * 1e3
            gb = np.asarray(rb.toarray()).reshape(-1)[idx]
            assert np.allclose(gb, want, rtol=1e-6), "map() and median() disagree"
            del rb
            b_rounds = b_once < 2000.0
        print("checks passed (64 records bit for bit; A3[1] == A; D == A); B's first call %.1f ms%s"
              % (b_once, "" if b_rounds else ": timed once per placement only"), flush=True)

        variants = [("A median", run_a), ("A3 pct", run_a3), ("C std", run_c), ("D cols", run_d)]
        if b_rounds:
            variants.insert(3, ("B map", run_b))
        times = dict((tag, []) for tag, _ in variants)
        if not b_rounds:
            times["B map"] = [b_once]
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
        for tag in order:
            med, lo, hi = summary(times[tag])
            total[tag] += times[tag]
            print("  %-9s median %9.3f ms  min %9.3f  max %9.3f" % (tag, med, lo, hi), flush=True)
        del base, cols, d, dc, rows, spacer
        torch.cuda.empty_cache()

    print("all placements:", flush=True)
    st = {}
    for tag in order:
        med, lo, hi = st[tag] = summary(total[tag])
        print("  %-9s median %9.3f ms  min %9.3f  max %9.3f  (%d spans)" % (tag, med, lo, hi, len(total[tag])),
              flush=True)
    c = st["C std"][0]
    print("A / C = %.2f;  A3 / C = %.2f;  A3 / A = %.2f (3 separate calls: 3.00);  D / C = %.2f;  B / A = %.1f"
          % (st["A median"][0] / c, st["A3 pct"][0] / c, st["A3 pct"][0] / st["A median"][0], st["D cols"][0] / c,
             st["B map"][0] / st["A median"][0]), flush=True)
    print("A reads the array's %.3f GB in %.3f ms: %.2f TB/s  (C: %.2f TB/s)"
          % (nbytes / 1e9, st["A median"][0], nbytes / st["A median"][0] / 1e9, nbytes / c / 1e9), flush=True)


if __name__ == "__main__":
    sys.exit(main())
