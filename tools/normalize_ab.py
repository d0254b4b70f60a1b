"""Interleaved timing of normalize() against the calls it fuses and the map()
it replaces.

    timeout -k 10 900 python tools/normalize_ab.py [--size c2|small] [--rounds 9] [--warmup 2] [--placements 2] [--no-map]

One process.  C2's array, float32 (2000, 512, 512), is made in HBM and swapped
to (512, 512, 2000): rows of 2000 at a pitch of 2048 elements (8192 B).  Every
timed call runs on a fresh array object over the same buffers, in rounds that
take the variants in turn, each between two hipEvents on torch's stream.  The
whole is repeated over several placements: the arrays are made anew behind a
spacer of another size, so that they lie elsewhere in HBM.
  N   s.normalize(axis=2, perc=20): bm_normalize_rows, one read and one write
  Nm  s.normalize(axis=2, method='mean'): the same with the mean baseline
  A   s.percentile(20, axis=2) alone: the baseline, one read (a host result)
  Z   s.zscore(axis=2) alone: one read and one write
  M   the map() route: s.map(v -> (v - q) / (q + 0.1), q = v.quantile(0.2));
      timed in every round only when one call takes under 2 s, else once per
      placement
  D   x.normalize(axis=0, perc=20) of the unswapped (2000, 512, 512): the
      columns route (permute, quantile rows, the baseline plane, the apply)
Moment states are off (BOLT_AMD_KEEP_MOMENTS=0, BOLT_AMD_FUSE_SWAP_MOMENTS=0,
set here).  Before timing, N is checked bit for bit against the numpy
restatement on a sample of records and within float32 rounding against the
two-call route (percentile(), then the arithmetic on its rounded float32
baseline), Nm against numpy, D bit for bit against N on the device, and M
against N.  Prints, per placement and over all, medians with min-max, N against
A + Z (the structural condition: N < A + Z) and how far N lands above A.
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
PERC, OFFSET = 20, 0.1


def summary(ts):
    a = np.asarray(ts)
    return float(np.median(a)), float(a.min()), float(a.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="c2", choices=sorted(SIZES))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--placements", type=int, default=2)
    ap.add_argument("--no-map", action="store_true", help="leave M out")
    a = ap.parse_args()
    assert a.rounds >= 5 and a.warmup >= 2 and 1 <= a.placements <= len(SPACERS)
    import torch
    import bolt_amd as bolt
    shape = SIZES[a.size]
    dev = torch.device("cuda:0")
    ctx = bolt.MI355XContext(device="cuda:0")
    nbytes = int(np.prod(shape)) * 4
    R, nout = shape[0], int(np.prod(shape[1:]))
    order = ("N norm", "Nm mean", "A pct", "Z zscore", "M map", "D cols")
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
            """A new array object over base's buffer (M compacts a padded one: that is part of its cost)."""
            if padded:
                return base._derive_padded(d["_pbuf"], d["_pitch"], base._shape, base._split)
            return base._derive(d["_data"], base._shape, base._split)

        def run_n():
            return fresh().normalize(axis=2, perc=PERC, offset=OFFSET)

        def run_nm():
            return fresh().normalize(axis=2, method="mean", offset=OFFSET)

        def run_a():
            return fresh().percentile(PERC, axis=2)

        def run_z():
            return fresh().zscore(axis=2)

        def dff(v):
            q = v.quantile(PERC / 100.0)
            return (v - q) / (q + OFFSET)

        def run_m():
            return fresh().map(dff, axis=keys)

        def run_d():
            return cols._derive(dc["_data"], cols._shape, cols._split).normalize(axis=0, perc=PERC, offset=OFFSET)

        def rows_of(arr):
            """(nout, >= R) device tensor of a (.., .., R) result's rows."""
            return arr._elements() if "_pbuf" in arr.__dict__ else arr._elements((nout, R))

        # ---- checks before timing
        idx = np.linspace(0, nout - 1, 64).astype(np.int64)
        tidx = torch.as_tensor(idx, device=dev)
        x = rows_of(base)[tidx].cpu().numpy()[:, :R]
        x64 = x.astype(np.float64)
        srt = np.sort(x, axis=1).astype(np.float64)
        pos = np.float64(PERC) / 100 * (R - 1)
        fl = int(np.floor(pos))
        gfr = float(pos - fl)
        bl = srt[:, fl] + (srt[:, fl + 1] - srt[:, fl]) * gfr if gfr != 0.0 else srt[:, fl]
        want = ((x64 - bl[:, None]) / (bl[:, None] + OFFSET)).astype(np.float32)
        rn = run_n()
        assert rn.shape == base.shape and rn.dtype == np.float32 and ("_pbuf" in rn.__dict__) == padded
        got = rows_of(rn)[tidx].cpu().numpy()[:, :R]
        assert np.array_equal(got, want), "normalize() is not the numpy restatement on the sampled records"
        f0 = np.asarray(run_a()).reshape(-1)[idx].astype(np.float64)   # the two-call route: a float32 baseline
        two = ((x64 - f0[:, None]) / (f0[:, None] + OFFSET)).astype(np.float32)
        tol = 4 * np.finfo(np.float32).eps * (1 + np.abs(want)) * (np.abs(x64).max() / np.abs(bl + OFFSET).min())
        assert np.all(np.abs(got.astype(np.float64) - two) <= tol), "normalize() and the two-call route disagree"
        m = x64.mean(axis=1, keepdims=True)
        gm = rows_of(run_nm())[tidx].cpu().numpy()[:, :R]
        assert np.allclose(gm, (x64 - m) / (m + OFFSET), rtol=1e-6, atol=1e-9), "the mean baseline disagrees with numpy"
        rd = run_d()
        assert rd.shape == cols.shape and torch.equal(rd._elements((R, nout)).t(), rows_of(rn)[:, :R]), \
            "the columns route disagrees with the rows"
        del rd
        m_once, m_rounds = float("nan"), False
        if not a.no_map:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rm = run_m()
            torch.cuda.synchronize()
            m_once = (time.perf_counter() - t0) * 1e3
            gmap = rows_of(rm)[tidx].cpu().numpy()[:, :R]
            assert np.allclose(gmap, want, rtol=1e-3, atol=1e-5), "map() and normalize() disagree"
            del rm
            m_rounds = m_once < 2000.0
        del rn
        print("checks passed (64 records bit for bit against numpy; the two-call route within float32 rounding; "
              "D == N); M's first call %.1f ms%s"
              % (m_once, "" if m_rounds else ": timed once per placement only"), flush=True)

        variants = [("N norm", run_n), ("Nm mean", run_nm), ("A pct", run_a), ("Z zscore", run_z), ("D cols", run_d)]
        if m_rounds:
            variants.insert(4, ("M map", run_m))
        times = dict((tag, []) for tag, _ in variants)
        if not m_rounds:
            times["M map"] = [m_once]
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
        del base, cols, d, dc, spacer
        torch.cuda.empty_cache()

    print("all placements:", flush=True)
    st = {}
    for tag in order:
        med, lo, hi = st[tag] = summary(total[tag])
        print("  %-9s median %9.3f ms  min %9.3f  max %9.3f  (%d spans)" % (tag, med, lo, hi, len(total[tag])),
              flush=True)
    n, pa, z = st["N norm"][0], st["A pct"][0], st["Z zscore"][0]
    print("N = %.3f ms against A + Z = %.3f ms (%s);  N - A = %.3f ms, N / A = %.2f;  Nm / Z = %.2f;  D / N = %.2f;  "
          "M / N = %.1f" % (n, pa + z, "N < A + Z holds" if n < pa + z else "N < A + Z FAILS", n - pa, n / pa,
                            st["Nm mean"][0] / z, st["D cols"][0] / n, st["M map"][0] / n), flush=True)
    print("N reads and writes %.3f GB in %.3f ms: %.2f TB/s  (Z: %.2f TB/s)"
          % (2 * nbytes / 1e9, n, 2 * nbytes / n / 1e9, 2 * nbytes / z / 1e9), flush=True)
    return 0 if n < pa + z else 1


if __name__ == "__main__":
    sys.exit(main())
