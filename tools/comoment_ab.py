"""Interleaved timing of corr() against the map() it replaces and against std().

    timeout -k 10 600 python tools/comoment_ab.py --layout c2_rows [--rounds 9] [--warmup 2]

One process per layout (run each under its own `timeout`).  The array is made
once in HBM; every timed call runs on a fresh array object over the same buffer,
in rounds that take the variants in turn, each between two hipEvents on torch's
stream (every call ends with the synchronise of its host result, so a span is
the call's time on the device and the host):
  A   s.corr(y, axis) with one signal
  A4  s.corr(y4, axis) with four signals: one read serves them all
  B   s.map(lambda v: ...) of the same arithmetic, the only way to do it on the
      device before corr() (rows layouts only: the reduced axis must be the
      record); float32 arithmetic
  C   the baseline: s.std(axis) over the same buffer with moment states off
      (BOLT_AMD_KEEP_MOMENTS=0, BOLT_AMD_FUSE_SWAP_MOMENTS=0, set here), so it
      reads the array: the existing reduction on exactly the bytes A must read
  F   bm_comoment_combine alone on a state of the result's size: what A
      launches beyond its one read
  S   bm_comoment_state alone, the signal already in HBM (S4: four signals):
      A without its host work, the signal's upload and the finish
Before timing, A and A4 are checked against the float128 truth on a sample of
records with the tests' tolerance, and B against A.  Prints medians with
min-max, A / C, A4 / A and the bytes A reads per second against the 8 TB/s peak,
then by the host clock what A, S, F, the signal's checks and its upload (page-locked
and pageable) take alone.

Layouts: c2_rows     float32 (512, 512, 2000) after swap, axis 2 (rows of 2000 at a pitch of 2048)
         c2_cols     the same data unswapped, (2000, 512, 512), axis 0 (columns)
         small_*     the same at a fraction of the size (a quick check of the tool)
"""
import argparse
import os
import sys

os.environ["BOLT_AMD_KEEP_MOMENTS"] = "0"
os.environ["BOLT_AMD_FUSE_SWAP_MOMENTS"] = "0"

import numpy as np  # noqa: E402

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
    from bolt_amd.mi355x._ops import backend_for
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
    R, nout = shape[0], int(np.prod(shape[1:]))
    rng = np.random.default_rng(2)
    y4 = rng.standard_normal((4, R)) + np.linspace(0, 3, R)
    y1 = y4[0]
    yc = y1 - y1.mean()
    yd = torch.as_tensor(yc, dtype=torch.float32, device=dev)
    m2y = float((yc * yc).sum())

    def fresh():
        """A new array object over base's buffer (B compacts a padded one: that is part of its cost)."""
        if padded:
            return base._derive_padded(d["_pbuf"], d["_pitch"], base._shape, base._split)
        return base._derive(d["_data"], base._shape, base._split)

    def run_a():
        return fresh().corr(y1, axis=axis)

    def run_a4():
        return fresh().corr(y4, axis=axis)

    def run_b():
        def r(v):
            dv = v - v.mean()
            return (dv * yd).sum() / torch.sqrt((dv * dv).sum() * m2y)
        return fresh().map(r, axis=keys)

    def run_c():
        return fresh().std(axis=axis)

    state = _empty(3 * nout * 8, dev).zero_()
    fout = _empty(nout * 4, dev)

    def run_f():
        be.comoment_combine(_lib.CO_CORR, state, [R], [0.0], [m2y], nout, 1, fout, _lib.BM_F32)

    from bolt_amd.mi355x._ops import dtype_code
    code = dtype_code(np.float32)
    O_, R_, I_, P_ = (nout, R, 1, d["_pitch"] if padded else R) if swap else (1, R, nout, R)
    ydev1 = torch.as_tensor(y1, dtype=torch.float64, device=dev)
    ydev4 = torch.as_tensor(y4.reshape(-1), dtype=torch.float64, device=dev)
    state4 = _empty(6 * nout * 8, dev)

    def run_s():
        be.comoment_state(buf, code, O_, R_, I_, P_, ydev1, [float(y1.mean())], [0.0], state)

    def run_s4():
        be.comoment_state(buf, code, O_, R_, I_, P_, ydev4, [float(v) for v in y4.mean(axis=1)], [0.0] * 4, state4)

    variants = [("A corr", run_a), ("A4 corr", run_a4), ("C std", run_c), ("F finish", run_f),
                ("S state", run_s), ("S4 state", run_s4)]
    if swap:
        variants.insert(2, ("B map", run_b))

    # ---- checks before timing
    ra, ra4 = np.asarray(run_a()), np.asarray(run_a4())
    assert ra4.shape == (4,) + ra.shape and ra4[0].tobytes() == ra.tobytes(), "plane 0 of A4 is not A"
    idx = np.linspace(0, nout - 1, 64).astype(np.int64)
    if swap:
        rows = base._elements() if padded else base._elements((nout, R))
        x = rows[torch.as_tensor(idx, device=dev)].cpu().numpy()[:, :R]
    else:
        x = base._elements((R, nout))[:, torch.as_tensor(idx, device=dev)].cpu().numpy().T
    v = x.astype(np.longdouble)
    dx = v - v.mean(axis=1, keepdims=True)
    fi = np.finfo(np.float32)
    worst = 0.0
    for k in range(4):
        w = y4[k].astype(np.longdouble)
        dy = w - w.mean()
        sx, sy = np.sqrt((dx * dx).mean(axis=1)), np.sqrt((dy * dy).mean())
        truth = (dx * dy).mean(axis=1) / (sx * sy)
        bound = 2 * fi.eps * np.abs(truth) + 1e-12 * (np.abs(v).max(axis=1) / sx + np.abs(w).max() / sy) \
            + fi.smallest_subnormal
        err = np.abs(ra4[k].reshape(-1)[idx].astype(np.longdouble) - truth)
        worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound), "corr misses the tolerance"
    print("A4 against the float128 truth on 64 records x 4 signals: max error / bound = %.3g" % worst, flush=True)
    if swap:
        rb = run_b()
        gb = np.asarray(rb.toarray()).reshape(-1)[idx]
        off = float(np.abs(gb.astype(np.float64) - ra.reshape(-1)[idx]).max())
        # (B's arithmetic is float32 throughout: a check that both do the same operation, not of A's accuracy)
        print("B against A: max |B - A| = %.3g" % off, flush=True)
        assert off <= 1e-2, "map() and corr() disagree"
        del rb
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
    am = stats["A corr"][0]
    a4 = stats["A4 corr"][0]
    cm, cl, ch = stats["C std"]
    fm = stats["F finish"][0]
    read = buf.numel() if padded else nbytes
    print("A / C = %.3f;  A - C = %.3f ms against C's spread %.3f + F %.3f -> %s"
          % (am / cm, am - cm, ch - cl, fm, "within" if am - cm <= (ch - cl) + fm else "MISSES the goal"), flush=True)
    print("A4 / A = %.3f (4 separate calls: 4.000)" % (a4 / am), flush=True)
    print("A reads %.3f GB (the array's %.3f) in %.3f ms: %.2f TB/s = %.3f of 8 TB/s  (C: %.3f of 8 TB/s)"
          % (read / 1e9, nbytes / 1e9, am, nbytes / am / 1e9, nbytes / (am * 1e-3) / PEAK,
             nbytes / (cm * 1e-3) / PEAK), flush=True)
    if swap:
        bm = stats["B map"][0]
        print("B / A = %.1f" % (bm / am), flush=True)

    # ---- what A's host path costs, by the host clock (medians of 20, the device drained around each)
    import time
    from bolt_amd.mi355x import reduction

    def wall(fn):
        ts = []
        for _ in range(20):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts))
    yk = y1.reshape(1, -1)
    print("host clock: A %.3f ms, S %.3f, F %.3f; signal checks + centring %.3f; upload page-locked %.3f, pageable %.3f"
          % (wall(run_a), wall(run_s), wall(run_f),
             wall(lambda: (np.isfinite(np.ascontiguousarray(y1, dtype=np.float64)).all(), reduction.signal_centre(yk))),
             wall(lambda: torch.from_numpy(y1).pin_memory().to(dev, non_blocking=True)),
             wall(lambda: torch.from_numpy(y1).to(dev))), flush=True)


if __name__ == "__main__":
    sys.exit(main())
