"""Shared by test_zzzzzzz_rows_matrix: every instantiation of the four kernel
families that hold a record in registers -- k_std_rows (bm_standardize.hip),
k_detrend_rows (bm_detrend.hip), k_norm_rows and k_q_rows (bm_quantile.hip) --
stated in Python, the case tables that reach each of them, and the plumbing
that drives the backend entry points on raw buffers and checks what they leave.

The census.  A launch picks its kernel by element type (bm_host.h: for_dtype,
bool through the uint8 kernels), by vector width (pick_vec / for_vec: the
widest power of two of at most 16 B and 8 elements that divides R and every
pitch and fits every pointer) and by plan (one wave per row up to 64 x what a
thread holds, min(8 vec, 32) elements; one block per row up to 256 x that,
with 256 rows or more).  stated() lists them: 35 (type, vec) pairs x 2 plans
for the three families that write rows, 13 (width, vec) pairs x 2 for
k_q_rows, which is built per key width.  pick_vec() here is the mirror of the
host's with the pointer terms in (standardize_cases.rows_vec assumes aligned
buffers); launch_rows() and launch_quantile() work the instantiation of every
call out from the call's own arguments -- R, the pitches, data_ptr() % 16 --
and record it.

Shapes.  With NV = lane_vecs(vec): wave per row R = 64 vec (NV - 1) + 5 vec,
37 rows; block per row R = 256 vec (NV - 1) + 5 vec, 261 rows.  R / vec is odd,
which pins the vector below the type's cap.  At the limits (R = 64 x held and
256 x held, every slot full) R is a multiple of every vector, so a narrower one
is pinned by the source pitch there (base + vec elements); R = 256 x held + vec
must be refused with dst untouched.  Everywhere else the pitches are multiples
of 16 elements, larger than R and different for src and dst.

Why the vector narrowed.  For uint8, float16, float32 and float64, at an R
that allows the widest vector, every narrower one is forced by the source
pitch, the destination pitch, a source offset and a destination offset of one
narrower vector.  One combination does not exist: uint8's results are float64,
whose stores are 16-B pieces for every vector of two or more, so a destination
offset of 4 or 2 results (32 / 16 B) narrows nothing; only the offset of one
result (vector 1) is in the table.

Values.  Floats 10 + 3 N(0, 1); integers uniform over the whole range of the
type with its minimum and maximum in every row (uint64 rows therefore straddle
2^63); bool 0 / 1.  The float64 numpy executors stay inside the project's
bounds on these values at every case, so no range is narrowed.

Truths and bounds are the project's own, unchanged: standardize_cases.
truth_and_bound, detrend_cases.truth_and_bound, normalize_cases.
mean_truth_and_bound and percentile_truth, quantile_cases.truth / same /
numpy_f64_bound -- longdouble from the raw integers where a bound is met,
the float64 restatement where the result is exact.
"""
import collections
import zlib

import numpy as np

import detrend_cases as D
import normalize_cases as N
import quantile_cases as Q
import standardize_cases as S

TYPES = ("uint8", "int8", "uint16", "int16", "uint32", "int32", "uint64", "int64", "float16", "float32", "float64")
VECS = {1: (1, 2, 4, 8), 2: (1, 2, 4, 8), 4: (1, 2, 4), 8: (1, 2)}
PLANS = ("wave", "block")
ROWS = {"wave": 37, "block": 261}
WAVES = {"wave": 64, "block": 256}  # threads a row is spread over
FAMILIES = ("std", "detrend", "norm", "quantile")
NARROW_TYPES = ("uint8", "float16", "float32", "float64")  # one per item size
WAYS = ("src_pitch", "dst_pitch", "src_ptr", "dst_ptr")
OFFSET = 0.1   # normalize()'s offset, as the existing tests use it
PERC = 20
FILL = 0xA5    # dst before a call, and its guards
GUARD = 4096


def kernel_type(dtype):
    """The element type whose kernels serve ``dtype`` (for_dtype)."""
    dt = np.dtype(dtype)
    return "uint8" if dt == np.bool_ else dt.name


def lane_vecs(vec):
    return 8 if vec * 8 <= 32 else 32 // vec


def held(vec):
    """Elements a thread holds."""
    return vec * lane_vecs(vec)


def pick_vec(es, whole, ptrs):
    """bm_host.h's pick_vec under the rows kernels' cap: ``whole`` the extents
    and pitches in elements, ``ptrs`` (address mod 16, element size) pairs."""
    vec = min(16 // es, 8)
    while vec > 1:
        if all(n % vec == 0 for n in whole) and all(p % min(16, vec * e) == 0 for p, e in ptrs):
            break
        vec >>= 1
    return vec


def plan_of(vec, O, R):
    if R <= 64 * held(vec):
        return "wave"
    if R <= 256 * held(vec) and O >= S.BLOCK_MIN_ROWS:
        return "block"
    return None


def stated(family):
    """The instantiations of a family: (type or key width, vec, plan)."""
    if family == "quantile":
        return {(es, v, p) for es in VECS for v in VECS[es] for p in PLANS}
    return {(t, v, p) for t in TYPES for v in VECS[np.dtype(t).itemsize] for p in PLANS}


# ------------------------------------------------------------------ cases --
# soff / doff: bytes the source / destination start past a 16-B boundary
Case = collections.namedtuple("Case", "kind dtype O R sp dp soff doff vec plan")


def _pitches(R):
    base = -(-R // 16) * 16
    return base + 16, base + 48


def _case(kind, dtype, O, R, sp=None, dp=None, soff=0, doff=0):
    dt = np.dtype(dtype)
    psp, pdp = _pitches(R)
    sp, dp = psp if sp is None else sp, pdp if dp is None else dp
    vec = pick_vec(dt.itemsize, (R, sp, dp), ((soff % 16, dt.itemsize), (doff % 16, S.out_dtype(dt).itemsize)))
    return Case(kind, dt.name, O, R, sp, dp, soff, doff, vec, plan_of(vec, O, R))


def matrix_cases(dtype, plan):
    """One case per vector of the type: every slot but the last full, the last held by 5 lanes."""
    es, W, O = np.dtype(dtype).itemsize, WAVES[plan], ROWS[plan]
    out = []
    for v in VECS[es]:
        c = _case("matrix", dtype, O, W * v * (lane_vecs(v) - 1) + 5 * v)
        assert (c.vec, c.plan) == (v, plan), c
        out.append(c)
    return out


def limit_cases(dtype, plan):
    """R = 64 x held (wave) or 256 x held (block) exactly, per vector, the
    narrower vectors pinned by the source pitch; block: also R = 256 x held +
    vec, which no kernel takes."""
    es, W, O = np.dtype(dtype).itemsize, WAVES[plan], ROWS[plan]
    cap, out = VECS[es][-1], []
    for v in VECS[es]:
        R = W * held(v)
        c = _case("limit", dtype, O, R, sp=_pitches(R)[0] + (v if v < cap else 0))
        assert (c.vec, c.plan) == (v, plan), c
        out.append(c)
        if plan == "block":
            c = _case("over", dtype, O, R + v)
            assert (c.vec, c.plan) == (v, None), c
            out.append(c)
    return out


def narrow_cases(dtype, plan):
    """[(aligned case, [(way, case), ...]), ...]: per narrower vector v an R
    that allows the widest vector and fits ``plan`` at v, aligned and with v
    forced each of the four ways."""
    dt = np.dtype(dtype)
    es, oes, W, O = dt.itemsize, S.out_dtype(dt).itemsize, WAVES[plan], ROWS[plan]
    cap, out = VECS[es][-1], []
    for v in VECS[es][:-1]:
        R = W * v * (lane_vecs(v) - 1) + 5 * cap
        sp, dp = _pitches(R)
        aligned = _case("aligned", dtype, O, R)
        assert aligned.vec == cap and aligned.plan is not None, aligned
        ways = []
        for way, kw in (("src_pitch", dict(sp=sp + v)), ("dst_pitch", dict(dp=dp + v)),
                        ("src_ptr", dict(soff=v * es)), ("dst_ptr", dict(doff=v * oes))):
            if way == "dst_ptr" and (v * oes) % 16 == 0:
                continue  # (uint8 -> float64 at v = 4, 2: see the module's docstring)
            c = _case(way, dtype, O, R, **kw)
            assert (c.vec, c.plan) == (v, plan), c
            ways.append((way, c))
        out.append((aligned, ways))
    return out


_DATA = {}


def data(dtype, O, R):
    """O distinct rows of R values of ``dtype`` (see the module's docstring); the
    same array for the same arguments until fresh() drops it, never written to."""
    key = (np.dtype(dtype).name, O, R)
    if key not in _DATA:
        _DATA[key] = _data(*key)
        _DATA[key].setflags(write=False)
    return _DATA[key]


def _data(dtype, O, R):
    dt = np.dtype(dtype)
    rng = np.random.default_rng(zlib.crc32(("%s %d %d" % (dt.name, O, R)).encode()))
    if dt == np.bool_:
        return rng.integers(0, 2, size=(O, R)).astype(bool)
    if dt.kind == "f":
        return (10 + 3 * rng.standard_normal((O, R))).astype(dt)
    info = np.iinfo(dt)
    x = rng.integers(info.min, info.max, size=(O, R), dtype=dt, endpoint=True)
    rows = np.arange(O)
    lo = (3 * rows + 1) % R
    hi = (lo + 1 + (5 * rows) % (R - 2)) % R   # (never lo's column)
    x[rows, lo] = info.min
    x[rows, hi] = info.max
    if dt == np.uint64:
        assert ((x >> np.uint64(63)).sum(axis=1) > 0).all() and ((x >> np.uint64(63)) == 0).any(axis=1).all()
    return x


def frac0_perc(R):
    """A percentile well inside the row whose position (perc / 100)(R - 1) is a whole rank."""
    for k in range((R - 1) // 3, R):
        perc = 100.0 * k / (R - 1)
        if 0 < k < R - 1 and Q.position(np.float64(perc) / 100, R)[2] == 0.0:
            return perc
    return 0.0


# -------------------------------------------------------------- executors --
CENSUS = {}   # executor name -> family -> {(type or width, vec, plan)}
RATIOS = {}   # executor name -> family -> worst error / bound
RAN = {}      # executor name -> launches


class Executor(object):
    """The entry points of one executor ('cpu': the float64 numpy executors of
    normalize_cases and detrend_cases; 'gpu': the HIP backend) and its buffers."""

    def __init__(self, name):
        import torch
        import cpu_backend as C
        self.name = name
        if name == "gpu":
            from bolt_amd.mi355x._ops import backend_for
            self.device = torch.device("cuda:0")
            be = backend_for(self.device)
            assert type(be).__name__ == "HipBackend", type(be)  # (no test executor left on 'cuda')
            self.be = dict.fromkeys(FAMILIES, be)
        else:
            self.device = torch.device("cpu")
            n, d = N.fused_backend(), D.fused_backend()
            self.be = {"std": n, "norm": n, "quantile": n, "detrend": d}
        self.code = lambda dt: C._CODES.index(np.dtype(dt).type)
        CENSUS.setdefault(name, {f: set() for f in FAMILIES})
        RATIOS.setdefault(name, {f: 0.0 for f in FAMILIES})
        RAN.setdefault(name, 0)

    def _bytes(self, n, off, fill=None):
        """A uint8 tensor of n bytes that starts ``off`` bytes past a 16-B boundary, inside its own allocation."""
        import torch
        whole = torch.empty(n + off + 32, dtype=torch.uint8, device=self.device)
        if fill is not None:
            whole.fill_(fill)
        at = (-whole.data_ptr()) % 16 + off
        t = whole[at:at + n]
        assert t.data_ptr() % 16 == off % 16
        return whole, t, at

    def source(self, x, sp, soff):
        """x's rows ``sp`` elements apart, the pad columns all-ones bytes (a NaN, or the type's largest)."""
        import torch
        O, R = x.shape
        h = np.full(O * sp * x.dtype.itemsize, 0xFF, dtype=np.uint8)
        h.view(np.uint8 if x.dtype == np.bool_ else x.dtype).reshape(O, sp)[:, :R] = x.view(np.uint8) \
            if x.dtype == np.bool_ else x
        _, t, _ = self._bytes(h.size, soff)
        t.copy_(torch.from_numpy(h))
        return t

    def target(self, nbytes, doff):
        """(whole buffer, the nbytes at GUARD + doff of it, their offset): all FILL."""
        whole, t, at = self._bytes(2 * GUARD + nbytes, doff, FILL)
        return whole, t[GUARD:GUARD + nbytes], at + GUARD

    def host(self, t):
        if self.name == "gpu":
            import torch
            torch.cuda.synchronize()
        return t.cpu().numpy()


def _note(ex, family, key, vec, plan):
    RAN[ex.name] += 1
    if plan is not None:
        CENSUS[ex.name][family].add((key, vec, plan))


def _rows_out(ex, whole, at, c, odt):
    """The (O, R) result of a rows launch; everything else of the buffer must hold FILL."""
    h = ex.host(whole)
    row = c.dp * odt.itemsize
    keep = np.ones(h.size, dtype=bool)
    keep[at:at + c.O * row].reshape(c.O, row)[:, :c.R * odt.itemsize] = False
    assert (h[keep] == FILL).all(), ("pad columns or guards written", c)
    return h[at:at + c.O * row].copy().view(odt).reshape(c.O, c.dp)[:, :c.R]


def launch_rows(ex, c, src, family, call):
    """One launch of a family that writes rows: ``call(be, code, dst, out code)``
    -> the backend's ``taken``.  Records the instantiation worked out from the
    real arguments, holds it to the case's, and returns the (O, R) result --
    None where the rows are not taken, dst then untouched."""
    dt = np.dtype(c.dtype)
    odt = S.out_dtype(dt)
    whole, dst, at = ex.target(c.O * c.dp * odt.itemsize, c.doff)
    vec = pick_vec(dt.itemsize, (c.R, c.sp, c.dp),
                   ((src.data_ptr() % 16, dt.itemsize), (dst.data_ptr() % 16, odt.itemsize)))
    plan = plan_of(vec, c.O, c.R)
    assert (vec, plan) == (c.vec, c.plan), (c, vec, plan)
    taken = call(ex.be[family], ex.code(dt), dst, ex.code(odt))
    _note(ex, family, kernel_type(dt), vec, plan)
    assert taken == (plan is not None), (family, c, taken)
    if not taken:
        assert (ex.host(whole) == FILL).all(), ("rows not taken, dst written", family, c)
        return None
    return _rows_out(ex, whole, at, c, odt)


def launch_quantile(ex, c, src, ranks, frac, odt):
    """bm_quantile_rows -> the (len(ranks), O) planes, or None where the rows are not taken."""
    dt = np.dtype(c.dtype)
    n = len(ranks) * c.O * odt.itemsize
    whole, out, at = ex.target(n, 0)
    vec = pick_vec(dt.itemsize, (c.R, c.sp), ((src.data_ptr() % 16, dt.itemsize),))
    plan = plan_of(vec, c.O, c.R)
    assert (vec, plan) == (c.vec, c.plan), (c, vec, plan)
    taken = ex.be["quantile"].quantile_rows(src, ex.code(dt), c.O, c.R, c.sp, list(ranks), list(frac), out,
                                            ex.code(odt))
    _note(ex, "quantile", dt.itemsize, vec, plan)
    assert taken == (plan is not None), (c, taken)
    h = ex.host(whole)
    if not taken:
        assert (h == FILL).all(), ("rows not taken, planes written", c)
        return None
    assert (h[:at] == FILL).all() and (h[at + n:] == FILL).all(), ("guards written", c)
    return h[at:at + n].copy().view(odt).reshape(len(ranks), c.O)


# ----------------------------------------------------------------- checks --
_TRUTHS = {}
_GROUP = [None]


def fresh(group):
    """At a test's start: drop the inputs and truths of the group of cases
    before, unless this test runs the same group (on the next executor)."""
    if _GROUP[0] != group:
        _GROUP[0] = group
        _DATA.clear()
        _TRUTHS.clear()
        D._TRUTHS.clear()


def _key(x, op):
    return (x.dtype.str, x.shape, op, zlib.crc32(np.ascontiguousarray(x).tobytes()))


def bound_of(x, op):
    """The bound of an operation run_case has checked on ``x``."""
    return _TRUTHS[_key(x, op)][1]


def _truth(x, op, make):
    key = _key(x, op)
    hit = _TRUTHS.get(key)
    if hit is None:
        hit = _TRUTHS[key] = make()
    return hit


def within(ex, family, got, x, t, bound, tag):
    """|got - t| <= bound everywhere; prints the worst error / bound ratio first and keeps the family's worst."""
    assert got.dtype == S.out_dtype(x.dtype) and got.shape == x.shape, (tag, got.dtype, got.shape)
    assert np.isfinite(t).all(), tag
    err = np.abs(got.astype(np.longdouble) - t)
    ratio = float((err / bound).max())
    print("%s %s: max error / bound = %.3g" % (ex.name, tag, ratio))
    RATIOS[ex.name][family] = max(RATIOS[ex.name][family], ratio)
    assert np.all(err <= bound), (tag, ratio)


def exact(got, want, tag):
    assert got.dtype == want.dtype and got.shape == want.shape, (tag, got.dtype, got.shape, want.dtype, want.shape)
    if not Q.same(got, want):
        bad = np.flatnonzero(~((got == want) | ((got != got) & (want != want))).reshape(-1))
        raise AssertionError("%s: %d of %d differ, first at %d: got %r, want %r"
                             % (tag, bad.size, want.size, bad[0], got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]]))


def run_case(ex, c, x, orders=(1, 8), quantiles=True):
    """Every operation of one case on one executor, each checked against the
    project's truth -> {operation: result} (None where the rows are not taken)."""
    dt = np.dtype(c.dtype)
    odt = S.out_dtype(dt)
    O, R, sp, dp = c.O, c.R, c.sp, c.dp
    tag = "%s %s vec %d %s (%d, %d)" % (c.dtype, c.kind, c.vec, c.plan, O, R)
    src = ex.source(x, sp, c.soff)
    res = {}

    for scale in (0, 1):
        op = ("center", "zscore")[scale]
        got = res[op] = launch_rows(ex, c, src, "std", lambda be, code, dst, ocode: be.standardize_rows(
            src, code, O, R, sp, dst, ocode, dp, scale))
        if got is not None:
            t, bound = _truth(x, op, lambda: S.truth_and_bound(x, 1, scale))
            within(ex, "std", got, x, t, bound, "%s %s" % (tag, op))

    got = res["mean"] = launch_rows(ex, c, src, "std", lambda be, code, dst, ocode: be.normalize_rows(
        src, code, O, R, sp, N.NORM_MEAN, 0, 0.0, OFFSET, dst, ocode, dp))
    if got is not None:
        t, bound = _truth(x, "mean", lambda: N.mean_truth_and_bound(x, 1, OFFSET))
        within(ex, "std", got, x, t, bound, "%s normalize mean" % tag)

    # perc 20, one perc at a whole rank, and where 20 is at one too (R - 1 a multiple of 5) one that is not
    percs = [PERC, frac0_perc(R)]
    if Q.position(np.float64(PERC) / 100, R)[2] == 0.0:
        percs.append(100 * Q.QG)
    fracs = [Q.position(np.float64(p) / 100, R)[2] for p in percs]
    assert fracs[1] == 0.0 and (fracs[0] != 0.0 or fracs[2] != 0.0), (R, percs, fracs)
    for perc in percs:
        rank, _, g = Q.position(np.float64(perc) / 100, R)
        got = res["perc", perc] = launch_rows(ex, c, src, "norm", lambda be, code, dst, ocode: be.normalize_rows(
            src, code, O, R, sp, N.NORM_RANK, rank, g, OFFSET, dst, ocode, dp))
        if got is not None:
            want = _truth(x, ("perc", perc), lambda: N.percentile_truth(x, 1, perc, OFFSET))
            exact(got, want, "%s normalize percentile %r" % (tag, perc))

    for order in orders:
        got = res["detrend", order] = launch_rows(ex, c, src, "detrend", lambda be, code, dst, ocode: be.detrend_rows(
            src, code, O, R, sp, order, dst, ocode, dp))
        if got is not None:
            t, bound = _truth(x, ("detrend", order), lambda: D.truth_and_bound(x, 1, order))
            within(ex, "detrend", got, x, t, bound, "%s detrend order %d" % (tag, order))

    if quantiles:
        pos = [Q.position(q, R) for q in Q.QS]
        assert pos[-1][2] != 0.0 and len(pos) + sum(1 for p in pos if p[2] != 0.0) <= Q.MAX_RANKS
        got = res["quantile"] = launch_quantile(ex, c, src, [p[0] for p in pos], [p[2] for p in pos], odt)
        if got is not None:
            for k, q in enumerate(Q.QS):
                qtag = "%s quantile %r" % (tag, q)
                exact(got[k], Q.truth(x, q, 1, "linear"), qtag)
                if odt == np.float64:
                    ref, bound = Q.numpy_f64_bound(x, q, 1)
                    ok = np.isfinite(bound) & np.isfinite(ref)
                    err = np.abs(got[k] - ref)[ok]
                    ratio = float((err / bound[ok]).max()) if err.size else 0.0
                    print("%s %s: max |got - np.quantile| / bound = %.3g" % (ex.name, qtag, ratio))
                    RATIOS[ex.name]["quantile"] = max(RATIOS[ex.name]["quantile"], ratio)
                    assert np.all(err <= bound[ok]), qtag
        # the elements themselves where the position is a whole rank
        whole = [(q, p[0]) for q, p in zip(Q.QS, pos) if p[2] == 0.0]
        assert len(whole) >= 2
        got = res["elements"] = launch_quantile(ex, c, src, [r for _, r in whole], [0.0] * len(whole), dt)
        if got is not None:
            for k, (q, _) in enumerate(whole):
                exact(got[k], Q.truth(x, q, 1, "lower"), "%s element at q=%r" % (tag, q))
    return res
