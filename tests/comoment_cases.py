"""Shared by the cov() / corr() tests: the float128 truth and the tolerance,
the data, and a numpy executor with bm_comoment_state / bm_comoment_combine, so
the orchestration the HIP backend takes (pitches, dropped pad columns, K
planes, rank parts) runs on the CPU.
"""
import numpy as np

import cpu_backend as C
from standardize_cases import axes_of, out_dtype, rand  # noqa: F401  (rand: the records' data)

METHODS = ("cov", "corr")
CO_COV, CO_CORR = 0, 1
MAX_SIGNALS = 4  # BM_COMOMENT_MAX_SIGNALS: more signals run in batches


def signals(x, axis, seed=0, k=None):
    """The two signals of a case -- noise, and 0.3 * the first record + noise
    so that r is away from 0 -- or ``k`` of them alternating, shaped
    (k,) + the reduced extents."""
    ax = tuple(sorted(axes_of(x, axis)))
    rshape = tuple(x.shape[a] for a in ax)
    rng = np.random.default_rng(100 + seed)
    kept = [i for i in range(x.ndim) if i not in ax]
    with np.errstate(all="ignore"):
        first = np.transpose(x.astype(np.float64), kept + list(ax)).reshape((-1,) + rshape)[0] if x.size else \
            np.zeros(rshape)
    out = []
    for j in range(2 if k is None else k):
        noise = rng.standard_normal(rshape)
        out.append(noise if j % 2 == 0 else 0.3 * np.nan_to_num(first) + noise)
    return np.stack(out) if out else np.zeros((0,) + rshape)


def truth_and_bound(x, y, axis, name):
    """(truth, bound) in longdouble for one signal ``y`` of the reduced extents:
    dx = x - mean(x) over the axes, dy = y - mean(y), cov = mean(dx dy),
    corr = cov / (std_x std_y), and
      corr: |got - truth| <= 2 eps(out) |truth| + 1e-12 (max|x_rec| / std_x + max|y| / std_y) + smallest_subnormal(out)
      cov:  |got - truth| <= 2 eps(out) |truth| + 1e-12 (max|x_rec| std_y + max|y| std_x) + smallest_subnormal(out)
    1e-12 is the project's float64 parity rtol and 2 eps the allowance for the
    final rounding (standardize_cases.truth_and_bound), applied to two inputs."""
    ax = tuple(sorted(axes_of(x, axis)))
    v = x.astype(np.longdouble)
    w = np.asarray(y, dtype=np.float64).astype(np.longdouble).reshape([x.shape[i] if i in ax else 1
                                                                       for i in range(x.ndim)])
    dx = v - v.mean(axis=ax, keepdims=True)
    dy = w - w.mean()
    cov = (dx * dy).mean(axis=ax)
    sx = np.sqrt((dx * dx).mean(axis=ax))
    sy = np.sqrt((dy * dy).mean())
    bx = np.abs(v).max(axis=ax)
    by = np.abs(w).max()
    fi = np.finfo(out_dtype(x.dtype))
    with np.errstate(all="ignore"):
        if name == "corr":
            t = cov / (sx * sy)
            floor = 1e-12 * (bx / sx + by / sy)
        else:
            t = cov
            floor = 1e-12 * (bx * sy + by * sx)
    return t, 2 * np.longdouble(fi.eps) * np.abs(t) + floor + np.longdouble(fi.smallest_subnormal)


def check_values(got, x, y, axis, name, tag=""):
    """``got`` (ndarray or scalar) against the truth for one signal; prints
    the worst error / bound ratio before asserting -> that ratio."""
    t, bound = truth_and_bound(x, y, axis, name)
    got = np.asarray(got)
    if got.ndim == 0 and t.size == 1:
        got = got.reshape(t.shape)  # toscalar() of a one-element result, as the statistics give it
    assert got.dtype == out_dtype(x.dtype), (tag, got.dtype)
    assert got.shape == t.shape, (tag, got.shape, t.shape)
    assert np.isfinite(t).all(), tag  # no zero variance outside the dedicated test
    err = np.abs(got.astype(np.longdouble) - t)
    ratio = float((err / bound).max()) if err.size else 0.0
    print("%s %s: max error / bound = %.3g" % (tag, name, ratio))
    assert np.all(err <= bound), (tag, name, ratio)
    if name == "corr":
        assert np.all(np.abs(got) <= 1), tag
    return ratio


def check_both(b, x, axis, tag="", seed=0):
    """cov and corr of ``b`` against both signals of the case, one call each."""
    ys = signals(x, axis, seed)
    for name in METHODS:
        for j, y in enumerate(ys):
            check_values(_host(getattr(b, name)(y, axis=axis)), x, y, axis, name, "%s signal %d" % (tag, j))


def _host(r):
    """A cov / corr result (BoltArrayLocal or numpy scalar) as an ndarray."""
    return np.asarray(r)


def fused_backend():
    """CpuBackend plus bm_comoment_state / bm_comoment_combine (include/bolt_mi355x.h) in numpy float64."""

    class ComomentCpuBackend(C.CpuBackend):
        def comoment_state(self, src, code, O, R, I, pitch, y, ymean, yresid, state, workspace=None):
            dt = np.dtype(C._CODES[code])
            K = len(ymean)
            assert pitch >= R and (I == 1 or pitch == R) and 1 <= K <= MAX_SIGNALS and len(yresid) == K
            if O == 0 or R == 0 or I == 0:
                return
            a = src.numpy().view(dt)
            if I == 1:
                x = a[:O * pitch].reshape(O, pitch)[:, :R].reshape(O, R, 1)
            else:
                x = a[:O * R * I].reshape(O, R, I)
            yk = y.numpy().view(np.float64).reshape(K, R)
            st = state.numpy().view(np.float64).reshape(2 + K, O * I)
            with np.errstate(all="ignore"):
                v = x.astype(np.float64)
                m = v.mean(axis=1, keepdims=True)
                d = v - m
                st[0] = m.reshape(-1)
                st[1] = (d * d).sum(axis=1).reshape(-1)
                for k in range(K):
                    yc = (yk[k] - ymean[k]).reshape(1, R, 1)
                    st[2 + k] = (d * yc).sum(axis=1).reshape(-1)

        def comoment_combine(self, what, states, counts, ymean, ym2, nout, K, out, out_code):
            assert what in (CO_COV, CO_CORR) and len(ymean) == len(ym2) == len(counts) * K
            odt = np.dtype(C._CODES[out_code])
            if nout == 0:
                return
            st = states.numpy().view(np.float64).reshape(len(counts), 2 + K, nout)
            n = 0.0
            with np.errstate(all="ignore"):
                for p, c in enumerate(counts):
                    c = float(c)
                    if c <= 0:
                        continue
                    yb = np.asarray(ymean[p * K:(p + 1) * K], dtype=np.float64)
                    qb = np.asarray(ym2[p * K:(p + 1) * K], dtype=np.float64)
                    if n == 0.0:
                        n, m, q, cc, ym, yq = c, st[p, 0].copy(), st[p, 1].copy(), st[p, 2:].copy(), yb, qb
                        continue
                    tot = n + c
                    d = st[p, 0] - m
                    dy = yb - ym
                    m = m + d * (c / tot)
                    q = q + st[p, 1] + d * d * (n * c / tot)
                    cc = cc + st[p, 2:] + d[None, :] * (dy * (n * c / tot))[:, None]
                    ym = ym + dy * (c / tot)
                    yq = yq + qb + dy * dy * (n * c / tot)
                    n = tot
                if n == 0.0:
                    r = np.full((K, nout), np.nan)
                elif what == CO_COV:
                    r = cc / n
                else:
                    den = q[None, :] * yq[:, None]
                    r = np.where(den > 0, cc / np.sqrt(den), np.nan)   # no variance, no correlation
                    r = np.where(r > 1, 1.0, np.where(r < -1, -1.0, r))
            out.numpy().view(odt)[:K * nout].reshape(K, nout)[...] = r.astype(odt)

    return ComomentCpuBackend()
