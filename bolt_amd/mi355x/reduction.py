"""Mechanics of the statistics: how the reduced axes of an array lie in HBM and
what is launched to reduce over them.  One plan, one source, one finish, for
array.py's _reduced (one statistic), _reduced_moments (stats()),
_standardized (center / zscore), _detrended (detrend), _normalized (normalize),
_comoment (cov / corr) and _quantile (quantile / percentile / median).  The rules -- what is kept, padded or fused,
and their switches -- stay in array.py; this module never imports it and is
handed the array.
"""
import collections

import numpy as np

from bolt_amd.mi355x import _lib
from bolt_amd.mi355x._ops import backend_for, dtype_code
from bolt_amd.mi355x.dist import all_gather_bytes, _empty
from bolt_amd.mi355x.plan import padded_strides, reduce_layout, stat_dtype
from bolt_amd.mi355x.transfer import SMALL as HOST_RESULT_MAX, current_stream, finish_host_result, host_result, to_host

MOMENTS = (_lib.STAT_MEAN, _lib.STAT_VAR, _lib.STAT_STD)
# reductions whose result keeps the input dtype (numpy's same-dtype ufunc rule)
_KEEP_DTYPE = (_lib.STAT_SUM, _lib.STAT_MAX, _lib.STAT_MIN, _lib.STAT_PROD, _lib.STAT_BAND,
               _lib.STAT_BOR, _lib.STAT_BXOR, _lib.STAT_FMAX, _lib.STAT_FMIN)
STANDARDIZE = 'standardize'  # plan_for's statistic for center / zscore: the dtype of ``record - 0.0``
COMOMENT = 'comoment'  # plan_for's statistic for cov / corr: the statistics dtype of the outputs
QUANTILE = 'quantile'  # plan_for's statistic for an interpolated quantile: the dtype of ``record - 0.0``, as STANDARDIZE
STATS_FIELDS = ('mean', 'var', 'std')  # the order of bm_reduce_moments' outputs

# What reducing ``axes`` (sorted) of an array needs, from its shapes and dtype
# alone: the outputs' shape, plan.reduce_layout's (perm, O, R, I) of the local
# slab, its element count ``nloc`` and output count ``nout``, the dtype's code;
# ``outs``: statistic -> (result dtype, its code), filled by plan_for.
Plan = collections.namedtuple('Plan', ('axes', 'lshape', 'shape', 'dtype', 'world', 'out_shape',
                                       'perm', 'O', 'R', 'I', 'nloc', 'nout', 'code', 'outs'))
_PLANS = {}  # (local shape, axes as given, dtype, shape, world) -> Plan

# What to launch on: ``buf`` read as [O][R][I], rows ``pitch`` elements apart
# when I == 1, ``nlaunch`` outputs; ``drop`` = (O, I // Rl, P, Rl): the outputs
# are (O, I // Rl, P) of which [:, :, :Rl] are the array's (the rest belong to
# pad columns); ``every``: every axis of a row-padded float array, one state
# per column of the (rows, pitch) matrix, merged by merge_equal_counts.
Source = collections.namedtuple('Source', ('buf', 'O', 'R', 'I', 'pitch', 'nlaunch', 'drop', 'every'))
_tuple_new = tuple.__new__


def plan_for(arr, axis, stat):
    """-> (the Plan of reducing ``axis`` of ``arr``, the result dtype of
    ``stat`` -- a _lib.STAT_*, STANDARDIZE, COMOMENT or QUANTILE -- and its code)."""
    lshape = arr._local_shape
    key = (lshape, tuple(axis), arr._dtype, arr._shape, arr._ctx.world_size)
    plan = _PLANS.get(key)
    if plan is None:
        axes = tuple(sorted(set(int(a) for a in axis)))
        kept = [i for i in range(len(lshape)) if i not in axes]
        perm, O, R, I = reduce_layout(lshape, axes)
        plan = Plan(axes, lshape, arr._shape, arr._dtype, key[4], tuple(arr._shape[i] for i in kept),
                    perm, O, R, I, int(np.prod(lshape, dtype=np.int64)),
                    int(np.prod([lshape[i] for i in kept], dtype=np.int64)), dtype_code(arr._dtype), {})
        if len(_PLANS) > 4096:
            _PLANS.clear()
        _PLANS[key] = plan
    out = plan.outs.get(stat)
    if out is None:
        if stat in _KEEP_DTYPE:
            dt = plan.dtype
        elif stat in (_lib.STAT_LAND, _lib.STAT_LOR):
            dt = np.dtype(bool)
        else:
            dt = stat_dtype(plan.dtype, (1,) if stat in (STANDARDIZE, QUANTILE) else plan.out_shape)
        out = plan.outs[stat] = (dt, dtype_code(dt))
    return plan, out[0], out[1]


def source(arr, plan, moments=True, compact=False):
    """Classify ``arr`` for ``plan`` -> Source.  A row-padded array is read in
    place where its layout allows: rows over the last axis; on one GPU also
    columns over the padded rows and, of a float array when the caller can
    merge column states (``moments``), every axis.  ``compact``: the caller
    reads a padded array in place only for rows; any other axes get a dense
    temporary (the array itself stays padded).  Otherwise the dense records,
    the reduced axes permuted to the front first if they are not one block
    (what _align's swap does physically, array.py:85-115)."""
    d = arr.__dict__
    pbuf = d.get("_pbuf")
    lshape, perm, O, R, I, nloc = plan.lshape, plan.perm, plan.O, plan.R, plan.I, plan.nloc
    if pbuf is None and perm is None:
        return _tuple_new(Source, (d["_data"], O, R, I, R, plan.nout, None, False))  # (the hot path)
    if pbuf is not None and perm is None:
        P, Rl, single = d["_pitch"], lshape[-1], plan.world == 1
        if I == 1 and R == Rl and (nloc if single else 0 not in plan.axes):
            # the last axis: every output is this rank's, the rows read in place
            return Source(pbuf, O, R, 1, P, plan.nout, None, False)
        if single and nloc and not compact:
            if I > 1 and I % Rl == 0:
                # leading / middle axes: the columns run over the padded rows
                # as if the last axis were P long; every column is its own
                # reduction, so the pad columns' (unwritten) values reach only
                # their own outputs, which are dropped
                Ip = I // Rl * P
                return Source(pbuf, O, R, Ip, R, O * Ip, (O, I // Rl, P, Rl), False)
            if moments and O == 1 and I == 1 and R == nloc and len(lshape) >= 2 \
                    and plan.dtype.kind == "f" and plan.dtype.itemsize >= 4:
                return Source(pbuf, 1, nloc // Rl, P, nloc // Rl, P, (1, 1, P, Rl), True)
    es = plan.dtype.itemsize
    if perm is not None:
        # the reduced axes first (_align's swap): a padded array is read in place
        dev = arr._device
        buf = _empty(nloc * es, dev)
        if pbuf is not None:
            pstr = padded_strides(lshape, d["_pitch"])
            pshape = [lshape[p] for p in perm]
            backend_for(dev).copy_strided(pbuf, 0, buf, 0, pshape, [pstr[p] for p in perm],
                                          padded_strides(pshape, pshape[-1]), es)
        elif nloc:
            backend_for(dev).permute(arr._data, lshape, perm, es, buf)
    elif pbuf is not None and compact:
        buf = _empty(nloc * es, pbuf.device)
        if nloc:
            backend_for(pbuf.device).copy_strided(pbuf, 0, buf, 0, [nloc // lshape[-1], lshape[-1]],
                                                  [d["_pitch"], 1], [lshape[-1], 1], es)
    else:
        buf = arr._data
    return Source(buf, O, R, I, R, plan.nout, None, False)


def sharded_states(ctx, be, dev, plan, stat, src):
    """The sharded axis is reduced: this rank's ``stat`` state of ``src``
    (zeroes where its slab is empty: ``src`` is not touched), gathered in rank
    order -> (states, per-rank counts) for a reduce_combine
    (statcounter.py:67-99, deterministic here).  Every rank takes part in the
    gather."""
    if plan.world > _lib.MAX_COMBINE_PARTS:
        raise NotImplementedError("reductions over the sharded axis merge at most %d ranks (got %d)"
                                  % (_lib.MAX_COMBINE_PARTS, plan.world))
    sbytes = be.state_bytes(stat, plan.code, plan.nout)
    state = _empty(sbytes, dev)
    if plan.nloc:
        be.reduce_state(stat, src.buf, plan.code, src.O, src.R, src.I, state)
    else:
        state.zero_()
    per = int(np.prod([plan.shape[i] for i in plan.axes if i != 0], dtype=np.int64))
    counts = [(hi - lo) * per for lo, hi in ctx.bounds(plan.shape[0])]
    return all_gather_bytes(ctx, state, [sbytes] * plan.world), counts


def gathered_sizes(ctx, plan, itemsize, k=1):
    """Bytes of every rank's ``k`` planes of its slab of the outputs."""
    return [k * int(np.prod((hi - lo,) + plan.out_shape[1:], dtype=np.int64)) * itemsize
            for lo, hi in ctx.bounds(plan.shape[0])]


def outputs(be, dev, out_dtype, k, n, host_ok):
    """Where a launch stores ``k`` planes of ``n`` values: page-locked host
    memory when the kernels can store into it (``host_ok``: one rank, and
    something is launched), else HBM.  -> (the k planes' tensors, host buffer |
    list of one per plane | None, device buffer | None), for the launch and
    then finish."""
    nb = n * out_dtype.itemsize
    host = host_result(be, k * nb, dev) if host_ok else None
    if host is None and host_ok and nb <= HOST_RESULT_MAX < k * nb:
        # the planes together pass the zero-copy limit, each alone does not
        # (C4's 8 MiB float64 planes): a page-locked buffer per plane, as the
        # single statistics get -- a staged D2H of the planes cost 0.76 ms
        # there, more than the saved read (profiles/stats_fused_ab.log)
        hosts = [host_result(be, nb, dev) for _ in range(k)]
        if all(h is not None for h in hosts):
            return hosts, hosts, None
    if host is not None:
        # the kernel stores the result into page-locked host memory
        return ([host] if k == 1 else [host[j * nb:(j + 1) * nb] for j in range(k)]), host, None
    buf = _empty(k * nb, dev)
    return ([buf] if k == 1 else [buf[j * nb:(j + 1) * nb] for j in range(k)]), None, buf


def record_event(dev):
    """An event recorded behind what the current stream of ``dev`` holds so far."""
    import torch
    ev = torch.cuda.Event()
    ev.record(current_stream(dev))
    return ev


class Queued(object):
    """A finish queued ahead of its call (array.py's FINISH_AHEAD): outputs'
    page-locked plane and the event behind the launch that fills it.  Dropped
    untaken, it waits for the event first: the page-locked block must not go
    back to the allocator while the kernel may still store into it."""
    __slots__ = ("outs", "event")

    def __init__(self, outs, event):
        self.outs, self.event = outs, event

    def take(self):
        outs, self.outs = self.outs, None
        return outs

    def __del__(self):
        if self.outs is not None:
            try:
                self.event.synchronize()
            except Exception:   # interpreter shutdown
                pass


def finish(outs, dev, plan, out_dtype, k, n, drop=None, ctx=None, event=None):
    """outputs' ``k`` planes of ``n`` values, after the launch into them -> list
    of k host arrays of plan.out_shape (one stream synchronise, or one D2H),
    the pad columns' outputs dropped (``drop``, see Source).  ``ctx``: across
    ranks every rank holds the planes of its slab of the outputs; they are
    gathered (every rank takes part, one that launched nothing too) and
    re-interleaved.  ``event``: page-locked planes are complete once it is;
    waited for instead of the stream (later launches may be queued already)."""
    _, host, buf = outs
    pshape = plan.out_shape if drop is None else drop[:3]
    shape = pshape if k == 1 else (k, n)   # the single statistic's plane is viewed as its result at once
    if ctx is not None:
        # per-rank (k, this rank's outputs) planes -> (k, every output)
        isz = out_dtype.itemsize
        sizes = gathered_sizes(ctx, plan, isz, k)
        flat = to_host(all_gather_bytes(ctx, buf, sizes), out_dtype, (-1,))
        parts, off = [], 0
        for s in sizes:
            m = s // isz
            parts.append(flat[off:off + m].reshape(k, m // k))
            off += m
        host = np.concatenate(parts, axis=1)
        if k == 1:
            host = host.reshape(pshape)
    elif host is None:
        host = to_host(buf, out_dtype, shape)
    elif type(host) is list:
        host = [finish_host_result(host[0], dev, out_dtype, (n,))] + [h.numpy().view(out_dtype) for h in host[1:]]
    else:
        host = finish_host_result(host, dev, out_dtype, shape, event)
    rows = [host] if k == 1 else [host[j].reshape(pshape) for j in range(k)]
    if drop is None:
        return rows
    return [np.ascontiguousarray(full[:, :, :drop[3]]).reshape(plan.out_shape) for full in rows]


def _slots(planes, want):
    """The planes of ``want`` as bm_reduce_moments' (mean, var, std), None where not asked for."""
    slots = [None, None, None]
    for t, f in zip(planes, want):
        slots[STATS_FIELDS.index(f)] = t
    return tuple(slots)


def combine_moments(be, code, ocode, want, states, counts, nout, planes):
    """STAT_VAR states of ``len(counts)`` parts -> the moments ``want`` into ``planes``."""
    if hasattr(be, "reduce_combine_moments"):
        return be.reduce_combine_moments(code, states, counts, nout, _slots(planes, want), ocode)
    # an executor without the fused entry points (the CPU test executor):
    # the same states merged once per moment; the mean's merge takes the
    # one-plane STAT_MEAN layout (the mean planes, part-major)
    om, ov, osd = _slots(planes, want)
    with np.errstate(all="ignore"):  # a numpy executor on pad columns' unwritten values (dropped later)
        if om is not None:
            means = states.view(len(counts), 2, nout * 8)[:, 0, :].contiguous().view(-1)
            be.reduce_combine(_lib.STAT_MEAN, code, means, counts, nout, om, ocode)
        if ov is not None:
            be.reduce_combine(_lib.STAT_VAR, code, states, counts, nout, ov, ocode)
        if osd is not None:
            be.reduce_combine(_lib.STAT_STD, code, states, counts, nout, osd, ocode)


def launch_moments(be, src, es, code, ocode, want, planes):
    """The moments ``want`` of one read of ``src`` (elements of ``es`` bytes) into ``planes``."""
    buf, O, R, I, pitch = src[:5]
    if hasattr(be, "reduce_moments"):
        return be.reduce_moments(buf, code, O, R, I, pitch, _slots(planes, want), ocode)
    # an executor without the fused entry points: still one read, into a
    # STAT_VAR state that every moment is finalised from
    if pitch != R:
        dense = _empty(O * R * es, buf.device)
        be.copy_strided(buf, 0, dense, 0, [O, R], [pitch, 1], [R, 1], es)
        buf = dense
    state = _empty(be.state_bytes(_lib.STAT_VAR, code, O * I), buf.device)
    with np.errstate(all="ignore"):  # pad columns' unwritten values, as in combine_moments
        be.reduce_state(_lib.STAT_VAR, buf, code, O, R, I, state)
    combine_moments(be, code, ocode, want, state, [R], O * I, planes)


def signal_centre(ys):
    """What the state launch needs of ``ys``, (K, n) float64 signals -> (mean,
    resid, centred): the float64 mean every signal is centred by (a constant
    signal's is its value, so it centres to exact zeros), the sum of the
    centred float64 values -- the mean's rounding residue, which the state is
    corrected by, so the mean need not be better than float64's -- K floats
    each, and the centred values (the differences the kernels form)."""
    K, n = ys.shape
    if n == 0:
        return [0.0] * K, [0.0] * K, ys
    mean = np.where(np.ptp(ys, axis=1) == 0.0, ys[:, 0], ys.mean(axis=1))
    c = ys - mean[:, None]
    return mean.tolist(), c.sum(axis=1).tolist(), c


def signal_m2(c, resid):
    """The signals' sums of squared deviations from signal_centre's centred
    values and residues (the finish needs them, not the state launch)."""
    n = c.shape[1]
    if n == 0:
        return [0.0] * c.shape[0]
    return (np.einsum("ij,ij->i", c, c) - np.square(resid) / n).tolist()


def comoment_state(be, src, dtype, code, ys, ymean, yresid, state):
    """The co-moment state of one read of ``src`` against the (K, R) float64
    signals ``ys`` into ``state``: (2 + K) float64 planes of src.nlaunch values,
    mean, M2, then C_k = sum (x - mean)(y_k - ymean_k) (bm_comoment_state)."""
    import torch
    buf, O, R, I, pitch = src[:5]
    K = len(ymean)
    if hasattr(be, "comoment_state"):
        yd = torch.from_numpy(np.ascontiguousarray(ys, dtype=np.float64).reshape(-1))
        if buf.device.type == "cuda":
            # page-locked + non-blocking: the upload queues behind earlier
            # kernels; the launch that reads it follows on the same stream
            yd = yd.pin_memory().to(buf.device, non_blocking=True)
        return be.comoment_state(buf, code, O, R, I, pitch, yd, ymean, yresid, state)
    # an executor without the entry points (the CPU test executor): torch
    # float64 arithmetic on views of the bytes, padded rows through a strided view
    from bolt_amd.mi355x import functional as F
    es = np.dtype(dtype).itemsize
    if pitch != R:
        x = F.view(buf[:O * pitch * es], (O, pitch), dtype)[:, :R].unsqueeze(2)
    else:
        x = F.view(buf, (O, R, I), dtype)
    x = x.to(torch.float64)
    d = x - x.mean(dim=1, keepdim=True)
    st = F.view(state, (2 + K, O * I), np.float64)
    st[0] = x.mean(dim=1).reshape(-1)
    st[1] = (d * d).sum(dim=1).reshape(-1)
    yc = torch.from_numpy(ys - np.asarray(ymean, dtype=np.float64)[:, None]).to(buf.device)
    for k in range(K):
        st[2 + k] = (d * yc[k].reshape(1, R, 1)).sum(dim=1).reshape(-1)


def comoment_combine(be, what, states, counts, ymean, ym2, nout, K, out, out_dtype, ocode):
    """comoment_state states of ``len(counts)`` parts (part-major), merged in
    part order and finalised to cov / corr into ``out``, K planes of ``nout``
    values; ``ymean`` / ``ym2``: per part, the K means and sums of squared
    deviations of its slice of the signals (bm_comoment_combine)."""
    flat_m = [v for part in ymean for v in part]
    flat_q = [v for part in ym2 for v in part]
    if hasattr(be, "comoment_combine"):
        return be.comoment_combine(what, states, counts, flat_m, flat_q, nout, K, out, ocode)
    # the same merge in torch float64 (an executor without the entry points)
    import torch
    from bolt_amd.mi355x import functional as F
    st = F.view(states, (len(counts), 2 + K, nout), np.float64)
    n, m, q, C = 0.0, None, None, None
    ym, yq = [0.0] * K, [0.0] * K
    for p, c in enumerate(counts):
        c = float(c)
        if c <= 0:
            continue
        if n == 0.0:
            n, m, q, C = c, st[p, 0].clone(), st[p, 1].clone(), st[p, 2:].clone()
            ym, yq = list(ymean[p]), list(ym2[p])
            continue
        tot = n + c
        d = st[p, 0] - m
        m = m + d * (c / tot)
        q = q + st[p, 1] + d * d * (n * c / tot)
        for k in range(K):
            dy = ymean[p][k] - ym[k]
            C[k] = C[k] + st[p, 2 + k] + d * (dy * (n * c / tot))
            ym[k] += dy * (c / tot)
            yq[k] += ym2[p][k] + dy * dy * (n * c / tot)
        n = tot
    if n == 0.0:
        r = torch.full((K, nout), float("nan"), dtype=torch.float64, device=states.device)
    elif what == _lib.CO_COV:
        r = C / n
    else:
        den = q.reshape(1, nout) * torch.tensor(yq, dtype=torch.float64, device=states.device).reshape(K, 1)
        r = torch.where(den > 0, torch.clamp(C / torch.sqrt(den), -1.0, 1.0),
                        torch.full_like(den, float("nan")))   # no variance, no correlation
    F.view(out, (K, nout), out_dtype).copy_(r.to(F.torch_dtype(out_dtype)))


_BASES = {}  # (n, order) -> detrend_basis' table


def detrend_basis(n, order):
    """p_1..p_order, the discrete orthonormal (Gram) polynomials on the n
    positions t_r = r - (n-1)/2, as an (order, n) float64 table (cached per
    (n, order), shared by its callers: not to be written): bm_detrend_rows' recurrence in numpy float64,
    b_k = (k/2) sqrt((n-k)(n+k) / (4k^2-1)), p_0 = 1/sqrt(n),
    p_1 = t p_0 / b_1, p_{k+1} = (t p_k - b_k p_{k-1}) / b_{k+1}, multiplying
    by 1/b_k as the kernel does.  No Vandermonde matrix is formed.  order < n."""
    key = (int(n), int(order))
    tab = _BASES.get(key)
    if tab is None:
        nf = np.float64(n)
        t = np.arange(n, dtype=np.float64) - (nf - 1.0) / 2.0
        k = np.arange(1, order + 1, dtype=np.float64)
        b = k / 2.0 * np.sqrt((nf - k) * (nf + k) / (4.0 * k * k - 1.0))
        rb = 1.0 / b
        tab = np.empty((order, n), dtype=np.float64)
        pm = np.full(n, 1.0 / np.sqrt(nf))
        pk = t * pm * rb[0]
        tab[0] = pk
        for q in range(1, order):
            pn = (t * pk - b[q - 1] * pm) * rb[q]
            pm, pk = pk, pn
            tab[q] = pk
        if len(_BASES) >= 8:   # (tables of long records are megabytes)
            _BASES.clear()
        _BASES[key] = tab
    return tab


def quantile_rows(be, buf, dtype, code, O, R, pitch, ranks, frac, out, out_dtype, ocode):
    """The quantiles of O rows of R elements, ``pitch`` elements apart in
    ``buf``, into ``out``: len(ranks) planes of O values of ``out_dtype``.
    Quantile k is the value lo of rank ranks[k] where frac[k] == 0, else
    lo + (hi - lo) * frac[k] in float64 with hi the value of the next rank
    (bm_quantile_rows; rows the registers do not hold: bm_quantile_select).  A
    row holding a NaN gives NaN."""
    if hasattr(be, "quantile_rows"):
        if not be.quantile_rows(buf, code, O, R, pitch, ranks, frac, out, ocode):
            be.quantile_select(buf, code, O, R, pitch, ranks, frac, out, ocode)
        return
    # an executor without the entry points (the CPU test executor): torch.sort
    # of the rows, the same ranks, the same formula.  torch sorts no uint16 /
    # uint32 / uint64: they are sorted as the signed type with the sign bit
    # flipped, which keeps their order
    import torch
    from bolt_amd.mi355x import functional as F
    dtype = np.dtype(dtype)
    es = dtype.itemsize
    sort_dt, flip = dtype, None
    if dtype == np.bool_:
        sort_dt = np.dtype(np.uint8)
    elif dtype.kind == "u" and es > 1:
        sort_dt = np.dtype("i%d" % es)
        flip = -(1 << (8 * es - 1))
    x = F.view(buf[:O * pitch * es], (O, pitch), sort_dt)[:, :R]
    if flip is not None:
        x = x ^ flip
    srt = torch.sort(x, dim=1).values   # (NaNs last)
    res = F.view(out, (len(ranks), O), out_dtype)
    for k, (r, g) in enumerate(zip(ranks, frac)):
        cols = srt[:, r:r + 2] if g != 0.0 else srt[:, r:r + 1]
        if flip is not None:
            cols = cols ^ flip
        v = cols.contiguous().cpu().numpy().view(dtype)
        if g == 0.0 and out_dtype == dtype:
            val = v[:, 0]
        else:
            lo = v[:, 0].astype(np.float64)
            with np.errstate(all="ignore"):
                val = (lo + (v[:, 1].astype(np.float64) - lo) * g) if g != 0.0 else lo
        if dtype.kind == "f":
            val = np.where(torch.isnan(srt[:, R - 1]).cpu().numpy(), np.nan, val)
        res[k] = torch.from_numpy(np.ascontiguousarray(val.astype(out_dtype))).to(res.device)


def baseline_request(dtype, rank, frac):
    """What to ask quantile_rows for so that the 'linear' quantile (``rank``,
    ``frac``) can be had in float64, unrounded -> (ranks, frac, out dtype).
    Where the statistics dtype is float64 that is the quantile itself.
    float16 / float32 keep theirs, and bm_quantile_rows gives no other, so a
    rounded interpolation is all it has: lo and hi are asked for as elements,
    bit for bit, and baseline_f64 interpolates."""
    dt = np.dtype(dtype)
    if stat_dtype(dt, (1,)) == np.float64:
        return [rank], [frac], np.dtype(np.float64)
    return ([rank, rank + 1], [0.0, 0.0], dt) if frac != 0.0 else ([rank], [0.0], dt)


def baseline_f64(planes, frac):
    """baseline_request's planes (numpy arrays or tensors, lo [, hi]) -> the
    float64 baseline: lo, or lo + (hi - lo) * frac as three separately rounded
    float64 operations (bm_quantile.hip's emit; a NaN row's lo is NaN)."""
    wide = (lambda p: p.astype(np.float64)) if isinstance(planes[0], np.ndarray) else (lambda p: p.double())
    lo = wide(planes[0])
    if len(planes) == 1:
        return lo
    with np.errstate(all="ignore"):
        d = wide(planes[1]) - lo
        t = d * frac
        return lo + t


def quantile_baseline(be, buf, dtype, code, O, R, pitch, rank, frac):
    """The float64 'linear' quantile (``rank``, ``frac``) of O rows of ``buf``
    as a device plane of O values (uint8 tensor): quantile_rows into HBM, no
    host round trip."""
    from bolt_amd.mi355x import functional as F
    ranks, fr, odt = baseline_request(dtype, rank, frac)
    out = _empty(len(ranks) * O * odt.itemsize, buf.device)
    quantile_rows(be, buf, dtype, code, O, R, pitch, ranks, fr, out, odt, dtype_code(odt))
    if odt == np.float64:
        return out
    planes = F.view(out, (len(ranks), O), odt)
    return F.as_bytes(baseline_f64([planes[k] for k in range(len(ranks))], frac))


def merge_equal_counts(planes, Rl, nrows):
    """The StatCounter merge (statcounter.py:67-99) of ``Rl`` column states of
    ``nrows`` values each, ``planes`` = their float64 (mean [, M2]) rows ->
    (mean, variance | None): mean = mean of the column means, M2 = sum of the
    column M2 + rows * sum of squared deviations of the column means."""
    means = planes[0, :Rl]
    mean = means.mean()
    if len(planes) < 2:
        return mean, None
    return mean, (planes[1, :Rl].sum() + nrows * np.square(means - mean).sum()) / (nrows * Rl)


def every_axis_moments(be, src, stat, code):
    """mean / var / std over every axis of a row-padded float array, read in
    place (a Source with ``every``): the padded rows are one (rows, pitch)
    matrix whose columns get a float64 mean (and M2 for var / std) state each
    over all rows (bm_reduce_state of ``stat``, the pad columns' states
    dropped); the row-length states, all of the same count, merge on the host
    -> merge_equal_counts' (mean, variance).  No dense copy of the array is
    made; the summation order differs from the dense layout's (results within
    1e-12 relative in float64, rounded once)."""
    nrows, P, Rl = src.R, src.I, src.drop[3]
    state = _empty(be.state_bytes(stat, code, P), src.buf.device)
    be.reduce_state(stat, src.buf, code, 1, nrows, P, state)
    return merge_equal_counts(to_host(state, np.float64, (-1, P)), Rl, nrows)   # mean [, M2] (bm_reduce_state)
