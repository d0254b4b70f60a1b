"""BoltArrayMI355X: the 'mi355x' mode array (drop-in for BoltArraySpark's hot path).

Data layout.  The logical array is C-order (keys..., values...) -- one record
is one contiguous value block, exactly the order of the Spark path's sorted
records (bolt/spark/array.py:1006-1014).  Each rank holds a slab of the
leading key axis as a flat uint8 tensor in HBM; shape/split/dtype are host
metadata (array.py:15-28).

Operations and what replaces the Spark machinery:
  swap / transpose / T / swapaxes / Keys.transpose / Values.transpose:
      the net permutation (plan.swap_perm, array.py:716-808) as ONE permute
      kernel (bm_permute); across GPUs pack -> RCCL all-to-all -> unpack.
  chunk: ChunkedArrayMI355X (chunk.py), the packed chunk layout in HBM.
  sum / mean / var / std: one reduction kernel over the aligned layout
      (array.py:243-395 + statcounter.py), float64 accumulation; across GPUs
      per-rank states -> all_gather -> ordered Chan combine.
  stats: several of mean / var / std from ONE read (the StatCounter's
      stats='all', statcounter.py:30-48): the variance's launch sequence
      storing every moment asked for (bm_reduce_moments).
  center / zscore: every record minus its mean [over its standard
      deviation] along an axis, a device array of the same shape: rows over
      the last axis in one read and one write (bm_standardize_rows), other
      axes as one moments read plus bm_standardize_apply.
  quantile / percentile / median: exact order statistics of every record
      along an axis, host results: rows over the last axis selected by rank
      from one read (bm_quantile_rows; longer rows bm_quantile_select), other
      axes permuted to rows first.
  toarray / tolocal: D2H (+ all_gather of the slabs).
"""
import collections
import functools
import os

import numpy as np

from bolt_amd.mi355x import _lib, reduction
from bolt_amd.mi355x._ops import backend_for, dtype_code
from bolt_amd.base import BoltArray
from bolt_amd.mi355x.context import local_shape
from bolt_amd.mi355x.dist import all_gather_bytes, concat_rows_sharded, gather_to_host, permute_sharded, redistribute_rows, select_sharded, _empty
from bolt_amd.mi355x.transfer import to_device, to_host
from bolt_amd.local import BoltArrayLocal
from bolt_amd.mi355x.plan import getplan, check_plan, padded_strides, swap_perm, swap_shape, reduce_layout
from bolt_amd.utils import tupleize, argpack, inshape, istransposeable, isreshapeable

_STAT_CODES = {'mean': _lib.STAT_MEAN, 'variance': _lib.STAT_VAR, 'stdev': _lib.STAT_STD}


def _ufunc_stats():
    """reduce(func) functions that run as one bm_reduce mode (array.py:243-282)."""
    import operator
    return {operator.add: _lib.STAT_SUM, np.add: _lib.STAT_SUM,
            np.maximum: _lib.STAT_MAX, np.minimum: _lib.STAT_MIN,
            operator.mul: _lib.STAT_PROD, np.multiply: _lib.STAT_PROD,
            np.logical_and: _lib.STAT_LAND, np.logical_or: _lib.STAT_LOR,
            np.bitwise_and: _lib.STAT_BAND, operator.and_: _lib.STAT_BAND,
            np.bitwise_or: _lib.STAT_BOR, operator.or_: _lib.STAT_BOR,
            np.bitwise_xor: _lib.STAT_BXOR, operator.xor: _lib.STAT_BXOR,
            np.fmax: _lib.STAT_FMAX, np.fmin: _lib.STAT_FMIN}


_UFUNC_STATS = _ufunc_stats()


def _hashable(f):
    try:
        hash(f)
        return True
    except TypeError:
        return False


def _tree(func, recs):
    """((r0 f r1) f (r2 f r3)) ... over the leading axis of a device tensor."""
    import torch
    from bolt_amd.mi355x.functional import apply_pairs
    while recs.shape[0] > 1:
        n = recs.shape[0]
        nxt = apply_pairs(func, recs[0:n - 1:2], recs[1:n:2])
        if n % 2:
            nxt = torch.cat([nxt, recs[n - 1:].to(nxt.dtype)])
        recs = nxt
    return recs[0]


_MOMENTS = reduction.MOMENTS


@functools.lru_cache(maxsize=256)
def _plan_ok(vshape, dtype, size):
    try:
        plan, pad = getplan(vshape, dtype, size, None, None)
        check_plan(plan, pad, vshape)
    except Exception as e:  # cache the failure too; re-raised below
        return e
    return None


def _check_swap_plan(vshape, dtype, size):
    """getplan + _chunk's checks for the swap's chunk size (chunk.py:120-129), cached."""
    try:
        err = _plan_ok(tuple(vshape), np.dtype(dtype), size)
    except TypeError:  # unhashable size: validate uncached
        plan, pad = getplan(vshape, dtype, size, None, None)
        check_plan(plan, pad, vshape)
        return
    if err is not None:
        raise type(err)(*err.args)


_SWAP_PLANS = {}   # (shape, split, dtype, kaxes, vaxes, size) -> (_move_plan, squeezed shape | None) | _NOOP
_NOOP = object()


def _move_plan(shape, perm, split):
    """What x.transpose(perm) with the given split needs, from the shape alone:
    (perm, split, new shape, identity, only unit axes move)."""
    perm = tuple(int(p) for p in perm)
    moved = [p for p in perm if shape[p] != 1]
    return (perm, int(split), tuple(shape[p] for p in perm), perm == tuple(range(len(shape))),
            moved == sorted(moved))


# Row pitch of transposed results.  A transpose writes its destination rows in
# 256-B tile segments; rows whose length is not a multiple of the 128-B line
# start mid-line (C2's 2000 float32 = 8000 B: every other row), so
# neighbouring tiles write parts of the same lines.  Such a result is stored
# with its rows padded to a 256-B multiple (C2: 8192 B): the C2 transpose
# 0.729 -> 0.675 ms, its time-axis statistics 0.298 -> 0.301-0.305 ms, the
# step -2.8% (profiles/r05s_pitch_prof.txt, r05s_pitch_ab.log; pitch sweep
# r05t_pitch_sweep.txt); other shapes gain more: float32 rows of 4400 B
# 2.26 -> 1.65 ms, of 12000 B 1.34 -> 1.18, C4's uint16 .T (20000-B rows)
# 9.2 -> 8.1 ms (r05zw_pitch_align.log: 256-B steps are the best or near it
# everywhere; 1 KiB steps lose 8% on the uint16 rows); rows of 2000 / 3000 B
# +10-16%, but 1000-B rows padded to 1024 lose 16%, hence the 1536-B floor
# (r05zz_short_rows.log).  Statistics over the
# last axis read the padded rows in place (bm_reduce_rows); swaps,
# transposes, indexing, map / filter / chunk of single-row records, column
# statistics and elementwise ops read them too; the rest compacts the rows
# once (_compact).  ROW_PITCH = False turns padding off (the tests' switch;
# the sweeps that chose the constants ran on round-5 builds with them as
# environment knobs: tools/pitch_sweep.sh, tools/pitch_align_sweep.sh).
ROW_PITCH = True
_PITCH_MIN_ROW = 1536   # bytes: shorter rows are not padded
_PITCH_ALIGN = 256      # bytes: padded rows start on this boundary
_PITCH_LINE = 128       # bytes: rows of a multiple of this stay dense
_PITCH_PAD_DIV = 16     # at most 1/16 of a row is padding
_PITCH_PLANS = {}  # (_move_plan, itemsize) -> None | pitched copy plan


def _pitch_plan(mv, shape, es):
    """The pitched copy for _move_plan ``mv`` of an array of ``shape``, or None:
    (pitch in elements, rows, output shape, source strides, pitched
    destination strides), all in elements."""
    perm, _, new_shape, _, _ = mv
    nd = len(new_shape)
    if nd < 2 or perm[-1] == nd - 1:
        return None
    R = new_shape[-1]
    rb = R * es
    if rb < _PITCH_MIN_ROW or rb % _PITCH_LINE == 0:
        return None
    pb = -(-rb // _PITCH_ALIGN) * _PITCH_ALIGN
    if (pb - rb) * _PITCH_PAD_DIV > rb or pb % es:
        return None
    P = pb // es
    rows = int(np.prod(new_shape[:-1], dtype=np.int64))
    if rows < 2:
        return None
    sstr = [1] * len(shape)
    for k in range(len(shape) - 2, -1, -1):
        sstr[k] = sstr[k + 1] * shape[k + 1]
    return P, rows, list(new_shape), [sstr[p] for p in perm], _padded_strides(new_shape, P)


_DEVICE_BYTES = {}  # device index -> total HBM bytes


def _pitch_fits(pp, es, device):
    """Room for the padded result AND a later dense compaction of it (a
    consumer that needs dense records copies them once, see _compact): checked
    against the device's free memory (plus what torch's allocator holds
    unused) only when the two together exceed 1/8 of the device, so the small
    results of a hot loop never query the driver."""
    if device.type != "cuda":
        return True
    import torch
    P, rows, oshape = pp[0], pp[1], pp[2]
    need = rows * (P + oshape[-1]) * es
    idx = device.index if device.index is not None else torch.cuda.current_device()
    total = _DEVICE_BYTES.get(idx)
    if total is None:
        total = _DEVICE_BYTES[idx] = torch.cuda.get_device_properties(idx).total_memory
    if need * 8 <= total:
        return True
    free = torch.cuda.mem_get_info(idx)[0] + torch.cuda.memory_reserved(idx) - torch.cuda.memory_allocated(idx)
    return need <= free


_padded_strides = padded_strides


@functools.lru_cache(maxsize=1024)
def _aligned_vshape_of(shape, split, axis):
    """BoltArrayMI355X._aligned_vshape for (shape, split, axes)."""
    tokeys = [a - split for a in axis if a >= split]
    tovalues = [a for a in range(split) if a not in axis]
    if not (tokeys or tovalues):
        return None
    ref = swap_shape(shape, split, tovalues, tokeys)
    if ref is None:
        return None
    vs = ref[0][ref[1]:]
    kept = tuple(d for i, d in enumerate(shape) if i not in set(axis))
    return None if vs == kept else vs


# mean() / var() / std() over the same axes of one array: the first call's read
# also stores the StatCounter state (n, mean, M2 -- statcounter.py:30-48, which
# the reference's _stat builds whole on every call) and a later var() / std()
# is finished from it (bm_reduce_combine of one part) without reading the
# array.  Records never change after construction, so the state is an
# invariant of (array, axes).  Kept only when the second read would come from
# HBM -- more bytes than the 256 MiB Infinity Cache -- and when the state (16 B
# per output) is at most 1/64 of the bytes read: its store and the memory it
# holds stay under 1.6% of the read.  One GPU, float inputs, row reductions
# (I == 1) whose plan does not split R into chunks (bm_reduce_keep).  A later mean() reads again: its bits
# come from other arithmetic than the state's mean.  unpersist() releases the
# states; KEEP_MOMENTS = False (BOLT_AMD_KEEP_MOMENTS=0) keeps none.
KEEP_MOMENTS = os.environ.get("BOLT_AMD_KEEP_MOMENTS", "1") != "0"
_KEEP_MIN_BYTES = 256 << 20
_KEEP_STATE_DIV = 64
# Column reductions (I > 1) keep nothing: storing the state cost their launch
# +3.1% on one box and +11% on another on the 64 GiB target's shape at 1/8 of
# its rows (1.280 / 1.383 against 1.236-1.243 ms, spread 0.015 ms), the same for
# the dual mean launch and for the var / std launch that only adds the stores,
# where the rows kernel's is within its spread (C2: +0.003 ms of 0.303;
# profiles/moments_kept_ab.log).  True: tools/moments_kept_ab.py --keep-cols,
# the run that measured it, and the tests of the column branches.
_KEEP_COLS = False

# swap(), then mean() / var() / std() over the last axis of the result (time
# series keyed by time, swapped to key = voxel, then per-voxel statistics):
# on one GPU the swap's transpose kernel also leaves the STAT_VAR state of
# every result row (bm_copy_strided_moments), remembered for the axes
# (ndim - 1,) like a kept state, and all three statistics -- the mean too --
# are finished from it without reading the array.  Asked for only of float32 /
# float64 swaps that move more bytes than _FUSE_SWAP_MIN_BYTES (the result
# would be re-read from HBM, as for _KEEP_MIN_BYTES, which tests lower on its
# own) and whose state is at most 1 / _FUSE_SWAP_STATE_DIV of them; the library
# fuses only tile transposes along the result's rows and says so.
# FUSE_SWAP_MOMENTS = False (BOLT_AMD_FUSE_SWAP_MOMENTS=0): the plain copy.
FUSE_SWAP_MOMENTS = os.environ.get("BOLT_AMD_FUSE_SWAP_MOMENTS", "1") != "0"
_FUSE_SWAP_MIN_BYTES = 256 << 20
_FUSE_SWAP_STATE_DIV = 64

# mean() and std() of a state the swap left are the pair of every z-score, and
# the host is still ahead of the GPU when the first of them is called (the swap
# is asynchronous).  So the first mean() finished from such a state also
# queues std's finish right behind its own -- into a page-locked plane of its
# own, with an event of its own -- and waits for the event behind its own
# launch, not for the stream; the std() that follows waits for std's event and
# returns the plane: no launch and no stream synchronise, where the GPU
# otherwise idles ~0.033 ms while the host returns mean, calls std and
# launches.  Symmetric: std() first queues mean's finish.  var() queues
# nothing (a var / std pair is not a pattern the reference's users show).  One
# plane per state, queued by the first of the two calls and handed out once;
# any later call goes the plain way.  Only where the result plane takes the
# page-locked result path.  unpersist() drops the queued plane.  The cost where
# the other statistic never follows: one 0.021 ms kernel and 1 MiB of
# page-locked memory (C2) per first mean(), queued behind the result the
# caller is waiting for.  FINISH_AHEAD = False (BOLT_AMD_FINISH_AHEAD=0): off.
FINISH_AHEAD = os.environ.get("BOLT_AMD_FINISH_AHEAD", "1") != "0"
_AHEAD_OF = {_lib.STAT_MEAN: _lib.STAT_STD, _lib.STAT_STD: _lib.STAT_MEAN}

# A moment state held for some axes (the ``_kept`` dict of an array, keyed by the
# sorted axes): the STAT_VAR ``state`` of ``nlaunch`` outputs over ``count``
# values each, ``drop`` as reduction.Source's; ``serves_mean``: mean() is
# finished from it too (a state the swap's transpose left), not only var / std;
# ``ahead``: of such a state, {statistic: reduction.Queued} of the finish
# queued ahead (see FINISH_AHEAD; non-empty once one was queued), else None.
Kept = collections.namedtuple('Kept', ('state', 'count', 'nlaunch', 'drop', 'serves_mean', 'ahead'))
Kept.__new__.__defaults__ = (None,)

# stats(): one StatCounter pass read for several moments (statcounter.py:30-48)
Stats = collections.namedtuple('Stats', ('count', 'mean', 'var', 'std'))
_STATS_FIELDS = reduction.STATS_FIELDS
_STATS_NAMES = {'mean': 'mean', 'var': 'var', 'variance': 'var', 'std': 'std', 'stdev': 'std'}
_STAT_AXES = {}  # (shape, split, axis as given) -> (validated axes, records after _align, record shape | None)


class BoltArrayMI355X(BoltArray):

    _metadata = {
        '_shape': None,
        '_split': None,
        '_dtype': None,
        '_ordered': True,
    }

    def __init__(self, data, shape=None, split=None, dtype=None, ordered=True, context=None,
                 npartitions=None):
        self._data = data
        self._shape = tuple(int(s) for s in shape)
        self._split = int(split)
        self._dtype = np.dtype(dtype)
        self._mode = 'mi355x'
        self._ordered = ordered
        self._ctx = context
        self._npartitions = npartitions

    # ------------------------------------------------------------ creation
    @property
    def _constructor(self):
        return BoltArrayMI355X

    @classmethod
    def _ingest(cls, arry, permutation, shape, split, dtype, ctx, npartitions):
        """Host ndarray -> sharded device array (spark/construct.py:43-70).

        Records are ``arry.transpose(permutation)`` in C order while the array
        keeps ``shape`` -- the reference takes the shape before transposing
        (construct.py:48 vs :55), so non-leading key axes come back as
        ``x.transpose(perm).reshape(x.shape)``; this is kept for parity.
        """
        import torch
        dev = ctx.device
        es = dtype.itemsize
        arry = np.ascontiguousarray(arry)
        identity = list(permutation) == list(range(len(shape)))
        lo, hi = ctx.local_bounds(shape[0])
        rowbytes = int(np.prod(shape[1:], dtype=np.int64)) * es
        if identity:
            data = to_device(arry[lo:hi].reshape(-1).view(np.uint8), dev)
        elif ctx.world_size == 1:
            # whole array to HBM, permuted on the GPU (the reference's records
            # are x.transpose(perm) reshaped to the old shape)
            full = to_device(arry.reshape(-1).view(np.uint8), dev)
            data = _empty(full.numel(), dev)
            if full.numel():
                backend_for(dev).permute(full, arry.shape, permutation, es, data)
        else:
            # this rank's slab is the flat element range [s, e) of
            # x.transpose(perm): upload only the source planes along axis
            # perm[0] that cover it, permute them on the GPU, cut the range
            pshape = tuple(arry.shape[i] for i in permutation)
            inner0 = int(np.prod(pshape[1:], dtype=np.int64))
            s0, e0 = lo * (rowbytes // es), hi * (rowbytes // es)
            if e0 == s0 or inner0 == 0:
                data = _empty(0, dev)
            else:
                i_lo, i_hi = s0 // inner0, min(pshape[0], -(-e0 // inner0))
                idx = [slice(None)] * arry.ndim
                idx[permutation[0]] = slice(i_lo, i_hi)
                sub = np.ascontiguousarray(arry[tuple(idx)])
                part = to_device(sub.reshape(-1).view(np.uint8), dev)
                perm_bytes = _empty(part.numel(), dev)
                backend_for(dev).permute(part, sub.shape, permutation, es, perm_bytes)
                off = (s0 - i_lo * inner0) * es
                data = perm_bytes[off:off + (e0 - s0) * es]
                if data.numel() != perm_bytes.numel():
                    data = data.clone()
        return cls(data, shape=shape, split=split, dtype=dtype, context=ctx, npartitions=npartitions)

    @classmethod
    def _filled(cls, value, shape, split, dtype, ctx, npartitions):
        """ones/zeros: one record built on the host, broadcast on the GPU (spark/construct.py:207-222)."""
        import torch
        dev = ctx.device
        es = dtype.itemsize
        lshape = local_shape(ctx, shape)
        n = int(np.prod(lshape, dtype=np.int64))
        data = _empty(n * es, dev)
        if n:
            unit = to_device(np.full(1, value, dtype=dtype).view(np.uint8), dev)
            backend_for(dev).copy_strided(unit, 0, data, 0, [n], [0], [1], es)
        return cls(data, shape=shape, split=split, dtype=dtype, context=ctx, npartitions=npartitions)

    @classmethod
    def _from_shard(cls, shard, shape, split, dtype, ctx, npartitions):
        import torch
        dev = ctx.device
        if isinstance(shard, np.ndarray):
            dtype = np.dtype(dtype or shard.dtype)
            data = to_device(np.ascontiguousarray(shard, dtype=dtype).reshape(-1).view(np.uint8), dev)
        else:
            if dtype is None:
                raise ValueError("dtype is required for a device shard")
            dtype = np.dtype(dtype)
            t = shard.contiguous()
            data = t.view(torch.uint8).reshape(-1) if t.dtype != torch.uint8 else t.reshape(-1)
            if data.device != dev:
                data = data.to(dev)
        want = int(np.prod(local_shape(ctx, shape), dtype=np.int64)) * dtype.itemsize
        if data.numel() != want:
            raise ValueError("shard holds %d bytes, rank %d of %s needs %d"
                             % (data.numel(), ctx.rank, str(shape), want))
        if split < 1 or split > len(shape):
            raise ValueError("split axis must be in [1, %d], got %d" % (len(shape), split))
        return cls(data, shape=shape, split=split, dtype=dtype, context=ctx, npartitions=npartitions)

    def _like(self, data, shape, split, dtype=None):
        return BoltArrayMI355X(data, shape=shape, split=split, dtype=self._dtype if dtype is None else dtype,
                               context=self._ctx, npartitions=self._npartitions)

    def _derive(self, data, shape, split):
        """_like for a ``shape`` that is already a tuple of ints and the same
        dtype: the constructor's coercions skipped (the swap's launch path)."""
        new = object.__new__(BoltArrayMI355X)
        new.__dict__.update(_data=data, _shape=shape, _split=split, _dtype=self._dtype, _mode='mi355x',
                            _ordered=True, _ctx=self._ctx, _npartitions=self._npartitions)
        return new

    def __getattr__(self, name):
        # only reached for attributes not set: a row-padded array's records
        # (see ROW_PITCH) are compacted the first time anything needs them dense
        if name == "_data" and "_pbuf" in self.__dict__:
            return self._compact()
        raise AttributeError("'%s' object has no attribute '%s'" % (type(self).__name__, name))

    def _compact(self):
        """Dense records of a row-padded array (one strided copy on the GPU)."""
        d = self.__dict__
        pbuf, P = d["_pbuf"], d["_pitch"]
        es = self._dtype.itemsize
        R = self._shape[-1]
        rows = int(np.prod(self._local_shape[:-1], dtype=np.int64))
        data = _empty(rows * R * es, pbuf.device)
        if rows and R:
            backend_for(pbuf.device).copy_strided(pbuf, 0, data, 0, [rows, R], [P, 1], [R, 1], es)
        d["_data"] = data
        del d["_pbuf"], d["_pitch"]
        return data

    def _derive_padded(self, pbuf, pitch, shape, split):
        """_derive for records stored with padded rows (see ROW_PITCH)."""
        new = self._derive(None, shape, split)
        nd = new.__dict__
        del nd["_data"]
        nd["_pbuf"], nd["_pitch"] = pbuf, pitch
        return new

    @property
    def _device(self):
        d = self.__dict__
        return (d["_pbuf"] if "_pbuf" in d else d["_data"]).device

    @property
    def _backend(self):
        return backend_for(self._device)

    @property
    def _local_shape(self):
        # shape and context never change after construction: computed once
        ls = self.__dict__.get("_lshape")
        if ls is None:
            ls = self.__dict__["_lshape"] = local_shape(self._ctx, self._shape)
        return ls

    # ---------------------------------------------------------- properties
    @property
    def shape(self):
        return self._shape

    @property
    def size(self):
        return int(np.prod(self._shape))

    @property
    def ndim(self):
        return len(self._shape)

    @property
    def split(self):
        return self._split

    @property
    def dtype(self):
        return self._dtype

    @property
    def context(self):
        return self._ctx

    @property
    def mask(self):
        return tuple([1] * self._split + [0] * (self.ndim - self._split))

    @property
    def keys(self):
        from bolt_amd.mi355x.shapes import Keys
        return Keys(self)

    @property
    def values(self):
        from bolt_amd.mi355x.shapes import Values
        return Values(self)

    def cache(self):
        """Records are resident in HBM already (array.py:37-41); only the flag
        the record view reports changes."""
        self._cached = True

    def unpersist(self):
        """(array.py:43-47) -- the records stay in HBM; clears the flag and
        releases the moment states kept by mean / var / std (see KEEP_MOMENTS)."""
        self._cached = False
        self.__dict__.pop("_kept", None)   # (a finish queued ahead goes with its state: reduction.Queued)

    # ------------------------------------------------------------ movement
    def _permute(self, perm, split):
        """x.transpose(perm) as a new array with the given split (one kernel / one all-to-all)."""
        return self._move(_move_plan(self._shape, perm, split))

    def _move(self, mv):
        """Run a _move_plan on this array."""
        perm, split, new_shape, relabel, units_only = mv
        if relabel or (units_only and (perm[0] == 0 or self._ctx.world_size == 1)):
            # no bytes move: the identity, or only unit axes move, so the C-order
            # bytes are already the result's (across GPUs the leading axis,
            # hence every slab, stays put)
            data = self._data
        elif ROW_PITCH and self._ctx.world_size == 1:
            es = self._dtype.itemsize
            pp = self._pitch_of(mv, es)
            d = self.__dict__
            if "_pbuf" in d:
                # a padded source is read in place: its strides, permuted
                src, pstr = d["_pbuf"], _padded_strides(self._shape, d["_pitch"])
                sstr = [pstr[p] for p in perm]
            else:
                src, sstr = self._data, None
            be = backend_for(src.device)
            R = new_shape[-1]
            if pp is not None:
                P, rows, oshape, psstr, dstr = pp
            else:
                P, oshape, dstr = R, list(new_shape), _padded_strides(new_shape, R)
                if sstr is None:
                    # bm_permute's own strides: the same kernels, through the entry that takes the state
                    cstr = _padded_strides(self._shape, self._shape[-1])
                    psstr = [cstr[p] for p in perm]
            csstr = psstr if sstr is None else sstr
            st = self._swap_state(be, src.device, new_shape, es, oshape, csstr, dstr, P)
            if pp is None and sstr is None and st is None:
                # dense to dense and no state wanted: bm_permute's own launch
                return self._derive(permute_sharded(self._ctx, be, src, self._shape, perm, es), new_shape, split)
            # the one-GPU copy: padded or dense rows, with or without their state
            n = rows * P if pp is not None else int(np.prod(new_shape, dtype=np.int64))
            dst = _empty(n * es, src.device)
            if st is None:
                be.copy_strided(src, 0, dst, 0, oshape, csstr, dstr, es)
                fused = False
            else:
                fused = be.copy_strided(src, 0, dst, 0, oshape, csstr, dstr, es, moments=(st[0], R, P, st[1], st[2]))
            out = self._derive_padded(dst, P, new_shape, split) if pp is not None \
                else self._derive(dst, new_shape, split)
            return out._with_swap_state(st, fused)
        else:
            # across GPUs: the exchange's pack reads a padded source in place
            # and its unpack writes the result's rows at the same pitch rule
            # as on one GPU
            es = self._dtype.itemsize
            pp = self._pitch_of(mv, es) if ROW_PITCH else None
            d = self.__dict__
            src = d["_pbuf"] if "_pbuf" in d else self._data
            data = permute_sharded(self._ctx, backend_for(src.device), src, self._shape, perm, es,
                                   src_pitch=d.get("_pitch"), out_pitch=None if pp is None else pp[0])
            if pp is not None:
                return self._derive_padded(data, pp[0], new_shape, split)
        return self._derive(data, new_shape, split)

    def _swap_state(self, be, dev, new_shape, es, oshape, sstr, dstr, pitch):
        """(dtype code, rows, state buffer) for a one-GPU move into ``new_shape``
        (the copy ``oshape`` / ``sstr`` / ``dstr``, rows ``pitch`` elements
        apart) that should also leave its rows' STAT_VAR state, or None: the
        rule is at FUSE_SWAP_MOMENTS, and the library's plan of the copy says
        whether it can fuse at all before anything is allocated."""
        if not FUSE_SWAP_MOMENTS or self._dtype.kind != 'f' or es not in (4, 8) or self._dtype.byteorder == '>' \
                or len(new_shape) < 2 \
                or not getattr(be, "fuses_swap_moments", False):
            return None
        rows = int(np.prod(new_shape[:-1], dtype=np.int64))
        nbytes = rows * new_shape[-1] * es
        if not rows or nbytes <= _FUSE_SWAP_MIN_BYTES or 16 * rows > nbytes // _FUSE_SWAP_STATE_DIV:
            return None
        code = dtype_code(self._dtype)
        if not be.copy_moments_plan(oshape, sstr, dstr, es, code, new_shape[-1], pitch, rows)[3]:
            return None
        return code, rows, _empty(be.state_bytes(_lib.STAT_VAR, code, rows), dev)

    def _with_swap_state(self, st, fused):
        """Remember the state a move left (``fused``) for the last axis; it
        serves mean() too (see _kept_for)."""
        if fused:
            self.__dict__["_kept"] = {(len(self._shape) - 1,): Kept(st[2], self._shape[-1], st[1], None, True, {})}
        return self

    def _pitch_of(self, mv, es):
        """The pitched copy plan of move ``mv`` (cached, see _pitch_plan), or
        None when the result stays dense or the device lacks room for it."""
        key = (mv, es)
        pp = _PITCH_PLANS.get(key, False)
        if pp is False:
            pp = _pitch_plan(mv, self._shape, es)
            if len(_PITCH_PLANS) > 4096:
                _PITCH_PLANS.clear()
            _PITCH_PLANS[key] = pp
        if pp is not None and not _pitch_fits(pp, es, self._device):
            return None
        return pp

    def chunk(self, size="150", axis=None, padding=None):
        """Chunk the values of every record (array.py:678-714) -> ChunkedArrayMI355X."""
        if type(size) is not str:
            size = tupleize((size))
        axis = tupleize((axis))
        padding = tupleize((padding))
        from bolt_amd.mi355x.chunk import ChunkedArrayMI355X
        return ChunkedArrayMI355X._from_array(self, size, axis, padding)

    def swap(self, kaxes, vaxes, size="150"):
        """Move key axes to the values and value axes to the keys (array.py:716-763).

        Same validation and result as the reference: x.transpose(P) with
        P = [keys kept] + [moved values] + [moved keys] + [values kept] and
        split' = split - #kaxes + #vaxes.  ``size`` only chooses the Spark
        chunking; it is validated the same way (getplan + _chunk checks) and
        does not change the result.  Executed as one permute kernel.
        """
        # host plan of an already validated (shape, split, dtype, axes, size):
        # first under the arguments as given, then canonicalised
        try:
            raw = (self._shape, self._split, self._dtype, kaxes, vaxes, size)
            hit = _SWAP_PLANS.get(raw)
        except TypeError:  # unhashable arguments (lists)
            raw = hit = None
        if hit is None:
            try:
                key = (self._shape, self._split, self._dtype, tuple(int(k) for k in tupleize(kaxes)),
                       tuple(int(v) for v in tupleize(vaxes)), size if type(size) is str else tupleize(size))
                hash(key)
            except (TypeError, ValueError):
                key = None
            hit = _SWAP_PLANS.get(key) if key is not None else None
            if hit is None:
                plan = self._swap_plan(kaxes, vaxes, size)
                if plan is None:
                    hit = _NOOP
                else:
                    mv = _move_plan(self._shape, *plan[:2])
                    ref = swap_shape(self._shape, self._split, *plan[2:])
                    # the reference's unit-axis squeezes (plan.swap_shape): a relabel
                    hit = (mv, ref[0] if ref is not None and ref[0] != mv[2] else None)
            if len(_SWAP_PLANS) > 4096:
                _SWAP_PLANS.clear()
            for k in (key, raw):
                if k is not None:
                    _SWAP_PLANS[k] = hit
        if hit is _NOOP:
            return self
        mv, squeezed = hit
        out = self._move(mv)
        return out if squeezed is None else out._relabel(squeezed)

    def _relabel(self, shape):
        """The same records under ``shape`` -- this shape with unit axes
        dropped, split unchanged (the reference's swap squeezes)."""
        d = self.__dict__
        if "_pbuf" in d and len(shape) >= 2 and shape[-1] == self._shape[-1]:
            return self._derive_padded(d["_pbuf"], d["_pitch"], shape, self._split)
        return self._derive(self._data, shape, self._split)

    def _swap_plan(self, kaxes, vaxes, size):
        """Validation and net permutation of swap: (perm, newsplit), or None for a no-op."""
        kaxes = np.asarray(tupleize(kaxes), 'int')
        vaxes = np.asarray(tupleize(vaxes), 'int')
        if type(size) is not str:
            size = tupleize(size)

        if len(kaxes) == self.keys.ndim and len(vaxes) == 0:
            raise ValueError('Cannot perform a swap that would '
                             'end up with all data on a single key')

        if len(kaxes) == 0 and len(vaxes) == 0:
            return None

        # the chunk plan the reference would build (errors surface the same way)
        if not (self._split == self.ndim):
            _check_swap_plan(self._shape[self._split:], self._dtype, size)
        # axes index boolean masks in the reference (chunk.py:224, :293):
        # negative axes count from the end, out-of-range ones raise IndexError
        nv = self.ndim - self._split
        for k in kaxes:
            if not -self._split <= k < self._split:
                raise IndexError("key axis %d out of range for %d keys" % (k, self._split))
        for v in vaxes:
            if not -nv <= v < nv:
                raise IndexError("value axis %d out of range for %d values" % (v, nv))
        kaxes = [int(k) % self._split for k in kaxes]
        vaxes = [int(v) % nv for v in vaxes] if nv else []

        return swap_perm(self.ndim, self._split, kaxes, vaxes) + (kaxes, vaxes)

    def transpose(self, *axes):
        """Permute the axes, split unchanged (array.py:765-808)."""
        if len(axes) == 0:
            p = np.arange(self.ndim - 1, -1, -1)
        else:
            p = np.asarray(argpack(axes))
        istransposeable(p, range(self.ndim))
        return self._permute([int(x) for x in p], self._split)

    @property
    def T(self):
        """Reverse the axes (array.py:810-815)."""
        return self.transpose()

    def swapaxes(self, axis1, axis2):
        """Interchange two axes (array.py:817-833)."""
        p = list(range(self.ndim))
        p[axis1] = axis2
        p[axis2] = axis1
        return self.transpose(p)

    def reshape(self, *shape):
        """Same data, new shape (array.py:835-877): only reshapes that split into
        an independent reshape of the keys and one of the values
        (NotImplementedError otherwise, as the reference).  On the dense
        layout both are metadata, plus a re-slab across GPUs when the leading
        key axis changes (shapes.py:40-64, :111-134)."""
        new = argpack(shape)
        isreshapeable(new, self.shape)
        if new == self.shape:
            return self
        i = self._reshapebasic(new)
        if i == -1:
            raise NotImplementedError("Currently no support for reshaping between "
                                      "keys and values for BoltArraySpark")
        return self.keys.reshape(new[:i]).values.reshape(new[i:])

    def _reshapebasic(self, shape):
        """Index in ``shape`` splitting it into key and value parts of the old
        key and value sizes, or -1 (array.py:861-877)."""
        new = tupleize(shape)
        old_key = int(np.prod(self.keys.shape, dtype=np.int64))
        old_val = int(np.prod(self.values.shape, dtype=np.int64))
        for i in range(len(new)):
            if int(np.prod(new[:i], dtype=np.int64)) == old_key and \
                    int(np.prod(new[i:], dtype=np.int64)) == old_val:
                return i
        return -1

    def astype(self, dtype, casting='unsafe'):
        """Cast every record to ``dtype`` (array.py:920-930), on the device.

        numpy's casting rule is checked on the host (np.can_cast raises the
        same TypeError numpy's astype would); the conversion itself is torch's
        elementwise cast, numpy's values for every finite in-range input."""
        from bolt_amd.mi355x import functional as F
        dtype = np.dtype(dtype)
        if not np.can_cast(self._dtype, dtype, casting):
            raise TypeError("Cannot cast array data from %r to %r according to the rule %r"
                            % (self._dtype, dtype, casting))
        d = self.__dict__
        if dtype == self._dtype:
            if "_pbuf" in d:
                return self._derive_padded(d["_pbuf"].clone(), d["_pitch"], self._shape, self._split)
            return self._like(self._data.clone(), self._shape, self._split)
        src = self._elements()
        out = F.as_bytes(src.to(F.torch_dtype(dtype)))
        return self._like(out, self._shape, self._split, dtype=dtype)

    def _elements(self, shape=None):
        """This rank's elements, in C order, as a torch view of ``shape``
        (default: flat -- for a row-padded array (rows, row length), a strided
        view of the padded rows, so elementwise work reads them in place)."""
        from bolt_amd.mi355x import functional as F
        d = self.__dict__
        if "_pbuf" in d:
            R = self._shape[-1]
            rows = int(np.prod(self._local_shape[:-1], dtype=np.int64))
            v = F.view(d["_pbuf"], (rows, d["_pitch"]), self._dtype)[:, :R]
            return v if shape is None else v.view(tuple(shape))
        n = self._data.numel() // max(1, self._dtype.itemsize)
        return F.view(self._data, (n,) if shape is None else tuple(shape), self._dtype)

    def clip(self, min=None, max=None):
        """Clip values below ``min`` / above ``max`` (array.py:932-945), on the device.

        The result dtype is numpy's for ``record.clip(min, max)`` (numpy is asked
        on a 1-element record, so its errors are numpy's too): a float bound on an
        integer array promotes.  torch has no max/min kernels for uint16/32/64,
        so unsigned records are compared in a wider signed type (uint64: with
        the sign bit flipped, which maps unsigned order onto signed order)."""
        import torch
        from bolt_amd.mi355x import functional as F
        rdt = np.zeros(1, self._dtype).clip(min=min, max=max).dtype
        x = self._elements(self._local_shape)
        vs = tuple(self._shape[self._split:])
        wide = {1: torch.int16, 2: torch.int32, 4: torch.int64}
        if rdt != self._dtype:
            x = x.to(F.torch_dtype(rdt))
        if rdt.kind == "u" and rdt.itemsize < 8:
            out, back = x.to(wide[rdt.itemsize]), F.torch_dtype(rdt)
        elif rdt.kind == "u":
            flip = torch.tensor(-(1 << 63), dtype=torch.int64, device=x.device)
            out, back = x.view(torch.int64) ^ flip, None
        else:
            out, back = x.clone(), None
        for bound, fn in ((min, torch.maximum), (max, torch.minimum)):
            if bound is None:
                continue
            nb = np.asarray(bound).astype(rdt)
            if nb.ndim > len(vs):
                raise ValueError("clip bound of shape %s does not broadcast to records %s" % (nb.shape, vs))
            if rdt.kind == "u" and rdt.itemsize < 8:
                b = torch.as_tensor(nb.astype(np.int64), device=out.device).to(out.dtype)
            elif rdt.kind == "u":
                b = torch.as_tensor(nb.view(np.int64), device=out.device) ^ flip
            else:
                b = torch.as_tensor(nb, device=out.device)
            out = fn(out, b)
        if rdt.kind == "u":
            out = out.to(back) if back is not None else (out ^ flip).view(torch.uint64)
        return self._like(F.as_bytes(out.contiguous()), self._shape, self._split, dtype=rdt)

    def repartition(self, npartitions):
        """Records stay sharded one slab per GPU; only the partition count the
        array reports changes, and, as after Spark's repartition, the array is
        marked unordered (array.py:49-60)."""
        out = self._like(self._data, self._shape, self._split)
        out._npartitions = npartitions
        out._ordered = False
        return out

    # ---------------------------------------------------------- functional
    def stack(self, size=None):
        """Group each partition's records into stacks of up to ``size`` (array.py:62-83)."""
        from bolt_amd.mi355x.stack import StackedArrayMI355X
        return StackedArrayMI355X._from_array(self, size)

    def _align(self, axis):
        """Swap so that ``axis`` are exactly the keys (array.py:85-115)."""
        inshape(self.shape, axis)
        tokeys = [(a - self._split) for a in axis if a >= self._split]
        tovalues = [a for a in range(self._split) if a not in axis]
        if tokeys or tovalues:
            return self.swap(tovalues, tokeys)
        return self

    def first(self):
        """The first record's value, on the host (array.py:117-123)."""
        from bolt_amd.mi355x.dist import all_gather_bytes
        es = self._dtype.itemsize
        rec = int(np.prod(self._shape[self._split:], dtype=np.int64))
        rb = rec * es
        d = self.__dict__
        if "_pbuf" in d and rec > self._shape[-1]:
            # padded rows: gather the first record's rows, no compaction
            R = self._shape[-1]
            buf = _empty(rb, d["_pbuf"].device)
            self._backend.copy_strided(d["_pbuf"], 0, buf, 0, [rec // R, R], [d["_pitch"], 1], [R, 1], es)
        elif "_pbuf" in d:
            buf = d["_pbuf"][:rb]  # within the first row
        else:
            buf = self._data[:rb]
        if self._ctx.world_size > 1:
            lo, hi = self._ctx.bounds(self._shape[0])[0]
            sizes = [rb if r == 0 else 0 for r in range(self._ctx.world_size)]
            buf = all_gather_bytes(self._ctx, buf if self._ctx.rank == 0 else buf[:0], sizes)
        return BoltArrayLocal(to_host(buf, self._dtype, self._shape[self._split:]))

    def _records_tensor(self):
        """This rank's records as a (records, *value shape) torch view."""
        from bolt_amd.mi355x import functional as F
        lshape = self._local_shape
        nrec = int(np.prod(lshape[:self._split], dtype=np.int64))
        vshape = tuple(self._shape[self._split:])
        d = self.__dict__
        if "_pbuf" in d and vshape and int(np.prod(vshape[:-1], dtype=np.int64)) == 1:
            # padded rows, one row per record: each record is still contiguous
            # (only the records are P elements apart), so the functions that
            # see them cannot tell; no compaction
            rows = F.view(d["_pbuf"], (nrec, d["_pitch"]), self._dtype)[:, :vshape[-1]]
            return rows.view((nrec,) + vshape)
        return F.view(self._data, (nrec,) + vshape, self._dtype)

    def map(self, func, axis=(0,), value_shape=None, dtype=None, with_keys=False):
        """Apply ``func`` to every record along ``axis`` (array.py:125-191).

        The array is aligned (swapped) so ``axis`` are the keys, then ``func``
        runs on every record -- a torch tensor on the GPU -- vmapped over all
        of this rank's records at once (record by record with keys when
        ``with_keys``: func((key tuple, value))).  Shape inference, checks and
        the result's shape/split follow the reference.
        """
        from bolt_amd.mi355x import functional as F
        axis = tupleize(axis)
        swapped = self._align(axis)
        dev = swapped._device
        func = F.user_fn(func)
        test_func = (lambda x: func((F.KeyTuple((0,) * len(axis)), x))) if with_keys else func
        if value_shape is None or dtype is None:
            try:
                mapped = F.to_device(test_func(F.random_like(swapped.values.shape, self._dtype, dev)), dev)
            except Exception:
                mapped = F.to_device(test_func(swapped._records_tensor()[0]), dev)
            if value_shape is None:
                value_shape = tuple(mapped.shape)
            if dtype is None:
                dtype = F.numpy_dtype(mapped.dtype)
        value_shape = tupleize(value_shape)
        dtype = np.dtype(dtype)
        shape = tuple([swapped._shape[ax] for ax in range(len(axis))]) + value_shape
        recs = swapped._records_tensor()
        if with_keys:
            import torch
            lo, _ = swapped._ctx.local_bounds(swapped._shape[0]) if swapped._shape else (0, 0)
            kshape = swapped._shape[:swapped._split]
            base = lo * int(np.prod(kshape[1:], dtype=np.int64))
            outs = [F.to_device(func((F.KeyTuple(int(k) for k in np.unravel_index(base + i, kshape)), recs[i])), dev)
                    for i in range(recs.shape[0])]
            out = torch.stack(outs) if outs else None
        else:
            out = F.apply_batched(func, recs)
        if out is not None and len(out.shape) > 1 and tuple(out.shape[1:]) != value_shape:
            raise Exception("Map operation did not produce values of uniform shape.")
        data = F.as_bytes(out.to(F.torch_dtype(dtype))) if out is not None else _empty(0, dev)
        return self._like(data, shape, swapped.split, dtype=dtype)

    def filter(self, func, axis=(0,), sort=False):
        """Keep the records along ``axis`` for which ``func`` is true (array.py:193-241).

        ``func`` runs on every record (a torch tensor, vmapped) and returns a
        boolean; the kept records are compacted with one gather kernel (and an
        all-to-all across GPUs) and re-keyed 0..count-1 in key order.
        """
        from bolt_amd.mi355x import functional as F
        from bolt_amd.mi355x.indexing import gather_units_sharded
        axis = tupleize(axis)
        swapped = self._align(axis)
        recs = swapped._records_tensor()
        func = F.user_fn(func)
        keep = F.apply_batched(lambda v: F.to_device(func(v), v.device).reshape(()).to(bool), recs)
        mask = keep.cpu().numpy().reshape(-1) if keep is not None else np.zeros(0, bool)
        ctx = swapped._ctx
        local_idx = np.nonzero(mask)[0].astype(np.int64)
        if ctx.world_size > 1:
            # every rank's mask (one byte per record, rank order) on every rank
            import torch
            per = int(np.prod(swapped.shape[1:swapped.split], dtype=np.int64))
            sizes = [(hi - lo) * per for lo, hi in ctx.bounds(swapped.shape[0])]
            mb = torch.from_numpy(mask.astype(np.uint8)).to(swapped._device)
            allm = all_gather_bytes(ctx, mb, sizes).cpu().numpy()
            glob = np.nonzero(allm)[0].astype(np.int64)
        else:
            glob = local_idx
        remaining = list(swapped.shape[len(axis):])
        count = int(glob.size)
        es = self._dtype.itemsize
        rowbytes = int(np.prod(remaining, dtype=np.int64)) * es
        nrec = int(np.prod(swapped.shape[:swapped.split], dtype=np.int64))
        if count == 0:
            return self._like(_empty(0, swapped._device), (0,), 1)
        # records are rows of the flattened key space; ragged per rank
        flat_rows_per_lead = int(np.prod(swapped.shape[1:swapped.split], dtype=np.int64))
        d = swapped.__dict__
        if "_pbuf" in d and remaining:
            # padded rows (one GPU): whole padded records move, the result keeps the pitch
            P = d["_pitch"]
            prb = rowbytes // (remaining[-1] * es) * P * es
            data = gather_units_sharded(ctx, swapped._backend, d["_pbuf"], swapped.shape[0],
                                        prb, flat_rows_per_lead, glob, count, 1)
            return self._derive_padded(data, P, tuple([count] + remaining), 1)
        data = gather_units_sharded(ctx, swapped._backend, swapped._data, swapped.shape[0],
                                    rowbytes, flat_rows_per_lead, glob, count, 1)
        return self._like(data, tuple([count] + remaining), 1)

    # ------------------------------------------------------------ indexing
    def __getitem__(self, index):
        """Index with ints, slices and lists (array.py:595-676).

        Same normalisation, bounds errors, result shape/split and element
        order as the reference (indexing.py): basic selections are one
        strided copy, list selections one gather kernel; across GPUs rows
        move with one all-to-all.  Int axes are squeezed out; an all-int
        index returns a scalar.
        """
        from bolt_amd.mi355x import indexing
        index, int_locs, kind = indexing.normalize(index, self._shape, self._split)
        es = self._dtype.itemsize
        if kind == 'basic':
            starts = [s.start for s in index]
            steps = [s.step for s in index]
            shape = tuple(int(np.ceil((s.stop - s.start) / float(s.step))) for s in index)
            d = self.__dict__
            if "_pbuf" in d:  # padded rows: selected in place, no compaction
                data = select_sharded(self._ctx, self._backend, d["_pbuf"], self._shape, starts, steps, shape, es,
                                      src_strides=_padded_strides(self._shape, d["_pitch"]))
            else:
                data = select_sharded(self._ctx, self._backend, self._data, self._shape, starts, steps, shape, es)
            result = self._like(data, shape, self._split)
        elif kind == 'advanced':
            pts, shape = indexing.advanced_points(index, self._shape, self._split)
            if len(shape) == 0:
                raise ValueError("0-d index arrays are not supported")
            out_upr = int(np.prod(shape[1:], dtype=np.int64))
            d = self.__dict__
            upr = int(np.prod(self._shape[1:], dtype=np.int64))
            if "_pbuf" in d:
                # padded rows: the elements' offsets in the padded layout
                Rl, P = self._shape[-1], d["_pitch"]
                src, pts, upr = d["_pbuf"], pts // Rl * P + pts % Rl, upr // Rl * P
            else:
                src = self._data
            data = indexing.gather_units_sharded(self._ctx, self._backend, src, self._shape[0], es, upr, pts,
                                                 shape[0], out_upr)
            result = self._like(data, shape, len(shape))
        else:
            loc, idx = indexing.mixed_take(index, self._shape, self._split)
            newshape = list(self._shape)
            newshape[loc] = len(idx)
            d = self.__dict__
            if "_pbuf" in d and self._ctx.world_size == 1:
                # padded rows (one GPU): taking along the last axis gathers
                # within the rows (a dense result); along another axis whole
                # padded rows move and the result keeps the pitch
                P, nd = d["_pitch"], self.ndim
                n_outer = int(np.prod(self._shape[:min(loc, nd - 1)], dtype=np.int64))
                if loc == nd - 1:
                    data = _empty(n_outer * len(idx) * es, d["_pbuf"].device)
                    if n_outer and len(idx):
                        self._backend.gather_rows(d["_pbuf"], 0, data, 0, n_outer, P, es, idx)
                    taken = self._like(data, tuple(newshape), self._split)
                else:
                    row = int(np.prod(self._shape[loc + 1:-1], dtype=np.int64)) * P * es
                    data = _empty(n_outer * len(idx) * row, d["_pbuf"].device)
                    if data.numel():
                        self._backend.gather_rows(d["_pbuf"], 0, data, 0, n_outer, self._shape[loc], row, idx)
                        taken = self._derive_padded(data, P, tuple(newshape), self._split)
                    else:
                        taken = self._like(data, tuple(newshape), self._split)
            else:
                data = indexing.take_sharded(self._ctx, self._backend, self._data, self._shape, es, loc, idx)
                taken = self._like(data, tuple(newshape), self._split)
            rest = list(index)
            rest[loc] = slice(0, None, None)
            full = all(isinstance(r, slice) and r.step in (None, 1) and (r.start or 0) == 0 and
                       (r.stop is None or r.stop >= d) for r, d in zip(rest, taken.shape))
            # the other axes untouched: the gathered array is the result (no second copy)
            result = taken if full and not int_locs else taken[tuple(rest)]
        if len(int_locs) == self.ndim:
            return result.toarray().reshape(())[()]
        return result.squeeze(tuple(int_locs)) if int_locs else result

    def concatenate(self, arry, axis=0):
        """Join with another array along ``axis`` (array.py:429-478).

        ndarrays (and local bolt arrays, which are ndarrays) are first built
        as mi355x arrays keyed on this array's key axes, as the reference does;
        the same shape checks and exceptions.  On the dense layout the result
        is two strided copies (rows of the two inputs interleaved at the
        concatenation axis); along the sharded leading axis across GPUs, one
        all-to-all re-slabs the rows.
        """
        from bolt_amd.mi355x.construct import ConstructMI355X
        if isinstance(arry, np.ndarray):
            arry = ConstructMI355X.array(arry, self._ctx, axis=range(0, self._split))
        elif not isinstance(arry, BoltArrayMI355X):
            raise ValueError("other must be local array or mi355x array, got %s" % type(arry))
        if not all([x == y if not i == axis else True
                    for i, (x, y) in enumerate(zip(self.shape, arry.shape))]):
            raise ValueError("all the input array dimensions except for "
                             "the concatenation axis must match exactly")
        if not self._split == arry.split:
            raise NotImplementedError("two arrays must have the same split ")
        if self.ndim != arry.ndim or not 0 <= axis < self.ndim:
            raise ValueError("arrays of %d and %d dimensions cannot be joined on axis %d"
                             % (self.ndim, arry.ndim, axis))
        if arry.dtype != self._dtype:
            raise NotImplementedError("concatenating %s with %s: cast one first (astype)"
                                      % (self._dtype, arry.dtype))
        shape = tuple([x + y if i == axis else x for i, (x, y) in enumerate(zip(self.shape, arry.shape))])
        es = self._dtype.itemsize
        if axis == 0:
            rowbytes = int(np.prod(self._shape[1:], dtype=np.int64)) * es
            data = concat_rows_sharded(self._ctx, self._data, self._shape[0], arry._data, arry.shape[0], rowbytes)
            return self._like(data, shape, self._split)
        lshape = self._local_shape
        outer = int(np.prod(lshape[:axis], dtype=np.int64))
        inner = int(np.prod(lshape[axis + 1:], dtype=np.int64))
        na, nb = self._shape[axis] * inner, arry.shape[axis] * inner
        data = _empty(outer * (na + nb) * es, self._data.device)
        if outer:
            be = self._backend
            if na:
                be.copy_strided(self._data, 0, data, 0, [outer, na], [na, 1], [na + nb, 1], es)
            if nb:
                be.copy_strided(arry._data, 0, data, na * es, [outer, nb], [nb, 1], [na + nb, 1], es)
        return self._like(data, shape, self._split)

    def squeeze(self, axis=None):
        """Drop singleton axes (array.py:879-918); the data does not move on one
        GPU, and re-slabs across GPUs when the leading axis goes away."""
        if not any(d == 1 for d in self._shape):
            return self
        if axis is None:
            drop = [i for i, d in enumerate(self._shape) if d == 1]
        elif isinstance(axis, int):
            drop = [axis]
        elif isinstance(axis, tuple):
            drop = [int(a) for a in axis]
        else:
            raise ValueError("an integer or tuple is required for the axis")
        if any(self._shape[i] > 1 for i in drop):
            raise ValueError("cannot select an axis to squeeze out which has size greater than one")
        if not drop:
            return self
        shape = tuple(d for i, d in enumerate(self._shape) if i not in drop)
        split = len([d for d in range(self._split) if d not in drop])
        d = self.__dict__
        if "_pbuf" in d and len(shape) >= 2 and (self.ndim - 1) not in drop and \
                (0 not in drop or self._ctx.world_size == 1):
            # unit axes only: a padded array's rows stay as they are
            return self._derive_padded(d["_pbuf"], d["_pitch"], shape, split)
        data = self._data
        if 0 in drop and self._ctx.world_size > 1:
            # the leading axis goes: re-slab on the new one (a 0-d result lives on rank 0)
            es = self._dtype.itemsize
            new_rows = shape[0] if shape else 1
            new_rowbytes = int(np.prod(shape[1:], dtype=np.int64)) * es if shape else es
            data = redistribute_rows(self._ctx, data, self._shape[0],
                                     int(np.prod(self._shape[1:], dtype=np.int64)) * es, new_rows, new_rowbytes)
        return self._like(data, shape, split)

    # ---------------------------------------------------------- statistics
    def _reduced(self, axis, stat):
        """Device reduction of ``axis`` -> host ndarray with the kept axes (ascending).

        Returns (result ndarray, out dtype).  Plan, source layouts and the
        finish are reduction.py's; what is kept and served is decided here.
        """
        plan, out_dtype, ocode = reduction.plan_for(self, axis, stat)
        axes, code = plan.axes, plan.code
        entry = self._kept_for(axes, stat) if "_kept" in self.__dict__ else None
        if entry is not None:
            return self._from_kept(entry, stat, plan, out_dtype, ocode), out_dtype
        src = reduction.source(self, plan, stat in _MOMENTS)
        buf, O, R, I, pitch, nlaunch, drop, every = src
        dev = buf.device
        be = backend_for(dev)
        if every:
            mean, var = reduction.every_axis_moments(be, src, stat, code)
            v = mean if stat == _lib.STAT_MEAN else var if stat == _lib.STAT_VAR else np.sqrt(var)
            return np.asarray(v, dtype=np.float64).astype(out_dtype).reshape(plan.out_shape), out_dtype
        single = plan.world == 1
        if single or 0 not in axes:
            # every output lives on this rank (or this rank's slab of them)
            run = nlaunch and plan.nloc
            outs = reduction.outputs(be, dev, out_dtype, 1, nlaunch, single and run)
            if run:
                # the one reduce / reduce_rows call; with a state buffer the launch
                # may keep its STAT_VAR state there, remembered for these axes (a
                # state kept after source's permute serves later calls without it;
                # a padded array's holds the pad columns' states too: dropped as
                # the outputs)
                st = self._keep_state(be, dev, axes, stat, code, nlaunch, O * R * I, I > 1)
                fn, last = (be.reduce_rows, pitch) if pitch != R else (be.reduce, I)
                if st is None:
                    fn(stat, buf, code, O, R, last, outs[0][0], ocode)
                elif fn(stat, buf, code, O, R, last, outs[0][0], ocode, state=st):
                    self.__dict__.setdefault("_kept", {})[axes] = Kept(st, R, nlaunch, drop, False)
            return reduction.finish(outs, dev, plan, out_dtype, 1, nlaunch, drop, None if single else self._ctx)[0], \
                out_dtype
        # the sharded axis is reduced: per-rank states, gathered and combined in rank order
        if plan.nout == 0:  # e.g. mean(axis=0) of (4, 0, 3): nothing to merge
            return np.empty(plan.out_shape, out_dtype), out_dtype
        states, counts = reduction.sharded_states(self._ctx, be, dev, plan, stat, src)
        outs = reduction.outputs(be, dev, out_dtype, 1, plan.nout, False)
        be.reduce_combine(stat, code, states, counts, plan.nout, outs[0][0], ocode)
        return reduction.finish(outs, dev, plan, out_dtype, 1, plan.nout)[0], out_dtype

    def _kept_for(self, axes, stat):
        """The kept state that serves ``stat`` over ``axes`` without a read of
        the array, or None.  The rule: var / std are served from any kept state
        when KEEP_MOMENTS is on (a later mean() reads again: its bits come from
        other arithmetic than the state's mean); mean, var and std are all
        served from a state that serves the mean -- one the swap's transpose
        left (_with_swap_state) -- whatever KEEP_MOMENTS says."""
        held = self.__dict__.get("_kept")
        entry = held.get(axes) if held else None
        if entry is not None and stat in _MOMENTS \
                and (entry.serves_mean or (KEEP_MOMENTS and stat != _lib.STAT_MEAN)):
            return entry
        return None

    def _keep_state(self, be, dev, axes, stat, code, nlaunch, nread, cols):
        """The buffer a mean / var / std launch of ``nlaunch`` outputs over
        ``nread`` elements stores its STAT_VAR state into, or None where none
        is kept (the rule is at KEEP_MOMENTS) or these axes' is held already.
        ``cols``: the launch is a column reduction (I > 1)."""
        if not KEEP_MOMENTS or stat not in _MOMENTS or self._dtype.kind != 'f' or self._ctx.world_size != 1 \
                or not getattr(be, "keeps_moments", False):
            return None
        if cols and not _KEEP_COLS:
            return None
        held = self.__dict__.get("_kept")
        if held and axes in held:
            return None
        nbytes = nread * self._dtype.itemsize
        if nbytes <= _KEEP_MIN_BYTES or 16 * nlaunch > nbytes // _KEEP_STATE_DIV:
            return None
        return _empty(be.state_bytes(_lib.STAT_VAR, code, nlaunch), dev)

    def _from_kept(self, entry, stat, plan, out_dtype, ocode):
        """A statistic finished from a kept state: one reduce_combine of one part
        into the host result of the launch that kept it, no read of the array."""
        dev = entry.state.device
        be = backend_for(dev)
        ahead = entry.ahead
        queued = ahead.pop(stat, None) if ahead else None
        with np.errstate(all="ignore"):  # pad columns' unwritten values, as in reduction.combine_moments
            if queued is not None:
                # finished ahead by the other statistic's call: its event, no launch
                return reduction.finish(queued.take(), dev, plan, out_dtype, 1, entry.nlaunch, entry.drop,
                                        event=queued.event)[0]
            outs = reduction.outputs(be, dev, out_dtype, 1, entry.nlaunch, True)
            be.reduce_combine(stat, plan.code, entry.state, [entry.count], entry.nlaunch, outs[0][0], ocode)
            event = None
            other = _AHEAD_OF.get(stat)
            if FINISH_AHEAD and other is not None and ahead is not None and not ahead and outs[1] is not None:
                odt, oc = reduction.plan_for(self, plan.axes, other)[1:]
                outs2 = reduction.outputs(be, dev, odt, 1, entry.nlaunch, True)
                if outs2[1] is not None:
                    event = reduction.record_event(dev)
                    be.reduce_combine(other, plan.code, entry.state, [entry.count], entry.nlaunch, outs2[0][0], oc)
                    ahead[other] = reduction.Queued(outs2, reduction.record_event(dev))
                    ahead[None] = True   # one plane per state: a later call queues no second one
            return reduction.finish(outs, dev, plan, out_dtype, 1, entry.nlaunch, entry.drop, event=event)[0]

    def _reduced_moments(self, axis, want):
        """_reduced for several moments of one read: ``want`` is a subset of
        ('mean', 'var', 'std') in that order -> {field: host ndarray with the
        kept axes (ascending)}.  The data is read by one STAT_VAR launch
        sequence (bm_reduce_moments), so var and std carry the bits of their
        own methods."""
        plan, out_dtype, ocode = reduction.plan_for(self, axis, _lib.STAT_VAR)
        src = reduction.source(self, plan)
        nlaunch, drop, every = src[5:]
        dev = src.buf.device
        be = backend_for(dev)
        code, k = plan.code, len(want)
        single = plan.world == 1
        if every:
            mean, var = reduction.every_axis_moments(be, src, _lib.STAT_VAR, code)
            vals = {'mean': mean, 'var': var, 'std': np.sqrt(var)}
            return dict((f, np.asarray(vals[f], dtype=np.float64).astype(out_dtype).reshape(plan.out_shape))
                        for f in want)
        if single or 0 not in plan.axes:
            # every output lives on this rank (or this rank's slab of them)
            run = nlaunch and plan.nloc
            outs = reduction.outputs(be, dev, out_dtype, k, nlaunch, single and run)
            if run:
                reduction.launch_moments(be, src, self._dtype.itemsize, code, ocode, want, outs[0])
            res = reduction.finish(outs, dev, plan, out_dtype, k, nlaunch, drop, None if single else self._ctx)
        elif plan.nout == 0:
            return dict((f, np.empty(plan.out_shape, out_dtype)) for f in want)
        else:
            # the sharded axis is reduced: one STAT_VAR state per rank, gathered
            # once and merged in rank order into every moment
            states, counts = reduction.sharded_states(self._ctx, be, dev, plan, _lib.STAT_VAR, src)
            outs = reduction.outputs(be, dev, out_dtype, k, plan.nout, False)
            reduction.combine_moments(be, code, ocode, want, states, counts, plan.nout, outs[0])
            res = reduction.finish(outs, dev, plan, out_dtype, k, plan.nout)
        return dict(zip(want, res))

    def stats(self, axis=None, keepdims=False, names=_STATS_FIELDS):
        """Several moments over ``axis`` from one read of the array: the
        reference's StatCounter (statcounter.py:30-48, stats='all') holds the
        count, mean and M2 of one pass, of which _stat (array.py:284-334)
        reads one per call.  An addition to the reference's API.

        ``names``: a non-empty subset of 'mean', 'var', 'std' (one string, or
        the reference's spellings 'variance' / 'stdev').  Returns a ``Stats``
        namedtuple (count, mean, var, std): count is the number of records
        reduced per output; each field asked for is what its method returns
        (var and std bit for bit, the mean within rounding: it is the Welford
        mean of the variance's state), the others None.
        """
        if isinstance(names, str):
            names = (names,)
        try:
            asked = set(_STATS_NAMES[n] for n in names)
        except (KeyError, TypeError):
            raise ValueError("stats: names must be among %s, got %r" % (sorted(_STATS_NAMES), names))
        if not asked:
            raise ValueError("stats: no statistic asked for")
        want = tuple(f for f in _STATS_FIELDS if f in asked)
        ax = tupleize(list(range(len(self.shape))) if axis is None else axis)
        inshape(self.shape, ax)
        count = self._nrecords(ax)
        if len(want) == 1:
            one = getattr(self, want[0])(axis=axis, keepdims=keepdims)
            return Stats(count=count, **dict((f, one if f == want[0] else None) for f in _STATS_FIELDS))
        if count == 0:
            # the empty StatCounter, as _stat gives it: mean 0.0, variance / stdev nan
            res = dict((f, 0.0 if f == 'mean' else float('nan')) for f in want)
        else:
            vs = self._aligned_vshape(ax)
            res = self._reduced_moments(ax, want)
            for f in want:
                arr = res[f]
                if vs is not None:
                    arr = arr.reshape(vs)
                if arr.ndim == 0:
                    arr = arr[()]
                res[f] = arr
        out = dict.fromkeys(_STATS_FIELDS)
        for f in want:
            arr = res[f]
            if keepdims:
                for i in ax:
                    arr = np.expand_dims(arr, axis=i)
            out[f] = BoltArrayLocal(arr).toscalar()
        return Stats(count=count, **out)

    def _standardized(self, axis, scale):
        """center (``scale`` False) / zscore (True) over ``axis``: a new device
        array of this array's shape and split, every record minus its mean [over
        its population standard deviation], in the dtype of ``record - 0.0``.

        Planned with plan.reduce_layout like _reduced_moments, and what it costs:
          * the last axis (rows dense or row-padded, read in place): one
            bm_standardize_rows launch, one read and one write; a padded input
            whose item size is kept gives a result padded alike;
          * rows that launch does not take, and reduced axes that form one
            block: the float64 mean / std planes from one read
            (bm_reduce_moments), then bm_standardize_apply: two reads and one
            write;
          * reduced axes that are not one block: permuted to the front first
            and the result permuted back -- two more reads and writes;
          * a row-padded input over other axes than the last: copied to a dense
            temporary first (the array itself stays padded) -- one more read
            and write;
          * the sharded axis reduced: per-rank states, gathered and merged in
            rank order as in _reduced_moments, then applied to this rank's slab.
        Moment states (KEEP_MOMENTS) are neither used nor left."""
        ax = tupleize(list(range(len(self.shape))) if axis is None else axis)
        inshape(self.shape, ax)
        plan, out_dtype, ocode = reduction.plan_for(self, ax, reduction.STANDARDIZE)
        code = plan.code
        dev = self._device
        if self.size == 0:
            return self._like(_empty(0, dev), self._shape, self._split, dtype=out_dtype)
        be = backend_for(dev)
        perm, O, R, I, nloc = plan.perm, plan.O, plan.R, plan.I, plan.nloc
        es, oes = self._dtype.itemsize, out_dtype.itemsize
        d = self.__dict__
        pbuf, P = d.get("_pbuf"), d.get("_pitch")
        # every reduced record lies whole on this rank
        local = plan.world == 1 or 0 not in plan.axes
        # the reduced axis is the last one: rows, a pitch apart
        rows_last = perm is None and I == 1 and local and (pbuf is None or R == plan.lshape[-1])

        if rows_last and nloc and hasattr(be, "standardize_rows"):
            keep_pad = pbuf is not None and oes == es
            dp = P if keep_pad else R
            dst = _empty(O * dp * oes, dev)
            src, sp = (pbuf, P) if pbuf is not None else (self._data, R)
            if be.standardize_rows(src, code, O, R, sp, dst, ocode, dp, scale):
                if not keep_pad:
                    return self._like(dst, self._shape, self._split, dtype=out_dtype)
                new = self._derive_padded(dst, P, self._shape, self._split)
                new.__dict__["_dtype"] = out_dtype
                return new

        # a rank with an empty slab launches nothing, so it needs no source
        src = reduction.source(self, plan, compact=True) if nloc else None
        want = ('mean', 'std') if scale else ('mean',)
        f64 = np.dtype(np.float64)
        fcode = dtype_code(f64)
        planes = None   # the float64 mean [, std] planes in HBM
        if local:
            nplane = O * I
            if nloc:
                tensors, _, planes = reduction.outputs(be, dev, f64, len(want), nplane, False)
                reduction.launch_moments(be, src, es, code, fcode, want, tensors)
        else:
            # the sharded axis is reduced: one STAT_VAR state per rank, gathered
            # and merged in rank order; every rank takes part, its launches only
            # where its slab has elements
            nplane = plan.nout
            states, counts = reduction.sharded_states(self._ctx, be, dev, plan, _lib.STAT_VAR, src)
            tensors, _, planes = reduction.outputs(be, dev, f64, len(want), nplane, False)
            reduction.combine_moments(be, code, fcode, want, states, counts, nplane, tensors)

        if not nloc:
            return self._like(_empty(0, dev), self._shape, self._split, dtype=out_dtype)
        return self._apply_planes(plan, src, planes[:nplane * 8],
                                  planes[nplane * 8:2 * nplane * 8] if scale else None, out_dtype, ocode)

    def _apply_planes(self, plan, src, mean, std, out_dtype, ocode):
        """_standardized's and _normalized's second half: (x - mean) [/ std]
        over ``src`` (reduction.source of ``plan``, compact) with the float64
        device planes ``mean`` / ``std`` (None: centre only) of O*I values
        (bm_standardize_apply: one read and one write), permuted back where
        the source was permuted -> the result array."""
        be, dev = self._backend, self._device
        perm, O, R, I, nloc = plan.perm, plan.O, plan.R, plan.I, plan.nloc
        es, oes = self._dtype.itemsize, out_dtype.itemsize
        f64 = np.dtype(np.float64)
        scale = std is not None
        dst = _empty(nloc * oes, dev)
        if nloc:
            src, pitch = src.buf, src.pitch
            if hasattr(be, "standardize_apply"):
                be.standardize_apply(src, plan.code, O, R, I, pitch, mean, std, dst, ocode, R)
            else:
                # an executor without the entry points (the CPU test executor):
                # torch float64 arithmetic on views of the bytes, padded rows
                # through a strided view
                import torch
                from bolt_amd.mi355x import functional as F
                if pitch != R:
                    x = F.view(src[:O * pitch * es], (O, pitch), self._dtype)[:, :R].unsqueeze(2)
                else:
                    x = F.view(src, (O, R, I), self._dtype)
                y = x.to(torch.float64) - F.view(mean, (O, 1, I), f64)
                if scale:
                    y = y / F.view(std, (O, 1, I), f64)
                dst = F.as_bytes(y.to(F.torch_dtype(out_dtype)).contiguous())
            if perm is not None:
                back = _empty(nloc * oes, dev)
                be.permute(dst, [plan.lshape[p] for p in perm], [int(i) for i in np.argsort(perm)], oes, back)
                dst = back
        return self._like(dst, self._shape, self._split, dtype=out_dtype)

    def center(self, axis=None):
        """Every record minus its mean over ``axis`` (None: every axis), as a
        new array of the same shape, split and sharding, resident on the
        device; its dtype is that of ``record - 0.0`` (float16 / float32 keep
        theirs, every other dtype gives float64).  ``axis`` is taken as mean()
        takes it.  The mean is formed, and subtracted, in float64, and the
        result rounded once.  An addition to the reference's API (the
        reference subtracts the array mean() returns, on the host)."""
        return self._standardized(axis, False)

    def zscore(self, axis=None):
        """center(axis) divided by the population standard deviation (ddof = 0,
        the StatCounter's stdev, statcounter.py:109-130) over ``axis``; the
        division is float64's, before the one rounding.  A record of zero
        variance gives nan (0/0, as numpy), a record holding a nan gives nan
        throughout.  An addition to the reference's API."""
        return self._standardized(axis, True)

    def _detrended(self, axis, order):
        """detrend(): every record over ``axis`` minus its least-squares
        polynomial of degree ``order``, as a new device array of this array's
        shape and split in the dtype of ``record - 0.0``.  The fit is a
        projection onto the discrete orthonormal polynomials p_1..p_order over
        the record's positions (reduction.detrend_basis), of d = x - mean:
        y = d - sum_k C_k p_k with C_k = sum d p_k, all float64.

        Planned with reduction.plan_for like _standardized, and what it costs:
          * the last axis (rows dense or row-padded, read in place), every
            record on this rank: one bm_detrend_rows launch, one read and one
            write; a padded input whose item size is kept gives a result
            padded alike;
          * rows that launch does not take, and reduced axes that form one
            block: the float64 mean and C_k planes from bm_comoment_state with
            the basis rows as the signals -- one read per batch of
            _lib.COMOMENT_MAX_SIGNALS, so one for order <= 4 and two for 5..8
            -- then bm_detrend_apply: one more read and one write;
          * reduced axes that are not one block: permuted to the front first
            and the result permuted back -- two more reads and writes;
          * a row-padded input over other axes than the last: copied to a dense
            temporary first (the array itself stays padded) -- one more read
            and write;
          * the sharded axis reduced: every rank's state over its slice of the
            basis, gathered; the co-moments merged in rank order
            (bm_comoment_combine as covariances, then one float64 multiply of
            the planes by n) and the mean from the same states' (mean, M2)
            planes (combine_moments), no second read; then applied to this
            rank's slab with its slice of the basis.  A rank with an empty slab
            launches nothing but takes part in every collective.
        Moment states (KEEP_MOMENTS, swap states) are neither used nor left."""
        ax = tupleize(list(range(len(self.shape))) if axis is None else axis)
        inshape(self.shape, ax)
        if isinstance(order, (bool, np.bool_)) or not isinstance(order, (int, np.integer)):
            raise ValueError("detrend: order must be an integer, got %r" % (order,))
        order = int(order)
        if not 0 <= order <= _lib.DETREND_MAX_ORDER:
            raise ValueError("detrend: order must be in 0..%d, got %d" % (_lib.DETREND_MAX_ORDER, order))
        n = self._nrecords(ax)
        if self.size and order >= n:
            raise ValueError("detrend: order %d needs records of more than %d values over axis %s (order < n)"
                             % (order, n, tuple(ax)))
        if order == 0:
            return self.center(axis)
        plan, out_dtype, ocode = reduction.plan_for(self, ax, reduction.STANDARDIZE)
        code = plan.code
        dev = self._device
        if self.size == 0:
            return self._like(_empty(0, dev), self._shape, self._split, dtype=out_dtype)
        be = backend_for(dev)
        perm, O, R, I, nloc = plan.perm, plan.O, plan.R, plan.I, plan.nloc
        es, oes = self._dtype.itemsize, out_dtype.itemsize
        d = self.__dict__
        pbuf, P = d.get("_pbuf"), d.get("_pitch")
        # every reduced record lies whole on this rank
        local = plan.world == 1 or 0 not in plan.axes
        # the reduced axis is the last one: rows, a pitch apart
        rows_last = perm is None and I == 1 and local and (pbuf is None or R == plan.lshape[-1])

        if rows_last and nloc and hasattr(be, "detrend_rows"):
            keep_pad = pbuf is not None and oes == es
            dp = P if keep_pad else R
            dst = _empty(O * dp * oes, dev)
            src, sp = (pbuf, P) if pbuf is not None else (self._data, R)
            if be.detrend_rows(src, code, O, R, sp, order, dst, ocode, dp):
                if not keep_pad:
                    return self._like(dst, self._shape, self._split, dtype=out_dtype)
                new = self._derive_padded(dst, P, self._shape, self._split)
                new.__dict__["_dtype"] = out_dtype
                return new

        from bolt_amd.mi355x import functional as F
        f64 = np.dtype(np.float64)
        batch = _lib.COMOMENT_MAX_SIGNALS
        basis = reduction.detrend_basis(n, order)
        # a rank with an empty slab launches nothing, so it needs no source
        src = reduction.source(self, plan, compact=True) if nloc else None
        means, coefs = [], []   # per batch: the float64 mean plane, its C_k planes (uint8 tensors)
        if local:
            if not nloc:
                return self._like(_empty(0, dev), self._shape, self._split, dtype=out_dtype)
            nplane = O * I
            mine = basis
            for k0 in range(0, order, batch):
                ys = basis[k0:k0 + batch]
                ymean, yresid, _ = reduction.signal_centre(ys)
                state = _empty((2 + len(ys)) * nplane * 8, dev)
                reduction.comoment_state(be, src, self._dtype, code, ys, ymean, yresid, state)
                means.append(state[:nplane * 8])
                coefs.append(state[2 * nplane * 8:])
        else:
            # the sharded axis is reduced: one state per rank and batch over its
            # slice of the basis (zeroes where its slab is empty), gathered;
            # every rank takes part, its launches only where its slab has elements
            ctx = self._ctx
            if plan.world > min(_lib.COMOMENT_MAX_PARTS, _lib.MAX_COMBINE_PARTS):
                raise NotImplementedError("detrend over the sharded axis merges at most %d ranks (got %d)"
                                          % (min(_lib.COMOMENT_MAX_PARTS, _lib.MAX_COMBINE_PARTS), plan.world))
            nplane = plan.nout
            fcode = dtype_code(f64)
            bounds = ctx.bounds(plan.shape[0])
            per = n // plan.shape[0]
            counts = [(hi - lo) * per for lo, hi in bounds]
            # the record's positions run over the reduced axes in C order, the sharded axis first
            table = basis.reshape(order, plan.shape[0], per)
            lo, hi = bounds[ctx.rank]
            mine = np.ascontiguousarray(table[:, lo:hi].reshape(order, -1))
            for k0 in range(0, order, batch):
                Kb = min(batch, order - k0)
                parts = [reduction.signal_centre(table[k0:k0 + Kb, a:b].reshape(Kb, -1)) for a, b in bounds]
                sbytes = (2 + Kb) * nplane * 8
                state = _empty(sbytes, dev)
                if nloc:
                    reduction.comoment_state(be, src, self._dtype, code, mine[k0:k0 + Kb], parts[ctx.rank][0],
                                             parts[ctx.rank][1], state)
                else:
                    state.zero_()
                states = all_gather_bytes(ctx, state, [sbytes] * plan.world)
                cov = _empty(Kb * nplane * 8, dev)
                reduction.comoment_combine(be, _lib.CO_COV, states, counts, [p[0] for p in parts],
                                           [reduction.signal_m2(p[2], p[1]) for p in parts], nplane, Kb, cov, f64,
                                           fcode)
                coefs.append(F.as_bytes(F.view(cov, (Kb, nplane), f64) * float(n)))
                if not means:
                    # the same states' (mean, M2) planes, part-major: a STAT_VAR state per rank
                    mm = states.view(plan.world, 2 + Kb, nplane * 8)[:, :2, :].contiguous().view(-1)
                    mean = _empty(nplane * 8, dev)
                    reduction.combine_moments(be, code, fcode, ('mean',), mm, counts, nplane, [mean])
                    means.append(mean)
            if not nloc:
                return self._like(_empty(0, dev), self._shape, self._split, dtype=out_dtype)

        import torch
        mean = means[0]
        coef = coefs[0] if len(coefs) == 1 else torch.cat(coefs)
        dst = _empty(nloc * oes, dev)
        buf, pitch = src.buf, src.pitch
        if hasattr(be, "detrend_apply"):
            tab = torch.from_numpy(np.ascontiguousarray(mine).reshape(-1))
            if dev.type == "cuda":
                # page-locked + non-blocking, as comoment_state uploads its signals
                tab = tab.pin_memory().to(dev, non_blocking=True)
            be.detrend_apply(buf, code, O, R, I, pitch, mean, coef, F.as_bytes(tab), order, dst, ocode, R)
        else:
            # an executor without the entry points (the CPU test executor):
            # torch float64 arithmetic on views of the bytes, padded rows
            # through a strided view
            if pitch != R:
                x = F.view(buf[:O * pitch * es], (O, pitch), self._dtype)[:, :R].unsqueeze(2)
            else:
                x = F.view(buf, (O, R, I), self._dtype)
            y = x.to(torch.float64) - F.view(mean, (O, 1, I), f64)
            tab = torch.from_numpy(np.ascontiguousarray(mine)).to(dev)
            c = F.view(coef, (order, O, 1, I), f64)
            fit = c[0] * tab[0].reshape(1, R, 1)
            for k in range(1, order):
                fit = fit + c[k] * tab[k].reshape(1, R, 1)
            dst = F.as_bytes((y - fit).to(F.torch_dtype(out_dtype)).contiguous())
        if perm is not None:
            back = _empty(nloc * oes, dev)
            be.permute(dst, [plan.lshape[p] for p in perm], [int(i) for i in np.argsort(perm)], oes, back)
            dst = back
        return self._like(dst, self._shape, self._split, dtype=out_dtype)

    def detrend(self, axis=None, order=1):
        """Every record over ``axis`` (None: every axis, the whole array as one
        record; taken as mean() takes it) minus its least-squares polynomial of
        degree ``order``: the removal of slow drift that comes before dF/F,
        z-scores or correlations (thunder's Series.detrend), as a new array of
        the same shape, split and sharding, resident on the device; its dtype
        is that of ``record - 0.0`` (float16 / float32 keep theirs, every other
        dtype gives float64), as zscore() returns its result.  The fit is over
        the record's positions 0..n-1; several reduced axes are flattened in C
        order of the ascending axes, as cov() takes its signal.  The convention
        is scipy.signal.detrend's: the mean goes too.  thunder instead zeroes
        the fit's constant coefficient and so keeps the fitted value at
        position 0; that variant is not offered.  ``order`` 0 returns
        center(axis).  All arithmetic is float64 and the result is rounded
        once; no Vandermonde matrix is formed: the record's deviations from its
        mean (formed as center() forms it) are projected onto the discrete
        orthonormal polynomials on its n positions, built by their three-term
        recurrence.  A constant record gives exact zeros; for ``order`` >= 1 a
        record holding a NaN or an infinity is NaN throughout, other records
        are untouched; ``order`` = n - 1 interpolates, leaving rounding noise;
        int64 / uint64 values beyond 2^53 round when converted to float64; bool
        runs as uint8.  ``order`` that is not an integer (a bool is refused),
        outside 0.._lib.DETREND_MAX_ORDER (8) or, for a non-empty array, not
        below n raises ValueError before any device work.  Over the last axis
        the array is read once and written once; what other layouts cost:
        _detrended.  An addition to the reference's API."""
        return self._detrended(axis, order)

    def _normalized(self, axis, method, perc, offset):
        """normalize(): every record over ``axis`` against its own baseline b,
        (x - b) / (b + offset), as a new device array of this array's shape and
        split in the dtype of ``record - 0.0``.  b is float64: the mean as
        _standardized forms it, or the 'linear' percentile as _quantile does,
        unrounded.

        Planned with reduction.plan_for like _standardized, and what it costs:
          * the last axis (rows dense or row-padded, read in place), every
            record on this rank: one bm_normalize_rows launch, one read and
            one write; a padded input whose item size is kept gives a result
            padded alike;
          * rows that launch does not take, and every other layout: the
            float64 baseline plane in HBM first, then bm_standardize_apply
            with mean = b and std = b + offset (one float64 add on the plane):
            one read and one write on top of the plane's cost.  The plane of
            'mean' is _standardized's (one read; the sharded axis reduced:
            per-rank states, gathered and merged in rank order).  The plane of
            'percentile' is _quantile's rows -- read in place where the
            reduced axes are the rows (one read for rows the registers hold,
            else sizeof(element) reads), else after one permute into a dense
            temporary with the kept axes first (one more read and write) --
            and stays on the device; only across ranks with the sharded axis
            reduced does it come through the host, as quantile()'s result
            (one exchange, one gather, one upload);
          * reduced axes that are not one block: the source permuted to the
            front for the apply and the result permuted back -- two more reads
            and writes; a row-padded input over other axes than the last:
            copied to a dense temporary first -- one more read and write.
        Moment states (KEEP_MOMENTS, swap states) are neither used nor left."""
        ax = tupleize(list(range(len(self.shape))) if axis is None else axis)
        inshape(self.shape, ax)
        if method not in ('percentile', 'mean'):
            raise ValueError("normalize: method must be 'percentile' or 'mean', got %r (thunder's sliding-window "
                             "baselines 'window' and 'window-exact' are not offered)" % (method,))

        def real(v, name, lo=None, hi=None):
            try:
                a = np.asarray(v)
            except Exception:
                a = None
            if a is None or a.dtype.kind not in "biuf" or a.ndim != 0 or not np.isfinite(a) \
                    or (lo is not None and not lo <= a <= hi):
                raise ValueError("normalize: %s must be a finite real scalar%s, got %r"
                                 % (name, "" if lo is None else " in [%g, %g]" % (lo, hi), v))
            return float(a)
        offset = real(offset, "offset")
        rank_baseline = method == 'percentile'
        if rank_baseline:
            perc = real(perc, "perc", 0, 100)
        plan, out_dtype, ocode = reduction.plan_for(self, ax, reduction.STANDARDIZE)
        if rank_baseline and plan.world > 1 and 0 in plan.axes and len(plan.axes) == self.ndim:
            raise NotImplementedError("normalize(method='percentile') over every axis of an array sharded across %d "
                                      "ranks needs a distributed select; reduce the sharded axis together with "
                                      "fewer axes, or use method='mean'" % plan.world)
        code = plan.code
        dev = self._device
        if self.size == 0:
            return self._like(_empty(0, dev), self._shape, self._split, dtype=out_dtype)
        rank, frac = 0, 0.0
        if rank_baseline:
            # pos = (perc / 100) (n - 1) in float64, as _quantile: lo the floor(pos)-th smallest, g the rest
            pos = np.float64(perc) / 100 * (self._nrecords(ax) - 1)
            rank, frac = int(np.floor(pos)), float(pos - np.floor(pos))
        be = backend_for(dev)
        perm, O, R, I, nloc = plan.perm, plan.O, plan.R, plan.I, plan.nloc
        es, oes = self._dtype.itemsize, out_dtype.itemsize
        d = self.__dict__
        pbuf, P = d.get("_pbuf"), d.get("_pitch")
        # every reduced record lies whole on this rank
        local = plan.world == 1 or 0 not in plan.axes
        # the reduced axis is the last one: rows, a pitch apart
        rows_last = perm is None and I == 1 and local and (pbuf is None or R == plan.lshape[-1])

        if rows_last and nloc and hasattr(be, "normalize_rows"):
            keep_pad = pbuf is not None and oes == es
            dp = P if keep_pad else R
            dst = _empty(O * dp * oes, dev)
            src, sp = (pbuf, P) if pbuf is not None else (self._data, R)
            if be.normalize_rows(src, code, O, R, sp, _lib.NORM_RANK if rank_baseline else _lib.NORM_MEAN, rank, frac,
                                 offset, dst, ocode, dp):
                if not keep_pad:
                    return self._like(dst, self._shape, self._split, dtype=out_dtype)
                new = self._derive_padded(dst, P, self._shape, self._split)
                new.__dict__["_dtype"] = out_dtype
                return new

        # the float64 baseline plane in HBM (a rank with an empty slab launches
        # nothing but takes part in every collective)
        f64 = np.dtype(np.float64)
        fcode = dtype_code(f64)
        base = None
        src = reduction.source(self, plan, compact=True) if nloc else None
        if not rank_baseline:
            if local:
                if nloc:
                    tensors, _, base = reduction.outputs(be, dev, f64, 1, O * I, False)
                    reduction.launch_moments(be, src, es, code, fcode, ('mean',), tensors)
            else:
                states, counts = reduction.sharded_states(self._ctx, be, dev, plan, _lib.STAT_VAR, src)
                tensors, _, base = reduction.outputs(be, dev, f64, 1, plan.nout, False)
                reduction.combine_moments(be, code, fcode, ('mean',), states, counts, plan.nout, tensors)
        elif local:
            if nloc:
                qbuf, qpitch, qO, qR = self._quantile_rows(plan)
                base = reduction.quantile_baseline(be, qbuf, self._dtype, code, qO, qR, qpitch, rank, frac)
        else:
            # the sharded axis is reduced with other axes kept: quantile()'s
            # exchange and gather; every rank ends with the whole plane
            ranks, fr, qdt = reduction.baseline_request(self._dtype, rank, frac)
            host = reduction.baseline_f64(self._quantile_planes(plan, qdt, dtype_code(qdt), ranks, fr), frac)
            if nloc:
                import torch
                from bolt_amd.mi355x import functional as F
                base = F.as_bytes(torch.from_numpy(np.ascontiguousarray(host)).to(dev))
        if not nloc:
            return self._like(_empty(0, dev), self._shape, self._split, dtype=out_dtype)
        from bolt_amd.mi355x import functional as F
        den = F.as_bytes(F.view(base, (-1,), f64) + offset)
        return self._apply_planes(plan, src, base, den, out_dtype, ocode)

    def normalize(self, axis=None, method='percentile', perc=20, offset=0.1):
        """Every record over ``axis`` (None: every axis; taken as mean() takes
        it) against its own baseline b: ``(x - b) / (b + offset)``, the dF/F of
        a calcium-imaging pipeline (thunder's Series.normalize), as a new array
        of the same shape, split and sharding, resident on the device; its
        dtype is that of ``record - 0.0`` (float16 / float32 keep theirs, every
        other dtype gives float64), as zscore() returns its result.  The
        baseline is float64 and is not rounded to that dtype: ``method``
        'percentile' takes the ``perc``-th percentile with 'linear'
        interpolation -- quantile()'s lo + (hi - lo) g with
        pos = (perc / 100)(n - 1), g == 0 giving lo -- and 'mean' the mean as
        center() forms it.  x - b, b + offset and the division (a true one)
        are three separately rounded float64 operations, nothing is fused, and
        the result is rounded once.  A record holding a NaN is NaN throughout;
        b + offset == 0 gives what IEEE gives (inf, or nan for 0/0), as numpy;
        int64 / uint64 values beyond 2^53 round when converted to float64; bool
        runs as uint8.  ``method`` other than the two, ``perc`` not a finite
        real scalar in [0, 100] and ``offset`` not a finite real scalar raise
        ValueError before any device work; 'percentile' over every axis of an
        array sharded over more than one rank raises NotImplementedError, as
        quantile() does.  thunder's sliding-window baselines ('window',
        'window-exact') are out of scope.  Over the last axis the array is
        read once and written once; what other layouts cost: _normalized.  An
        addition to the reference's API."""
        return self._normalized(axis, method, perc, offset)

    def _comoment(self, y, axis, keepdims, what):
        """cov / corr (``what``: _lib.CO_COV / CO_CORR) of every record over
        ``axis`` with the signal(s) ``y`` -> host result.

        Planned with reduction.plan_for / source like _reduced, and what it
        costs: one read of the array per batch of _lib.COMOMENT_MAX_SIGNALS
        signals (bm_comoment_state), then bm_comoment_combine of one part into
        the host result.  Rows over the last axis are read in place, padded or
        not; columns over padded rows too (the pad columns' outputs dropped);
        reduced axes that are not one block are permuted to the front first
        (``y`` is flattened in C order of the sorted reduced axes, so it
        indexes the permuted rows unchanged); every axis of a padded array
        compacts, as sum() does.  Across ranks: the sharded axis kept, every
        rank finishes its slab's outputs and they are gathered; reduced, every
        rank's state over its slice of ``y`` is gathered and merged in rank
        order (at most _lib.COMOMENT_MAX_PARTS ranks).  Moment states
        (KEEP_MOMENTS) are neither used nor left; nothing is cached."""
        ax = tupleize(list(range(len(self.shape))) if axis is None else axis)
        inshape(self.shape, ax)
        axes = tuple(sorted(set(int(a) for a in ax)))
        rshape = tuple(int(self._shape[a]) for a in axes)
        try:
            ys = np.asarray(y)
        except Exception:
            raise ValueError("cov / corr: the signal is not array-like")
        if ys.dtype.kind not in "biuf":
            raise ValueError("cov / corr: the signal must be real (bool, int or float), got dtype %s" % ys.dtype)
        one = ys.shape == rshape
        if not one and not (ys.ndim == len(rshape) + 1 and ys.shape[1:] == rshape and ys.shape[0] >= 1):
            raise ValueError("cov / corr: a signal of shape %s or (K,) + %s with K >= 1 is needed for axis %s, got %s"
                             % (rshape, rshape, axes, ys.shape))
        ys = np.ascontiguousarray(ys, dtype=np.float64).reshape((1 if one else ys.shape[0],) + rshape)
        if not np.isfinite(ys).all():
            raise ValueError("cov / corr: the signal holds a non-finite value")
        K = ys.shape[0]
        plan, out_dtype, ocode = reduction.plan_for(self, ax, reduction.COMOMENT)
        if self._ctx.world_size > _lib.COMOMENT_MAX_PARTS and 0 in axes:
            raise NotImplementedError("cov / corr over the sharded axis merge at most %d ranks (got %d)"
                                      % (_lib.COMOMENT_MAX_PARTS, self._ctx.world_size))
        if self._nrecords(ax) == 0:
            planes = [np.full(plan.out_shape, np.nan, dtype=out_dtype) for _ in range(K)]
        else:
            planes = []
            for k0 in range(0, K, _lib.COMOMENT_MAX_SIGNALS):
                planes += self._comoment_batch(plan, out_dtype, ocode, ys[k0:k0 + _lib.COMOMENT_MAX_SIGNALS], what)
        vs = self._aligned_vshape(ax)
        res = []
        for arr in planes:
            if vs is not None:
                arr = arr.reshape(vs)
            if keepdims:
                for i in ax:
                    arr = np.expand_dims(arr, axis=i)
            res.append(arr)
        arr = res[0] if one else np.stack(res)
        if arr.ndim == 0:
            arr = arr[()]
        return BoltArrayLocal(arr).toscalar()

    def _comoment_batch(self, plan, out_dtype, ocode, ys, what):
        """_comoment for the Kb <= _lib.COMOMENT_MAX_SIGNALS signals ``ys``
        ((Kb,) + the reduced extents) -> list of Kb host arrays of plan.out_shape."""
        Kb, code = ys.shape[0], plan.code
        src = reduction.source(self, plan, moments=False)
        nlaunch, drop = src.nlaunch, src.drop
        dev = src.buf.device
        be = backend_for(dev)
        single = plan.world == 1
        if single or 0 not in plan.axes:
            # every output lives on this rank (or this rank's slab of them);
            # every reduced record lies whole on it, so the signals are whole too
            run = nlaunch and plan.nloc
            if run:
                # the read is launched first; what only the finish needs is
                # worked out, and its buffers made, while the read runs
                yk = ys.reshape(Kb, -1)
                ymean, yresid, yc = reduction.signal_centre(yk)
                state = _empty((2 + Kb) * nlaunch * 8, dev)
                with np.errstate(all="ignore"):  # a numpy executor on pad columns' unwritten values (dropped later)
                    reduction.comoment_state(be, src, self._dtype, code, yk, ymean, yresid, state)
            # (the Kb planes are stored by one launch, so they share one buffer:
            # page-locked only when all of them fit the zero-copy limit)
            outs = reduction.outputs(be, dev, out_dtype, Kb, nlaunch, single and run and
                                     Kb * nlaunch * out_dtype.itemsize <= reduction.HOST_RESULT_MAX)
            if run:
                with np.errstate(all="ignore"):
                    reduction.comoment_combine(be, what, state, [src.R], [ymean], [reduction.signal_m2(yc, yresid)],
                                               nlaunch, Kb, outs[2] if outs[2] is not None else outs[1], out_dtype,
                                               ocode)
            return reduction.finish(outs, dev, plan, out_dtype, Kb, nlaunch, drop, None if single else self._ctx)
        # the sharded axis is reduced: one state per rank over its slice of the
        # signals (zeroes where its slab is empty), gathered and merged in rank order
        if plan.nout == 0:  # e.g. axis 0 of (4, 0, 3): nothing to merge
            return [np.empty(plan.out_shape, out_dtype) for _ in range(Kb)]
        ctx = self._ctx
        bounds = ctx.bounds(plan.shape[0])
        per = int(np.prod([plan.shape[i] for i in plan.axes if i != 0], dtype=np.int64))
        counts = [(hi - lo) * per for lo, hi in bounds]
        parts = [reduction.signal_centre(ys[:, lo:hi].reshape(Kb, -1)) for lo, hi in bounds]
        sbytes = (2 + Kb) * plan.nout * 8
        state = _empty(sbytes, dev)
        if plan.nloc:
            lo, hi = bounds[ctx.rank]
            mine = parts[ctx.rank]
            reduction.comoment_state(be, src, self._dtype, code, ys[:, lo:hi].reshape(Kb, -1), mine[0], mine[1],
                                     state)
        else:
            state.zero_()
        states = all_gather_bytes(ctx, state, [sbytes] * plan.world)
        outs = reduction.outputs(be, dev, out_dtype, Kb, plan.nout, False)
        reduction.comoment_combine(be, what, states, counts, [p[0] for p in parts],
                                   [reduction.signal_m2(p[2], p[1]) for p in parts],
                                   plan.nout, Kb, outs[2], out_dtype, ocode)
        return reduction.finish(outs, dev, plan, out_dtype, Kb, plan.nout)

    def cov(self, y, axis=None, keepdims=False):
        """Population covariance (ddof = 0, as var / std) of every record over
        ``axis`` (None: every axis; taken as mean() takes it) with the signal
        ``y``: mean((x - mean(x)) (y - mean(y))).  ``y`` is array-like and real,
        of the reduced axes' extents in ascending axis order -- or (K,) + those
        for K >= 1 signals, which share reads of the array, four signals a read
        (more signals read it again per four); anything else raises ValueError
        before any device work.  The result is a host result as stats() returns
        its fields, of the kept axes' shape ((K,) + that for K signals;
        ``keepdims`` re-inserts the reduced axes after the K axis) and the
        statistics dtype (float16 / float32 keep theirs, every other dtype
        gives float64).  The arithmetic is float64, rounded once; a constant
        record or signal gives 0; a record holding a NaN or an infinity gives
        NaN, as numpy's x - mean(x) makes it (inf - inf), wherever in the
        record the value sits, and other records are untouched (the co-moment
        state's mean plane of such a record is what a sum over it gives: +inf,
        -inf, or NaN for inf - inf or a NaN); no records give nan.  Plane k of a K-signal call has the bytes of the
        one-signal call with y[k].  An addition to the reference's API."""
        return self._comoment(y, axis, keepdims, _lib.CO_COV)

    def corr(self, y, axis=None, keepdims=False):
        """Pearson correlation cov(y) / (std_x std_y) of every record over
        ``axis`` with the signal(s) ``y``, taken and returned as cov() takes and
        returns them; clamped to [-1, 1] before the one rounding, as
        numpy.corrcoef does.  A record or a signal of zero variance gives nan,
        and so does a record holding a NaN or an infinity, as for cov().
        An addition to the reference's API."""
        return self._comoment(y, axis, keepdims, _lib.CO_CORR)

    def _quantile(self, q, axis, keepdims, method, scale, who):
        """``who`` (quantile / percentile / median) of every record over
        ``axis`` at ``q`` / ``scale`` -> host result.

        Planned with reduction.plan_for / plan.reduce_layout like _comoment,
        and what it costs, per batch of quantiles (_lib.QUANTILE_MAX_RANKS
        ranks: eight 'lower' / 'higher' quantiles, four 'linear' ones, each of
        which needs two ranks):
          * the last axis (rows dense or row-padded, read in place at their
            pitch): one read of the array (bm_quantile_rows) for rows the
            registers hold, else sizeof(element) reads (bm_quantile_select);
          * every other layout -- columns, reduced axes that are not one
            block, a padded array over other axes than the last -- is first
            permuted into a dense temporary with the kept axes first, in
            ascending order, and the reduced axes last (one bm_permute, or
            one strided copy out of padded rows: one more read and write,
            once for all batches), then runs as rows;
          * across ranks, the sharded axis kept: every rank finishes its
            slab's outputs and they are gathered (reduction.finish);
          * across ranks, the sharded axis reduced with other axes kept: one
            exchange (permute_sharded) brings the kept axes to the front, so
            every rank holds whole records, then as the case before;
          * across ranks, every axis reduced: NotImplementedError.
        Moment states (KEEP_MOMENTS, swap states) are neither used nor left;
        nothing is cached."""
        ax = tupleize(list(range(len(self.shape))) if axis is None else axis)
        inshape(self.shape, ax)
        if method not in ('linear', 'lower', 'higher'):
            raise ValueError("%s: method must be 'linear', 'lower' or 'higher', got %r" % (who, method))
        try:
            qs = np.asarray(q)
        except Exception:
            raise ValueError("%s: q is not array-like" % who)
        if qs.dtype.kind not in "biuf" or qs.ndim > 1 or (qs.ndim == 1 and qs.size == 0):
            raise ValueError("%s: q must be a real scalar or a 1-D sequence of at least one, got dtype %s, shape %s"
                             % (who, qs.dtype, qs.shape))
        one = qs.ndim == 0
        qs = qs.astype(np.float64).reshape(-1)
        if not (np.isfinite(qs).all() and (qs >= 0).all() and (qs <= scale).all()):
            raise ValueError("%s: q must be finite and in [0, %g], got %s" % (who, scale, qs))
        if scale != 1:
            qs = qs / scale
        axes = tuple(sorted(set(int(a) for a in ax)))
        n = self._nrecords(ax)
        if n == 0 and method != 'linear':
            raise ValueError("%s: method %r of no records" % (who, method))
        world = self._ctx.world_size
        if world > 1 and 0 in axes and len(axes) == self.ndim:
            raise NotImplementedError("%s over every axis of an array sharded across %d ranks needs a distributed "
                                      "select; reduce the sharded axis together with fewer axes" % (who, world))
        plan, out_dtype, ocode = reduction.plan_for(self, ax, reduction.QUANTILE)
        if method != 'linear':
            out_dtype, ocode = self._dtype, plan.code   # one of the record's own values
        K = len(qs)
        if n == 0:
            planes = [np.full(plan.out_shape, np.nan, dtype=out_dtype) for _ in range(K)]
        else:
            # pos = q (n - 1) in float64: lo / hi the floor(pos)-th / ceil(pos)-th smallest, g the rest
            pos = qs * (n - 1)
            fl = np.floor(pos)
            if method == 'higher':
                ranks, frac = np.ceil(pos).astype(np.int64).tolist(), [0.0] * K
            elif method == 'lower':
                ranks, frac = fl.astype(np.int64).tolist(), [0.0] * K
            else:
                ranks, frac = fl.astype(np.int64).tolist(), (pos - fl).tolist()
            planes = self._quantile_planes(plan, out_dtype, ocode, ranks, frac)
        vs = self._aligned_vshape(ax)
        res = []
        for arr in planes:
            if vs is not None:
                arr = arr.reshape(vs)
            if keepdims:
                for i in ax:
                    arr = np.expand_dims(arr, axis=i)
            res.append(arr)
        arr = res[0] if one else np.stack(res)
        if arr.ndim == 0:
            arr = arr[()]
        return BoltArrayLocal(arr).toscalar()

    def _quantile_planes(self, plan, out_dtype, ocode, ranks, frac):
        """_quantile's device work -> list of len(ranks) host arrays of
        plan.out_shape.  The rows are laid out once; the quantiles run in
        batches of at most _lib.QUANTILE_MAX_RANKS ranks."""
        ctx, es = self._ctx, self._dtype.itemsize
        d = self.__dict__
        if plan.world > 1 and 0 in plan.axes:
            # the sharded axis is reduced: the kept axes to the front across
            # ranks (one exchange, as _tree_reduce's), whole records per rank
            kept = [i for i in range(self.ndim) if i not in plan.axes]
            gperm = kept + list(plan.axes)
            pbuf = d.get("_pbuf")
            data = permute_sharded(ctx, self._backend, pbuf if pbuf is not None else d["_data"], self._shape, gperm,
                                   es, src_pitch=d.get("_pitch") if pbuf is not None else None)
            tmp = self._like(data, tuple(self._shape[p] for p in gperm), len(kept))
            tplan, _, _ = reduction.plan_for(tmp, tuple(range(len(kept), self.ndim)), reduction.QUANTILE)
            return tmp._quantile_planes(tplan, out_dtype, ocode, ranks, frac)
        buf, pitch, O, R = self._quantile_rows(plan)
        nloc = plan.nloc
        dev = self._device
        be = backend_for(dev)
        single = plan.world == 1
        run = O and nloc
        planes = []
        k0 = 0
        while k0 < len(ranks):
            k1, S = k0, 0
            while k1 < len(ranks) and S + (2 if frac[k1] != 0.0 else 1) <= _lib.QUANTILE_MAX_RANKS:
                S += 2 if frac[k1] != 0.0 else 1
                k1 += 1
            Kb = k1 - k0
            outs = reduction.outputs(be, dev, out_dtype, Kb, O, single and run and
                                     Kb * O * out_dtype.itemsize <= reduction.HOST_RESULT_MAX)
            if run:
                reduction.quantile_rows(be, buf, self._dtype, plan.code, O, R, pitch, ranks[k0:k1], frac[k0:k1],
                                        outs[2] if outs[2] is not None else outs[1], out_dtype, ocode)
            planes += reduction.finish(outs, dev, plan, out_dtype, Kb, O, None, None if single else ctx)
            k0 = k1
        return planes

    def _quantile_rows(self, plan):
        """This rank's records over ``plan``'s reduced axes as rows (every
        record whole on this rank) -> (buffer, row pitch in elements, O rows,
        R elements a row): the array itself where the reduced axes are its
        rows, dense or a pitch apart, else a dense temporary with the kept axes
        first, in ascending order, and the reduced axes last (one bm_permute,
        or one strided copy out of padded rows)."""
        es = self._dtype.itemsize
        d = self.__dict__
        lshape, nloc = plan.lshape, plan.nloc
        R = int(np.prod([lshape[a] for a in plan.axes], dtype=np.int64))
        O = nloc // R if R else 0
        pbuf = d.get("_pbuf")
        dev = self._device
        be = backend_for(dev)
        if plan.perm is None and plan.I == 1 and plan.R == R and (pbuf is None or R == lshape[-1]):
            # the reduced axes are the rows: read in place, dense or a pitch apart
            buf, pitch = (pbuf, d["_pitch"]) if pbuf is not None else (d["_data"], R)
        else:
            kept = [i for i in range(len(lshape)) if i not in plan.axes]
            perm = kept + list(plan.axes)
            buf, pitch = _empty(nloc * es, dev), R
            if nloc and pbuf is not None:
                pstr = padded_strides(lshape, d["_pitch"])
                pshape = [lshape[p] for p in perm]
                be.copy_strided(pbuf, 0, buf, 0, pshape, [pstr[p] for p in perm], padded_strides(pshape, pshape[-1]),
                                es)
            elif nloc:
                be.permute(d["_data"], lshape, perm, es, buf)
        return buf, pitch, O, R

    def quantile(self, q, axis=None, keepdims=False, method='linear'):
        """The ``q``-quantile(s) of every record over ``axis`` (None: every
        axis; taken as mean() takes it): exact order statistics.  ``q`` is a
        real scalar or a 1-D sequence of K >= 1 values, each finite and in
        [0, 1]; ``method`` is 'linear', 'lower' or 'higher'; anything else
        raises ValueError before any device work.  With n values reduced per
        output, pos = q (n - 1) in float64, lo / hi the floor(pos)-th /
        ceil(pos)-th smallest values and g = pos - floor(pos):
        'lower' / 'higher' return lo / hi in the array's dtype, bit for bit
        numpy.quantile's; 'linear' returns lo where g == 0, else
        lo + (hi - lo) g evaluated in float64 (three separately rounded
        operations) and rounded once to the statistics dtype (float16 /
        float32 keep theirs, every other dtype gives float64: numpy's result
        dtypes).  int64 / uint64 values beyond 2^53 round when 'linear'
        converts them to float64.  Floats order as IEEE values, -0.0 before
        +0.0; a record holding a NaN gives NaN for every q and method; bool
        runs as uint8.  No records: 'linear' gives nan, 'lower' / 'higher'
        raise ValueError.  The result is a host result as cov() returns its
        planes, of the kept axes' shape ((K,) + that for a sequence;
        ``keepdims`` re-inserts the reduced axes after the K axis).  Over the
        last axis the array is read once per four 'linear' (eight 'lower' /
        'higher') quantiles; what other layouts cost: _quantile.  An addition
        to the reference's API."""
        return self._quantile(q, axis, keepdims, method, 1, "quantile")

    def percentile(self, q, axis=None, keepdims=False, method='linear'):
        """quantile(q / 100): ``q`` in [0, 100].  An addition to the reference's API."""
        return self._quantile(q, axis, keepdims, method, 100, "percentile")

    def median(self, axis=None, keepdims=False):
        """quantile(0.5): the median of every record over ``axis``.  An
        addition to the reference's API."""
        return self._quantile(0.5, axis, keepdims, 'linear', 1, "median")

    def _stat(self, axis=None, func=None, name=None, keepdims=False):
        """Statistic over ``axis`` (array.py:284-334); results are host arrays / scalars."""
        if name and not func:
            try:  # axes already validated for this shape and split, keyed by the argument as given
                ak = (self._shape, self._split, axis)
                hit = _STAT_AXES.get(ak)
            except TypeError:  # unhashable axis (a list)
                ak = hit = None
            if hit is None:
                ax = tupleize(list(range(len(self.shape))) if axis is None else axis)
                inshape(self.shape, ax)
                hit = (ax, self._nrecords(ax), self._aligned_vshape(ax))
                if ak is not None:
                    if len(_STAT_AXES) > 4096:
                        _STAT_AXES.clear()
                    _STAT_AXES[ak] = hit
            axis, nrec, vs = hit
            if nrec == 0:
                # no records after _align: the merged StatCounter is the empty one
                # (statcounter.py:28-41, :109-130): mean 0.0, variance / stdev nan
                arr = 0.0 if name == 'mean' else float('nan')
            else:
                arr, _ = self._reduced(axis, _STAT_CODES[name])
                if vs is not None:
                    arr = arr.reshape(vs)
                if arr.ndim == 0:
                    arr = arr[()]
            if keepdims:
                for i in axis:
                    arr = np.expand_dims(arr, axis=i)
            return BoltArrayLocal(arr).toscalar()

        if axis is None:
            axis = list(range(len(self.shape)))
        axis = tupleize(axis)
        if func and not name:
            return self.reduce(func, axis, keepdims)

        raise ValueError('Must specify either a function or a statistic name.')

    def reduce(self, func, axis=(0,), keepdims=False):
        """Reduce with ``func`` over ``axis`` (array.py:243-282).

        The reference treeReduces ``func`` over the aligned records.  numpy
        ufuncs (add, multiply, maximum, minimum, fmax, fmin, logical_and /
        or, bitwise_and / or / xor and their ``operator`` spellings) run as
        one bm_reduce mode on the GPU, with numpy's result dtype for
        ``func(record, record)``; any other binary function receives device
        tensors and is applied as a pairwise tree in record order,
        ((r0 f r1) f (r2 f r3)) ..., vmapped over the pairs of each level.
        A single record is returned as is, as treeReduce returns it.
        """
        axis = tupleize(axis)
        inshape(self.shape, axis)
        nrec = self._nrecords(axis)
        if nrec == 0:
            raise ValueError("Can not reduce() empty RDD")  # treeReduce of no records (array.py:269)
        stat = _UFUNC_STATS.get(func) if _hashable(func) else None
        vs = self._aligned_vshape(axis)
        if nrec == 1:
            # treeReduce of one record returns it untouched (no func call)
            kept = [d for i, d in enumerate(self._shape) if i not in set(int(a) for a in axis)]
            arr = self.toarray().reshape(kept if vs is None else vs)
        elif stat is not None and self._reduce_dtype_ok(func, stat):
            arr, _ = self._reduced(axis, stat)
        else:
            from bolt_amd.mi355x.functional import user_fn
            arr = self._tree_reduce(user_fn(func), axis, vs)
        if vs is not None:
            arr = arr.reshape(vs)
        if arr.ndim == 0:
            arr = arr[()]
        if keepdims:
            for i in axis:
                arr = np.expand_dims(arr, axis=i)
        if not isinstance(arr, np.ndarray):
            return arr
        elif arr.shape == (1,):
            return arr[0]
        return BoltArrayLocal(arr)

    def _reduce_dtype_ok(self, func, stat):
        """numpy's own rule for func(record, record) (raises numpy's TypeError for
        bitwise ufuncs on floats); True if the kernel mode produces that dtype."""
        probe = np.asarray(func(np.zeros(1, self._dtype), np.zeros(1, self._dtype)))
        want = np.dtype(bool) if stat in (_lib.STAT_LAND, _lib.STAT_LOR) else self._dtype
        return probe.dtype == want

    def _tree_reduce(self, func, axis, vshape=None):
        """Pairwise tree of a user function over the aligned records, on the
        device; ``vshape``: the records' shape when the reference's _align
        squeezes a unit axis (see _aligned_vshape)."""
        import torch
        from bolt_amd.mi355x.functional import view, apply_pairs, numpy_dtype
        ctx = self._ctx
        axset = sorted(set(int(a) for a in axis))
        kept = [i for i in range(self.ndim) if i not in axset]
        gshape = self._shape
        lshape = self._local_shape
        src = self._data
        if ctx.world_size > 1 and 0 not in axset:
            # a rank's slab of the sharded axis is a slab of every record: a
            # function that is not elementwise must see whole records, as the
            # reference's treeReduce after _align does (array.py:268-269).  Bring
            # the reduced axes to the front across GPUs (one exchange), so each
            # rank holds whole records, and reduce the sharded axis below.
            gperm = axset + kept
            src = permute_sharded(ctx, self._backend, src, gshape, gperm, self._dtype.itemsize)
            gshape = tuple(gshape[p] for p in gperm)
            lo, hi = ctx.local_bounds(gshape[0])
            lshape = (hi - lo,) + gshape[1:]
            axset = list(range(len(axset)))
            kept = list(range(len(axset), len(gshape)))
        perm, O, R, I = reduce_layout(lshape, axset)
        if perm is not None:
            tmp = _empty(src.numel(), src.device)
            if src.numel():
                self._backend.permute(src, lshape, perm, self._dtype.itemsize, tmp)
            src = tmp
        rec_shape = tuple(lshape[i] for i in kept) if vshape is None else tuple(vshape)
        recs = view(src, (O, R, I), self._dtype).permute(1, 0, 2).reshape((R,) + rec_shape)
        if R:
            part = _tree(func, recs)
        else:
            # a rank with no records still needs the result's dtype and shape
            z = torch.zeros((1,) + rec_shape, dtype=recs.dtype, device=recs.device)
            part = apply_pairs(func, z, z)[0]
        out_dtype = numpy_dtype(part.dtype)
        if ctx.world_size == 1:
            return part.cpu().numpy().astype(out_dtype, copy=False)
        from bolt_amd.mi355x.functional import as_bytes
        # the sharded axis is reduced: rank partials, then the same tree over
        # the ranks that hold records, in rank order
        pbytes = as_bytes(part)
        allp = all_gather_bytes(ctx, pbytes, [pbytes.numel()] * ctx.world_size)
        per = view(allp, (ctx.world_size,) + tuple(part.shape), out_dtype)
        has = [r for r, (lo, hi) in enumerate(ctx.bounds(gshape[0])) if hi > lo]
        res = _tree(func, per[has])
        return res.cpu().numpy().astype(numpy_dtype(res.dtype), copy=False)

    def _aligned_vshape(self, axis):
        """The record shape after the reference's _align(axis) (array.py:85-115)
        when its swap squeezes a unit axis (plan.swap_shape), else None: the
        kept axes' extents in ascending order."""
        try:
            return _aligned_vshape_of(self._shape, self._split, tuple(int(a) for a in axis))
        except TypeError:
            return _aligned_vshape_of.__wrapped__(self._shape, self._split, tuple(axis))

    def _nrecords(self, axis):
        """Records the reduction sees after _align: the product of the reduced extents."""
        n = 1
        for a in axis:
            n *= int(self._shape[int(a)])
        return n

    def mean(self, axis=None, keepdims=False):
        """Mean over ``axis`` (array.py:336-349)."""
        return self._stat(axis, name='mean', keepdims=keepdims)

    def var(self, axis=None, keepdims=False):
        """Population variance over ``axis`` (array.py:351-364)."""
        return self._stat(axis, name='variance', keepdims=keepdims)

    def std(self, axis=None, keepdims=False):
        """Population standard deviation over ``axis`` (array.py:366-379)."""
        return self._stat(axis, name='stdev', keepdims=keepdims)

    def sum(self, axis=None, keepdims=False):
        """Sum over ``axis`` in the input dtype (array.py:381-395; integer sums wrap)."""
        import operator
        return self._stat(axis, func=operator.add, keepdims=keepdims)

    def max(self, axis=None, keepdims=False):
        """Maximum over ``axis`` (array.py:397-411): numpy.maximum, NaNs propagate."""
        return self._stat(axis, func=np.maximum, keepdims=keepdims)

    def min(self, axis=None, keepdims=False):
        """Minimum over ``axis`` (array.py:413-427): numpy.minimum, NaNs propagate."""
        return self._stat(axis, func=np.minimum, keepdims=keepdims)

    # -------------------------------------------------------------- egress
    def toarray(self):
        """The whole array on the host (array.py:1006-1014).  Across GPUs the
        slabs are gathered window by window (dist.gather_to_host): device
        memory per rank stays at its slab plus one window."""
        ctx = self._ctx
        d = self.__dict__
        if "_pbuf" in d and ctx.world_size == 1:
            return self._padded_to_host()
        if ctx.world_size == 1:
            return to_host(self._data, self._dtype, self._shape)
        rowbytes = int(np.prod(self._shape[1:], dtype=np.int64)) * self._dtype.itemsize
        rows = self._shape[0] if self._shape else 1  # a 0-d array lives on rank 0
        sizes = [(hi - lo) * rowbytes for lo, hi in ctx.bounds(rows)]
        if "_pbuf" in d:
            # padded rows: each egress window compacted on the way
            es = self._dtype.itemsize
            spec = (self._shape[-1] * es, d["_pitch"] * es, self._backend)
            return gather_to_host(ctx, d["_pbuf"], sizes, rows=spec).view(self._dtype).reshape(self._shape)
        return gather_to_host(ctx, self._data, sizes).view(self._dtype).reshape(self._shape)

    def _padded_to_host(self):
        """toarray of a row-padded array (one GPU): the rows are compacted
        window by window into two device windows of at most transfer.CHUNK
        bytes, each DMA'd to page-locked memory while the next is compacted
        -- no dense copy of the whole array on the device (array.py:1006-1014)."""
        from bolt_amd.mi355x import transfer
        d = self.__dict__
        pbuf, P = d["_pbuf"], d["_pitch"]
        es = self._dtype.itemsize
        R = self._shape[-1]
        rows = int(np.prod(self._local_shape[:-1], dtype=np.int64))
        rb = R * es
        out = np.empty(rows * rb, dtype=np.uint8)
        if rows == 0 or rb == 0:
            return out.view(self._dtype).reshape(self._shape)
        wrows = max(1, min(rows, transfer.CHUNK // rb)) if pbuf.device.type == "cuda" else rows
        be = backend_for(pbuf.device)
        wins = [_empty(wrows * rb, pbuf.device) for _ in range(2 if rows > wrows else 1)]

        def produce(lo, hi, k):
            r0, r1 = lo // rb, hi // rb
            be.copy_strided(pbuf, r0 * P * es, wins[k], 0, [r1 - r0, R], [P, 1], [R, 1], es)
            return wins[k][:(r1 - r0) * rb]
        transfer.copy_to_host(pbuf, out, produce=produce, chunk=wrows * rb)
        return out.view(self._dtype).reshape(self._shape)

    def tolocal(self):
        """As a local bolt array (array.py:999-1004)."""
        return BoltArrayLocal(self.toarray())

    def __array__(self, dtype=None, copy=None):
        a = self.toarray()
        return a if dtype is None else a.astype(dtype)

    def records(self):
        """(key tuple, value ndarray) pairs in key order -- the content of
        ``tordd().sortByKey().collect()`` of the Spark path."""
        x = self.toarray()
        kshape = self._shape[:self._split]
        flat = x.reshape((int(np.prod(kshape, dtype=np.int64)),) + self._shape[self._split:])
        for i, key in enumerate(np.ndindex(*kshape)):
            yield tuple(int(k) for k in key), flat[i]

    def display(self):
        """Print the first 10 records as (key, value) pairs, as the Spark
        mode's ``rdd.take(10)`` does (array.py:1022-1027).  Only the
        leading-axis rows that hold them leave the GPU; every rank takes part
        in the gather, rank 0 prints (the driver's console in Spark)."""
        kshape = self._shape[:self._split]
        nrec = int(np.prod(kshape, dtype=np.int64))
        n = min(10, nrec)
        if n == 0:
            return
        per_row = int(np.prod(kshape[1:], dtype=np.int64))
        rows = -(-n // per_row)
        part = self if rows >= self._shape[0] else self[0:rows]
        for i, rec in enumerate(part.records()):
            if i >= n:
                break
            if self._ctx.rank == 0:
                print(rec)

    def tordd(self):
        from bolt_amd.mi355x.records import RecordView
        return RecordView(list(self.records()), self._npartitions or self._ctx.world_size,
                          cached=getattr(self, "_cached", False))

    @property
    def _rdd(self):
        """A host view of the records (RecordView), for code written against
        the Spark mode's ``_rdd`` (collect, map, sortByKey, ...)."""
        return self.tordd()

    def __repr__(self):
        s = "BoltArray\n"
        s += "mode: %s\n" % self._mode
        s += "shape: %s\n" % str(self.shape)
        return s
