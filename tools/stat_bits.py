"""Record of what the statistics entry points (bm_reduce*, bm_standardize_*,
bm_comoment_*) plan and write, to compare two builds of the library whose
kernels are the same (tools/kernel_isa_diff.py): any difference is then one of
the host's making -- a vector width, a tile, a chunk count, a split launch.

    BOLT_AMD_LIB=<library A> python tools/stat_bits.py [--host] --out a.json
    BOLT_AMD_LIB=<library B> python tools/stat_bits.py [--host] --out b.json
    python tools/stat_bits.py --compare a.json b.json   # exit 1 on any difference

Each library runs in a process of its own, on the same seeded inputs.

"host" entries (no GPU needed; --host records nothing else): the return code
and byte count of bm_reduce_workspace_bytes for every statistic x dtype and of
bm_comoment_workspace_bytes for every dtype x K = 1..4 over the layouts of
HOST_GRID -- the chunk counts of both plans -- and the return codes and
messages for the dtype codes -1 and 12.

"device" entries: SHA-256 of every output, of the caller's workspace (preset
to 0xEE, so the chunks' partial states and how many there are show) and of the
kept states, plus the kept / taken flags.  Every reduction runs twice, the
second time with the source one element further on: the pointer's alignment,
not the extents, then picks the vector.  The launch loops that split a grid at
2^32 threads are not reached at these sizes.
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DTYPES = ["bool", "uint8", "int8", "uint16", "int16", "uint32", "int32", "uint64", "int64", "float16", "float32",
          "float64"]  # index: the BM_* dtype code
HOST_GRID = [(1, 1, 1), (3, 4100, 1), (3, 4101, 1), (8192, 4100, 1), (5, 100, 1), (2, 2000, 12), (2, 2000, 13),
             (2, 600, 12), (1, 70000, 3), (300, 9, 4096), (64, 5000, 1), (7, 250, 1), (1, 1 << 20, 1), (1, 100000, 64)]
# (O, R, I, row pitch): rows in one chunk; chunked at vec 4 (float32); vec 1;
# pitched rows; columns chunked over a narrow tile; columns at vec 1; columns
# in one chunk over full 64-vector tiles
RED_SHAPES = [(5, 100, 1, 100), (3, 4100, 1, 4100), (3, 4101, 1, 4101), (7, 250, 1, 256), (2, 2000, 12, 2000),
              (2, 2000, 13, 2000), (300, 9, 4096, 9)]
RED_STATS = [("mean", 0), ("var", 1), ("sum", 3), ("max", 4), ("prod", 6), ("lor", 8)]
RED_DTYPES = ["float16", "float32", "float64", "uint8", "int16", "int64", "bool"]
FLOATS = ["float16", "float32", "float64"]
# bm_standardize_rows (dtype, O, R, pitch): wave per row; padded rows; block
# per row; too few rows for a block each (taken == 0); widened 1-byte input
STD_ROWS = [("float32", 64, 100, 100), ("float32", 64, 2000, 2048), ("float32", 256, 5000, 5000),
            ("float32", 8, 5000, 5000), ("uint8", 64, 2000, 2000)]
STD_APPLY = [("float32", 3, 4100, 1), ("float32", 2, 2000, 12)]
# bm_comoment_state: rows in three chunks; columns, chunked; pitched rows
CO_SHAPES = [(64, 5000, 1, 5000), (2, 2000, 12, 2000), (7, 250, 1, 256)]
CO_DTYPES = ["float32", "int16"]


def stat_dtype(name):
    return name if name in ("float16", "float32") else "float64"


def values(name, n, seed):
    """n seeded values around 10 in dtype `name` (bool: about half set)"""
    x = np.random.default_rng(seed).standard_normal(n) * 3 + 10
    if name == "bool":
        return x > 10
    return (np.clip(x, 0, 255) if name == "uint8" else x).astype(name)


def record_host(lib):
    rec = {}
    n = ctypes.c_size_t(0)
    for O, R, I in HOST_GRID:
        for dt in range(12):
            for stat in range(14):
                rc = lib.bm_reduce_workspace_bytes(stat, dt, O, R, I, ctypes.byref(n))
                rec["reduce_ws stat %d dtype %d (%d, %d, %d)" % (stat, dt, O, R, I)] = [rc, n.value]
            for K in range(1, 5):
                rc = lib.bm_comoment_workspace_bytes(dt, O, R, I, K, ctypes.byref(n))
                rec["comoment_ws dtype %d K %d (%d, %d, %d)" % (dt, K, O, R, I)] = [rc, n.value]
    for dt in (-1, 12):
        rc = lib.bm_reduce_workspace_bytes(0, dt, 3, 4100, 1, ctypes.byref(n))
        rec["reduce_ws dtype %d" % dt] = [rc, lib.bm_last_error().decode()]
        rc = lib.bm_comoment_workspace_bytes(dt, 3, 4100, 1, 1, ctypes.byref(n))
        rec["comoment_ws dtype %d" % dt] = [rc, lib.bm_last_error().decode()]
    return rec


def record_device(lib):
    import torch
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev).cuda_stream or None
    rec = {}

    def filled(nbytes, byte):
        return torch.full((max(int(nbytes), 1),), byte, dtype=torch.uint8, device=dev)

    def upload(a, off=0):
        """a on the device, `off` elements past an aligned start -> (owner, pointer)"""
        raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        buf = filled(raw.size + (off + 16) * a.itemsize, 0)
        buf[off * a.itemsize: off * a.itemsize + raw.size] = torch.from_numpy(raw.copy()).to(dev)
        return buf, buf.data_ptr() + off * a.itemsize

    def digest(t):
        torch.cuda.synchronize()
        return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()

    def call(name, *args):
        rc = getattr(lib, name)(*args)
        if rc == -2:  # BM_E_HIP: nothing more on this device
            raise SystemExit("%s: %s" % (name, lib.bm_last_error().decode()))
        return rc

    def reduce_ws(stat, code, O, R, I):
        n = ctypes.c_size_t(0)
        call("bm_reduce_workspace_bytes", stat, code, O, R, I, ctypes.byref(n))
        return filled(n.value, 0xEE), n.value

    for O, R, I, pitch in RED_SHAPES:
        nout = O * I
        for name in RED_DTYPES:
            code = DTYPES.index(name)
            x = values(name, O * pitch * I, O * 4099 + R * 7 + I)
            for off in (0, 1):
                owner, src = upload(x, off)
                where = "%s (%d, %d, %d) pitch %d off %d" % (name, O, R, I, pitch, off)
                for sname, stat in RED_STATS:
                    isf = name in FLOATS
                    oname = ("bool" if sname == "lor" else name if sname == "max" or (sname in ("sum", "prod") and not isf)
                             else stat_dtype(name))
                    out = filled(nout * np.dtype(oname).itemsize, 0xAB)
                    ws, nws = reduce_ws(stat, code, O, R, I)
                    if I == 1:
                        rc = call("bm_reduce_rows", stat, src, code, O, R, pitch, out.data_ptr(), DTYPES.index(oname),
                                  ws.data_ptr(), nws, stream)
                    else:
                        rc = call("bm_reduce", stat, src, code, O, R, I, out.data_ptr(), DTYPES.index(oname),
                                  ws.data_ptr(), nws, stream)
                    rec["reduce %s %s" % (sname, where)] = [rc, nws, digest(out), digest(ws)]
                if name not in FLOATS:
                    continue
                ocode = DTYPES.index(stat_dtype(name))
                oes = np.dtype(stat_dtype(name)).itemsize
                for sname, stat in RED_STATS[:2]:
                    out, state = filled(nout * oes, 0xAB), filled(nout * 16, 0xCD)
                    ws, nws = reduce_ws(stat, code, O, R, I)
                    kept = ctypes.c_int(-1)
                    rc = call("bm_reduce_keep", stat, src, code, O, R, I, pitch, out.data_ptr(), ocode,
                              state.data_ptr(), ctypes.byref(kept), ws.data_ptr(), nws, stream)
                    rec["keep %s %s" % (sname, where)] = [rc, kept.value, digest(out), digest(state), digest(ws)]
                outs = [filled(nout * oes, 0xAB) for _ in range(3)]
                ws, nws = reduce_ws(1, code, O, R, I)
                rc = call("bm_reduce_moments", src, code, O, R, I, pitch, outs[0].data_ptr(), outs[1].data_ptr(),
                          outs[2].data_ptr(), ocode, ws.data_ptr(), nws, stream)
                rec["moments %s" % where] = [rc] + [digest(o) for o in outs] + [digest(ws)]

    for name, O, R, pitch in STD_ROWS:
        x = values(name, O * pitch, O * 31 + R)
        owner, src = upload(x)
        oname = stat_dtype(name)
        for scale in (0, 1):
            dst = filled(O * pitch * np.dtype(oname).itemsize, 0xAB)
            taken = ctypes.c_int(-1)
            rc = call("bm_standardize_rows", src, DTYPES.index(name), O, R, pitch, dst.data_ptr(), DTYPES.index(oname),
                      pitch, scale, ctypes.byref(taken), stream)
            rec["standardize_rows %s (%d, %d) pitch %d scale %d" % (name, O, R, pitch, scale)] = [
                rc, taken.value, digest(dst)]
    for name, O, R, I in STD_APPLY:
        x = values(name, O * R * I, O * 37 + R + I)
        x64 = x.reshape(O, R, I).astype(np.float64)
        owner, src = upload(x)
        mean, sd = upload(x64.mean(axis=1)), upload(x64.std(axis=1))
        for scale in (0, 1):
            dst = filled(x.nbytes, 0xAB)
            rc = call("bm_standardize_apply", src, DTYPES.index(name), O, R, I, R, mean[1], sd[1] if scale else None,
                      dst.data_ptr(), DTYPES.index(name), R, stream)
            rec["standardize_apply %s (%d, %d, %d) scale %d" % (name, O, R, I, scale)] = [rc, digest(dst)]

    for O, R, I, pitch in CO_SHAPES:
        nout = O * I
        for name in CO_DTYPES:
            code = DTYPES.index(name)
            owner, src = upload(values(name, O * pitch * I, O * 41 + R + I))
            for K in range(1, 5):
                y = np.random.default_rng(R + K).standard_normal((K, R))
                ym = y.mean(axis=1)
                yd = y - ym[:, None]
                yown, yptr = upload(y)
                n = ctypes.c_size_t(0)
                call("bm_comoment_workspace_bytes", code, O, R, I, K, ctypes.byref(n))
                ws, state = filled(n.value, 0xEE), filled((2 + K) * nout * 8, 0xCD)
                f64 = lambda v: (ctypes.c_double * K)(*[float(t) for t in v])  # noqa: E731
                rc = call("bm_comoment_state", src, code, O, R, I, pitch, yptr, f64(ym), f64(yd.sum(axis=1)), K,
                          state.data_ptr(), ws.data_ptr(), n.value, stream)
                item = [rc, n.value, digest(state), digest(ws)]
                for what in (0, 1):
                    out = filled(K * nout * 8, 0xAB)
                    item.append(call("bm_comoment_combine", what, state.data_ptr(), (ctypes.c_int64 * 1)(R), f64(ym),
                                     f64((yd * yd).sum(axis=1)), 1, nout, K, out.data_ptr(), 11, stream))
                    item.append(digest(out))
                rec["comoment %s (%d, %d, %d) pitch %d K %d" % (name, O, R, I, pitch, K)] = item
    torch.cuda.synchronize()
    return rec


def compare(a, b):
    ra, rb = json.load(open(a)), json.load(open(b))
    print("A:", ra["lib"])
    print("B:", rb["lib"])
    bad = 0
    for part in ("host", "device"):
        pa, pb = ra.get(part), rb.get(part)
        if pa is None and pb is None:
            print("%s: not recorded" % part)
            continue
        keys = sorted(set(pa or {}) | set(pb or {}))
        diff = [k for k in keys if (pa or {}).get(k) != (pb or {}).get(k)]
        for k in diff:
            print("DIFFERENT %s: %s | %s" % (k, (pa or {}).get(k), (pb or {}).get(k)))
        failed = [k for k in keys if k not in diff and part == "device" and pa[k][0] != 0]
        for k in failed:
            print("FAILED in both %s: %s" % (k, pa[k]))
        print("%s: %d entries, %d different, %d failed calls" % (part, len(keys), len(diff), len(failed)))
        bad += len(diff) + len(failed)
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--host", action="store_true", help="the host entries only (no GPU)")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    if not args.host:
        import torch  # noqa: F401  (before the library: both then share torch's HIP runtime)
    from bolt_amd.mi355x import _lib
    lib = _lib.load()
    rec = {"lib": os.path.abspath(_lib.LIB_PATH), "host": record_host(lib)}
    if not args.host:
        rec["device"] = record_device(lib)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    print("%s: %d host entries, %d device entries -> %s" % (rec["lib"], len(rec["host"]), len(rec.get("device", {})),
                                                             args.out))
