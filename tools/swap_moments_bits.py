"""Byte-for-byte record of bm_copy_strided_moments, to compare two builds of the
library: the destination, the raw tile workspace (K, mean - K, M2 per b-tile)
and the merged state of one call per shape, as SHA-256 digests.

    BOLT_AMD_LIB=<library A> python tools/swap_moments_bits.py --out a.json
    BOLT_AMD_LIB=<library B> python tools/swap_moments_bits.py --out b.json
    python tools/swap_moments_bits.py --compare a.json b.json   # exit 1 on any difference

Each library runs in a process of its own, on the same inputs (seeded).  The
shapes are those of tests/test_zz_swap_moments_diet.py as (La rows, R values,
pitch) plus C2's own (262144 rows of 2000 float32 at pitch 2048); rows 3 and 5
carry a NaN and two infinities at tile starts.

The destination and the tile workspace -- all the transpose kernel writes --
are compared whole, rows 3 and 5 included.  The merged state is compared
whole for every other row; the (mean, M2) of rows 3 and 5 is printed and
compared apart (``state_nonfinite``), because the merge kernel's M2 of a row
with a NaN or an infinity is NaN from this tree on, where the parent's merge
stored 0: a difference there is reported, not counted.
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (dtype, La, R, pitch)
CASES = [
    ("float32", 128, 256, 256), ("float32", 128, 260, 260), ("float32", 128, 40, 40), ("float32", 128, 442, 448),
    ("float32", 128, 758, 768), ("float32", 120, 760, 768), ("float32", 72, 760, 768), ("float32", 128, 760, 768),
    ("float64", 32, 256, 256), ("float64", 64, 258, 258), ("float64", 64, 66, 66), ("float64", 128, 24, 24),
    ("float64", 64, 221, 224), ("float64", 32, 1001, 1024), ("float64", 54, 1000, 1024), ("float64", 70, 260, 260),
    ("float32", 262144, 2000, 2048),
]


def _digest(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def run(out):
    import torch
    from bolt_amd.mi355x import _lib
    from bolt_amd.mi355x._ops import backend_for, dtype_code
    dev = torch.device("cuda:0")
    be = backend_for(dev)
    rec = {"lib": os.path.abspath(_lib.LIB_PATH), "cases": {}}
    for dtype, La, R, pitch in CASES:
        dt = np.dtype(dtype)
        es = dt.itemsize
        gen = torch.Generator(device="cpu").manual_seed(La * 4099 + R)
        x = torch.randn((R, La), generator=gen, dtype=getattr(torch, dtype)).mul_(3).add_(10)
        x[0, 3] = float("nan")
        x[0, 5] = float("inf")
        if R > 256:
            x[256, 5] = float("inf")
        src = x.to(dev).view(torch.uint8).reshape(-1)
        dst = torch.full((La * pitch * es,), 0xAB, dtype=torch.uint8, device=dev)
        arrs = (_lib.i64_array([La, R]), _lib.i64_array([1, La]), _lib.i64_array([pitch, 1]))
        code = dtype_code(dt)
        n = ctypes.c_size_t(0)
        _lib.check(be.lib.bm_copy_strided_moments_workspace_bytes(2, arrs[0], arrs[1], arrs[2], es, code, R, pitch,
                                                                  La, ctypes.byref(n)), "workspace_bytes")
        ws = torch.full((max(n.value, 1),), 0xEE, dtype=torch.uint8, device=dev)
        nstate = be.state_bytes(_lib.STAT_VAR, code, La)
        state = torch.full((nstate,), 0xCD, dtype=torch.uint8, device=dev)
        fused = ctypes.c_int(-1)
        _lib.check(be.lib.bm_copy_strided_moments(src.data_ptr(), dst.data_ptr(), 2, arrs[0], arrs[1], arrs[2], es,
                                                  code, R, pitch, La, ws.data_ptr(), n.value, state.data_ptr(),
                                                  nstate, ctypes.byref(fused), be._stream(src)),
                   "bm_copy_strided_moments")
        torch.cuda.synchronize()
        key = "%s %dx%d pitch %d" % (dtype, La, R, pitch)
        st = state.cpu().numpy().view(np.float64).reshape(2, La)
        fin = np.ones(La, dtype=bool)
        fin[[3, 5]] = False
        rec["cases"][key] = {"fused": fused.value, "b_tiles": n.value // (24 * La), "dst": _digest(dst),
                             "workspace": _digest(ws),
                             "state": hashlib.sha256(np.ascontiguousarray(st[:, fin]).tobytes()).hexdigest(),
                             "state_nonfinite": [repr(float(v)) for v in st[:, ~fin].reshape(-1)]}
        print(key, rec["cases"][key], flush=True)
        del src, dst, ws, state, x
    with open(out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)


def compare(a, b):
    ra, rb = json.load(open(a)), json.load(open(b))
    print("A:", ra["lib"])
    print("B:", rb["lib"])
    bad = 0
    for key in sorted(set(ra["cases"]) | set(rb["cases"])):
        ca, cb = ra["cases"].get(key), rb["cases"].get(key)
        strict = lambda c: c and dict((k, v) for k, v in c.items() if k != "state_nonfinite")
        same = ca is not None and strict(ca) == strict(cb) and ca["fused"] == 1
        bad += not same
        print("%-36s %s  b-tiles %s" % (key, "identical (dst, workspace, state)" if same else "DIFFERENT %s | %s" % (ca, cb),
                                        ca and ca["b_tiles"]))
        if same:
            print("%-36s rows 3, 5 (mean, mean, M2, M2): A %s  B %s" % ("", ca["state_nonfinite"], cb["state_nonfinite"]))
    print("%d cases, %d different" % (len(ra["cases"]), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    run(args.out)
