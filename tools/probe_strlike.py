#!/usr/bin/env python3
"""CONTAINS perf probe: the two raw substring kernels and the FSST kernel of
sdb_gpu_strpred_mask / sdb_gpu_strpred_like on one synthetic column, in one
process, alternately, against the existing `prefix` op on the same table as
the launch-and-offsets floor. It is the measurement behind the dispatch rule
of DESIGN.md (strings section).

  python tools/probe_strlike.py [--out profiles/strlike_probe.log]

runs one child process per column shape, each under its own `timeout`, one
after the other, and stops at the first that fails; the children's lines are
appended to the log. A child is `python tools/probe_strlike.py --case NAME`.

Column (NumPy only, no per-row Python): random lowercase bytes, an 8-byte
literal planted in about 1% of the rows, and enough rows that the blob
exceeds the 256 MiB last-level cache.

  uniform  row lengths uniform in 20..100 bytes
  skewed   99% of the rows 20 bytes, 1% 4000 bytes

Arms, each the median of ROUNDS calls after one warm-up of every arm:

  coop     CONTAINS on the raw slot, cooperative kernel (the default)
  rowwise  the same under SDB_LIKE_ROWWISE=1, row-wise kernel
  fsst     CONTAINS on an FSST slot of the same rows. Its table is the 26
           one-byte symbols a..z (code = byte - 'a'), which NumPy can encode:
           it exercises the decode loop and compresses nothing, so its
           traffic equals the raw blob's
  prefix   the existing PREFIX op with the same literal on the raw slot

Times are the host clock around each call; every call ends in a device
synchronise. Each arm is reported as rows/s and as the bytes it has to move,
blob + 8 * rows (offsets) + rows / 8 (mask), over time, against the 8 TB/s
HBM peak. With --prefix-only the prefix arm runs alone, through calls that
older checkouts have too: copied into the tools/ of a checkout of the parent
commit, this file measures that commit's prefix op on the same column and
the same machine."""
import argparse
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

CASES = ("uniform", "skewed")
ROWS = int(os.environ.get("SDB_PROBE_ROWS", 6_000_000))
ROUNDS = 9
LIT = b"qzjxkvwy"
PEAK = 8e12
STEP_TIMEOUT = int(os.environ.get("SDB_PROBE_STEP_TIMEOUT", 280))


def make_column(name, rows=None):
    """(offsets uint64[rows + 1], blob uint8[], planted row ids)"""
    import numpy as np

    rows = rows or ROWS
    rng = np.random.default_rng(53)
    if name == "uniform":
        lens = rng.integers(20, 101, rows).astype(np.uint64)
    else:
        lens = np.where(rng.random(rows) < 0.01, 4000, 20).astype(np.uint64)
    off = np.zeros(rows + 1, dtype=np.uint64)
    np.cumsum(lens, out=off[1:])
    blob = rng.integers(97, 123, int(off[-1]), dtype=np.uint8)
    hit = np.flatnonzero(rng.random(rows) < 0.01)
    at = off[hit] + (rng.random(len(hit)) *
                     (lens[hit] - len(LIT) + 1).astype(np.float64)
                     ).astype(np.uint64)
    blob[(at[:, None] + np.arange(len(LIT), dtype=np.uint64)).ravel()] = \
        np.tile(np.frombuffer(LIT, dtype=np.uint8), len(hit))
    return off, blob, hit


def run_case(name, prefix_only):
    import ctypes as C

    import numpy as np

    import serenedb_amd as sa

    off, blob, hit = make_column(name)
    rows = len(off) - 1
    moved = len(blob) + 8 * rows + rows // 8
    ctx = sa.GpuContext(0)
    tab = ctx.load_table([np.zeros(rows, dtype=np.int64)])
    ctx.attach_strcol(tab, 0, off, blob)
    lit = (C.c_uint8 * len(LIT))(*LIT)

    def prefix():
        rc = ctx._lib.sdb_gpu_strpred_mask(
            ctx._ctx, tab, C.c_uint32(0), C.c_int(8), lit,
            C.c_uint32(len(LIT)), lit, C.c_uint32(0))
        assert rc == 0, rc

    def passed(slot):
        return ctx.scan_agg(tab, 0, 1, [(slot, 7, 0, 0)], [(0, 0)])[2]

    def contains(slot, rowwise):
        def f():
            if rowwise:
                os.environ["SDB_LIKE_ROWWISE"] = "1"
            else:
                os.environ.pop("SDB_LIKE_ROWWISE", None)
            ctx.strpred_mask(tab, slot, "contains", LIT)
        return f

    arms = {"prefix": prefix}
    if not prefix_only:
        ctx.attach_strcol_fsst(tab, 1, off, blob - np.uint8(97),
                               [bytes([c]) for c in range(97, 123)])
        arms = {"coop": contains(0, False), "rowwise": contains(0, True),
                "fsst": contains(1, False), "prefix": prefix}
        counts = {}
        for arm in ("coop", "rowwise", "fsst"):
            arms[arm]()
            counts[arm] = passed(0 if arm != "fsst" else 1)
        assert len(set(counts.values())) == 1, counts
        assert counts["coop"] >= len(hit), (counts, len(hit))
        print(f"{name}: rows {rows} blob {len(blob)} bytes "
              f"({len(blob) / 2**20:.0f} MiB) literal {LIT!r} planted in "
              f"{len(hit)} rows, {counts['coop']} rows match on all three "
              f"CONTAINS arms", flush=True)
    for fn in arms.values():
        fn()
    t = {a: [] for a in arms}
    for _ in range(ROUNDS):
        for arm, fn in arms.items():
            t0 = time.perf_counter()
            fn()
            t[arm].append(time.perf_counter() - t0)
    for arm, v in t.items():
        med = float(np.median(v))
        print(f"{name} {arm}: median {med * 1e3:.3f} ms (min "
              f"{min(v) * 1e3:.3f}, max {max(v) * 1e3:.3f}) | "
              f"{rows / med / 1e9:.2f} G rows/s | {moved / med / 1e12:.3f} "
              f"TB/s = {100 * moved / med / PEAK:.1f}% of 8 TB/s", flush=True)
    os.environ.pop("SDB_LIKE_ROWWISE", None)
    ctx.free_table(tab)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=CASES)
    ap.add_argument("--prefix-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles",
                                                  "strlike_probe.log"))
    args = ap.parse_args()
    if args.case:
        run_case(args.case, args.prefix_only)
        return 0
    with open(args.out, "a") as log:
        for name in CASES:
            cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT), sys.executable,
                   os.path.abspath(__file__), "--case", name]
            if args.prefix_only:
                cmd.append("--prefix-only")
            p = subprocess.run(cmd, stdout=subprocess.PIPE,
                               stderr=subprocess.STDOUT, text=True)
            sys.stdout.write(p.stdout)
            sys.stdout.flush()
            log.write(p.stdout)
            log.flush()
            if p.returncode != 0:   # nothing more on the GPU after a failure
                msg = f"{name}: exit status {p.returncode}; stopping\n"
                sys.stdout.write(msg)
                log.write(msg)
                return p.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
