#!/usr/bin/env python3
"""Hash-aggregate perf probe (dense kernel vs hash kernel, dense and
sparse keys), and the composite-key arm: GROUP BY two columns (a, b)
through scan_agg_hash_multi against scan_agg_hash over ONE precombined key
with the same grouping, on the same rows, predicates and aggregates. The
pairs run alternately in one process; median and min of the host clock
around each call (every call ends in a device synchronise and includes its
per-call workspace and readback)."""
import sys, os, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import serenedb_amd as sa

rows = int(os.environ.get("SDB_PROBE_ROWS", 400_000_000))
rng = np.random.default_rng(44)
keys = rng.integers(0, 1024, rows).astype(np.int64)
v1 = rng.integers(0, 1 << 20, rows).astype(np.int64)
v2 = rng.normal(0, 1, rows).astype(np.float32)
ctx = sa.GpuContext(0)
# columns 3, 4: the dense key split in two, keys == a * 32 + b; columns 5 to
# 7: the same for its low 8 bits, 256 groups
tab = ctx.load_table([keys, v1, v2, keys >> 5, keys & 31,
                      keys & 255, (keys >> 4) & 15, keys & 15])
c = int((1 << 20) * 0.1)
PREDS = [(1, 1, c, 0)]
AGGS = [(0, 0), (1, 1), (2, 2)]
arms = [
    ("dense", lambda: ctx.scan_agg(tab, 0, 1024, PREDS, AGGS)),
    ("hash-dense-keys", lambda: ctx.scan_agg_hash(tab, 0, 2048, PREDS, AGGS)),
]
for name, fn in arms:
    fn()
    t0 = time.time(); n = 4
    for _ in range(n): fn()
    dt = (time.time() - t0) / n
    print(f"{name}: {dt*1000:.2f} ms/pass = {rows/dt/1e9:.1f}G rows/s",
          flush=True)


def pair(label, one, two, rounds=9):
    """one-key and two-key arm alternately; the results must agree"""
    k1, i1, f1, p1 = one()
    k2, n2, i2, f2, p2 = two()
    assert p1 == p2 and len(k1) == len(k2) and not n2.any(), label
    assert np.array_equal(i1, i2), label      # COUNT and SUM_I64 are exact
    t = {"one": [], "two": []}
    for _ in range(rounds):
        for name, fn in (("one", one), ("two", two)):
            t0 = time.perf_counter()
            fn()
            t[name].append(time.perf_counter() - t0)
    med = {k: float(np.median(v)) for k, v in t.items()}
    for name, what in (("one", "one precombined key"), ("two", "two keys")):
        print(f"{label} {what}: median {med[name]*1000:.2f} ms "
              f"(min {min(t[name])*1000:.2f}) = "
              f"{rows/med[name]/1e9:.2f}G rows/s, {len(k1)} groups",
              flush=True)
    print(f"{label} two keys / one key rows/s: "
          f"{med['one']/med['two']:.3f}", flush=True)


pair("multi-dense-1024-groups",
     lambda: ctx.scan_agg_hash(tab, 0, 2048, PREDS, AGGS),
     lambda: ctx.scan_agg_hash_multi(tab, [3, 4], 2048, PREDS, AGGS))
# a quarter of the groups: the two-key LDS table (1024 slots at 3 aggregates,
# against 4096 for one key) is a quarter full, not full
pair("multi-dense-256-groups",
     lambda: ctx.scan_agg_hash(tab, 5, 2048, PREDS, AGGS),
     lambda: ctx.scan_agg_hash_multi(tab, [6, 7], 2048, PREDS, AGGS))
ctx.free_table(tab)
del keys

svals = rng.integers(-(1 << 60), 1 << 60, 100_000).astype(np.int64)
pick = rng.integers(0, 100_000, rows)
skeys = svals[pick]
# column 3: a second sparse key, a function of the group: (skeys, bkeys) has
# the groups of skeys
bkeys = rng.integers(-(1 << 60), 1 << 60, 100_000).astype(np.int64)[pick]
del pick
tab2 = ctx.load_table([skeys, v1, v2, bkeys])
def hs():
    return ctx.scan_agg_hash(tab2, 0, 200_000, PREDS, AGGS)
hs()
t0 = time.time(); n = 3
for _ in range(n): hs()
dt = (time.time() - t0) / n
print(f"hash-sparse-100k-groups: {dt*1000:.2f} ms/pass = "
      f"{rows/dt/1e9:.1f}G rows/s", flush=True)
pair("multi-sparse-100k-groups", hs,
     lambda: ctx.scan_agg_hash_multi(tab2, [0, 3], 200_000, PREDS, AGGS))
