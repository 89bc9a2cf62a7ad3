#!/usr/bin/env python3
"""ORDER BY col LIMIT k perf probe: scan_topn (k = 1000, DESC) against the
dense scan_agg with one group and COUNT(*) under the same predicates — code
this feature does not touch — on the same synthetic table, in the same
process, alternately. Four order columns (uniform-random i64, sorted i64,
constant, FoR timestamp-like), each with no predicate and with a 10 %
BETWEEN on a second column.

  python tools/probe_topn.py [--out profiles/topn_probe.log]

runs one child process per order column, each under its own `timeout`, one
after the other, and stops at the first that fails (the steps are chained as
with &&); the children's lines are appended to the log. A child is
`python tools/probe_topn.py --case NAME`.

Times are the host clock around each call; every call ends in a device
synchronise and includes its readbacks and the host-side select / sort.
Median of ROUNDS after one warm-up of each arm. A scan_topn call runs
hist_passes histogram scans and one collect scan (the row-order arm adds a
count scan), so the figure to read is
    ratio = t_topn / ((hist_passes + 1) * t_reference):
1.0 means every scan of the call runs at the reference scan's speed."""
import argparse
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

CASES = ("uniform", "sorted", "constant", "for_ts")
ROWS = int(os.environ.get("SDB_PROBE_ROWS", 100_000_000))
ROUNDS = 9
K = 1000
STEP_TIMEOUT = int(os.environ.get("SDB_PROBE_STEP_TIMEOUT", 280))


def run_case(name):
    import numpy as np

    import serenedb_amd as sa

    rng = np.random.default_rng(47)
    codec = "for" if name == "for_ts" else "raw"
    if name == "uniform":
        order = rng.integers(-(1 << 62), 1 << 62, ROWS).astype(np.int64)
    elif name == "sorted":
        order = np.arange(ROWS, dtype=np.int64) * 3 + 1_700_000_000
    elif name == "constant":
        order = np.full(ROWS, 7, dtype=np.int64)
    else:   # microsecond timestamps, a few events per millisecond
        order = 1_700_000_000_000_000 + np.cumsum(
            rng.integers(0, 500, ROWS).astype(np.int64))
    filt = rng.integers(0, 1 << 20, ROWS).astype(np.int64)
    one = np.zeros(ROWS, dtype=np.int64)
    ctx = sa.GpuContext(0)
    tab = ctx.load_table([order, filt, one], [codec] * 3)
    band = int((1 << 20) * 0.1)
    for label, preds in (("nopred", []), ("between10", [(1, 3, 0, band - 1)])):
        ref = lambda: ctx.scan_agg(tab, 2, 1, preds, [(0, 0)])     # noqa: E731
        top = lambda: ctx.scan_topn(tab, 0, K, preds, desc=True,   # noqa: E731
                                    stats=True)
        i64, _, passed = ref()
        rows, vals, isnull, tpassed, st = top()
        assert tpassed == passed == int(i64[0, 0]), (tpassed, passed)
        assert len(rows) == min(K, passed) and not isnull.any()
        assert (np.diff(vals) <= 0).all()
        sel = np.ones(ROWS, bool) if not preds else (filt < band)
        assert vals[0] == order[sel].max(), "top value"
        del sel
        t = {"ref": [], "top": []}
        for _ in range(ROUNDS):
            for arm, fn in (("ref", ref), ("top", top)):
                t0 = time.perf_counter()
                fn()
                t[arm].append(time.perf_counter() - t0)
        med = {a: float(np.median(v)) for a, v in t.items()}
        scans = st["hist_passes"] + 1
        print(f"{name} {label}: rows {ROWS} passed {passed} k {K} | "
              f"reference scan_agg median {med['ref'] * 1e3:.3f} ms "
              f"(min {min(t['ref']) * 1e3:.3f}) | scan_topn median "
              f"{med['top'] * 1e3:.3f} ms (min {min(t['top']) * 1e3:.3f}) | "
              f"hist_passes {st['hist_passes']} tie_arm {st['tie_arm']} "
              f"candidates {st['candidates']} rowgroups_skipped "
              f"{st['rowgroups_skipped']} | ratio t_topn / ({scans} x t_ref) "
              f"= {med['top'] / (scans * med['ref']):.2f}", flush=True)
    ctx.free_table(tab)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=CASES)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles",
                                                  "topn_probe.log"))
    args = ap.parse_args()
    if args.case:
        run_case(args.case)
        return 0
    with open(args.out, "a") as log:
        for name in CASES:
            cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT), sys.executable,
                   os.path.abspath(__file__), "--case", name]
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
