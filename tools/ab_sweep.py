#!/usr/bin/env python3
"""Same-box A/B of the lean sweep-kernel geometries (SDB_SWEEP_GEOM is read
per execute call, so one resident corpus serves every variant).

  python tools/ab_sweep.py [--docs 100000000] [--steps 10] [--warmup 2]
         [--geoms 0,24576x1024,...] [--k 1000] [--wand]
         [--libs name=path[@C],...] [--rounds N] [--skip-default]
         [--sels 0.10,0.05,0.02,0.01]

Prints one line per library and geometry: ms/step, kernel ms, postings/s,
the candidate count of the last step (what the kernel appended and the host
read back) and the hit-set parity against the first variant measured. With
--rounds N every arm is measured N times, arms alternating within each
round, and the line carries the median and the min..max spread over rounds,
of the candidate count too. A library
given as name=path@C is measured with SDB_SWEEP_ROUND_ITEMS=C (the sweep
kernel's posting-stage capacity clamped to C slots), so one library can
appear as several arms. --sels gives the plan: one OR term per selectivity
(e.g. 0.6,0.5 for a dense two-term plan).
"""

import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import serenedb_amd as sa  # noqa: E402

DEFAULT_GEOMS = "0,24576x1024,16384x1024,12288x512,8192x512,8192x256,4096x256"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--geoms", default=DEFAULT_GEOMS)
    ap.add_argument("--wand", action="store_true")
    ap.add_argument("--libs", default="",
                    help="name=path[@C],... : extra GPU libs to compare on "
                         "the same corpus (fresh context + segment reload "
                         "per lib; ablation/timing builds); @C runs the arm "
                         "with SDB_SWEEP_ROUND_ITEMS=C")
    ap.add_argument("--rounds", type=int, default=1,
                    help="measure every arm N times, the arms alternating "
                         "round by round on the one resident corpus; prints "
                         "per arm the median and min..max over rounds of "
                         "kernel ms and ms/step")
    ap.add_argument("--sels", default="0.10,0.05,0.02,0.01",
                    help="term selectivities of the synthetic corpus; the "
                         "plan is the OR of all of them")
    ap.add_argument("--skip-default", action="store_true",
                    help="with --libs: leave the in-tree library out")
    args = ap.parse_args()

    sels = [float(x) for x in args.sels.split(",")]
    nt = len(sels)
    t0 = time.time()
    blob = sa.build_synth_segment(43, 1, args.docs, sels)
    print(f"build {time.time()-t0:.1f}s blob {len(blob)/1e6:.0f}MB",
          flush=True)
    term_idx = list(range(nt))
    boosts = [1.0] * nt

    import ctypes as CT

    # postings per query = sum of term dfs (parse once)
    host = sa.host()
    v = np.frombuffer(blob, dtype=np.uint8)

    class _View(CT.Structure):
        _fields_ = [("hdr", CT.c_void_p), ("terms", CT.c_void_p),
                    ("desc", CT.c_void_p), ("norms", CT.c_void_p),
                    ("payload", CT.c_void_p)]

    class _Term(CT.Structure):
        _fields_ = [("desc_begin", CT.c_uint64),
                    ("desc_end", CT.c_uint64),
                    ("payload_begin", CT.c_uint64),
                    ("payload_end", CT.c_uint64),
                    ("df", CT.c_uint32), ("max_freq", CT.c_uint32),
                    ("total_freq", CT.c_uint64)]
    vw = _View()
    host.sdb_host_segment_parse(v.ctypes.data_as(CT.c_void_p),
                                CT.c_uint64(len(v)), CT.byref(vw))
    terms = CT.cast(vw.terms, CT.POINTER(_Term * nt)).contents
    postings = sum(terms[t].df for t in range(nt))

    libspecs = [("default", None)]
    round_items = {}
    for ent in (args.libs.split(",") if args.libs else []):
        nm, pth = ent.split("=", 1)
        if "@" in pth:
            pth, round_items[nm] = pth.rsplit("@", 1)
        libspecs.append((nm, pth))
    if args.skip_default and len(libspecs) > 1:
        libspecs = libspecs[1:]
    # every arm keeps its own library instance, context and resident copy
    # of the one corpus, so rounds can alternate between arms
    arms = []
    for libname, libpath in libspecs:
        if libpath is None:
            # leave an externally exported SDB_GPU_LIB alone unless this
            # run itself is comparing libs
            if len(libspecs) > 1:
                os.environ.pop("SDB_GPU_LIB", None)
        else:
            os.environ["SDB_GPU_LIB"] = libpath
        sa._gpu = None  # re-resolve the GPU library for this arm
        ctx = sa.GpuContext(0)
        arms.append((libname, ctx, ctx.load_segment(blob)))

    def measure(libname, ctx, seg):
        if libname in round_items:
            os.environ["SDB_SWEEP_ROUND_ITEMS"] = round_items[libname]
        else:
            os.environ.pop("SDB_SWEEP_ROUND_ITEMS", None)
        for _ in range(args.warmup):
            hits, total = ctx.execute_topk([seg], term_idx, boosts, args.k,
                                           wand=args.wand)
        kms = 0.0
        t1 = time.time()
        for _ in range(args.steps):
            hits, total = ctx.execute_topk([seg], term_idx, boosts, args.k,
                                           wand=args.wand)
            ms = CT.c_double(0)
            ctx._lib.sdb_gpu_last_kernel_ms(ctx._ctx, CT.byref(ms))
            kms += ms.value
        el = time.time() - t1
        nc = CT.c_uint(0)
        ctx._lib.sdb_gpu_last_stats(ctx._ctx, None, CT.byref(nc), None, None,
                                    None)
        cur = (hits["doc"].copy(), hits["score"].view(np.uint32).copy(),
               total)
        return el * 1000 / args.steps, kms / args.steps, cur, nc.value

    ref = None
    for geom in args.geoms.split(","):
        if geom == "wave":
            os.environ.pop("SDB_SWEEP_GEOM", None)
            os.environ["SDB_TOPK_PATH"] = "wave"
        else:
            os.environ.pop("SDB_TOPK_PATH", None)
            os.environ["SDB_SWEEP_GEOM"] = geom
        step_ms = {nm: [] for nm, _, _ in arms}
        kern_ms = {nm: [] for nm, _, _ in arms}
        ncands = {nm: [] for nm, _, _ in arms}
        parity = {}
        for _ in range(args.rounds):
            for libname, ctx, seg in arms:   # arms alternate within a round
                sms, kms, cur, nc = measure(libname, ctx, seg)
                ncands[libname].append(nc)
                step_ms[libname].append(sms)
                kern_ms[libname].append(kms)
                if ref is None:
                    ref = cur
                    parity[libname] = "ref"
                elif not (np.array_equal(ref[0], cur[0]) and
                          np.array_equal(ref[1], cur[1]) and
                          ref[2] == cur[2]):
                    parity[libname] = "MISMATCH"
                else:
                    parity.setdefault(libname, "OK")
        for libname, _, _ in arms:
            sm, km = step_ms[libname], kern_ms[libname]
            ncd = ncands[libname]
            if args.rounds == 1:
                print(f"lib={libname:8s} geom={geom:12s} "
                      f"{sm[0]:8.3f} ms/step "
                      f"kernel {km[0]:7.3f} ms  "
                      f"{postings/sm[0]/1e6:7.2f}G postings/s  "
                      f"cands {ncd[0]}  "
                      f"parity={parity[libname]}", flush=True)
            else:
                print(f"lib={libname:8s} geom={geom:12s} "
                      f"rounds={args.rounds} "
                      f"kernel ms median {np.median(km):7.4f} "
                      f"[{min(km):7.4f} .. {max(km):7.4f}]  "
                      f"ms/step median {np.median(sm):7.4f} "
                      f"[{min(sm):7.4f} .. {max(sm):7.4f}]  "
                      f"{postings/np.median(sm)/1e6:7.2f}G postings/s  "
                      f"cands median {int(np.median(ncd))} "
                      f"[{min(ncd)} .. {max(ncd)}]  "
                      f"parity={parity[libname]}", flush=True)


if __name__ == "__main__":
    main()
