"""bench.py as a command: a plain run prints the headline line and nothing
that needs runs of its own; --full adds the CPU baselines and the embedded
scan/hybrid benches; --dump-outputs writes the last timed step's results,
identical from run to run. Small corpora (the workload shape is the
benchmark's own; only --docs/--rows shrink) keep each run to seconds."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--docs", "200000", "--rows", "1000000"]


def _bench(*extra):
    p = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1",
         *SMALL, *extra],
        cwd=REPO, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, p.stdout  # ONE JSON result line
    return json.loads(lines[0])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_reproducible_outputs(tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    r = _bench("--steps", "3", "--warmup", "1", "--dump-outputs", a)
    assert r["metric"] == \
        "docs scored/sec BM25 top-1000 (+ rows/sec filter-agg)"
    assert r["unit"] == "docs/s" and r["higher_is_better"] is True
    assert r["dtype"] == "f32"
    assert r["steps"] == 3 and r["warmup"] == 1
    assert r["ms_per_step"] > 0
    # value is docs scored per second of timed step; ms_per_step is
    # printed rounded to 1e-3 ms, which bounds the disagreement
    docs_per_step = r["config"]["total_matches"]
    assert r["value"] == pytest.approx(
        docs_per_step / (r["ms_per_step"] / 1e3),
        rel=0.0005 / r["ms_per_step"] + 1e-3)
    # nothing that takes runs of its own
    assert r["cpu_baseline"] is None
    assert "extra_benches" not in r

    out = _load(a)
    assert set(out) == {"bm25_scores", "bm25_docs", "bm25_total_matches"}
    assert out["bm25_scores"].dtype == np.float32
    assert out["bm25_docs"].dtype == np.float64
    assert out["bm25_scores"].shape == out["bm25_docs"].shape == (1000,)
    assert out["bm25_total_matches"][0] == docs_per_step
    # engine order: score descending, doc ascending on ties
    s, d = out["bm25_scores"], out["bm25_docs"]
    assert (np.diff(s) <= 0).all()
    assert (np.diff(d)[np.diff(s) == 0] > 0).all()

    # same arguments (another step count: every step recomputes the same
    # query) -> the same arrays, bit for bit
    _bench("--steps", "2", "--warmup", "0", "--dump-outputs", b)
    out_b = _load(b)
    assert set(out_b) == set(out)
    for name in out:
        np.testing.assert_array_equal(out[name], out_b[name])


@pytest.mark.gpu
def test_full_run_embeds_baselines_and_extra_benches(tmp_path):
    d = str(tmp_path / "full")
    r = _bench("--steps", "2", "--warmup", "1", "--full",
               "--cpu-seconds", "0.2", "--dump-outputs", d)
    assert r["metric"] == \
        "docs scored/sec BM25 top-1000 (+ rows/sec filter-agg)"
    assert r["cpu_baseline"]["value"] > 0
    scan, hyb = r["extra_benches"]
    assert scan["metric"] == "rows/sec filter-agg"
    assert scan["cpu_baseline"]["value"] > 0
    assert hyb["metric"].endswith("+ range filter-agg")
    assert hyb["cpu_baseline"]["value"] > 0
    for sub in (r, scan, hyb):
        assert sub["steps"] == 2 and sub["ms_per_step"] > 0
        assert sub["roofline"]["peak"] == 8000.0

    out = _load(d)
    assert {"bm25_scores", "scan_count", "scan_sum_i64", "scan_sum_f64",
            "scan_rows_passed", "hybrid_scores", "hybrid_bucket_count",
            "hybrid_bucket_sum"} <= set(out)
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    # the scan counts every row that passes the predicate exactly once
    assert out["scan_count"].shape == (1024,)
    assert out["scan_count"].sum() == out["scan_rows_passed"][0] > 0
    # hybrid buckets count the filtered matches
    assert out["hybrid_bucket_count"].sum() == \
        out["hybrid_total_matches"][0] > 0
