"""A plain `bench.py` run: the headline figure and nothing beside it -- one JSON line with the contract's headline keys, no
per-kernel times, no CPU baseline, no detail record -- and `--dump-outputs`: what the last timed step handed its caller, the
same from run to run and the same as the CPU oracle's words and the input symbols."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def _plain_run(out_dir):
    res = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out_dir)],
                         capture_output=True, text=True, timeout=600, cwd=str(ROOT))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_reports_the_headline_and_dumps_the_last_step(tmp_path):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    import bench
    from oracle import oracle as O
    detail = ROOT / "bench_detail.json"
    detail_before = detail.stat().st_mtime_ns if detail.exists() else None
    runs = [_plain_run(tmp_path / f"run{k}") for k in range(2)]
    assert (detail.stat().st_mtime_ns if detail.exists() else None) == detail_before       # a plain run writes no detail record
    for line in runs:
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert key in line, key
        for key in ("roofline", "encode_ms", "cpu_baseline", "configs_reported", "detail"):
            assert key not in line, key
        assert line["steps"] == 3 and line["warmup"] == 1 and line["bit_exact"] is True and line["higher_is_better"] is True
        assert line["value"] > 0 and abs(line["value"] - 65536 * 4096 / line["ms_per_step"] / 1e3) < 1e-3 * line["value"]

    first = {p.stem: np.load(p) for p in (tmp_path / "run0").glob("*.npy")}
    assert sorted(first) == ["decode_status", "decoded", "encode_status", "n_words", "sample_streams", "words"]
    assert sum(a.nbytes for a in first.values()) <= 64 << 20
    for name, a in first.items():
        assert np.array_equal(np.load(tmp_path / "run1" / f"{name}.npy"), a), f"{name} differs between two runs with the same arguments"
    assert first["n_words"].shape == (65536,) and (first["n_words"] > 0).all()
    assert not first["encode_status"].any() and not first["decode_status"].any()

    cdf = O.GaussianModel(bench.LO, bench.HI, bench.MEAN, bench.STD, bench.P, 32).cdf_table()
    pick = first["sample_streams"].astype(np.int64)
    for i in (0, 1, len(pick) - 1):
        s = int(pick[i])
        sym = O.synth_symbols(bench.SEED, s, 1, bench.N_PER, bench.LO, cdf, bench.P)
        want_words, want_n, _ = O.ans_encode_batch(sym, bench.LO, cdf, bench.P)
        n = int(want_n[0])
        assert first["n_words"][s] == n
        assert np.array_equal(first["words"][i, :n], want_words[0, :n].astype(np.float64)) and not first["words"][i, n:].any()
        assert np.array_equal(first["decoded"][i], sym[0].astype(np.float32))
