"""bench.py's stdout line stays parseable by the round-end driver.

Round 5's line grew to 23 KB and the driver's bounded tail cut it
(BENCH_r05 parsed: null).  The compact line is built here from recorded full
results (every line the bench measures) and must fit LINE_LIMIT, round-trip
through json, and carry the contract's keys plus roofline and cpu_baseline.
"""
import glob
import json
import os

import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
            "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline")


def recorded():
    out = []
    for p in sorted(glob.glob(os.path.join(ROOT, "profiles", "round5_bench_r5*.json"))):
        with open(p) as f:
            try:
                d = json.load(f)
            except ValueError:
                continue
        if isinstance(d, dict) and "metric" in d and "roofline" in d:
            out.append((os.path.basename(p), d))
    return out


@pytest.mark.parametrize("name,full", recorded(), ids=[n for n, _ in recorded()])
def test_compact_line_fits_and_round_trips(name, full):
    full = json.loads(json.dumps(full))
    big = len(json.dumps(full))
    line = bench.compact_line(full, "gpurun_out/bench_detail.json")
    s = json.dumps(line)
    assert len(s) <= bench.LINE_LIMIT, (name, len(s))
    assert "\n" not in s
    back = json.loads(s)
    for k in CONTRACT:
        assert k in back, k
    assert back["value"] == full["value"]
    assert back["ms_per_step"] == full["ms_per_step"]
    assert back["roofline"]["frac"] == full["roofline"]["frac"]
    assert back["roofline"]["traffic"] == full["roofline"]["traffic"]
    assert back["cpu_baseline"]["value"] == full["cpu_baseline"]["value"]
    assert back["detail_file"] == "gpurun_out/bench_detail.json"
    assert big > len(s)


def test_compact_line_bounded_even_with_huge_extras():
    full = {"metric": "m", "value": 1.0, "unit": "u", "n_gpus": 1, "steps": 1, "warmup": 0,
            "ms_per_step": 1.0, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "u32", "data": "synthetic", "config": {"workload": "C2"},
            "roofline": {"bound": "valu", "frac": 0.3, "traffic": None},
            "cpu_baseline": {"value": 1.0, "lines": [{"impl": "x", "value": 1.0}] * 3},
            "sha256_stage": {"pad": "x" * 20000},
            "go_wiring_latency": {"pad": "y" * 50000}}
    s = json.dumps(bench.compact_line(full, None))
    assert len(s) <= bench.LINE_LIMIT
    assert json.loads(s)["value"] == 1.0


def test_plain_line_holds_the_headline_keys():
    """Without --full the line is built from the headline alone."""
    full = {"metric": "m", "value": 3.0, "unit": "verifies/s", "n_gpus": 1, "steps": 7, "warmup": 2,
            "ms_per_step": 0.5, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "u32", "data": "synthetic", "config": {"workload": "C2"}, "kernel_ms": {}}
    back = json.loads(json.dumps(bench.compact_line(full, None)))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps"):
        assert back[k] == full[k], k
    assert back["cpu_baseline"] is None and back["detail_file"] is None
    assert "p50_batch_latency_definition" not in back


def test_options_full_and_dump_outputs(monkeypatch):
    monkeypatch.setattr("sys.argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 3
    monkeypatch.setattr("sys.argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"


def test_dump_outputs_float32_bounded_and_repeatable(tmp_path, monkeypatch):
    import numpy as np
    st = (np.arange(1 << 12) % 3).astype(np.uint8)
    bench.dump_outputs(str(tmp_path / "a"), 0, {"statuses": st})
    got = np.load(tmp_path / "a" / "statuses.npy")
    assert got.dtype == np.float32 and (got == st).all()
    # past the size limit: the same seeded rows every time, in order
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4 * 1000)
    bench.dump_outputs(str(tmp_path / "b"), 0, {"statuses": st})
    bench.dump_outputs(str(tmp_path / "c"), 1, {"statuses": st})
    b = np.load(tmp_path / "b" / "statuses.npy")
    c = np.load(tmp_path / "c" / "statuses_rank1.npy")
    assert b.nbytes <= 4 * 1000 and b.shape == (1000,) and (b == c).all()
    assert set(np.unique(b)) <= {0.0, 1.0, 2.0}


def test_reject_mix_construction():
    """The timed batch's mix: every 97th item altered, kinds cycling; want
    marks the three rejecting kinds, high s (N - s) stays an accept."""
    import torch
    B = 97 * 8 + 5
    g = torch.Generator().manual_seed(7)
    e, r, s = (torch.randint(0, 256, (B, 32), dtype=torch.uint8, generator=g) for _ in range(3))
    s[:, 0] = 0x7F                                           # s < N
    e2, r2, s2, want, counts = bench.reject_mix(torch, torch.device("cpu"), e, r, s, B)
    assert counts == {"altered": 9, "rejects": 7, "high_s_accepts": 2}
    assert want.nonzero().flatten().tolist() == [0, 97, 194, 388, 485, 582, 776]
    same = torch.ones(B, dtype=torch.bool)
    same[::97] = False
    assert torch.equal(e2[same], e[same]) and torch.equal(r2[same], r[same]) and torch.equal(s2[same], s[same])
    assert (e2[0] != e[0]).sum() == 1 and torch.equal(e2[97], e[97])
    assert int.from_bytes(s2[97].numpy().tobytes(), "big") == bench.N_ORDER
    assert not r2[194].any()
    hi = int.from_bytes(s2[291].numpy().tobytes(), "big")
    assert hi == bench.N_ORDER - int.from_bytes(s[291].numpy().tobytes(), "big")


def test_detail_file_written(tmp_path):
    full = {"metric": "m", "value": 2.0, "nested": {"a": [1, 2, 3]}}
    p = str(tmp_path / "sub" / "d.json")
    got = bench.write_detail(full, p)
    assert got == p
    with open(p) as f:
        assert json.load(f) == full
