"""bench.py's plain run and --dump-outputs: a run without --full prints the headline line and nothing it does not need, and writes
what the timed path handed its caller in the last timed step, the same from run to run with the same arguments. CPU part: the
writer on hand-made messages of two ranks. GPU part: two plain runs of a small batch."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAMES = ("bits", "stream_index", "frames", "consumed")


def _bench():
    import importlib
    return importlib.import_module("bench")


def _load(d):
    return {n: np.load(os.path.join(str(d), n + ".npy")) for n in NAMES}


def test_dump_outputs_writes_a_fixed_sample_of_the_messages(tmp_path, monkeypatch):
    import torch
    from pirip_amd.shard import make_payload
    b = _bench()
    B, maxf, nbits = 150, 12, 50
    rng = np.random.default_rng(1)
    bits = rng.integers(0, 2, (2 * B, maxf, nbits), dtype=np.uint8)
    nfr = rng.integers(0, maxf + 1, 2 * B).astype(np.int32)
    msgs = [make_payload(torch.from_numpy(bits[r * B:(r + 1) * B]), torch.from_numpy(nfr[r * B:(r + 1) * B])) for r in range(2)]
    cons = torch.arange(B, dtype=torch.int64) * 1200
    monkeypatch.setattr(b, "DUMP_BITS_BYTES", 40 * maxf * nbits * 4)        # room for 40 of the 300 streams
    b.dump_outputs(str(tmp_path / "a"), msgs, B, maxf, nbits, cons)
    b.dump_outputs(str(tmp_path / "b"), msgs, B, maxf, nbits, cons)
    a, a2 = _load(tmp_path / "a"), _load(tmp_path / "b")
    for n in NAMES:
        assert a[n].dtype in (np.float32, np.float64) and np.array_equal(a[n], a2[n])
    idx = a["stream_index"].astype(np.int64)
    assert len(idx) == 40 and np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < 2 * B
    assert idx.min() < B <= idx.max()                                        # both ranks' messages are sampled
    assert np.array_equal(a["frames"], nfr.astype(np.float32))
    assert np.array_equal(a["consumed"], cons.numpy().astype(np.float64))
    assert a["bits"].shape == (40, maxf, nbits)
    for k, s in enumerate(idx):
        n = nfr[s]
        assert np.array_equal(a["bits"][k, :n], bits[s, :n].astype(np.float32))
        assert not a["bits"][k, n:].any()


def test_dump_of_the_default_batch_stays_below_64_mb():
    b = _bench()
    B = 16384
    maxf = 1_200_000 // (2 * 1200 - 1212) + 2                                # HipDemod.max_frames_for at the defaults
    per_stream = maxf * 50 * 4
    n = min(B, b.DUMP_BITS_BYTES // per_stream)
    assert 0 < n and n * per_stream + B * (8 + 4 + 8) < 64 << 20


@pytest.mark.gpu
def test_plain_run_is_lean_and_its_outputs_repeat(tmp_path):
    """Two plain runs with the same arguments: the headline line without what --full adds, and the same dumped outputs."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--streams", "96", "--samples", "240000", "--steps", "3",
           "--warmup", "1"]
    runs = []
    for k in range(2):
        d = tmp_path / f"run{k}"
        r = subprocess.run(cmd + ["--dump-outputs", str(d)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        runs.append((json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]), _load(d)))
        assert sum(os.path.getsize(os.path.join(str(d), f)) for f in os.listdir(str(d))) < 64 << 20
    out, arrs = runs[0]
    assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0 and out["value"] > 0
    assert out["unit"] == "IQ Msamples/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    for key in ("cpu_baseline", "bit_check", "bit_errors_vs_cpu_ref", "extra_configs", "opt_in_band_only_estimator"):
        assert key not in out
    assert arrs["frames"].shape == (96,) and arrs["frames"].min() > 0 and arrs["consumed"].min() > 0
    assert arrs["bits"].shape[0] == 96 and set(np.unique(arrs["bits"])) <= {0.0, 1.0} and arrs["bits"].any()
    for n in NAMES:
        assert np.array_equal(arrs[n], runs[1][1][n]), n
