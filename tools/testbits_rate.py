#!/usr/bin/env python3
"""Time of the test-frame counter (include/pirip_hip.h section L) behind the benchmark's batch.

    python tools/testbits_rate.py [--streams 16384] [--frames 1000] [--reps 5] [--cpu-streams 256] [--parent-ms MS]

bench.py's batch (BASELINE config 2) leaves 16 384 streams x 1000 frames of 50 bits, packed (7 bytes per row), on the device. This times
ONE pirip_hip_tbits_push over rows of that shape -- test frames, every stream at its own bit offset, a few streams with bit errors --
as the median of --reps runs after one warm-up, bracketed by device synchronisation, and checks the counters of the streams it also
counts on the host. The comparison: downloading the bits and running the CPU counter (oracle.put_test_bits) on 16 processes; the
host count runs on --cpu-streams streams and is scaled to the batch (the streams cost the same), the download is timed in full.
--parent-ms: bench.py's ms_per_step, to print the push as a share of a step. No test runs this; no threshold depends on it."""
import argparse
import multiprocessing as mp
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _count(bits):
    from oracle import binding as ob
    r = ob.put_test_bits(bits)
    return r["packets"], r["bits"], r["errors"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=16384)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-streams", type=int, default=256)
    ap.add_argument("--parent-ms", type=float, default=0.0)
    a = ap.parse_args()
    from oracle import binding as ob
    B, R, nb = a.streams, a.frames, 50
    rng = np.random.default_rng(3)
    base = []
    for k in range(100):                                     # 100 base rows: every bit offset of the frame; every 7th with 1 % bit errors
        b = ob.get_test_bits(R * nb + 100)[k:k + R * nb].copy()
        if k % 7 == 3:
            b[rng.random(b.size) < 0.01] ^= 1
        base.append(np.packbits(b.reshape(R, nb), axis=-1))
    base = np.stack(base)                                    # [100, R, 7]
    pool = mp.get_context("spawn").Pool(16)                  # (before the GPU is opened in this process)
    pool.map(_count, [np.zeros(200, np.uint8)] * 16)

    import torch
    import pirip_amd
    dbase = torch.from_numpy(base).cuda()
    bits = dbase[torch.arange(B, device="cuda") % 100].contiguous()                   # [B, R, 7]
    nfr = torch.full((B,), R, dtype=torch.int32, device="cuda")
    tb = pirip_amd.HipTestBits(nstreams=B)
    print(f"device: {torch.cuda.get_device_name(0)}; {B} streams x {R} rows of {nb} bits, packed: {bits.numel() / 1e6:.1f} MB")

    def timed(f):
        f()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts))

    t_push = timed(lambda: tb.push(bits, nframes=nfr, row_bits=nb, packed=True))
    t_down = timed(lambda: bits.cpu())
    tb.reset()
    tb.push(bits, nframes=nfr, row_bits=nb, packed=True)
    got = tb.counters()
    n = min(a.cpu_streams, B)
    host = [np.unpackbits(base[s % 100], axis=-1)[:, :nb].reshape(-1) for s in range(n)]
    t0 = time.perf_counter()
    res = pool.map(_count, host, chunksize=max(1, n // 64))
    t_cpu = (time.perf_counter() - t0) * B / n
    pool.close()
    for s in range(n):
        assert (got["packets"][s], got["bits"][s], got["errors"][s]) == res[s], (s, res[s])
    print(f"push: {t_push * 1e3:.3f} ms ({B * R * nb / t_push / 1e9:.1f} G positions/s); counters of {n} streams equal the CPU counter's")
    print(f"host path: download {t_down * 1e3:.1f} ms + oracle.put_test_bits on 16 processes {t_cpu * 1e3:.0f} ms "
          f"(measured on {n} streams, scaled to {B}) = {(t_down + t_cpu) / t_push:.0f} x the push")
    if a.parent_ms > 0:
        print(f"share of a benchmark step of {a.parent_ms:.2f} ms: {100 * t_push * 1e3 / a.parent_ms:.2f} %")


if __name__ == "__main__":
    main()
