#!/usr/bin/env python3
"""Rate of the band monitor (include/pirip_hip.h section P): averaged wideband spectra and band powers on the device.

    python tools/spec_rate.py [--shape all|wide1|wide64|narrow] [--calls N] [--reps 5] [--warmup 2] [--ceiling-gbs 6300]

Shapes (u8 input, six bands per stream):
    wide1   nfft 4096, half overlap, 16 segments per row, 1 stream of 2^22 samples per call
    wide64  the same, 64 streams
    narrow  nfft 256, no overlap, 1 segment per row, 4096 streams of 2^16 samples per call
Printed per shape, with rows stored and without: input samples/s of pirip_hip_spec_push over consecutive calls (--calls; by default 400
for wide1 and 20 for the others, so that a run is a large fraction of a second; the second and later calls carry a tail and, with avg > 1,
a running row), and the share of the HBM read ceiling that reading the input once, at 2 bytes per sample, takes at that rate (--ceiling-gbs: the read-only ceiling of tools/hbm_read_ceiling.hip, 6.3 TB/s in profiles/README.md).
Times are medians of --reps runs after --warmup warm-up runs, each run bracketed by device synchronisation."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {
    "wide1": dict(nfft=4096, hop=2048, avg=16, nstreams=1, n=1 << 22, calls=400),
    "wide64": dict(nfft=4096, hop=2048, avg=16, nstreams=64, n=1 << 22, calls=20),
    "narrow": dict(nfft=256, hop=256, avg=1, nstreams=4096, n=1 << 16, calls=20),
}


def med(f, reps, warmup):
    import torch
    for _ in range(warmup):
        f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    import torch
    import pirip_amd
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["all"] + list(SHAPES), default="all")
    ap.add_argument("--calls", type=int, default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ceiling-gbs", type=float, default=6300.0)
    a = ap.parse_args()
    Fs = 2400000
    print(f"device: {torch.cuda.get_device_name(0)}; median of {a.reps} runs after {a.warmup} warm-up runs")
    for name in (list(SHAPES) if a.shape == "all" else [a.shape]):
        s = SHAPES[name]
        S, n, nfft = s["nstreams"], s["n"], s["nfft"]
        calls = a.calls or s["calls"]
        bands = [(r, lo, lo + 150000) for r in range(S) for lo in (-1200000, -800000, -400000, 0, 400000, 800000)]
        sp = pirip_amd.HipSpectrum(Fs, nfft, hop=s["hop"], avg=s["avg"], nstreams=S, bands=bands)
        x = torch.randint(0, 256, (S, n, 2), dtype=torch.uint8, device="cuda")
        most = n // s["hop"] // s["avg"] + 1                          # a call completes at most this many rows
        rows = torch.zeros((S, most, nfft), dtype=torch.float32, device="cuda")
        entries = torch.zeros((len(bands), most, 12), dtype=torch.uint8, device="cuda")
        for keep in (True, False):
            def run():
                sp.reset()
                for _ in range(calls):
                    sp.push_raw(x, n * 2, n, rows if keep else None, nfft, most * nfft, entries, most)

            t, lo, hi = med(run, a.reps, a.warmup)
            sps = S * n * calls / t
            print(f"{name} (nfft {nfft}, hop {s['hop']}, avg {s['avg']}, {S} streams x {n} samples, {calls} calls per run), rows {'stored' if keep else 'not stored'}: "
                  f"{t / calls * 1e3:8.3f} ms per call (runs {lo / calls * 1e3:.3f} .. {hi / calls * 1e3:.3f}), {sps / 1e9:7.2f} G input samples/s, "
                  f"2 B per sample -> {2 * sps / 1e9:7.1f} GB/s = {100 * 2 * sps / 1e9 / a.ceiling_gbs:5.2f} % of the {a.ceiling_gbs:.0f} GB/s read ceiling")
        sp.close()


if __name__ == "__main__":
    main()
