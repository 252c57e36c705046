#!/usr/bin/env python3
"""Rate of the channel (include/pirip_hip.h section O): T transmitted wideband IQ streams onto R received ones on the device.

    python tools/air_rate.py [--receivers 64] [--paths 2] [--n 1048576] [--calls 1000] [--reps 5] [--sigma 0.1] [--clock-ppb 0]
                             [--fade-millihz 0] [--rice-k 0] [--in-format u8] [--out-format u8] [--digest]

R receivers x K paths each (two transmitters; every path rotated, delays up to 4097 samples), u8 (or cf32) in and out, n samples per call.
Printed per variant -- with noise, and with sigma 0 (no Box-Muller) --: wideband samples/s of pirip_hip_air_push over --calls consecutive
calls, and the HBM traffic it implies at (2 K + 2) bytes per output sample (every path's input read once, every output written once;
--hbm-gbs, default 8000). Times are medians of --reps runs after one warm-up run, each a
fraction of a second of back-to-back calls bracketed by device synchronisation.
--clock-ppb Q (default 0: the run above and nothing else) adds, behind that run and in the same session, the same paths with a clock
offset of Q parts per billion each: every delay grows by 8 + max_slip, max_slip being what one run of --calls calls
slips, and every run starts from a reset, which enqueues nothing.
--fade-millihz N [--rice-k K] (default 0: nothing more) adds, in the same session, the static paths with a fade of N millihertz and Rician
K on every one of them, keyed by the path's index.
--digest times nothing: with torch seeded, every variant makes two calls from a reset -- the second reads the rings -- and the sha256 of
both calls' output rows is printed. Two builds of the library (PIRIP_HIP_LIB, as tools/ab_rates.py) that compute the same words print
the same lines."""
import argparse
import hashlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def med(f, reps):
    import torch
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
    ap.add_argument("--receivers", type=int, default=64)
    ap.add_argument("--paths", type=int, default=2)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--calls", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sigma", type=float, default=0.1)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0)
    ap.add_argument("--clock-ppb", type=int, default=0)
    ap.add_argument("--fade-millihz", type=int, default=0)
    ap.add_argument("--rice-k", type=float, default=0.0)
    ap.add_argument("--in-format", choices=("u8", "cf32"), default="u8")
    ap.add_argument("--out-format", choices=("u8", "cf32"), default="u8")
    ap.add_argument("--digest", action="store_true")
    a = ap.parse_args()
    R, K, n, Fs, T = a.receivers, a.paths, a.n, 2400000, 2
    print(f"device: {torch.cuda.get_device_name(0)}; {R} receivers x {K} paths, {T} transmitters, {a.in_format} -> {a.out_format}, {n} samples per call, {a.calls} calls per run")
    rng = np.random.default_rng(1)
    paths = [(r, k % T, 0.3 / K, int(rng.integers(0, 4098)), int(rng.integers(1, Fs // 2))) for r in range(R) for k in range(K)]
    if a.digest:
        torch.manual_seed(1)
    fmt = {"u8": pirip_amd.IN_CU8_CSDR, "cf32": pirip_amd.IN_CF32}
    bsi, bso = (2 if f == "u8" else 8 for f in (a.in_format, a.out_format))
    if a.in_format == "u8":
        d_in = torch.randint(0, 256, (T, n * 2), dtype=torch.uint8, device="cuda")
    else:
        d_in = torch.rand((T, n * 2), dtype=torch.float32, device="cuda") * 2.0 - 1.0
    d_out = torch.zeros((R, n * 2), dtype=torch.uint8 if a.out_format == "u8" else torch.float32, device="cuda")
    bps = float(bsi * K + bso)
    variants = [("", paths, 0, None)]
    if a.clock_ppb:
        slip = abs(a.clock_ppb) * n * a.calls // 10 ** 9 + 1
        variants.append((f"clock {a.clock_ppb} ppb, max_slip {slip}, ", [(r, t, g, d + 8 + slip, f, a.clock_ppb) for r, t, g, d, f in paths], slip, None))
    if a.fade_millihz:
        fades = [pirip_amd.AirFade(i, a.fade_millihz, a.rice_k, i) for i in range(len(paths))]
        variants.append((f"fade {a.fade_millihz} mHz, K {a.rice_k:g}, ", paths, 0, fades))
    for tag, pth, slip, fades, sigma in [(t, p, s, fd, sg) for t, p, s, fd in variants for sg in (a.sigma, 0.0)]:
        air = pirip_amd.HipAir(Fs, pth, T, R, sigma=sigma, seed=1, max_slip=slip, fades=fades, in_format=fmt[a.in_format], out_format=fmt[a.out_format])

        def run():
            if slip:
                air.reset(0)                                      # the budget starts again; nothing is enqueued
            for _ in range(a.calls):
                air.push(d_in, n * bsi, n, d_out, n * bso)

        if a.digest:
            sha = hashlib.sha256()
            air.reset(0)
            for _ in range(2):
                d_out.zero_()
                air.push(d_in, n * bsi, n, d_out, n * bso)
                sha.update(d_out.cpu().numpy().tobytes())
            print(f"DIGEST {a.in_format} -> {a.out_format}, {tag}sigma {sigma}: {sha.hexdigest()}")
            air.close()
            continue

        t, lo, hi = med(run, a.reps)
        sps = R * n * a.calls / t
        print(f"{tag}sigma {sigma}: {t / a.calls * 1e3:8.3f} ms per call (runs {lo / a.calls * 1e3:.3f} .. {hi / a.calls * 1e3:.3f}), {sps / 1e9:7.2f} G wideband samples/s, "
              f"{bps:.0f} B per output sample -> {bps * sps / 1e9:7.1f} GB/s = {100 * bps * sps / 1e9 / a.hbm_gbs:5.2f} % of {a.hbm_gbs:.0f} GB/s")
        air.close()

if __name__ == "__main__":
    main()
