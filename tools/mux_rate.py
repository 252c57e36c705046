#!/usr/bin/env python3
"""Rate of the multiplexer (include/pirip_hip.h section J): K modem-rate channels -> W wideband u8 IQ streams on the device.

    python tools/mux_rate.py [--outputs 64] [--channels 8] [--n-in 20000] [--reps 5]

W outputs x K channels each, complex float noise in, the default FIR, u8 out, at D = 30 (2.4 MS/s) and D = 6 (240 kS/s). Per shape:
wideband samples/s of pirip_hip_mux_batch and the HBM traffic it implies at 8 K / D + 2 bytes per output sample (every input read once,
every output written once; --hbm-gbs, default 8000). Times are medians of --reps runs after one warm-up, bracketed by device
synchronisation. Then the one comparison there is: x45 linear interpolation and u8 quantisation of one channel in numpy on the host --
what this repository's tools and tests do wherever they need wideband input -- against HipMux(kind=MUX_LINEAR, D=45) on the same data,
with and without the copies to and from the device.

    python tools/mux_rate.py --pmc-run    # one D = 30 call and nothing else: the program of a counter-only rocprofv3 --pmc SQ_INSTS_VALU
                                          # pass (VALU per (channel, output) = mux_kernel's count * 64 / (K * W * outputs))"""
import argparse
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
    return float(np.median(ts))


def main():
    import torch
    import pirip_amd
    ap = argparse.ArgumentParser()
    ap.add_argument("--outputs", type=int, default=64)
    ap.add_argument("--channels", type=int, default=8)
    ap.add_argument("--n-in", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0)
    ap.add_argument("--pmc-run", action="store_true")
    a = ap.parse_args()
    W, K = a.outputs, a.channels
    print(f"device: {torch.cuda.get_device_name(0)}; {W} outputs x {K} channels, FIR, u8 out, {a.n_in} input samples per channel")
    rng = np.random.default_rng(1)
    for Fs, D in ((2400000, 30), (240000, 6)):
        offs = [int(v) for v in rng.integers(-Fs // 2 + 1, Fs // 2, W * K)]
        outs = [c // K for c in range(W * K)]
        mx = pirip_amd.HipMux(Fs, D, offs, outputs=outs, gains=[0.3 / K] * (W * K))
        z = torch.randn((W * K, a.n_in, 2), dtype=torch.float32, device="cuda")
        no = mx.nout(a.n_in)
        out = torch.zeros((W, no * 2), dtype=torch.uint8, device="cuda")

        def run():
            mx.batch(z.data_ptr(), a.n_in * 8, a.n_in, out.data_ptr(), no * 2)

        if a.pmc_run:
            run()
            torch.cuda.synchronize()
            print(f"pmc run: D {D} Q {mx.Q}: {W} outputs x {no} samples x {K} channels = {W * no * K} (channel, output) pairs, 1 call; "
                  f"floor 2 Q = {2 * mx.Q} packed fma per pair")
            return
        t = med(run, a.reps)
        sps = W * no / t
        bps = 8.0 * K / D + 2.0
        print(f"D {D:3d} Q {mx.Q}: {t * 1e3:9.3f} ms, {sps / 1e9:7.2f} G wideband samples/s, {K * sps / 1e9:7.2f} G (channel, output)/s, "
              f"{bps:.2f} B per output sample -> {bps * sps / 1e9:7.1f} GB/s = {100 * bps * sps / 1e9 / a.hbm_gbs:5.2f} % of {a.hbm_gbs:.0f} GB/s")
        del mx, z, out

    # the host path: one channel, x45 linear interpolation and the u8 quantiser in numpy
    D, n = 45, 40000
    x = (rng.normal(size=n) + 1j * rng.normal(size=n)).astype(np.complex64) * np.float32(0.3)

    def host():
        t = np.arange((n - 1) * D) / float(D)
        i0 = np.floor(t).astype(np.int64)
        fr = (t - i0).astype(np.float32)
        hi = (1 - fr) * x[i0] + fr * x[i0 + 1]
        v = np.stack([hi.real, hi.imag], axis=-1)
        return np.clip(np.rint(127.5 * v + 127.5), 0, 255).astype(np.uint8)

    host()
    ts = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        ref = host()
        ts.append(time.perf_counter() - t0)
    t_host = float(np.median(ts))
    mx = pirip_amd.HipMux(1800000, D, [0], kind=pirip_amd.MUX_LINEAR)
    xin = np.concatenate([np.zeros(mx.Q - 1, np.complex64), x])
    no = mx.nout(len(xin))
    d_out = torch.zeros(no * 2, dtype=torch.uint8, device="cuda")
    d_in = torch.from_numpy(xin.view(np.float32).copy()).cuda()

    def dev():
        mx.batch(d_in.data_ptr(), len(xin) * 8, len(xin), d_out.data_ptr(), no * 2, m0=-(mx.Q - 1))

    def dev_copies():
        d = torch.from_numpy(xin.view(np.float32).copy()).cuda()
        mx.batch(d.data_ptr(), len(xin) * 8, len(xin), d_out.data_ptr(), no * 2, m0=-(mx.Q - 1))
        return d_out.cpu()

    t_dev, t_devc = med(dev, a.reps), med(dev_copies, a.reps)
    got = d_out.cpu().numpy().reshape(-1, 2)[D - 1:D - 1 + len(ref)]               # the LINEAR kind is D - 1 samples late
    diff = int(np.abs(got.astype(np.int64) - ref.astype(np.int64)).max())
    print(f"one channel x{D}, {n} samples in: numpy on the host {t_host * 1e3:.2f} ms; HipMux LINEAR {t_dev * 1e3:.3f} ms on the device "
          f"({t_host / t_dev:.0f} x), {t_devc * 1e3:.3f} ms with upload and download ({t_host / t_devc:.1f} x); largest byte difference {diff}")


if __name__ == "__main__":
    main()
