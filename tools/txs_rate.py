#!/usr/bin/env python3
"""Rate of the streaming transmitter (include/pirip_hip.h section K) against the two stages it fuses (sections I and J).

    python tools/txs_rate.py [--outputs 64] [--channels 8] [--symbols 500] [--reps 5]

W outputs x K channels each, FIR, u8 out, 2-FSK at 40 kS/s and 1000 symbols/s, at D = 6 (240 kS/s) and D = 30 (1.2 MS/s). Every queue is
filled with random symbols' worth of frames first, so that no call underruns. Per shape: wideband samples/s of one pirip_hip_txs_process
call of --symbols symbols per channel, and of pirip_hip_tx_modulate (complex float) + pirip_hip_mux_batch on the same symbols; the bytes
are compared. HBM bytes per output sample: 8K/D written + 8K/D read + 2 for the two stages, about 2 for the fused call (--hbm-gbs,
default 8000). Times are medians of --reps runs after one warm-up, bracketed by device synchronisation; the fused call is timed on
fresh queue contents each time (reset, send, synchronise, then the clock)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def med(f, reps, before=None):
    import torch
    ts = []
    for i in range(reps + 1):
        if before:
            before()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        if i:
            ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def main():
    import torch
    import pirip_amd
    ap = argparse.ArgumentParser()
    ap.add_argument("--outputs", type=int, default=64)
    ap.add_argument("--channels", type=int, default=8)
    ap.add_argument("--symbols", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0)
    a = ap.parse_args()
    W, K, S = a.outputs, a.channels, a.symbols
    N = W * K
    mFs, Rs, M = 40000, 1000, 2
    print(f"device: {torch.cuda.get_device_name(0)}; {W} outputs x {K} channels, FIR, u8 out, {S} symbols per channel and call")
    rng = np.random.default_rng(1)
    for D in (6, 30):
        Fs = mFs * D
        offs = [int(v) for v in rng.integers(-Fs // 2 + 1, Fs // 2, N)]
        tx = pirip_amd.HipTx(pirip_amd.STANDIN_CODE, mFs, Rs, M, nstreams=N, f1=1000, shift=2000)
        ref = pirip_amd.HipTx(pirip_amd.STANDIN_CODE, mFs, Rs, M, nstreams=N, f1=1000, shift=2000)
        mx = pirip_amd.HipMux(Fs, D, offs, outputs=[c // K for c in range(N)], gains=[0.3 / K] * N)
        nrec = -(-S // tx.frame_syms)
        rec = torch.from_numpy(rng.integers(0, 256, (N, nrec, tx.record_bytes)).astype(np.uint8))
        rec[:, :, 0] = 0
        rec = rec.cuda()
        block = S * D * tx.Ts
        txs = pirip_amd.HipTxStream(tx, mx, block, nrec * tx.frame_syms)
        out = torch.zeros((W, block * 2), dtype=torch.uint8, device="cuda")

        def fill():
            txs.reset()
            txs.send(rec.data_ptr(), rec[0].numel(), nrec)

        def fused():
            txs.process(out.data_ptr(), block * 2)

        t_f = med(fused, a.reps, before=fill)
        assert not txs.counters()["underrun"].any()
        # the two stages on the same symbols
        cap = ref.max_syms(nrec)
        syms = torch.zeros((N, cap), dtype=torch.uint8, device="cuda")
        ref.frame(rec.data_ptr(), rec[0].numel(), nrec, syms.data_ptr(), cap, cap)
        Q = mx.Q
        n_in = Q - 1 + S * tx.Ts
        rows = torch.zeros((N, n_in, 2), dtype=torch.float32, device="cuda")
        out2 = torch.zeros((W, block * 2), dtype=torch.uint8, device="cuda")

        def staged():
            ref.modulate(syms.data_ptr(), cap, S, rows.data_ptr() + (Q - 1) * 8, n_in * 8, out_format=pirip_amd.IN_CF32)
            mx.batch(rows.data_ptr(), n_in * 8, n_in, out2.data_ptr(), block * 2, m0=-(Q - 1))

        t_s = med(staged, a.reps, before=ref.reset)
        same = bool(torch.equal(out, out2))
        sps_f, sps_s = W * block / t_f, W * block / t_s
        b_s, b_f = 16.0 * K / D + 2.0, 2.0 + 5.0 * K / (D * tx.Ts)
        print(f"D {D:3d} Q {Q}: fused {t_f * 1e3:8.3f} ms {sps_f / 1e9:6.2f} G wideband samples/s ({b_f:.3f} B per output sample -> "
              f"{b_f * sps_f / 1e9:6.1f} GB/s); modulate + mux {t_s * 1e3:8.3f} ms {sps_s / 1e9:6.2f} G samples/s ({b_s:.2f} B -> "
              f"{b_s * sps_s / 1e9:6.1f} GB/s = {100 * b_s * sps_s / 1e9 / a.hbm_gbs:5.2f} % of {a.hbm_gbs:.0f} GB/s); "
              f"fused / staged rate {t_s / t_f:.2f}; bytes equal: {same}")
        del txs, tx, ref, mx, rows, out, out2


if __name__ == "__main__":
    main()
