#!/usr/bin/env python3
"""Time per block of the streaming repeater (include/pirip_hip.h section M) against the same steps driven from the host.

    python tools/rpt_rate.py [--channels 4] [--symbols 100] [--blocks 80] [--reps 3]

K FSK_LDPC channels (the stand-in code, 2-FSK, 1000 symbols/s at 40 kS/s) on one wideband stream at D = 6, K / 4 groups of the offsets
tests/muxshapes.py's loopback uses. A terminal's bursts of three frames are made once with HipTxStream; then, per repetition, --blocks
blocks go through
  device: HipRepeater.push per block -- receiver, filter, state machine, pending ring, offer, framer, queue, multiplexer; nothing waits;
  host:   HipRx.push, a synchronise and the download of the frame counts behind it, HipTx.repeat_records on the received rows, a second
          synchronise for the record counts, HipTxStream.send of whatever came out, HipTxStream.process
and the wall time per block of either is printed, bracketed by device synchronisation. The host loop knows no hold-off and no pending
ring (a refused send is lost), so the two outputs are not compared: this is a cost figure, not a check."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OFFSETS = [-90000, -30000, 30001, 90000]


def main():
    import torch
    import pirip_amd
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=4)
    ap.add_argument("--symbols", type=int, default=100)
    ap.add_argument("--blocks", type=int, default=80)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    K, S, nblk = a.channels, a.symbols, a.blocks
    if K < 1 or K > 4:
        ap.error("--channels 1 .. 4: the offsets of one 240 kS/s stream")
    Fs, D, mFs, Rs, M, nframes, gap = 240000, 6, 40000, 1000, 2, 3, 64
    offs = OFFSETS[:K]
    print(f"device: {torch.cuda.get_device_name(0)}; {K} channels, {S} symbols per block, {nblk} blocks")
    rng = np.random.default_rng(2)

    def tx_side():
        tx = pirip_amd.HipTx(pirip_amd.STANDIN_CODE, mFs, Rs, M, nstreams=K, f1=1000, shift=2000, gap=gap)
        mux = pirip_amd.HipMux(Fs, D, offs, gains=[0.1] * K)
        block = S * D * tx.Ts
        burst = tx.preamble_syms + nframes * tx.frame_syms + gap
        return tx, mux, pirip_amd.HipTxStream(tx, mux, block, burst + S), block

    def rx_side(block):
        dem = pirip_amd.HipDemod(mFs, Rs, M, P=10, est_min=500, est_max=15000, in_format=pirip_amd.IN_CF32, nstreams=K)
        ld = pirip_amd.HipLdpc(pirip_amd.STANDIN_CODE, M, nstreams=K)
        ch = pirip_amd.HipChan(Fs, D, offs)
        return dem, ld, ch, pirip_amd.HipRx(dem, ldpc=ld, chan=ch, block=block)

    # the terminal's blocks
    tx0, mux0, txs0, block = tx_side()
    rec = rng.integers(0, 256, (K, nframes + 1, tx0.record_bytes)).astype(np.uint8)
    rec[:, :, 0] = [1] + [0] * (nframes - 1) + [2]
    rec[:, :nframes, 1] = 1
    rec[:, nframes, 1:] = 0
    d_rec = torch.from_numpy(rec).cuda()
    blocks = torch.zeros((nblk, block * 2), dtype=torch.uint8, device="cuda")
    for k in range(nblk):
        if k == 2:
            txs0.send(d_rec.data_ptr(), rec[0].size, rec.shape[1])
        txs0.process(blocks[k].data_ptr(), block * 2)
    torch.cuda.synchronize()
    out = torch.zeros(block * 2, dtype=torch.uint8, device="cuda")

    # device: one call per block
    tx, mux, txs, _ = tx_side()
    handles = rx_side(block)
    rpt = pirip_amd.HipRepeater(tx, txs, list(range(K)), 2, filter=2, holdoff=1, max_burst=nframes, rx=handles[3])
    t_dev = []
    for _ in range(a.reps + 1):
        rpt.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(nblk):
            rpt.push(blocks[k], block * 2, out, block * 2)
        torch.cuda.synchronize()
        t_dev.append((time.perf_counter() - t0) / nblk)
    c = rpt.counters()

    # host: the same steps with a synchronise after the receive
    tx2, mux2, txs2, _ = tx_side()
    dem, ld, ch, rx = rx_side(block)
    R, kb = rx.max_frames, ld.data_bytes
    st = torch.zeros((K, R), dtype=torch.uint8, device="cuda")
    pl = torch.zeros((K, R, kb), dtype=torch.uint8, device="cuda")
    info = torch.zeros((K, R, pirip_amd.LDPC_INFO_PER_CALL), dtype=torch.int32, device="cuda")
    nfr = torch.zeros(K, dtype=torch.int32, device="cuda")
    cap = tx2.repeat_max_records(R)
    recs = torch.zeros((K, cap, 1 + kb), dtype=torch.uint8, device="cuda")
    nrec = torch.zeros(K, dtype=torch.int32, device="cuda")
    t_host, sent = [], 0
    for _ in range(a.reps + 1):
        rx.reset()
        tx2.reset()
        txs2.reset()
        sent = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(nblk):
            rx.push(blocks[k].data_ptr(), block * 2, d_status=st.data_ptr(), d_payload=pl.data_ptr(), d_info=info.data_ptr(), d_nframes=nfr.data_ptr())
            torch.cuda.synchronize()
            n = nfr.cpu().numpy()
            if n.any():
                tx2.repeat_records(st.data_ptr(), R, pl.data_ptr(), R * kb, R, 2, recs.data_ptr(), cap * (1 + kb), cap, d_ncalls=nfr.data_ptr(),
                                   d_nrec=nrec.data_ptr())
                torch.cuda.synchronize()
                m = nrec.cpu().numpy()
                if m.any():
                    txs2.send(recs.data_ptr(), cap * (1 + kb), int(m.max()), d_nrec=nrec.data_ptr())
                    sent += int(m.sum())
            txs2.process(out.data_ptr(), block * 2)
        torch.cuda.synchronize()
        t_host.append((time.perf_counter() - t0) / nblk)
    td, th = float(np.median(t_dev[1:])), float(np.median(t_host[1:]))
    print(f"device: {td * 1e6:9.1f} us per block   (bursts in {c['bursts_in'].tolist()}, out {c['bursts_out'].tolist()})")
    print(f"host:   {th * 1e6:9.1f} us per block   ({sent} records sent)")
    print(f"block duration {block / Fs * 1e6:.0f} us; host / device {th / td:.2f}")


if __name__ == "__main__":
    main()
