#!/usr/bin/env python3
"""Time per call of the medium-access layer on the packet link's call (include/pirip_hip.h section T).

    python tools/mac_rate.py [--channels 256] [--rows 64] [--reps 20]

HipPacket.push_records with and without a HipMac attached, on the same rows: --channels channels, --rows rows per channel and call of
full-length packets (max_frags 8, eight fragments each) on the stand-in code (kb 32, cap 24), both handles with a transmitter of the same
shape (100 symbols per call, four channels per output). The layer adds two launches to the packet handle's: the sense step of one wave per
receive channel, which also writes the copy of the status rows that the reassembly reads, and the gate step of one thread per transmit
channel. The two handles alternate within a repetition; every time is a host clock around one call that ends in a device synchronise, the
first repetition is a warm-up and is dropped, and median, minimum and maximum are printed. The delivered and the carrier counts are
compared with what the rows hold, so that a call that did nothing is not reported as a time."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

OFFSETS = [-90000, -30000, 30001, 90000]
MF = 8


def main():
    import torch
    import pirip_amd
    import pktref
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    K, rows = a.channels, a.rows
    if K % 4 or K < 4:
        ap.error("--channels: a multiple of 4")
    npk = rows // MF
    if npk < 1 or npk > 64:
        ap.error("--rows: %d .. %d" % (MF, MF * 64))
    rng = np.random.default_rng(5)
    kb = pktref.KB
    mp = pktref.max_packet(kb, MF)
    ev = [("pkt", rng.integers(0, 256, mp).astype(np.uint8).tobytes(), 2, 1, s, MF) for s in range(npk)]
    st, pl = pktref.rows_of(ev)
    assert len(st) == npk * MF
    d_st, d_pl = torch.from_numpy(np.tile(st, (K, 1))).cuda(), torch.from_numpy(np.tile(pl, (K, 1, 1))).cuda()
    print(f"device: {torch.cuda.get_device_name(0)}; {K} channels, {len(st)} rows per call ({npk} packets of {mp} bytes), {a.reps} repetitions")

    def terminal():
        tx = pirip_amd.HipTx(pirip_amd.STANDIN_CODE, 40000, 1000, 2, nstreams=K, f1=1000, shift=2000, gap=64)
        mux = pirip_amd.HipMux(240000, 6, OFFSETS * (K // 4), outputs=[c // 4 for c in range(K)], gains=[0.1] * K)
        block = 100 * 6 * tx.Ts
        txs = pirip_amd.HipTxStream(tx, mux, block, tx.preamble_syms + MF * tx.frame_syms + 64)
        pkt = pirip_amd.HipPacket(tx=tx, txs=txs, nrx=K, source=1, filter=1, address=1, max_frags=MF, ring_entries=64)
        out = torch.zeros((K // 4, block * 2), dtype=torch.uint8, device="cuda")
        return (tx, mux, txs), pkt, out

    keep_p, plain, out_p = terminal()
    keep_m, under, out_m = terminal()
    mac = pirip_amd.HipMac(under, sense_mask=1, slot_calls=3, cw=8, ifs_calls=1, mute_calls=4, txop_bursts=1, key=7)
    handles = {"HipPacket": (plain, out_p), "with HipMac": (under, out_m)}
    times = {name: [] for name in handles}
    for rep in range(a.reps + 1):
        for name, (h, out) in handles.items():
            h.reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h.push_records(d_st, d_pl, out=out, out_stride=out.stride(0))
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
            if rep == 0:
                got = h.counters()["delivered"]
                assert (got == npk).all(), (name, got[:4])
        if rep == 0:
            assert (mac.counters()["carrier"] == 1).all()
    med = {}
    for name, t in times.items():
        t = np.array(t[1:]) * 1e6
        med[name] = float(np.median(t))
        print(f"push_records {name:11s} median {np.median(t):9.1f} us   min {t.min():9.1f}   max {t.max():9.1f}")
    print(f"the layer adds {med['with HipMac'] - med['HipPacket']:.1f} us to a call of {med['HipPacket']:.1f} us (medians)")


if __name__ == "__main__":
    main()
