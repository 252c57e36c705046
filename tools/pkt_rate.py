#!/usr/bin/env python3
"""Time per call of the packet link's reassembly and of its send (include/pirip_hip.h section R), plain handles against handles with
parity fragments.

    python tools/pkt_rate.py [--channels 256] [--rows 4096] [--reps 20]

push_records on a receive-only handle of --channels channels over --rows rows per channel of full-length packets on the stand-in code
(kb 32, cap 24), three cases:
  plain:     HipPacket, max_frags 84: bursts of 84 frames back to back;
  fec:       HipPacketFec, max_frags 84, R 16, 100 %: bursts of 84 + 16 frames, nothing lost (the parity is surplus);
  fec-loss:  the same handle, 16 fragments of every burst lost, data and parity mixed: every packet is rebuilt.
send of two full-length packets per channel, plain against FEC, on --channels transmit channels (four per output).
The cases alternate within a repetition; every time is a host clock around calls that end in a device synchronise, the first repetition
is a warm-up and is dropped, and median, minimum and maximum are printed. The rows come from the tests' host model; the counters are
compared with the model's on one channel, so that a case that decoded nothing is not reported as a time."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

OFFSETS = [-90000, -30000, 30001, 90000]
MF, R, PCT = 84, 16, 100


def main():
    import torch
    import pirip_amd
    import pktfecref as fr
    import pktref
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    K, rows = a.channels, a.rows
    if K % 4 or K < 4:
        ap.error("--channels: a multiple of 4")
    rng = np.random.default_rng(3)
    kb, sh, B = pktref.KB, (MF, R, PCT), pktref.SYNC | pktref.BITS
    mp = pktref.max_packet(kb, MF)
    npk = rows // MF + 1
    packets = [rng.integers(0, 256, mp).astype(np.uint8).tobytes() for _ in range(npk)]

    def table(events):
        st, pl = fr.rows_of(events)
        assert len(st) >= rows
        return st[:rows], pl[:rows]

    bursts = [fr.segment_fec(p, 2, 7, i, kb, *sh)[:-1] for i, p in enumerate(packets)]
    tables = {
        "plain": table([("frames", pktref.segment(p, 2, 7, i, kb, MF)[:-1], B) for i, p in enumerate(packets)]),
        "fec": table([("frames", b, B) for b in bursts]),
        "fec-loss": table([("lose", b, rng.choice(MF + R, R, replace=False).tolist()) for b in bursts]),
    }
    print(f"device: {torch.cuda.get_device_name(0)}; {K} channels, {rows} rows per call, {a.reps} repetitions")
    dem = pirip_amd.HipDemod(40000, 1000, 2, P=10, est_min=500, est_max=20000, nstreams=K)
    ld = pirip_amd.HipLdpc(pirip_amd.STANDIN_CODE, 2, nstreams=K)
    rx = pirip_amd.HipRx(dem, ldpc=ld, block=8000)                             # tells the handles their shape; never run
    plain = pirip_amd.HipPacket(rx=rx, max_frags=MF, ring_entries=64)
    fec = pirip_amd.HipPacketFec(rx=rx, max_frags=MF, ring_entries=64, max_parity=R, parity_pct=PCT)
    handles = {"plain": plain, "fec": fec, "fec-loss": fec}
    dev = {}
    for name, (st, pl) in tables.items():
        dev[name] = (torch.from_numpy(np.tile(st, (K, 1))).cuda(), torch.from_numpy(np.tile(pl, (K, 1, 1))).cuda())
    times = {name: [] for name in tables}
    for rep in range(a.reps + 1):
        for name in tables:
            h = handles[name]
            h.reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h.push_records(*dev[name])
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
            if rep == 0:                                                      # the device did what the model does
                if name == "plain":
                    m = pktref.run_rows([[tables[name]]], filt=None, address=None, max_frags=MF, ring_entries=64)
                    want = m.counters()
                else:
                    m = fr.run_rows([[tables[name]]], sh, ring_entries=64, filt=None, address=None)
                    want = dict(m.counters(), **m.fec_counters())
                got = h.counters()
                if name != "plain":
                    got.update(h.fec_counters())
                for k, v in want.items():
                    assert (got[k] == v[0]).all(), (name, k, got[k][:4], v)
                print(f"{name}: per channel delivered {int(got['delivered'][0])}" +
                      (f", recovered {int(got['recovered'][0])}, repaired {int(got['repaired'][0])}" if name != "plain" else ""))
    for name, t in times.items():
        t = np.array(t[1:]) * 1e6
        print(f"push_records {name:9s} median {np.median(t):9.1f} us   min {t.min():9.1f}   max {t.max():9.1f}   "
              f"({np.median(t) * 1e3 / (K * rows):.2f} ns per row)")

    # send: two full-length packets per channel
    tx = pirip_amd.HipTx(pirip_amd.STANDIN_CODE, 40000, 1000, 2, nstreams=K, f1=1000, shift=2000, gap=64)
    mux = pirip_amd.HipMux(240000, 6, OFFSETS * (K // 4), outputs=[c // 4 for c in range(K)], gains=[0.1] * K)
    block = 100 * 6 * tx.Ts
    txs = pirip_amd.HipTxStream(tx, mux, block, tx.preamble_syms + (MF + R) * tx.frame_syms + 64)
    senders = {"plain": pirip_amd.HipPacket(tx=tx, txs=txs, nrx=1, max_frags=MF),
               "fec": pirip_amd.HipPacketFec(tx=tx, txs=txs, nrx=1, max_frags=MF, max_parity=R, parity_pct=PCT)}
    by = torch.from_numpy(rng.integers(0, 256, (K, 2, mp)).astype(np.uint8)).cuda()
    ln = torch.full((K, 2), mp, dtype=torch.int32, device="cuda")
    ds = torch.full((K, 2), 7, dtype=torch.uint8, device="cuda")
    tk = torch.zeros(K, dtype=torch.int32, device="cuda")
    times = {name: [] for name in senders}
    for rep in range(a.reps + 1):
        for name, h in senders.items():
            h.reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h.send(by, ds, lengths=ln, taken=tk)
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
            assert tk.cpu().tolist() == [2] * K
    for name, t in times.items():
        t = np.array(t[1:]) * 1e6
        print(f"send         {name:9s} median {np.median(t):9.1f} us   min {t.min():9.1f}   max {t.max():9.1f}   ({2 * K} packets of {mp} bytes)")


if __name__ == "__main__":
    main()
