#!/usr/bin/env python3
"""Rate of the batch FSK_LDPC transmitter (include/pirip_hip.h section I): records -> symbols -> u8 IQ on the device.

    python tools/tx_rate.py [--streams 256,4096,16384] [--reps 5] [--baseline-streams 4096]

Config 4's burst shape (4-FSK, Fs 240 k, Rs 10 k, preamble + 3 frames of the stand-in (512,256) code, 40 symbols of silence in
front and 100 behind), a distinct payload per stream. Per stream count: samples/s of pirip_hip_tx_records_to_iq and its share of
the HBM write rate at 2 B per sample (--hbm-gbs, default 8000). Then, at --baseline-streams, the same job the only way it could be
done before: fsk_ldpc_framer on the host per stream, upload, pirip_hip_synth_cu8 -- timed end to end and for the device call alone.
Times are medians of --reps runs after one warm-up, bracketed by device synchronisation: wall clock around a reset and four launches, so the
256-stream line is mostly launch overhead, not kernel rate. The ratio to the baseline is taken on the burst alone (no lead, no tail).

    python tools/tx_rate.py --pmc-run     # one records -> IQ call at 4096 streams and nothing else: the program of a counter-only
                                          # rocprofv3 --pmc SQ_INSTS_VALU pass (VALU per sample = tx_mod_kernel's count * 64 / samples)"""
import argparse
import os
import subprocess
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
    ap.add_argument("--streams", default="256,4096,16384")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--baseline-streams", type=int, default=4096)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0)
    ap.add_argument("--pmc-run", action="store_true")
    a = ap.parse_args()
    if a.pmc_run:
        a.streams, a.reps, a.baseline_streams = "4096", 1, -1
    Fs, Rs, M, f1, shift, amp = 240000, 10000, 4, 10000, 10000, 32.0
    Ts, nfr, lead, tail = Fs // Rs, 3, 40, 100
    ctl = [1] + [0] * (nfr - 1) + [2]
    print(f"device: {torch.cuda.get_device_name(0)}; 4-FSK Fs {Fs} Rs {Rs}, burst of {nfr} frames, lead {lead} tail {tail} symbols")
    for B in [int(v) for v in a.streams.split(",")]:
        tx = pirip_amd.HipTx(pirip_amd.STANDIN_CODE, Fs, Rs, M, nstreams=B, f1=f1, shift=shift, lead=lead, gap=tail)
        rng = np.random.default_rng(B)
        rec = rng.integers(0, 256, (B, len(ctl), tx.record_bytes)).astype(np.uint8)
        rec[:, :, 0] = ctl
        nsym = lead + tx.preamble_syms + nfr * tx.frame_syms + tail
        nsamp = nsym * Ts
        d_rec = torch.from_numpy(rec).cuda()
        out = torch.zeros((B, nsamp * 2), dtype=torch.uint8, device="cuda")

        def run():
            tx.reset()
            tx.records_to_iq(d_rec.data_ptr(), rec[0].size, len(ctl), nsym, out.data_ptr(), nsamp * 2, amp=amp)

        if a.pmc_run:
            run()
            torch.cuda.synchronize()
            print(f"pmc run: {B} streams x {nsamp} samples = {B * nsamp} samples per records -> IQ call, 1 call")
            return
        t = med(run, a.reps)
        sps = B * nsamp / t
        print(f"streams {B:6d}: records -> u8 IQ {t * 1e3:9.3f} ms, {sps / 1e9:8.2f} G samples/s, {2 * sps / 1e9:8.1f} GB/s written "
              f"= {100 * 2 * sps / 1e9 / a.hbm_gbs:5.1f} % of {a.hbm_gbs:.0f} GB/s")
        if B == a.baseline_streams:
            framer = os.path.join(ROOT, "pirip_amd", "bin", "fsk_ldpc_framer")
            burst = tx.preamble_syms + nfr * tx.frame_syms
            seg = torch.zeros((B, burst * Ts * 2), dtype=torch.uint8, device="cuda")
            state = {}

            def host_frame():
                bits = []
                for s in range(B):
                    p = subprocess.run([framer, "--code", pirip_amd.STANDIN_CODE, "-m", str(M), "--packed", "-", "-"], input=rec[s].tobytes(),
                                       capture_output=True, check=True)
                    bits.append(np.frombuffer(p.stdout, dtype=np.uint8))
                state["bits"] = np.stack(bits)

            def upload_and_synth():
                d_bits = torch.from_numpy(state["bits"]).cuda()
                pirip_amd.binding.synth_cu8(Fs, Rs, M, [f1] * B, shift, d_bits.data_ptr(), state["bits"].shape[1], burst, seg.data_ptr(),
                                            burst * Ts * 2, burst * Ts, amp=amp)

            t0 = time.perf_counter()
            host_frame()
            t_frame = time.perf_counter() - t0
            t_synth = med(upload_and_synth, a.reps)
            tb = t_frame + t_synth
            print(f"baseline at {B} streams (burst only, {burst * Ts} samples per stream): fsk_ldpc_framer x {B} {t_frame * 1e3:.1f} ms + upload + "
                  f"pirip_hip_synth_cu8 {t_synth * 1e3:.3f} ms = {tb * 1e3:.1f} ms, {B * burst * Ts / tb / 1e9:.3f} G samples/s; "
                  f"synth_cu8 alone {B * burst * Ts / t_synth / 1e9:.3f} G samples/s")
            # like for like: the same burst and nothing else (no lead, no tail) through the new path
            txb = pirip_amd.HipTx(pirip_amd.STANDIN_CODE, Fs, Rs, M, nstreams=B, f1=f1, shift=shift)
            d_burst = torch.from_numpy(np.ascontiguousarray(rec[:, :nfr])).cuda()

            def run_burst():
                txb.reset()
                txb.records_to_iq(d_burst.data_ptr(), nfr * txb.record_bytes, nfr, burst, seg.data_ptr(), burst * Ts * 2, amp=amp)

            t_new = med(run_burst, a.reps)
            print(f"new path on the burst alone: {t_new * 1e3:.3f} ms, {B * burst * Ts / t_new / 1e9:.2f} G samples/s: {t_synth / t_new:.1f} x the baseline's "
                  f"device part (upload + synth_cu8), {tb / t_new:.0f} x the whole baseline")
            assert t_new < t_synth, "the parallel-in-samples transmitter must beat one thread per stream"


if __name__ == "__main__":
    main()
