#!/usr/bin/env python3
"""Channelizer (include/pirip_hip.h section H) rate, on the device.

For each shape: W wideband u8 IQ captures of `seconds` at Fs (random bytes), K channels per capture,
  (a) pirip_hip_chan_batch alone over the whole captures (device events, best of --reps),
  (b) the streaming chain: HipRx(chan=...) with the demodulator behind it, block after block (a quarter second per call; the block copy
      into the receiver's input included), on the first --stream-seconds of the same captures.
Printed per shape (one JSON line): wideband input samples/s, the HBM fraction of the algorithmic traffic (2 B in + 8 K / D B out per input
sample against 8 TB/s) and, with --counters FILE (a counter-only `rocprofv3 --pmc` run of `--pmc-run`, csv output), the executed VALU
lane-instructions per (channel, output) against the 2 Lp floor (SQ_INSTS_VALU x 64 / (W K nout)) and the LDS bank-conflict share.
Shapes: main (W = 64 x 2.4 MS/s x 10 s, K = 8, D = 30, tbw 0.05 -> Lp = 80; 80 kS/s 2-FSK Rs = 10 k behind it) and second (README.md:109's
1.8 MS/s / 45, K = 8, s16 out; 40 kS/s 2-FSK Rs = 1000 behind it).
usage: tools/chan_rate.py [--shape main|second|all] [--reps R] [--seconds S] [--stream-seconds S] [--pmc-run] [--counters CSV ...]"""
import argparse
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12
# name: (Fs, D, W, K, out_s16, modem Fs, Rs, P, est_min, est_max)
SHAPES = {
    "main": (2400000, 30, 64, 8, False, 80000, 10000, 8, 5000, 40000),
    "second": (1800000, 45, 64, 8, True, 40000, 1000, 8, 500, 20000),
}


def offsets(Fs, D, K):
    """K channels spread over the band, none on a multiple of the output rate"""
    step = Fs // (K + 1)
    return [-Fs // 2 + step * (k + 1) + 1237 * k + 1 for k in range(K)]


def setup(name, seconds):
    import torch
    import pirip_amd
    Fs, D, W, K, s16, _, _, _, _, _ = SHAPES[name]
    n_in = int(Fs * seconds) // D * D
    ch = pirip_amd.HipChan(Fs, D, offsets(Fs, D, K) * W, inputs=[w for w in range(W) for _ in range(K)], out_s16=s16)
    g = torch.Generator(device="cuda").manual_seed(1)
    cap = torch.randint(0, 256, (W, 2 * n_in), dtype=torch.uint8, device="cuda", generator=g)
    no = ch.nout(n_in)
    out = torch.empty((W * K, no * ch.bytes_per_sample), dtype=torch.uint8, device="cuda")
    return ch, cap, n_in, no, out


def time_batch(ch, cap, n_in, out, reps):
    import torch
    ch.batch(cap.data_ptr(), cap.stride(0), n_in, out.data_ptr(), out.stride(0))
    torch.cuda.synchronize()
    best = None
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ch.batch(cap.data_ptr(), cap.stride(0), n_in, out.data_ptr(), out.stride(0))
        e1.record()
        torch.cuda.synchronize()
        t = e0.elapsed_time(e1) / 1e3
        best = t if best is None else min(best, t)
    return best


def time_stream(name, ch, cap, n_stream):
    import torch
    import pirip_amd
    Fs, D, W, K, s16, mFs, Rs, P, lo, hi = SHAPES[name]
    dem = pirip_amd.HipDemod(mFs, Rs, 2, P=P, est_min=lo, est_max=hi, in_format=pirip_amd.IN_CS16 if s16 else pirip_amd.IN_CF32,
                             nstreams=W * K)
    block = (Fs // 4) // D * D
    rx = pirip_amd.HipRx(dem, chan=ch, block=block)
    R = rx.max_frames
    bits = torch.empty((W * K, R, dem.Nbits), dtype=torch.uint8, device="cuda")
    nfr = torch.zeros(W * K, dtype=torch.int32, device="cuda")
    nblk = n_stream // block
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(nblk):
        rx.push(cap.data_ptr() + 2 * k * block, cap.stride(0), bits.data_ptr(), R * dem.Nbits, d_nframes=nfr.data_ptr())
    e1.record()
    torch.cuda.synchronize()
    tot, _ = rx.counters()
    rx.close()
    dem.close()
    return e0.elapsed_time(e1) / 1e3, nblk, block, int(tot.sum())


def read_counters(paths):
    """{counter: summed value over the channelizer's dispatches, 'dispatches': n} from rocprofv3 counter_collection.csv files"""
    vals, disp = {}, set()
    for p in paths:
        for f in ([p] if p.endswith(".csv") else glob.glob(os.path.join(p, "**", "*counter_collection.csv"), recursive=True)):
            for r in csv.DictReader(open(f)):
                if "chan_kernel" not in r.get("Kernel_Name", ""):
                    continue
                vals[r["Counter_Name"]] = vals.get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
                disp.add((f, r.get("Dispatch_Id")))
    return vals, disp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--stream-seconds", type=float, default=2.0)
    ap.add_argument("--pmc-run", action="store_true", help="one channelizer call per shape (for a counter-only rocprofv3 --pmc run)")
    ap.add_argument("--counters", nargs="*", default=None, help="rocprofv3 csv output dirs/files of --pmc-run, per shape: SHAPE=PATH[,PATH]")
    a = ap.parse_args()
    names = list(SHAPES) if a.shape == "all" else [a.shape]
    if a.counters is not None:
        for spec in a.counters:
            name, paths = spec.split("=", 1)
            Fs, D, W, K, s16, *_ = SHAPES[name]
            n_in = int(Fs * a.seconds) // D * D
            no = (n_in - 80) // D + 1
            vals, disp = read_counters(paths.split(","))
            nd = max(1, len({d for d in disp}) // max(1, len(paths.split(","))))
            r = {"shape": name, "dispatches_per_pass": nd}
            if "SQ_INSTS_VALU" in vals:
                r["valu_lane_instr_per_channel_output"] = round(vals["SQ_INSTS_VALU"] / nd * 64 / (W * K * no), 1)
                r["floor_2Lp"] = 160
                r["over_floor"] = round(r["valu_lane_instr_per_channel_output"] / 160, 3)
            if "SQ_LDS_BANK_CONFLICT" in vals and vals.get("SQ_LDS_IDX_ACTIVE"):
                r["lds_bank_conflict_share"] = round(vals["SQ_LDS_BANK_CONFLICT"] / vals["SQ_LDS_IDX_ACTIVE"], 4)
            if "FETCH_SIZE" in vals:   # KiB; x 2: gfx950's half count (MI355X_MICROARCH.md HBM recipe)
                r["fetch_bytes_per_input_sample"] = round(vals["FETCH_SIZE"] / nd * 1024 * 2 / (W * n_in), 3)
            if "WRITE_SIZE" in vals:
                r["write_bytes_per_input_sample"] = round(vals["WRITE_SIZE"] / nd * 1024 / (W * n_in), 3)
            r["algorithmic_bytes_per_input_sample"] = round(2 + (4 if s16 else 8) * K / D, 3)
            print(json.dumps(r))
        return
    import torch
    for name in names:
        Fs, D, W, K, s16, *_ = SHAPES[name]
        ch, cap, n_in, no, out = setup(name, a.seconds)
        if a.pmc_run:
            ch.batch(cap.data_ptr(), cap.stride(0), n_in, out.data_ptr(), out.stride(0))
            torch.cuda.synchronize()
            print(json.dumps({"shape": name, "pmc_run": True, "inputs": W, "n_in": n_in, "nout": no}))
            continue
        t = time_batch(ch, cap, n_in, out, a.reps)
        rate = W * n_in / t
        algo = 2 + (4 if s16 else 8) * K / D
        r = {"shape": name, "Fs": Fs, "D": D, "Lp": ch.Lp, "inputs": W, "channels_per_input": K, "out_s16": s16, "seconds": a.seconds,
             "chan_batch_ms": round(t * 1e3, 3), "input_samples_per_s": round(rate / 1e9, 2), "unit": "G wideband samples/s",
             "algorithmic_bytes_per_input_sample": round(algo, 3), "hbm_fraction": round(rate * algo / HBM_BYTES_PER_S, 4),
             "floor_valu_lane_instr_per_input_sample": round(2 * ch.Lp * K / D, 1)}
        n_stream = int(Fs * min(a.stream_seconds, a.seconds))
        try:
            ts, nblk, block, consumed = time_stream(name, ch, cap, n_stream)
        except Exception as e:          # (a receiver the demodulator's kernel cannot serve at this block: reported, not fatal)
            r["stream_error"] = str(e)
            print(json.dumps(r), flush=True)
            continue
        r.update({"stream_blocks": nblk, "stream_block": block, "stream_ms": round(ts * 1e3, 3),
                  "stream_input_samples_per_s": round(W * nblk * block / ts / 1e9, 2), "stream_consumed_modem_samples": consumed})
        print(json.dumps(r), flush=True)
        del cap, out
        ch.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
