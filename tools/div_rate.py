#!/usr/bin/env python3
"""Time of the diversity stage (include/pirip_hip.h section Q) behind the config-4 receive stage.

    python tools/div_rate.py [--receivers 8192] [--ebno-db 3.5] [--reps 5]

8192 receivers of the config-4 chain (4-FSK, 240 kS/s, 10 kBd, the stand-in (512,256) code, 600 000 samples each: one burst of 93 test
frames, every receiver with its own timing phase, the noise shared) as 4096 groups of 2 branches and as 2048 groups of 4. Per shape:
the receive call (pirip_hip_fsk_ldpc_rx_batch) and pirip_hip_div_collect behind it, each timed with events on the stream, medians of
--reps runs after two warm-up runs; every run starts from reset handles, so that collect sees the same candidates each time. The
branches of a group here differ by one sample of delay and share their noise: the figures time the stage, they say nothing about
what combining gains."""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    import torch
    import pirip_amd
    import bench_configs
    ap = argparse.ArgumentParser()
    ap.add_argument("--receivers", type=int, default=8192)
    ap.add_argument("--ebno-db", type=float, default=3.5)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    R, nsamp, Ts = a.receivers, 600_000, 24
    L = pirip_amd.lib()
    st = torch.cuda.current_stream()
    framer = os.path.join(ROOT, "pirip_amd", "bin", "fsk_ldpc_framer")
    fb = subprocess.run([framer, "--code", pirip_amd.STANDIN_CODE, "--testframes", "93", "--seq", "--source", "0x1", "/dev/zero", "-"],
                        capture_output=True, check=True).stdout
    x, _ = bench_configs.modulate(L, 240000, 10000, 4, 10000, 10000, 0, 3, bits=np.frombuffer(fb, dtype=np.uint8))
    rng = np.random.default_rng(5)
    sigma = np.sqrt((4.0 * Ts / 2.0) / (10 ** (a.ebno_db / 10.0)) / 2.0)
    xn = x[:nsamp + Ts] + rng.normal(0.0, sigma, (nsamp + Ts, 2)).astype(np.float32)
    d = torch.from_numpy(np.clip(np.rint(127.0 + 14.0 * xn.astype(np.float64)), 0, 255).astype(np.uint8)).cuda()
    dev = torch.empty((R, nsamp, 2), dtype=torch.uint8, device="cuda")
    for c in range(Ts):
        dev[c::Ts] = d[c:c + nsamp].unsqueeze(0)
    dem = pirip_amd.HipDemod(240000, 10000, 4, P=8, est_min=500, est_max=60000, nstreams=R)
    maxf = dem.max_frames_for(nsamp)
    ld = pirip_amd.HipLdpc(pirip_amd.STANDIN_CODE, 4, nstreams=R)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    stt, pay, inf = z((R, maxf), torch.uint8), z((R, maxf, 32), torch.uint8), z((R, maxf, pirip_amd.LDPC_INFO_PER_CALL), torch.int32)
    stats, nfr, cons = z((R, maxf, pirip_amd.STATS_PER_FRAME), torch.float32), z((R,), torch.int32), z((R,), torch.int64)
    print(f"device: {torch.cuda.get_device_name(0)}; {R} receivers x {nsamp} samples, {maxf} rows per call, Eb/N0 {a.ebno_db} dB")

    def chain():
        ld.chain_batch(dem, dev.data_ptr(), nsamp * 2, nsamp, stt.data_ptr(), pay.data_ptr(), inf.data_ptr(), nfr.data_ptr(), cons.data_ptr(), maxf,
                       stats.data_ptr(), maxf * pirip_amd.STATS_PER_FRAME, stream=st.cuda_stream)

    for B in (2, 4):
        dv = pirip_amd.HipDiversity(ld, B, Ts, dem.N, 2 * Ts, maxf, log_entries=256)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        t_rx, t_div = [], []
        for i in range(a.reps + 2):
            dem.reset(st.cuda_stream); ld.reset(st.cuda_stream); dv.reset(stream=st.cuda_stream)
            ev[0].record(st); chain(); ev[1].record(st)
            dv.collect(stt, inf, stats, nframes=nfr, stream=st.cuda_stream)
            ev[2].record(st); torch.cuda.synchronize()
            if i >= 2:
                t_rx.append(ev[0].elapsed_time(ev[1])); t_div.append(ev[1].elapsed_time(ev[2]))
        c = dv.counters()
        cand = int((inf[..., 6] >= 0).sum())
        print(f"{R // B} groups x {B} branches: receive {np.median(t_rx):8.3f} ms, collect {np.median(t_div):8.3f} ms "
              f"({100 * np.median(t_div) / np.median(t_rx):.1f} % of it); candidates {cand}, clusters {int(c['clusters'].sum())}, with BITS "
              f"{int(c['bits'].sum())}, rescued {int(c['rescued'].sum())}, members {int(c['members'].sum())}, dropped {int(c['dropped'].sum())}; "
              f"pending rows per group {dv.pending}")
        dv.close()


if __name__ == "__main__":
    main()
