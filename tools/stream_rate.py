#!/usr/bin/env python3
"""Streaming receiver (include/pirip_hip.h section G) against one batch call over the same recording, on the device.

For each shape the recording (synthesised on the device: pirip_hip_synth_cu8) is processed
  (a) as K blocks through pirip_hip_rx_process -- each block copied into the receiver's input first (timed apart: the ingest),
  (b) as ONE pirip_hip_demod_batch / pirip_hip_fsk_ldpc_rx_batch call (after one pirip_hip_decim_batch over all of it),
timed with device events, best of --reps. One JSON line per shape. With --profile the same run is repeated in a child process under
`rocprofv3 --kernel-trace --stats` and the advance kernel's share of the streaming run's kernel time is added.

Shapes: headline (CFG1 u8 `fsk_demod -p 24`, 16384 channels), config3 (u8 at 1.8 MS/s /45 -> s16 -> Ts = 40),
deployed (u8 at 240 kS/s /6 -> complex float, 2-FSK Rs = 1000 P = 10, FSK_LDPC with the stand-in code).
usage: tools/stream_rate.py [--shape headline|config3|deployed|all] [--blocks K] [--reps R] [--profile]"""
import argparse
import ctypes as C
import glob
import json
import os
import sqlite3
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name: (Fs_tuner, D, Fs, Rs, M, P, f1, shift, est_min, est_max, in_format, channels, frames per block, ldpc)
SHAPES = {
    "headline": (240000, 1, 240000, 10000, 2, 24, 10000, 10000, 500, 25000, "u8", 16384, 100, False),
    "config3": (1800000, 45, 40000, 1000, 2, 8, 1000, 2000, 500, 20000, "s16", 512, 20, False),
    "deployed": (240000, 6, 40000, 1000, 2, 10, 1000, 2000, 500, 15000, "cf32", 4096, 20, True),
}


def _hip():
    import torch
    path = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    h = C.CDLL(path if os.path.exists(path) else "libamdhip64.so")
    h.hipMemcpy2DAsync.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p]
    return h


def run_shape(name, K, reps, one_shot=True):
    import numpy as np
    import torch
    import pirip_amd
    Fs_t, D, Fs, Rs, M, P, f1, shift, est_min, est_max, fmt, nch, fpb, ldpc = SHAPES[name]
    inf = {"u8": pirip_amd.IN_CU8_FSKDEMOD, "s16": pirip_amd.IN_CS16, "cf32": pirip_amd.IN_CF32}[fmt]
    N = (Fs // Rs) * 50
    block = D * (fpb * N + 17)                         # (not a whole number of frames: carries of every length occur)
    n_in = K * block
    hip = _hip()
    # the recording, u8 IQ at the tuner rate (the demodulator's own u8 format when there is no decimator)
    rec = torch.empty((nch, n_in * 2), dtype=torch.uint8, device="cuda")
    nsym = n_in // (Fs_t // Rs) + 2
    rng = np.random.default_rng(1)
    if ldpc:
        fr = subprocess.run([os.path.join(ROOT, "pirip_amd", "bin", "fsk_ldpc_framer"), "--code", pirip_amd.STANDIN_CODE, "-m", str(M),
                             "--testframes", "3", "--bursts", "1", "--seq", "--source", "0x4", "/dev/zero", "-"], capture_output=True, check=True).stdout
        bits = np.resize(np.frombuffer(fr, dtype=np.uint8), nsym)
    else:
        bits = rng.integers(0, 2, nsym).astype(np.uint8)
    d_bits = torch.from_numpy(bits).cuda()
    ch0 = 0
    while ch0 < nch:                                    # (the synthesiser's skip is per channel: distinct timing phases)
        n = min(1024, nch - ch0)
        pirip_amd.binding.synth_cu8(Fs_t, Rs, M, [f1] * n, shift, d_bits.data_ptr(), 0, nsym, rec[ch0].data_ptr(), n_in * 2, n_in,
                                    amp=20.0, sigma=6.0, seed=7 + ch0, skip=[(7 * s) % (Fs_t // Rs) for s in range(ch0, ch0 + n)])
        ch0 += n
    torch.cuda.synchronize()

    def handles():
        dem = pirip_amd.HipDemod(Fs, Rs, M, P=P, est_min=est_min, est_max=est_max, in_format=inf, nstreams=nch)
        ld = pirip_amd.HipLdpc(pirip_amd.STANDIN_CODE, M, nstreams=nch) if ldpc else None
        dec = pirip_amd.HipDecim(D, out_s16=(fmt == "s16")) if D > 1 else None
        return dem, ld, dec

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    # (b) one call over the whole recording
    dem, ld, dec = handles()
    bps = {"u8": 2, "s16": 4, "cf32": 8}[fmt]
    n_mod = dec.nout(n_in) if dec else n_in
    mod = torch.empty((nch, n_mod * bps), dtype=torch.uint8, device="cuda") if dec else rec
    rows = dem.max_frames_for(n_mod)
    nfr = torch.zeros(nch, dtype=torch.int32, device="cuda")
    cons = torch.zeros(nch, dtype=torch.int64, device="cuda")
    if ldpc:
        outs = [torch.empty((nch, rows), dtype=torch.uint8, device="cuda"), torch.empty((nch, rows, ld.data_bytes), dtype=torch.uint8, device="cuda"),
                torch.empty((nch, rows, 10), dtype=torch.int32, device="cuda")]
    else:
        outs = [torch.empty((nch, rows, dem.Nbits), dtype=torch.uint8, device="cuda")]
    one = []
    for _ in range(reps if one_shot else 0):
        dem.reset()
        if ld:
            ld.reset()
        torch.cuda.synchronize()
        ev[0].record()
        if dec:
            dec.batch(rec.data_ptr(), n_in * 2, n_in, mod.data_ptr(), n_mod * bps, nch)
        if ldpc:
            ld.chain_batch(dem, mod.data_ptr(), n_mod * bps, n_mod, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), nfr.data_ptr(),
                           cons.data_ptr(), rows)
        else:
            dem.demod_batch(mod.data_ptr(), n_mod * bps, n_mod, outs[0].data_ptr(), rows * dem.Nbits, 0, 0, 0, 0, nfr.data_ptr(), cons.data_ptr(), rows)
        ev[1].record()
        torch.cuda.synchronize()
        one.append(ev[0].elapsed_time(ev[1]))
    frames_one = int(nfr.sum())
    fused_one = ld.last_path_fused() if ld else None
    del outs, mod
    dem.close()
    # (a) K blocks through the streaming receiver
    dem, ld, dec = handles()
    rx = pirip_amd.HipRx(dem, ldpc=ld, dec=dec, block=block)
    R = rx.max_frames
    d_block, stride = rx.input()
    nfr_k = torch.zeros((K, nch), dtype=torch.int32, device="cuda")
    if ldpc:
        so = [torch.empty((nch, R), dtype=torch.uint8, device="cuda"), torch.empty((nch, R, ld.data_bytes), dtype=torch.uint8, device="cuda"),
              torch.empty((nch, R, 10), dtype=torch.int32, device="cuda")]
    else:
        so = [torch.empty((nch, R, dem.Nbits), dtype=torch.uint8, device="cuda")]
    in_bps = 2 if (dec or fmt == "u8") else bps
    stream = torch.cuda.current_stream().cuda_stream
    best = None
    for _ in range(reps):
        rx.reset()
        torch.cuda.synchronize()
        t_proc = t_copy = 0.0
        evs = []
        for k in range(K):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            if hip.hipMemcpy2DAsync(C.c_void_p(d_block), stride, C.c_void_p(rec.data_ptr() + k * block * 2), n_in * 2, block * in_bps, nch, 3,
                                    C.c_void_p(stream)) != 0:
                raise RuntimeError("hipMemcpy2DAsync")
            e[1].record()
            if ldpc:
                rx.process(d_status=so[0].data_ptr(), d_payload=so[1].data_ptr(), d_info=so[2].data_ptr(), d_nframes=nfr_k[k].data_ptr())
            else:
                rx.process(so[0].data_ptr(), R * dem.Nbits, d_nframes=nfr_k[k].data_ptr())
            e[2].record()
            evs.append(e)
        torch.cuda.synchronize()
        for e in evs:
            t_copy += e[0].elapsed_time(e[1])
            t_proc += e[1].elapsed_time(e[2])
        if best is None or t_proc < best[0]:
            best = (t_proc, t_copy)
    tot, backlog = rx.counters()
    frames_stream = int(nfr_k.sum())
    res = dict(shape=name, channels=nch, decimation=D, fmt=fmt, ldpc=ldpc, block=block, blocks=K, frames_per_block=round(block / D / N, 2),
               max_frames=R, one_shot_ms=round(min(one), 3) if one else None, stream_process_ms=round(best[0], 3), ingest_copy_ms=round(best[1], 3),
               stream_over_one_shot=round(best[0] / min(one), 4) if one else None, frames_one_shot=frames_one, frames_stream=frames_stream,
               consumed_equal=bool(int(tot.sum()) == int(cons.sum())), backlog_max=int(backlog.max()), nin_max=dem.info.nin_max,
               fused_one_shot=fused_one, fused_stream=ld.last_path_fused() if ld else None)
    rx.close()
    return res


def advance_share(name, K):
    """the same shape once more in a child under rocprofv3 --kernel-trace --stats: the advance kernel's share of the streaming kernels"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "rx", "--", sys.executable, os.path.abspath(__file__),
               "--shape", name, "--blocks", str(K), "--reps", "1", "--stream-only"]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=1200)
        if p.returncode != 0:
            return {"profile_error": p.returncode, "profile_tail": p.stderr[-400:]}
        dbs = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)
        tot = adv = 0.0
        calls = 0
        for db in dbs:
            c = sqlite3.connect(db)
            for kname, n, t in c.execute("select name, count(*), sum(end-start) from kernels group by name"):
                if "synth" in kname:                       # (the recording's synthesis is not part of the receiver)
                    continue
                tot += t
                if "rx_advance_kernel" in kname:
                    adv += t
                    calls += n
        if not dbs:
            return {"profile_error": "no database", "profile_tail": p.stdout[-400:]}
        return {"advance_kernel_calls": calls, "advance_kernel_ms_per_call": round(adv / max(calls, 1) / 1e6, 4),
                "advance_share_of_stream_kernel_time": round(adv / tot, 5) if tot else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all", choices=["all"] + list(SHAPES))
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--stream-only", action="store_true", help="skip the one-shot run (the profiled child)")
    a = ap.parse_args()
    for name in (SHAPES if a.shape == "all" else [a.shape]):
        r = run_shape(name, a.blocks, a.reps, one_shot=not a.stream_only)
        if a.profile:
            r.update(advance_share(name, a.blocks))
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
