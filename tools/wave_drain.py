#!/usr/bin/env python3
"""tools/wave_drain.py -- per-wave timeline of one launch of the headline wave demodulator: how the launch drains.

Needs a library built with -DPIRIP_WAVE_TIMING (kept apart from the product build):
    make -C pirip_amd/csrc -j8 LIBDIR=../lib_timing EXTRA=-DPIRIP_WAVE_TIMING ../lib_timing/libpirip_hip.so
    PIRIP_HIP_LIB=pirip_amd/lib_timing/libpirip_hip.so python tools/wave_drain.py [--tail 0|1] [streams ...]
    python tools/wave_drain.py --load DIR/wave_drain_*.npy      (rows saved with --dump DIR, analysed again without a device)
In such a build every wave leaves s_memtime before its first frame and after its last, its frame count and where it ran (HW_ID, XCC_ID)
in a buffer named through pirip_hip_wave_timeline(). For each batch size (default 3072, 4096, 16384 streams x 1.2 M samples) this prints
  - resident waves per SIMD against time over the last 15 ms of the launch,
  - the spread of finish times among the waves that shared a SIMD at its end (the last `waves per SIMD` to finish there),
  - the idle wave-slot time between the first wave's end and the kernel's end, as a share of the launch's slot time.
--tail: pirip_hip_set_launch_tail_first (0: nothing raised, the launch as it was before the setter existed; default 1, the library's).
The per-phase marks of the same build cost about 10 % of a wave's time: read the shapes, not the milliseconds."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np

FS, RS, M, P, NSAMP = 240000, 10000, 2, 24, 1_200_000
WPS = 3                                     # waves per SIMD of the headline instance
TAIL_MS = 15.0


def simd_key(where):
    """(XCC, shader engine, shader array, CU, SIMD) of a wave: HW_ID bits 15:13, 12, 11:8, 5:4 under XCC_ID"""
    return ((where >> np.uint64(32)) << np.uint64(16)) | (where & np.uint64(0xFF30))


def run(B, mode, base):
    import torch
    import pirip_amd
    L = pirip_amd.lib()
    dev = torch.from_numpy(base).cuda().unsqueeze(0).expand(B, NSAMP, 2).contiguous()
    h = pirip_amd.HipDemod(FS, RS, M, P=P, est_min=500, est_max=25000, in_format=pirip_amd.IN_CU8_FSKDEMOD, nstreams=B)
    h.set_launch_tail_first(mode)
    h.set_bit_packing(True)
    maxf = h.max_frames_for(NSAMP)
    nb = (h.Nbits + 7) // 8
    bits = torch.zeros((B, maxf, nb), dtype=torch.uint8, device="cuda")
    nfr = torch.zeros(B, dtype=torch.int32, device="cuda")
    cons = torch.zeros(B, dtype=torch.int64, device="cuda")
    rows = torch.zeros((B, 4), dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def launch():
        h.demod_batch(dev.data_ptr(), NSAMP * 2, NSAMP, bits.data_ptr(), maxf * nb, 0, 0, 0, 0, nfr.data_ptr(), cons.data_ptr(), maxf, st)

    launch()                                                   # warm-up (and the streams' first frames)
    torch.cuda.synchronize()
    assert L.pirip_hip_wave_timeline(C.c_void_p(rows.data_ptr()), B) == 0
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); launch(); e1.record()
    torch.cuda.synchronize()
    assert L.pirip_hip_wave_timeline(None, 0) == 0
    ms = e0.elapsed_time(e1)
    t = rows.cpu().numpy().astype(np.uint64)
    R = h.launch_resident_blocks()
    h.close()
    del dev, bits
    return ms, t, R


def report(B, mode, ms, t, R):
    first, last, frames, where = t[:, 0].astype(np.int64).astype(np.float64), t[:, 1].astype(np.int64).astype(np.float64), t[:, 2], t[:, 3]
    # every CU counts s_memtime (shader clocks) from an origin of its own: each one's clock is read against its first wave's start (a launch
    # of at least one workgroup per CU reaches every CU at once), and the longest of their spans is the launch as the HIP events time it
    cu = simd_key(where) & ~np.uint64(0x30)
    span = 0.0
    for x in np.unique(cu):
        m = cu == x
        org = first[m].min()
        first[m] -= org; last[m] -= org
        span = max(span, last[m].max())
    tick_ms = ms / span
    a, b = first * tick_ms, last * tick_ms
    t_end, t0 = span, 0.0
    key = simd_key(where)
    simds = np.unique(key)
    nS = len(simds)
    print(f"## {B} streams x {NSAMP} samples, launch tail first {mode}: {ms:.3f} ms by HIP events; {int(frames.min())} .. {int(frames.max())} frames per wave; "
          f"{nS} SIMDs on {len(np.unique(key & ~np.uint64(0x30)))} CUs seen; {R} workgroups = {4 * R} streams resident at once; "
          f"{(t_end - t0) / ms / 1e3:.1f} s_memtime ticks per us")
    print(f"wave life: min {np.min(b - a):.3f}  median {np.median(b - a):.3f}  max {np.max(b - a):.3f} ms")
    # resident waves per SIMD against time
    print(f"resident waves per SIMD over the last {TAIL_MS:.0f} ms (time before the kernel's end: mean; share of SIMDs with 0 / 1 / 2 / 3 waves)")
    idx = np.searchsorted(simds, key)
    for back in np.arange(TAIL_MS, -0.01, -0.5):
        now = ms - back
        if now < 0:
            continue
        live = (a <= now) & (b > now)
        per = np.bincount(idx[live], minlength=nS)
        share = [float((per == k).mean()) for k in range(WPS + 1)]
        print(f"  -{back:5.1f} ms  {per.mean():5.2f}   " + "  ".join(f"{100 * s:5.1f} %" for s in share))
    # finish-time spread among the waves that shared a SIMD at its end
    spread = np.zeros(nS)
    order = np.lexsort((b, idx))
    bs, ids = b[order], idx[order]
    ends = np.searchsorted(ids, np.arange(nS), side="right")
    starts = np.searchsorted(ids, np.arange(nS), side="left")
    for s in range(nS):
        lastk = bs[max(starts[s], ends[s] - WPS):ends[s]]
        spread[s] = lastk[-1] - lastk[0] if len(lastk) > 1 else 0.0
    print(f"finish-time spread of the last {WPS} waves of a SIMD: median {np.median(spread):.3f} ms ({100 * np.median(spread) / ms:.1f} % of the launch), "
          f"90th percentile {np.percentile(spread, 90):.3f} ms ({100 * np.percentile(spread, 90) / ms:.1f} %), max {spread.max():.3f} ms ({100 * spread.max() / ms:.1f} %)")
    # idle wave-slot time between the first wave's end and the kernel's end
    t_fe = b.min()
    overlap = np.clip(np.minimum(b, ms) - np.maximum(a, t_fe), 0, None).sum()
    slots = nS * WPS
    idle = slots * (ms - t_fe) - overlap
    simd_end = np.zeros(nS); np.maximum.at(simd_end, idx, b)
    print(f"first wave ends at {t_fe:.3f} ms; idle wave-slot time from there to the end: {idle / slots:.3f} ms per slot = {100 * idle / (slots * ms):.2f} % of the launch's "
          f"slot time; SIMDs with no wave at all: {(ms - simd_end).mean():.3f} ms each on average = {100 * (ms - simd_end).mean() / ms:.2f} %")
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tail", dest="mode", type=int, default=1)
    ap.add_argument("--dump", metavar="DIR", default=None, help="also save each launch's raw rows as DIR/wave_drain_<streams>_tail<0|1>.npy")
    ap.add_argument("--load", metavar="FILE", nargs="+", default=None, help="analyse rows saved by --dump again (no device)")
    ap.add_argument("streams", nargs="*", type=int, default=[3072, 4096, 16384])
    args = ap.parse_args()
    if args.load:
        for f in args.load:
            d = np.load(f)
            B, mode = (int(v.replace("tail", "")) for v in os.path.basename(f)[:-4].split("_")[2:4])
            report(B, mode, float(d[-2]) / 1e6, d[:-2].reshape(-1, 4), int(d[-1]))
        return
    import pirip_amd
    import bench_configs
    L = pirip_amd.lib()
    if not hasattr(L, "pirip_hip_wave_timeline"):
        raise SystemExit("wave_drain.py: PIRIP_HIP_LIB does not point at a -DPIRIP_WAVE_TIMING build (no pirip_hip_wave_timeline)")
    L.pirip_hip_wave_timeline.argtypes = [C.c_void_p, C.c_int]
    x, _ = bench_configs.modulate(L, FS, RS, M, 10000, 10000, NSAMP // (FS // RS) + 50, 7)
    base = np.clip(np.rint(127.0 + 32.0 * x[:NSAMP].astype(np.float64)), 0, 255).astype(np.uint8)
    print(f"# tools/wave_drain.py --tail {args.mode}: timing build, kernel code object {pirip_amd.kernel_source_hash()}")
    for B in args.streams:
        ms, t, R = run(B, args.mode, base)
        if args.dump:
            np.save(os.path.join(args.dump, f"wave_drain_{B}_tail{args.mode}.npy"), np.concatenate([t.reshape(-1), np.array([int(ms * 1e6), R], dtype=np.uint64)]))
        report(B, args.mode, ms, t, R)


if __name__ == "__main__":
    main()
