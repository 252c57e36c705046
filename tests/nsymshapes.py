"""Frame lengths (Nsym, the symbols per demodulator call) other than the 50 every instance is compiled for: the shapes, what the general
kernel does at each of them, and the signal they are tested on. Pure Python, no GPU: tests/test_frame_lengths_cpu.py proves the rows on
the oracle and on the restatement below, tests/test_frame_lengths.py runs them on the device.

Every wave and block instance compares Nsym == 50, so each row lands on fsk_demod_general.hip, where the frame length selects the path:
the workgroup's thread count, whether the next frame is read ahead into registers, whether u8 input is staged in LDS at all, whether the
down-converted samples share the FFT work array, and how many estimator FFTs fit a frame (none: Sf stays zero, every tone estimate is
-Fs/2, both sides decide bit 0 everywhere -- the degenerate regime)."""
import math
from collections import namedtuple

import numpy as np

# fmt: "u8d" (fsk_demod -d), "csdr" (u8 as csdr converts it), "s16", "f32"
# threads / pre (register read-ahead) / alias (fdc shares X) / ffts (estimator FFTs per frame at nin = N) / direct (u8 read from global
# memory): what the row claims; test_frame_lengths_cpu.py holds the claim to path() below. lds_fits False: create must refuse the shape.
Row = namedtuple("Row", "name Fs Rs M P fmt Nsym threads pre alias ffts direct lds_fits note")

ROWS = [
    Row("ts24_n8", 240000, 10000, 2, 24, "u8d", 8, 64, True, True, 0, False, True, "no FFT fits, aliasing, 64 threads at Ts = 24"),
    Row("ts24_n10", 240000, 10000, 2, 24, "u8d", 10, 64, True, False, 0, False, True, "no FFT fits, not aliased"),
    Row("ts24_n11", 240000, 10000, 2, 24, "u8d", 11, 64, True, False, 1, False, True, "first frame length with an FFT; Nbits = 11"),
    Row("ts24_p8_s16_n20", 240000, 10000, 2, 8, "s16", 20, 64, True, True, 2, False, True, "aliasing (groups of 3) with a live estimator"),
    Row("ts24_4fsk_f32_n21", 240000, 10000, 4, 8, "f32", 21, 64, False, True, 2, False, True, "Nbits = 42"),
    Row("ts24_n49", 240000, 10000, 2, 24, "u8d", 49, 128, True, False, 8, False, True, "neighbour of the compiled length"),
    Row("ts24_n51", 240000, 10000, 2, 24, "u8d", 51, 128, True, False, 8, False, True, "neighbour of the compiled length"),
    Row("ts24_4fsk_csdr_n100", 240000, 10000, 4, 6, "csdr", 100, 128, False, False, 17, False, True, "read-ahead off on a u8 frame"),
    Row("ts24_n127", 240000, 10000, 2, 24, "u8d", 127, 512, True, False, 22, False, True, "wide kernel with read-ahead"),
    Row("ts24_s16_n128", 240000, 10000, 2, 24, "s16", 128, 512, True, False, 23, False, True, "nin 3066 / 3072 / 3078 straddle 24 half-FFTs"),
    Row("ts24_p8_n340", 240000, 10000, 2, 8, "u8d", 340, 512, False, False, 62, False, True, "last staged u8 frame"),
    Row("ts24_p8_n342", 240000, 10000, 2, 8, "u8d", 342, 256, False, False, 63, True, True, "first direct-input frame"),
    Row("ts40_4fsk_f32_n30", 40000, 1000, 4, 10, "f32", 30, 128, False, False, 3, False, True, ""),
    Row("ts40_s16_n100", 40000, 1000, 2, 8, "s16", 100, 128, False, False, 14, False, True, ""),
    Row("ts240_n10", 240000, 1000, 2, 15, "u8d", 10, 128, False, True, 0, False, True, "Ndft = 4096, no FFT fits, groups of 4"),
    Row("ts240_4fsk_n33", 240000, 1000, 4, 15, "u8d", 33, 512, False, True, 2, False, True, "wide kernel + aliasing + grouped memory"),
    Row("ts80_f32_n25", 8000, 100, 2, 8, "f32", 25, 128, False, True, 2, False, True, "groups of 10"),
    Row("ts24_4fsk_f32_n400", 240000, 10000, 4, 8, "f32", 400, None, None, None, None, None, False, "LDS over 160 KiB: create must refuse"),
]
BY_NAME = {r.name: r for r in ROWS}
DEVICE_ROWS = [r for r in ROWS if r.lds_fits]                 # every row a device comparison runs
DEGENERATE = [r.name for r in ROWS if r.ffts == 0]            # no estimator FFT fits a frame

# Bit sequences are seeded by the row's position, except where that sequence breaks a condition the INPUT must meet before any device
# comparison (test_frame_lengths_cpu.py, on the oracle alone): eleven-symbol frames of the default sequence hold a frame with so few
# transitions that the oracle's timing sum has condition 0.0047 < 0.005.
SEEDS = {"ts24_n11": 2008}

BYTES_PER_SAMPLE ={"u8d": 2, "csdr": 2, "s16": 4, "f32": 8}
LDS_LIMIT = 160 * 1024
K_PRE = 12                                                    # read-ahead registers per thread (kPre)
RED_BYTES = 2 * 16 * 4                                        # reduction scratch in front of the carved LDS (kRedBytes)
EYE_TRACES, EYE_POINTS = 8, 160


def dims(r):
    """FskPlan::init (pirip_amd/csrc/fsk_plan.cpp) at the recalled defaults: the sizes the kernel's path rules read."""
    Ts = r.Fs // r.Rs
    N = Ts * r.Nsym
    nin_step = Ts // 4
    hist_len = 2 * Ts + nin_step
    Ndft = 1 << math.ceil(math.log2(r.Fs / (0.1 * r.Rs)))
    return dict(Ts=Ts, N=N, Nmem=N + 2 * Ts, Ndft=Ndft, Nbits=r.Nsym * (1 if r.M == 2 else 2), nint=(r.Nsym + 1) * r.P, nin_step=nin_step,
                hist_len=hist_len, grp=math.gcd(math.gcd(Ts // r.P, nin_step), hist_len))


def _align16(x):
    return (x + 15) & ~15


def direct_input(r, d):
    """direct_input() of fsk_demod_general.hip: u8 frames over 16 KiB are read from global memory, not staged."""
    return r.fmt in ("u8d", "csdr") and (d["N"] + d["nin_step"]) * 2 > 16384


def carve(r, d):
    """carve() of fsk_demod_general.hip -> (bytes of LDS carved, fdc aliases X)."""
    nin_max = d["N"] + d["nin_step"]
    off = _align16(16 if direct_input(r, d) else BYTES_PER_SAMPLE[r.fmt] * nin_max)
    xbytes = max(8 * d["Ndft"], d["Nbits"])
    off += _align16(xbytes)
    off += _align16(4 * d["Ndft"])
    fdc_bytes = 8 * (d["Nmem"] // d["grp"])
    alias = fdc_bytes <= xbytes
    if not alias:
        off += _align16(fdc_bytes)
    off += _align16(8 * r.M * (d["hist_len"] // d["grp"]))
    off += _align16(8 * r.M * d["nint"])
    return off, alias


def path(r):
    """launch_demod_general() and the kernel body's can_pre of fsk_demod_general.hip, with carve() and direct_input() above: what a row
    runs as. lds_fits False is pirip_hip_create's refusal (demod_general_lds_bytes over 160 KiB)."""
    d = dims(r)
    carved, alias = carve(r, d)
    lds = RED_BYTES + carved
    if lds > LDS_LIMIT:
        return dict(lds=lds, lds_fits=False)
    direct = direct_input(r, d)
    nin_max = d["N"] + d["nin_step"]
    nt = 128
    if nin_max < 512:
        nt = 64
    elif lds > 80 * 1024:
        nt = 512
    elif direct:
        nt = 256
    pre = (not direct) and r.fmt != "f32" and nin_max <= K_PRE * nt
    return dict(lds=lds, lds_fits=True, threads=nt, pre=pre, alias=alias, direct=direct, ffts=numffts(d, d["N"]))


def numffts(d, nin):
    """estimator FFTs in a frame of nin samples (half-overlapped Ndft-point windows)"""
    return max(nin // (d["Ndft"] // 2) - 1, 0)


def eye_shape(r):
    """(rows, points per row) of the eye diagram: 8 / M traces per tone, fewer where the frame's (Nsym + 1) P window sums do not hold
    them (the kernel's `traces` loop, pirip_hip_get_eye)."""
    d = dims(r)
    dec = (2 * r.P + EYE_POINTS - 1) // EYE_POINTS
    npts = (2 * r.P) // dec
    traces = EYE_TRACES // r.M
    while traces > 0 and 2 * r.P * traces + (r.P // 2 + 1) + (npts - 1) * dec >= d["nint"]:
        traces -= 1
    return traces * r.M, npts


def config(r):
    """the modem both sides are created with (tests/test_gpu_parity.py::test_general_kernel_configuration_sweep's tone plan)"""
    return dict(Fs=r.Fs, Rs=r.Rs, M=r.M, P=r.P, f1=r.Rs, shift=r.Rs, est_min=r.Rs // 2, est_max=min(r.Fs // 2, r.Rs * (r.M + 2)))


def nframes(r):
    """30 .. 120 frames of the row's length inside about 120 k samples; the few rows whose 30 frames would be twice that (N > 4000)
    keep the sample budget and run 14 or 15 frames."""
    N = dims(r)["N"]
    n = min(120, 120000 // N)
    return n if n >= 30 or N > 4000 else 30


def signal(ob, sigutil, r, ebno_db=None, seed=None):
    """-> (buffer in the row's format, transmitted bits). Random bits through the oracle's modulator in its own 50-symbol configuration
    (only the receiver's Nsym changes), Ts // 3 leading samples dropped, optional AWGN, then the row's sample format."""
    c = config(r)
    Ts = r.Fs // r.Rs
    rng = np.random.default_rng(SEEDS.get(r.name, ROWS.index(r) + 1000) if seed is None else seed)
    nsym = (nframes(r) + 2) * r.Nsym
    bits = rng.integers(0, 2, nsym * (1 if r.M == 2 else 2)).astype(np.uint8)
    x = sigutil.mod_complex(ob, c, bits)[Ts // 3:]
    if ebno_db is not None:
        x = sigutil.add_awgn(x, ebno_db, c, rng)
    if r.fmt in ("u8d", "csdr"):
        buf = ob.quantise_cu8(x, amp=20.0)
    elif r.fmt == "s16":
        buf = np.clip(np.rint(x * 6000.0), -32768, 32767).astype(np.int16)
    else:
        buf = np.ascontiguousarray(x, dtype=np.float32)
    return np.ascontiguousarray(buf), bits


def formats(ob, A, r):
    """(oracle format code, device format code) of a row"""
    name = {"u8d": "IN_CU8_FSKDEMOD", "csdr": "IN_CU8_CSDR", "s16": "IN_CS16", "f32": "IN_CF32"}[r.fmt]
    return getattr(ob, name), (getattr(A, name) if A is not None else None)


def oracle_for(ob, r):
    c = config(r)
    return ob.OracleFsk(r.Fs, r.Rs, r.M, P=r.P, Nsym=r.Nsym, est_min=c["est_min"], est_max=c["est_max"])
