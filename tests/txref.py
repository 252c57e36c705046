"""Float64 statement of the transmitter's modulator (include/pirip_hip.h section I) and record helpers, for
tests/test_tx*.py.

    sample r of symbol i:  x = 2 exp(j 2 pi p / Fs),  p = (A_i + (r + 1) f_i) mod Fs,  A_i = (p0 + Ts * sum_{q<i} f_q) mod Fs

with f_i = (f1 + sym_i * shift) mod Fs in exact integers; a carrier-off symbol (0xFF) gives x = 0 and moves no phase."""
import os

import numpy as np

OFF = 0xFF
RX_SYNC, RX_BITS = 2, 4
REPEAT_MAX_FRAMES = 100                    # PIRIP_TX_REPEAT_MAX_FRAMES, the original's MAX_FRAMES
# DESIGN.md 4.9, derived: the angle 2p/Fs as a fraction of pi is formed as float(p) * float(2/Fs) -- p < 2^24 exact, two roundings of
# 2^-24 relative on |t| <= 1 -> pi * 2^-23 (1 + 2^-25) in the angle; sincospif is documented to 1 ulp, at most 2^-23 for results in [-1, 1];
# the factor 2 is exact and doubles both.
BOUND = 2.0 * (np.pi * 2.0 ** -23 * (1 + 2.0 ** -25) + 2.0 ** -23)


def phase_ints(syms, f1, shift, Fs, Ts, p0=0):
    """syms: uint8 [nsym] -> (p int64 [nsym * Ts], on bool [nsym * Ts], final phase)"""
    syms = np.asarray(syms, dtype=np.int64)
    on = syms != OFF
    f = np.where(on, (f1 + syms * shift) % Fs, 0)
    A = (p0 + np.concatenate([[0], np.cumsum((f * Ts) % Fs)])) % Fs
    r = np.arange(1, Ts + 1, dtype=np.int64)
    p = (A[:-1, None] + r[None, :] * f[:, None]) % Fs
    return p.reshape(-1), np.repeat(on, Ts), int(A[-1])


def mod_f64(syms, f1, shift, Fs, Ts, p0=0):
    """complex128 [nsym * Ts]"""
    p, on, _ = phase_ints(syms, f1, shift, Fs, Ts, p0)
    return np.where(on, 2.0 * np.exp(2j * np.pi * p.astype(np.float64) / Fs), 0.0)


def quantise(x, amp):
    """the u8 quantiser clamp(rint(127 + amp x)) on float64 components [n, 2]; also returns the unrounded values"""
    v = 127.0 + amp * np.stack([x.real, x.imag], axis=-1)
    return np.clip(np.rint(v), 0, 255).astype(np.int64), v


def near_tie(v, amp, bound=BOUND):
    """where the float64 value lies within bound * amp of a rounding tie k + 1/2"""
    return np.abs(np.abs(v - np.floor(v)) - 0.5) <= bound * amp


def bits_to_syms(bits, M):
    b = np.asarray(bits, dtype=np.uint8)
    return b.copy() if M == 2 else (b[0::2] << 1 | b[1::2]).astype(np.uint8)


def burst_plan(rng, nbursts, max_frames):
    """burst-control bytes of nbursts bursts of 1..max_frames frames: 1 0 ... 0 2 per burst"""
    ctl = []
    for _ in range(nbursts):
        ctl += [1] + [0] * int(rng.integers(0, max_frames)) + [2]
    return ctl


def records(rng, ctl, kb):
    """uint8 [len(ctl), 1 + kb]: random payloads, zeros for the end-of-burst records (as frame_repeater.c:101 writes them)"""
    rec = rng.integers(0, 256, (len(ctl), 1 + kb)).astype(np.uint8)
    rec[:, 0] = ctl
    rec[np.asarray(ctl) == 2, 1:] = 0
    return rec


def carrier_mask(ctl, lead, gap, pre_syms, frame_syms):
    """bool [nsym]: True where the carrier is off, for one stream's control bytes"""
    m = [np.ones(lead, dtype=bool)]
    for c in ctl:
        if c == 1:
            m.append(np.zeros(pre_syms + frame_syms, dtype=bool))
        elif c == 0:
            m.append(np.zeros(frame_syms, dtype=bool))
        elif c == 2:
            m.append(np.ones(gap, dtype=bool))
    return np.concatenate(m)


def repeater_replay(status, data, source):
    """tx/frame_repeater.c:68-107 on one stream's records -> the Tx records it writes (uint8 [n, 1 + kb]); pinned to the program's own
    output by tests/test_tx_repeater_cpu.py over tests/golden/repeater_cases.npz"""
    out, buf, receiving = [], [], False
    for st, d in zip(status, data):
        if not receiving:
            if st == (RX_SYNC | RX_BITS):
                buf, receiving = [d.copy()], True
        else:
            if st & RX_BITS:
                buf.append(d.copy())
            if not (st & RX_SYNC):
                for i, fr in enumerate(buf):
                    fr[0] = source
                    out.append(np.concatenate([[1 if i == 0 else 0], fr]))
                out.append(np.concatenate([[2], np.zeros(data.shape[1], dtype=np.uint8)]))
                receiving = False
    return np.array(out, dtype=np.uint8).reshape(-1, 1 + data.shape[1])


def repeater_cases():
    """tests/golden/repeater_cases.npz (oracle/make_repeater_golden.py): what the reference's frame_repeater read and wrote, per case
    -> list of dicts kb, source, name, status uint8 [n], payload uint8 [n, kb], out uint8 [nout, 1 + kb]"""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "repeater_cases.npz"))
    cases, i0, o0 = [], 0, 0
    for c in range(z["kb"].size):
        kb, i1, o1 = int(z["kb"][c]), int(z["stdin_end"][c]), int(z["stdout_end"][c])
        rec = z["stdin"][i0:i1].reshape(-1, 1 + kb)
        cases.append(dict(kb=kb, source=int(z["source"][c]), name=z["name"][c].decode(), status=rec[:, 0].copy(), payload=rec[:, 1:].copy(),
                          out=z["stdout"][o0:o1].reshape(-1, 1 + kb)))
        i0, o0 = i1, o1
    return cases


# ---------------------------------------------------------------- the noise as a function of its key (synth_kernels.hip's generator)

def _splitmix(z):
    """SplitMix64's finaliser on uint64 arrays, exact (numpy wraps modulo 2^64)"""
    z = z + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def noise_uniforms(seed, stream, nabs):
    """(u1 in (0, 1], u2 in [0, 1)) of key (seed, stream, absolute sample), float64 holding the kernel's float values exactly:
    24 bits each, (bits 40..63 + 1) / 2^24 and bits 8..31 / 2^24"""
    with np.errstate(over="ignore"):
        n = np.asarray(nabs, dtype=np.int64).astype(np.uint64)
        r = _splitmix(np.uint64(seed) ^ _splitmix((np.uint64(stream) << np.uint64(40)) ^ n))
    u1 = ((r >> np.uint64(40)).astype(np.float64) + 1.0) / 16777216.0
    u2 = ((r >> np.uint64(8)) & np.uint64(0xFFFFFF)).astype(np.float64) / 16777216.0
    return u1, u2


def noise_f64(seed, stream, nabs, sigma):
    """complex128 [len(nabs)]: sigma * N(0, 1) per component by Box-Muller in float64 on the kernel's uniforms"""
    u1, u2 = noise_uniforms(seed, stream, nabs)
    return sigma * np.sqrt(-2.0 * np.log(u1)) * np.exp(2j * np.pi * u2)


# DESIGN.md 4.9, derived. u1 and u2 are exact in float (24-bit integers scaled by 2^-24). Relative to the sample's own magnitude
# mag = sigma sqrt(-2 ln u1), with e = 2^-24 (one rounding) and 1 ulp <= 2e relative:
#   logf to 1 ulp, halved by the square root: e;  sqrtf to 1 ulp: 2e;  sigma * sqrt: e                       -> the magnitude: 4e
#   the angle float(2 pi) * u2 < 2 pi: the constant is 2.79e-8 relative above 2 pi, the product rounds by e   -> 2 pi (2.79e-8 + e)
#   sincosf to 1 ulp, at most 2e on [-1, 1]; mag * cos, mag * sin: e (the sum with a carrier-off zero is exact) -> 3e
_E = 2.0 ** -24
NOISE_REL_BOUND = (4 * _E + 2 * np.pi * ((6.2831854820251465 - 2 * np.pi) / (2 * np.pi) + _E) + 3 * _E) * (1 + 2.0 ** -20)
NOISE_MAX_MAG = float(np.sqrt(2.0 * np.log(2.0 ** 24)))       # u1 >= 2^-24: no sample is larger than sigma * 5.768
