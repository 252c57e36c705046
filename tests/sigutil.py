"""Synthetic IQ generation shared by the tests (uses the CPU oracle's modulator).

Configurations follow BASELINE.json / SURVEY.md 8d:
  cfg1/2: 2-FSK Fs=240k Rs=10k P=24, tones 10/20 kHz, u8 IQ, `fsk_demod -d -p 24`
  cfg3  : u8 IQ at 1.8 MS/s -> /45 -> 2-FSK Rs=1k at 40 kS/s, `fsk_demod -c 2 40000 1000`
  cfg4  : 4-FSK Fs=240k Rs=10k, tones 10/20/30/40 kHz
"""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STANDIN_CODE = os.path.join(ROOT, "pirip_amd", "data", "standin_256_512_4.code")

CFG1 = dict(Fs=240000, Rs=10000, M=2, P=24, f1=10000, shift=10000, est_min=500, est_max=25000)
CFG3 = dict(Fs=40000, Rs=1000, M=2, P=8, f1=1000, shift=2000, est_min=500, est_max=20000)
CFG4 = dict(Fs=240000, Rs=10000, M=4, P=8, f1=10000, shift=10000, est_min=500, est_max=60000)


def mod_complex(ob, cfg, bits, f1=None):
    tx = ob.OracleFsk(cfg["Fs"], cfg["Rs"], cfg["M"], P=cfg["P"], f1_tx=f1 if f1 is not None else cfg["f1"],
                      tone_spacing=cfg["shift"])
    return tx.mod_c(bits)     # float32 [n,2], peak 2.0


def add_awgn(x, ebno_db, cfg, rng):
    """complex AWGN for a given Eb/N0 (signal power = |x|^2 mean, Eb = Ps*Ts/log2(M))."""
    ps = float(np.mean(x[:, 0].astype(np.float64) ** 2 + x[:, 1].astype(np.float64) ** 2))
    ts = cfg["Fs"] // cfg["Rs"]
    eb = ps * ts / np.log2(cfg["M"])
    n0 = eb / (10 ** (ebno_db / 10.0))
    sigma = np.sqrt(n0 / 2.0)
    return (x + rng.normal(0.0, sigma, x.shape)).astype(np.float32)


def make_u8_stream(ob, cfg, nbits, seed=0, offset=0, tone_bins=0, ebno_db=None, random_bits=False, amp=32.0,
                   noise_amp_scale=1.0):
    """u8 IQ [n,2] for one stream. offset: leading samples dropped (timing phase);
    tone_bins: tone plan shifted by k*Fs/Ndft-ish (k*937.5 Hz at cfg1)."""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2, nbits).astype(np.uint8) if random_bits else ob.get_test_bits(nbits)
    f1 = cfg["f1"] + int(round(tone_bins * 937.5))
    x = mod_complex(ob, cfg, bits, f1=f1)
    if ebno_db is not None:
        x = add_awgn(x, ebno_db, cfg, rng)
        amp = amp * noise_amp_scale
    u8 = ob.quantise_cu8(x, amp=amp)
    return np.ascontiguousarray(u8[offset:]), bits


# ---- the signal rows of the wave-kernel tests (50-symbol frames; tone steps in bins of the 256-point estimator FFT) ----
def frame_bits(c, nsym=50):
    return nsym * (1 if c["M"] == 2 else 2)


def mod_frames(ob, c, nframes, seed, tone_bins=0):
    """nframes frames of random bits drawn from `seed`, the tone plan tone_bins FFT bins (Fs / 256) up"""
    bits = np.random.default_rng(seed).integers(0, 2, nframes * frame_bits(c)).astype(np.uint8)
    return mod_complex(ob, c, bits, f1=c["f1"] + int(round(tone_bins * (c["Fs"] / 256.0))))


def resample_steps(x, step):
    """x read at positions 0, step[0], step[0] + step[1], ... up to two samples short of its end (linear interpolation)"""
    from demodrun import resample_at
    t = np.concatenate([[0.0], np.cumsum(step)[:-1]])
    return resample_at(x, t[t < x.shape[0] - 2])


def mover(ob, c, seed, frames):
    """frames[i] frames from seed + i, every odd segment one FFT bin up (two segments: up; three: and back); the first 3 samples dropped"""
    return np.concatenate([mod_frames(ob, c, n, seed + i, tone_bins=i % 2) for i, n in enumerate(frames)])[3:]


def convert(ob, c, x):
    """to the shape's input format c["fmt"]: cf32 (3) scaled by 0.37, else u8"""
    if c.get("fmt", 0) == 3:
        return np.ascontiguousarray(x.astype(np.float32) * np.float32(0.37))
    return ob.quantise_cu8(x)


def batch(ob, c, rows):
    """the rows converted, cut to the shortest and stacked"""
    rows = [convert(ob, c, r) for r in rows]
    n = min(r.shape[0] for r in rows)
    return np.stack([r[:n] for r in rows])


def mixed_batch(ob, c, nframes, mover_frames, clock_step):
    """[steady, mover, steady on other bins, a sample clock of clock_step(n) samples per sample, steady at another timing phase]"""
    x = mod_frames(ob, c, nframes + 2, 20)
    return batch(ob, c, [mod_frames(ob, c, nframes + 1, 1), mover(ob, c, 10, mover_frames), mod_frames(ob, c, nframes + 1, 2, tone_bins=-1)[7:],
                         resample_steps(x, clock_step(x.shape[0])), mod_frames(ob, c, nframes + 1, 3, tone_bins=2)[17:]])


def rel_err(a, b):
    """max |a-b| relative to the peak of b, per call (the stated rx_filt tolerance metric)."""
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    peak = max(float(np.max(np.abs(b))), 1e-30)
    return float(np.max(np.abs(a - b))) / peak


def code_variant(src, outdir, llr_map):
    """A copy of code file `src` with the `llr_map` key set (pirip_amd/csrc/fsk_ldpc.hpp: upstream | rician), for tests that run both
    soft-decision mappings of the FSK_LDPC receiver. Returns the new path."""
    lines = [ln for ln in open(src).read().split("\n") if not ln.startswith("llr_map")]
    i = next(k for k, ln in enumerate(lines) if ln.startswith("rows"))
    lines.insert(i, "llr_map " + llr_map)
    out = os.path.join(str(outdir), os.path.basename(src).replace(".code", "_" + llr_map + ".code"))
    with open(out, "w") as f:
        f.write("\n".join(lines))
    return out


def run_framer(args, stdin=b"", code=STANDIN_CODE):
    """`fsk_ldpc_framer --code code args` on stdin: its stdout as bytes; a non-zero exit status fails"""
    import subprocess
    p = subprocess.run([os.path.join(ROOT, "pirip_amd", "bin", "fsk_ldpc_framer"), "--code", code] + list(args), input=stdin, capture_output=True)
    assert p.returncode == 0, p.stderr
    return np.frombuffer(p.stdout, dtype=np.uint8)


def hip_runtime():
    """the HIP runtime this process has loaded (device-to-device copies out of a handle's rows)"""
    import ctypes as C
    with open("/proc/self/maps") as f:
        path = next(line.split()[-1] for line in f if "libamdhip64" in line)
    rt = C.CDLL(path)
    rt.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    return rt


def d2d(rt, dst, src, n):
    assert rt.hipMemcpyAsync(dst, src, n, 3, None) == 0
