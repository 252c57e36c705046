"""Float64 regime predictor for complex-float (cf32) recordings scaled by 2^k (tests/test_dynamic_range*.py).

Multiplying a cf32 recording by 2^k is exact in float32, and every operation of the demodulator (FFT, |X|, the Sf IIR,
down-conversion, window sums, correctly rounded roots, ratios, arg-max) commutes exactly with that scaling as long as no
intermediate leaves the normal range. Regime computes, in float64 from the recording and the oracle's own outputs at k = 0, the
extremes of the intermediates the kernels branch on, and from them the "clean" interval of k and a ladder of k on either side of
every range boundary of the kernels:

  |X|^2 of the estimator FFT   the estimator's root tiers switch at 2^-96 (wave / block kernels)
  |f|^2 (tmax)                 the fused hand-over's quick path needs every value in {0} u [2^-96, 2^121]
  ssig, snse, sum - mx         the hand-over's frame sums (before the division by Nsym) and a symbol's "other tones" sum
  rx_sig_pow, rx_nse_pow       the frame powers; llr_frame_gain_quick takes its root for sig - nse in [2^-96, 2^126]

Linear intermediates (samples, windowed samples, |X|, Sf, |f|) scale by 2^k, quadratic ones (powers) by 4^k. Products of a sample
with a phasor or twiddle component close to zero are not counted: their rounding error, even when denormal, is more than 2^40 times
below half an ulp of the sums they feed.
"""
import math

import numpy as np

LO_E, HI_E = -126, 128           # float32: smallest normal 2^-126; every finite value is below 2^128

# the complex-float wave instance families (fsk_demod_wave.hip, kInst): Ts 40 / Ndft 512, Ts 20 and 18 / Ndft 256, Ts 10 and 8 / Ndft 128;
# M = 2 and 4, peak and mask estimator. f1 / shift: the transmitter's tone plan; mask: the mask estimator's tone spacing (0: peak)
SHAPES = {
    "ts40_m2": dict(Fs=40000, Rs=1000, M=2, P=10, f1=1000, shift=2000, mask=0, Ndft=512),
    "ts40_m4_mask": dict(Fs=40000, Rs=1000, M=4, P=8, f1=1000, shift=1000, mask=1000, Ndft=512),
    "ts20_m4_mask": dict(Fs=200000, Rs=10000, M=4, P=10, f1=10000, shift=10000, mask=10000, Ndft=256),
    "ts18_m2": dict(Fs=180000, Rs=10000, M=2, P=9, f1=10000, shift=10000, mask=0, Ndft=256),
    "ts10_m4": dict(Fs=100000, Rs=10000, M=4, P=10, f1=5000, shift=10000, mask=0, Ndft=128),
    "ts8_m2_mask": dict(Fs=80000, Rs=10000, M=2, P=8, f1=10000, shift=10000, mask=10000, Ndft=128),
}


def est_limits(sh):
    return sh["Rs"] // 2, min(sh["Fs"] // 2 - sh["Rs"], 90000)


def recording(oracle, sh, seed, frames=(10, 8), ebno_db=7.0):
    """Noisy random-bit bursts (AWGN at ebno_db on the bursts only) between gaps of digital silence (exact zeros), unit scale
    (fsk_mod_c: |x| = 2 on the tones). float32 [n, 2]."""
    import sigutil
    rng = np.random.default_rng(seed)
    Ts = sh["Fs"] // sh["Rs"]
    bps = 1 if sh["M"] == 2 else 2
    c = dict(sh, est_min=0, est_max=0)
    segs = [np.zeros((int(rng.integers(3, 9)) * 13 * Ts, 2), np.float32)]
    for nf in frames:
        bits = rng.integers(0, 2, nf * 50 * bps).astype(np.uint8)
        segs.append(sigutil.add_awgn(sigutil.mod_complex(oracle, c, bits), ebno_db, c, rng))
        segs.append(np.zeros((int(rng.integers(60, 140)) * Ts, 2), np.float32))
    return np.ascontiguousarray(np.concatenate(segs).astype(np.float32))


def scaled(x, k):
    """x * 2^k, exact in float32 inside the clean interval (np.ldexp: no rounding of the factor)."""
    return np.ascontiguousarray(np.ldexp(x, k).astype(np.float32))


def sums_overflow_k(oracle, x, sh, reg, x2_finite=True):
    """The first candidate k (Regime.k_sums_overflow) at which the oracle's frame signal power overflows in some frame while every soft
    magnitude and timing estimate stays finite: the hand-over's sums overflow, nothing before them does (x2_finite=False: the
    estimator's |X|^2 may overflow as well -- what the soft-bit hand-over sees is the same). None if no candidate does."""
    for k in reg.k_sums_overflow(x2_finite):
        r = demod(oracle, sh, scaled(x, k))
        if r["nframes"] == reg.nframes and np.isfinite(r["rx_filt"]).all() and np.isfinite(r["stats"][:, 4]).all() \
                and np.isinf(r["stats"][:, 8]).any():
            return k
    return None


def oracle_fsk(oracle, sh):
    lo, hi = est_limits(sh)
    return oracle.OracleFsk(sh["Fs"], sh["Rs"], sh["M"], P=sh["P"], est_min=lo, est_max=hi,
                            tone_spacing=sh["mask"] if sh["mask"] else 100, mask=bool(sh["mask"]))


def demod(oracle, sh, x):
    """A fresh oracle stream over the whole recording."""
    return oracle_fsk(oracle, sh).demod(x, oracle.IN_CF32)


def _log2(v):
    return math.log2(v) if v > 0 and math.isfinite(v) else None


def estimator_power(x, ndft):
    """|X|^2 of Hann-windowed Ndft-point FFTs at a quarter-block stride over the whole recording (float64): (min nonzero, max)."""
    z = x[:, 0].astype(np.float64) + 1j * x[:, 1].astype(np.float64)
    hann = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(ndft) / ndft)
    step = ndft // 4
    nb = (len(z) - ndft) // step + 1
    mn, mx = math.inf, 0.0
    for b0 in range(0, nb, 256):
        idx = np.arange(ndft)[None, :] + step * np.arange(b0, min(nb, b0 + 256))[:, None]
        p = np.abs(np.fft.fft(z[idx] * hann, axis=1)) ** 2
        nz = p[p > 0]
        if nz.size:
            mn = min(mn, float(nz.min()))
        mx = max(mx, float(p.max()))
    return mn, mx


class Regime:
    """Extremes (float64, at k = 0) of one recording on one shape, and what follows from them for x * 2^k.

    x: float32 [n, 2] recording; sh: a SHAPES entry; ro: the oracle's demod() result for x."""

    def __init__(self, x, sh, ro, nsym=50):
        M, P, Ts, ndft = sh["M"], sh["P"], sh["Fs"] // sh["Rs"], sh["Ndft"]
        self.nsym = nsym
        a = np.abs(x.astype(np.float64))
        nz = a[a > 0]
        hann_min = 0.5 - 0.5 * math.cos(2.0 * math.pi / ndft)              # the smallest nonzero window weight
        self.lin_min = float(nz.min()) * hann_min if nz.size else math.inf   # the smallest nonzero windowed sample
        self.X2_min, self.X2_max = estimator_power(x, ndft)
        # the fine-timing phasor sum: (Nsym+1)*P terms sum_m |f_int|^2 with |f_int| <= Ts * max|x| (a bound)
        amax = float(np.sqrt((x.astype(np.float64) ** 2).sum(axis=1)).max())
        self.tc_max = (nsym + 1) * P * M * (Ts * amax) ** 2
        f = ro["rx_filt"].astype(np.float64).reshape(-1, M, nsym)
        t = f * f                                                            # |f|^2 per frame, tone, symbol (tmax of the kernels)
        self.nframes = t.shape[0]
        tz = t[t > 0]
        self.tmax_min = float(tz.min()) if tz.size else math.inf
        self.tmax_max = float(t.max()) if t.size else 0.0
        mx = t.max(axis=1)                                                   # [frame][sym]
        oth = t.sum(axis=1) - mx                                             # sum - mx per symbol
        oz = oth[oth > 0]
        self.oth_min = float(oz.min()) if oz.size else math.inf
        self.ssig = mx.sum(axis=1)                                           # the hand-over's frame sums before / Nsym
        self.snse = (oth / (M - 1)).sum(axis=1)
        self.ssig_max = float(self.ssig.max()) if self.nframes else 0.0
        self.sum2_max = float(t.sum(axis=1).max()) if t.size else 0.0
        # each frame's first nonzero noise term: the oracle's rx_nse_pow is 1e-12 + the terms in order, so the constant vanishes there or never
        first = np.zeros(self.nframes)
        for i in range(self.nframes):
            nzi = np.flatnonzero(oth[i] > 0)
            first[i] = oth[i, nzi[0]] / (M - 1) if nzi.size else 0.0
        self.first_nse = first
        self.snse_min = float(self.snse[self.snse > 0].min()) if (self.snse > 0).any() else math.inf

    def quad_max(self):
        return max(self.X2_max, self.tc_max, self.ssig_max, self.sum2_max)

    def quad_min(self):
        return min(self.X2_min, self.tmax_min, self.oth_min)

    def clean(self):
        """(k_lo, k_hi): every k in it keeps every counted intermediate below 2^127 (a binade of headroom under overflow) and every
        nonzero one at or above 2^-125 (a binade above the smallest normal)."""
        hi = math.floor((HI_E - 1 - _log2(self.quad_max())) / 2)
        lo = max(math.ceil(LO_E + 1 - _log2(self.lin_min)), math.ceil((LO_E + 1 - _log2(self.quad_min())) / 2))
        return lo, hi

    def is_clean(self, k):
        lo, hi = self.clean()
        return lo <= k <= hi

    def eps_clean(self, k):
        """The oracle's rx_nse_pow starts at 1e-12 and the LLR stage adds 1e-12 to snse / Nsym: rx_nse_pow, SNRest and the soft bits
        scale exactly only where that constant is below half an ulp (2^-24, with a binade of headroom: 2^-25) of what it meets, in
        every frame with any noise term (a frame without one keeps the bare constant, the same at every k)."""
        s = 4.0 ** k
        live = self.first_nse > 0
        if live.any() and float(self.first_nse[live].min()) * s * 2.0 ** -25 <= 1e-12:
            return False
        if (self.snse > 0).any() and self.snse_min / self.nsym * s * 2.0 ** -25 <= 1e-12:
            return False
        return self.is_clean(k)

    @staticmethod
    def k_quad_at(v, e):
        """The smallest k with v * 4^k >= 2^e (v: a quadratic intermediate at k = 0): k - 1 puts it below 2^e."""
        return math.ceil((e - _log2(v)) / 2)

    def k_sums_overflow(self, x2_finite=True):
        """Candidates for a k where the hand-over's sum of the frame's largest |f|^2 overflows (passes 2^128) while every |f|^2 and a
        symbol's tone sum stay below 2^127 (and, with x2_finite, every |X|^2 finite). The fine-timing sum is a cancelling phasor sum whose
        size this bound-based predictor does not know: which candidate keeps it finite is for the oracle at that k to say (sums_overflow_k)."""
        k = self.k_quad_at(self.ssig_max, 128)
        return [j for j in (k, k + 1) if max(self.tmax_max, self.sum2_max) * 4.0 ** j < 2.0 ** 127
                and (not x2_finite or self.X2_max * 4.0 ** j < 2.0 ** 128)]

    def k_oth_denormal(self):
        """A k where the smallest nonzero sum - mx of a symbol is denormal (below 2^-127)."""
        return self.k_quad_at(self.oth_min, -127) - 1

    def ladder(self):
        """{name: k}: k = 0 and 15 (s16 samples converted to float without normalising), both ends of the clean interval, one k on each
        side of the range boundaries (the smallest |X|^2 and |f|^2 at 2^-96, the smallest nonzero power at 2^-126, the largest
        intermediate -- a bound, see clean() -- at 2^127), and an overflow k for |X|^2 and |f|^2; the hand-over's sums-only overflow k
        needs the oracle (sums_overflow_k)."""
        lo, hi = self.clean()
        L = {"k0": 0, "k15": 15, "clean_lo": lo, "clean_hi": hi}
        kx = self.k_quad_at(self.X2_min, -96)
        L["X2min_below_2^-96"], L["X2min_above_2^-96"] = kx - 1, kx
        kt = self.k_quad_at(self.tmax_min, -96)
        L["tmin_below_2^-96"], L["tmin_above_2^-96"] = kt - 1, kt
        kd = self.k_quad_at(self.quad_min(), -126)
        L["min_below_2^-126"], L["min_above_2^-126"] = kd - 1, kd
        # (no rungs at llr_frame_gain_quick's upper bound 2^126: the frame power is a finite sum / Nsym = 50, at most FLT_MAX / 50 < 2^123,
        #  so that bound is unreachable from below; past it the sum itself has overflowed -- the sums_overflow rung)
        kh = self.k_quad_at(self.quad_max(), 127)
        L["max_below_2^127"], L["max_above_2^127"] = kh - 1, kh
        L["X2_overflow"] = self.k_quad_at(max(self.X2_max, self.tmax_max), 128) + 1
        return L
