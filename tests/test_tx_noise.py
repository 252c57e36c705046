"""The transmitter's noise as a function of its key (include/pirip_hip.h section I: "keyed by (seed, stream, samples sent since create /
reset)", pirip_hip_synth_cu8's generator). tests/txref.py restates it -- SplitMix64 in exact uint64 arithmetic, the kernel's two 24-bit
uniforms, Box-Muller in float64. On the CPU the restatement alone is tested for what a noise source owes its users (FER curves are drawn
from it): unit variance and normal kurtosis per component, no correlation between streams, between I and Q and between neighbouring
samples. On the device every noise sample is compared with the restatement at the same key."""
import numpy as np
import pytest

import txref

N = 1 << 20                                 # samples per stream in the CPU statistics; every bar below is three standard errors at this N
STREAMS = [0, 1, 63, 64, 129]


def test_noise_restatement_is_unit_normal_and_uncorrelated():
    sigma, seed = 0.6, 5
    x = {s: txref.noise_f64(seed, s, np.arange(N), sigma) for s in STREAMS}
    se_var, se_kurt, se_mean, se_rho = np.sqrt(2.0 / N), np.sqrt(24.0 / N), 1.0 / np.sqrt(N), 1.0 / np.sqrt(N)
    for s, z in x.items():
        for name, c in (("I", z.real / sigma), ("Q", z.imag / sigma)):
            var = float(np.mean(c * c))
            kurt = float(np.mean(c ** 4)) / var ** 2
            print(f"stream {s} {name}: mean {c.mean():+.2e} var {var:.5f} kurtosis {kurt:.4f} (3 se: {3 * se_mean:.1e}, {3 * se_var:.1e}, {3 * se_kurt:.1e})")
            assert abs(float(c.mean())) < 3 * se_mean, (s, name)
            assert abs(var - 1.0) < 3 * se_var, (s, name, var)
            assert abs(kurt - 3.0) < 3 * se_kurt, (s, name, kurt)
            rho1 = float(np.mean(c[1:] * c[:-1])) / var
            assert abs(rho1) < 3 * se_rho, (s, name, "lag 1", rho1)
        rho_iq = float(np.mean(z.real * z.imag)) / sigma ** 2
        assert abs(rho_iq) < 3 * se_rho, (s, "I-Q", rho_iq)
        assert abs(float(np.mean(z.real[1:] * z.imag[:-1])) / sigma ** 2) < 3 * se_rho, (s, "I-Q lag 1")
    for a, b in ((0, 1), (63, 64), (0, 129), (1, 64)):
        for ca, cb in ((x[a].real, x[b].real), (x[a].imag, x[b].imag), (x[a].real, x[b].imag)):
            rho = float(np.mean(ca * cb)) / sigma ** 2
            assert abs(rho) < 3 * se_rho, (a, b, rho)
        assert not np.array_equal(x[a][:64], x[b][:64])
    # another seed is another sequence, uncorrelated with the first
    y = txref.noise_f64(seed + 1, 0, np.arange(N), sigma)
    assert abs(float(np.mean(x[0].real * y.real)) / sigma ** 2) < 3 * se_rho
    # the key's sample index is absolute: a window is the same numbers
    assert np.array_equal(txref.noise_f64(seed, 64, np.arange(1000, 1100), sigma), x[64][1000:1100])


def test_noise_restatement_uniforms_and_largest_magnitude():
    # (a three-standard-error bar on one fixed sample fails by chance once in 370: over 48 keys -- seeds 5, 6, 77, eight streams, u1 and u2 --
    # the means' z-scores have standard deviation 1.04 and one of them, (5, 3) u1, is at -3.5; the key used here is the first of them)
    u1, u2 = txref.noise_uniforms(5, 0, np.arange(N))
    assert u1.min() >= 2.0 ** -24 and u1.max() <= 1.0 and u2.min() >= 0.0 and u2.max() < 1.0
    assert np.array_equal(u1 * 2 ** 24, np.rint(u1 * 2 ** 24)) and np.array_equal(u2 * 2 ** 24, np.rint(u2 * 2 ** 24))     # 24 bits each: exact in float
    se = np.sqrt(1.0 / 12.0 / N)
    assert abs(u1.mean() - 0.5) < 3 * se + 2.0 ** -24 and abs(u2.mean() - 0.5) < 3 * se + 2.0 ** -24
    assert abs(float(np.mean((u1 - 0.5) * (u2 - 0.5))) * 12.0) < 3 / np.sqrt(N)
    # u1 >= 2^-24: no sample is larger than sigma sqrt(2 ln 2^24), and that is the value at u1 = 2^-24
    sigma = 1.7
    z = txref.noise_f64(5, 0, np.arange(N), sigma)
    top = sigma * np.sqrt(2.0 * np.log(2.0 ** 24))
    assert abs(txref.NOISE_MAX_MAG * sigma - top) < 1e-12 and np.abs(z).max() <= top * (1 + 1e-15)
    assert abs(sigma * np.sqrt(-2.0 * np.log(2.0 ** -24)) - top) < 1e-12
    assert np.abs(z).max() > sigma * np.sqrt(2.0 * np.log(N / 8.0))                 # and the tail is populated as far as N samples reach
    # SplitMix64: the published first outputs of the generator seeded with 0 are the finaliser of 0 + gamma, 0 + 2 gamma, ...
    g = np.uint64(0x9E3779B97F4A7C15)
    with np.errstate(over="ignore"):
        assert int(txref._splitmix(np.array([0], dtype=np.uint64))[0]) == 0xE220A8397B1DCDAF
        assert int(txref._splitmix(np.array([g], dtype=np.uint64))[0]) == 0x6E789E6AA1B965F4


def _carrier_off_noise(tx, B, nsym, blocks, fmt, sigma, seed, amp=32.0, syms=None):
    import torch
    import pirip_amd
    Ts = tx.Ts
    bs = 2 if fmt == pirip_amd.IN_CU8_FSKDEMOD else 8
    d = torch.full((B, nsym), txref.OFF, dtype=torch.uint8, device="cuda") if syms is None else syms
    out = torch.zeros((B, nsym * Ts * bs), dtype=torch.uint8, device="cuda")
    at = 0
    for n in blocks:
        tx.modulate(d.data_ptr() + at, nsym, n, out.data_ptr() + at * Ts * bs, out.shape[1], out_format=fmt, amp=amp, sigma=sigma, seed=seed)
        at += n
    assert at == nsym
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    return o.reshape(B, -1, 2) if bs == 2 else o.view(np.float32).reshape(B, -1, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("sigma", [0.6, 40.0])
def test_device_noise_equals_the_restatement_at_the_same_key(built_lib, sigma):
    """cf32 output of carrier-off rows is the noise alone. Every sample of streams 0, 1, 63, 64 and the last equals noise_f64 at (seed,
    stream, absolute sample) within NOISE_REL_BOUND of its own magnitude (tests/txref.py, DESIGN.md 4.9: from the documented errors of
    logf, sqrtf and sincosf), across calls cut at sample counts that are no multiple of 8 (Ts = 9), after a reset, and running on
    without one."""
    import pirip_amd
    Fs, Rs, B, nsym, seed = 90000, 10000, 130, 700, 77
    Ts = Fs // Rs
    assert STREAMS[-1] == B - 1
    tx = pirip_amd.HipTx(pirip_amd.STANDIN_CODE, Fs, Rs, 2, nstreams=B, f1=10000, shift=10000)
    blocks = [1, 3, 7, 29, 64, 100, 496]
    assert all((n * Ts) % 8 for n in blocks[:4])
    one = _carrier_off_noise(tx, B, nsym, [nsym], pirip_amd.IN_CF32, sigma, seed)
    more = _carrier_off_noise(tx, B, nsym, blocks, pirip_amd.IN_CF32, sigma, seed)               # no reset: samples nsym Ts .. 2 nsym Ts
    tx.reset()
    parts = _carrier_off_noise(tx, B, nsym, blocks, pirip_amd.IN_CF32, sigma, seed)
    assert np.array_equal(one.view(np.uint32), parts.view(np.uint32))
    worst_rel = worst_abs = 0.0
    for s in STREAMS:
        for got, n0 in ((one[s], 0), (more[s], nsym * Ts)):
            z = txref.noise_f64(seed, s, n0 + np.arange(nsym * Ts), sigma)
            err = np.maximum(np.abs(got[:, 0] - z.real), np.abs(got[:, 1] - z.imag))
            mag = np.abs(z)
            worst_abs = max(worst_abs, float(err.max()))
            worst_rel = max(worst_rel, float(np.max(err[mag > 0] / mag[mag > 0])))
            assert (err <= txref.NOISE_REL_BOUND * mag).all(), (s, n0, int(np.argmax(err - txref.NOISE_REL_BOUND * mag)))
    print(f"sigma {sigma}: largest noise error / magnitude {worst_rel:.3e} (bound {txref.NOISE_REL_BOUND:.3e}); largest error {worst_abs:.3e} "
          f"(bound at the largest magnitude {txref.NOISE_REL_BOUND * txref.NOISE_MAX_MAG * sigma:.3e})")
    # every other stream: its own sequence too (the bound at the largest possible magnitude)
    for s in range(B):
        z = txref.noise_f64(seed, s, np.arange(nsym * Ts), sigma)
        assert np.max(np.abs(one[s, :, 0] - z.real)) <= txref.NOISE_REL_BOUND * txref.NOISE_MAX_MAG * sigma, s


@pytest.mark.gpu
def test_u8_noise_equals_pirip_hip_synth_cu8_at_equal_keys(built_lib):
    """The header calls it pirip_hip_synth_cu8's generator. Both paths on an identical signal -- tone 0, symbol 0: the float recursion
    and the exact phase both send (2, 0) -- with the same amp, sigma and seed give the same u8 at every (stream, sample); a difference
    is allowed only where the float64 value is within amp * (noise bound) of a rounding tie."""
    import torch
    import pirip_amd
    Fs, Rs, M, B, nsym, amp, sigma, seed = 90000, 10000, 2, 130, 600, 20.0, 0.6, 5
    Ts = Fs // Rs
    nsamp = nsym * Ts
    tx = pirip_amd.HipTx(pirip_amd.STANDIN_CODE, Fs, Rs, M, nstreams=B, f1=0, shift=10000)
    zeros = torch.zeros((B, nsym), dtype=torch.uint8, device="cuda")
    clean = _carrier_off_noise(tx, B, nsym, [nsym], pirip_amd.IN_CF32, 0.0, seed, syms=zeros)
    assert (clean[:, :, 0] == 2.0).all() and (clean[:, :, 1] == 0.0).all()                      # the signal is exactly (2, 0)
    tx.reset()
    new = _carrier_off_noise(tx, B, nsym, [5, 1, 94, 500], pirip_amd.IN_CU8_FSKDEMOD, sigma, seed, amp=amp, syms=zeros)
    old = torch.zeros((B, nsamp * 2), dtype=torch.uint8, device="cuda")
    pirip_amd.binding.synth_cu8(Fs, Rs, M, [0] * B, 10000, zeros.data_ptr(), nsym, nsym, old.data_ptr(), nsamp * 2, nsamp, amp=amp, sigma=sigma, seed=seed)
    torch.cuda.synchronize()
    old = old.cpu().numpy().reshape(B, nsamp, 2)
    ndiff = ntie = 0
    for s in range(B):
        z = txref.noise_f64(seed, s, np.arange(nsamp), sigma)
        q, v = txref.quantise(2.0 + z, amp)
        tie = txref.near_tie(v, amp, bound=txref.NOISE_REL_BOUND * np.abs(z)[:, None])
        # each path against the float64 quantiser: here the window also holds what both kernels round alike -- the float sum 2 + noise
        # (2^-24 relative), amp * x (2^-24 relative) and 127 + amp * x (2^-17 below 256), DESIGN.md 4.9
        e = 2.0 ** -24
        wide = (txref.NOISE_REL_BOUND * np.abs(z) + e * (2.0 + np.abs(z)))[:, None] * amp + e * amp * (2.0 + np.abs(z))[:, None] + 2.0 ** -17
        near = np.abs(np.abs(v - np.floor(v)) - 0.5) <= wide
        for got in (new[s], old[s]):
            d = np.abs(got.astype(np.int64) - q)
            assert d.max() <= 1 and not d[~near].any(), s
        d = new[s] != old[s]                                          # path against path: the stated bound and nothing more
        assert not d[~tie].any(), s
        ndiff += int(np.count_nonzero(d)); ntie += int(np.count_nonzero(tie))
    print(f"{B} streams x {nsamp} samples: {ndiff} u8 values differ between HipTx and pirip_hip_synth_cu8, {ntie} within the bound of a tie")
    assert ntie <= 1e-3 * B * nsamp * 2
