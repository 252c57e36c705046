"""include/pirip_hip.h section H (channelizer) without a GPU: the library exports it, the header declares it so that a plain-C caller
compiles and links (tests/cprog/chan_like_multichannel.c), the binding exposes it, and the float64 statement the GPU tests hold the kernel
to (tests/chanref.py) has the sign convention of csdr shift_addition_cc (-f_c/Fs): a tone at f_c + a Hz comes out at +a Hz."""
import inspect
import os
import subprocess

import numpy as np
import pytest

import chanref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHAN_SYMBOLS = ("pirip_hip_chan_create", "pirip_hip_chan_destroy", "pirip_hip_chan_get_info", "pirip_hip_chan_taps", "pirip_hip_chan_nout",
                "pirip_hip_chan_batch", "pirip_hip_rx_create_chan")


def test_library_exports_the_channelizer(built_lib):
    import pirip_amd
    out = subprocess.run(["nm", "-D", "--defined-only", pirip_amd.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for n in CHAN_SYMBOLS:
        assert n in exported, n
        assert hasattr(built_lib, n), n


def test_header_declares_section_h():
    hdr = open(os.path.join(ROOT, "include", "pirip_hip.h")).read()
    assert "section H" in hdr
    for n in CHAN_SYMBOLS:
        assert n + "(" in hdr, n


def test_header_compiles_as_plain_c_and_links(built_lib, tmp_path):
    import pirip_amd
    libdir = os.path.dirname(pirip_amd.lib_path())
    exe = str(tmp_path / "chan_like_multichannel")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cprog", "chan_like_multichannel.c"), "-L", libdir, "-lpirip_hip",
                           "-Wl,-rpath," + libdir, "-lm"])
    assert os.path.exists(exe)


def test_binding_exposes_hipchan_and_rx_chan():
    import pirip_amd
    sig = inspect.signature(pirip_amd.HipChan)
    assert list(sig.parameters)[:3] == ["Fs", "D", "offsets"]
    for k, v in (("inputs", None), ("transition_bw", 0.05), ("out_s16", False), ("device", -1)):
        assert sig.parameters[k].default == v, k
    for m in ("nout", "taps", "batch", "close"):
        assert callable(getattr(pirip_amd.HipChan, m)), m
    assert sig.parameters  # (constructed only on a GPU)
    assert inspect.signature(pirip_amd.HipChan.batch).parameters["t0"].default == 0
    rx = inspect.signature(pirip_amd.HipRx)
    assert rx.parameters["chan"].default is None and rx.parameters["dec"].default is None


def test_cli_is_built(built_lib):
    assert os.access(os.path.join(ROOT, "pirip_amd", "bin", "rtl_fsk_channels"), os.X_OK)


def _taps(D, tbw=0.05):
    """csdr's Hamming low-pass, cutoff 0.5/D (what HipDecim(D).taps() holds), restated in numpy for the CPU check"""
    L = int(4.0 / tbw)
    L += 1 - L % 2
    mid = L // 2
    cut = 0.5 / D
    w = lambda r: 0.54 - 0.46 * np.cos(2 * np.pi * (0.5 + r / 2))
    h = np.zeros(L)
    h[mid] = 2 * np.pi * cut * w(0.0)
    for i in range(1, mid + 1):
        h[mid - i] = h[mid + i] = np.sin(2 * np.pi * cut * i) / i * w(i / mid)
    return (h / h.sum()).astype(np.float32)


@pytest.mark.parametrize("fc,a", [(300000, 12000), (-700003, -20000), (0, 15000), (1159999, -30000)])
def test_reference_sign_convention(fc, a):
    """a tone at f_c + a Hz in the capture is a tone at +a Hz in channel c (not -a, not at f_c - a)"""
    Fs, D = 2400000, 30
    h = _taps(D)
    n = 30 * 4000 + 80
    t = np.arange(n)
    z = 40.0 * np.exp(2j * np.pi * (fc + a) * t / Fs)
    u8 = chanref.quantise_u8(z)
    y = chanref.channel(u8, h, D, Fs, fc, t0=0)
    spec = np.abs(np.fft.fft(y * np.hanning(len(y))))
    f = np.fft.fftfreq(len(y), d=D / Fs)
    peak = f[np.argmax(spec)]
    assert abs(peak - a) < 2 * Fs / D / len(y), (peak, a)
    # and t0 only turns the phase: the same tone, the same magnitude
    y7 = chanref.channel(u8[7:], h, D, Fs, fc, t0=7)
    assert np.allclose(np.abs(y7[:100]), np.abs(chanref.channel(u8[7:], h, D, Fs, fc, t0=0)[:100]))
