"""include/pirip_hip.h section H (channelizer) without a GPU: the library exports it, the header declares it so that a plain-C caller
compiles and links (tests/cprog/chan_like_multichannel.c), the binding exposes it, and the float64 statement the GPU tests hold the kernel
to (tests/chanref.py) has the sign convention of csdr shift_addition_cc (-f_c/Fs): a tone at f_c + a Hz comes out at +a Hz."""
import inspect
import os
import subprocess

import numpy as np
import pytest

import chanref
import test_channelizer_shapes as shapes

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
    L = chanref.filter_len(tbw)
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


# ---- the shape tables of tests/test_channelizer_shapes.py reach the paths they are there for -------------------------------------------
def _geometry(D, Lp):
    g = chanref.tile_geometry(D, Lp)
    assert g is not None, (D, Lp)
    return g


def test_geometry_helpers_restate_the_host_rule():
    """the values chan_kernels.hip's constants give at shapes worked out by hand"""
    assert chanref.filter_len(0.05) == 79 and chanref.filter_len(0.0125) == 319 and chanref.filter_len(0.5) == 9 and chanref.filter_len(1.0) == 5
    assert chanref.tile_geometry(1, 80) == (1, 256, 256, (256 + 80) * 8)
    assert chanref.tile_geometry(30, 80) == (31, 128, 128, (128 + 3) * 31 * 8)
    assert chanref.tile_geometry(45, 80) == (45, 64, 64, (64 + 2) * 45 * 8)
    assert chanref.tile_geometry(125, 80) == (125, 64, 64, 65000)
    assert chanref.tile_geometry(127, 80) == (127, 64, 63, 65024)
    assert chanref.tile_geometry(4095, 80) == (4095, 64, 1, 65520)
    assert chanref.tile_geometry(4096, 80) is None
    # the splits tests/test_channelizer.py's channel lists get: never more than 5 to a group
    assert chanref.group_sizes(8, 128) == [4, 4] and chanref.group_sizes(11, 64) == [3, 3, 3, 2] and chanref.group_sizes(5, 256) == [5]
    assert chanref.group_sizes(1, 64) == [1] and chanref.group_sizes(3, 64) == [1, 1, 1] and chanref.group_sizes(33, 256) == [7, 7, 7, 6, 6]


def test_bound_is_unchanged_for_the_filters_in_use():
    for D in (6, 30, 45):
        h = _taps(D)
        assert chanref.lp_of(h) == 80 and chanref.bound(h) == 1e-5 * float(np.sum(np.abs(h.astype(np.float64))))
    h = _taps(30, 0.049)
    assert chanref.lp_of(h) == 84 and chanref.bound(h) == 1e-5 * float(np.sum(np.abs(h.astype(np.float64))))
    h = _taps(6, 0.0125)
    assert chanref.lp_of(h) == 320 and chanref.bound(h) == 648 * 2.0 ** -24 * float(np.sum(np.abs(h.astype(np.float64))))


def test_shape_tables_reach_every_path():
    seen_groups, full, partial, one = set(), set(), set(), set()
    short = long_ = odd = even = False
    for name, (D, tbw, Lp, offsets, n_out) in shapes.GEOMETRY.items():
        L = chanref.filter_len(tbw)
        assert Lp == L + 3 - (L + 3) % 4, name
        P, Tpad, T, lds = _geometry(D, Lp)
        assert P == D | 1 and lds <= 64 * 1024
        assert n_out > 2 * T and (T == 1 or n_out % T != 0), name              # two full tiles and a partial one
        assert shapes.capture_len(n_out, D, Lp) <= 25000 and chanref.nout(shapes.capture_len(n_out, D, Lp), Lp, D) == n_out, name
        assert 4 <= len(offsets) <= 5 and min(offsets) < 0 and 0 in offsets and (1 in offsets or -1 in offsets), name
        assert max(abs(f) for f in offsets) == shapes.FS // 2 - 1, name
        seen_groups.update(chanref.group_sizes(len(offsets), Tpad))
        (full if T == Tpad else partial).add(Tpad)
        if T == 1:
            one.add(Tpad)
        short |= Lp < D
        long_ |= Lp > 4 * D
        odd |= D % 2 == 1
        even |= D % 2 == 0
    assert full == {64, 128, 256}, full                                         # T = Tpad at every Tpad
    assert partial == {64} and one == {64}                                      # T < 64 and T = 1 (only Tpad = 64 can have them)
    assert short and long_ and odd and even
    assert chanref.tile_geometry(4096, 80) is None
    assert max(chanref.lp_of(_taps(D, tbw)) for D, tbw, *_ in shapes.GEOMETRY.values()) == 324
    for D, K, sizes in shapes.GROUPS:
        Tpad = _geometry(D, 80)[1]
        assert chanref.group_sizes(K, Tpad) == sizes and sum(sizes) == K, (D, K)
        assert len(set(shapes.GROUP_OFFSETS[:K])) == K and min(shapes.GROUP_OFFSETS[:K]) < 0
        seen_groups.update(sizes)
    assert seen_groups == set(range(1, 9)), seen_groups
    for Fs, D in shapes.FS_LIMIT:
        T = _geometry(D, 80)[2]
        assert any(s % T for s in shapes.FS_SPLITS[1:-1]) and shapes.FS_NOUT > 2 * T
        for fc in shapes.fs_offsets(Fs):
            assert -Fs < 2 * fc < Fs
    assert {Fs for Fs, _ in shapes.FS_LIMIT} == {1 << 24, (1 << 24) - 1, 16000000}
    assert _geometry(6, 80)[1] == 256                                          # k reaches 255 at D = 6


def test_test_signals_do_not_vanish_in_the_bound():
    """for every shape and offset of the geometry and Fs tables: max |want| > 10 bound on the test's own bytes; and the constant capture's
    reference has one magnitude at every output, above the half of sqrt 2 that the cutoff |f_c| = Fs / (2 D) would give"""
    for i, (name, (D, tbw, Lp, offsets, n_out)) in enumerate(shapes.GEOMETRY.items()):
        h = _taps(D, tbw)
        host = shapes.random_capture(i, 1, shapes.capture_len(n_out, D, Lp))
        for fc in offsets:
            assert np.abs(chanref.channel(host[0], h, D, shapes.FS, fc)).max() > 10 * chanref.bound(h), (name, fc)
    for Fs, D in shapes.FS_LIMIT:
        h = _taps(D)
        n = shapes.capture_len(shapes.FS_NOUT, D, 80)
        rnd, const = shapes.random_capture(Fs % 1000 + D, 1, n), shapes.constant_capture(n)
        inside = [fc for fc in shapes.fs_offsets(Fs) if shapes.in_passband(fc, Fs, D)]
        assert {-1, -3, 1} <= set(inside)
        for t0 in shapes.FS_T0:
            for fc in shapes.fs_offsets(Fs):
                assert np.abs(chanref.channel(rnd[0], h, D, Fs, fc, t0)).max() > 10 * chanref.bound(h), (Fs, D, fc)
            for fc in inside:
                mag = np.abs(chanref.channel(const[0], h, D, Fs, fc, t0))
                assert mag.min() > 0.5 * np.sqrt(2.0) and np.ptp(mag) < 1e-9, (Fs, D, fc, mag.min())
                if abs(fc) <= 3:
                    assert abs(mag[0] - np.sqrt(2.0)) < 1e-4, (Fs, D, fc, mag[0])
