"""include/pirip_hip.h section O (the channel) without a GPU: the library, the header, the binding and the CLI are there; the bound of
tests/airref.py is the arithmetic of its derivation; and the inputs of tests/test_air.py reach what they claim, on the float64 model
alone -- the u8 identity, the tie windows, the delays and the rings' wraps, the clipping, and both legs of the shared-medium loop, which the
reference chain (channelizer, oracle demodulator, decoder) decodes without a bit error."""
import inspect
import os
import subprocess

import numpy as np
import pytest

import airref
import airshapes as sh
import chanref
import muxref
import muxshapes as ms
import txref

AIR_SYMBOLS = ("pirip_hip_air_create", "pirip_hip_air_destroy", "pirip_hip_air_get_info", "pirip_hip_air_set_sigma", "pirip_hip_air_push",
               "pirip_hip_air_reset")


def test_library_header_binding_and_cli(built_lib):
    import pirip_amd
    out = subprocess.run(["nm", "-D", "--defined-only", pirip_amd.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    hdr = open(os.path.join(ms.ROOT, "include", "pirip_hip.h")).read()
    assert "section O" in hdr
    for n in AIR_SYMBOLS:
        assert n in exported and hasattr(built_lib, n) and n + "(" in hdr, n
    sig = inspect.signature(pirip_amd.HipAir)
    assert list(sig.parameters)[:4] == ["Fs", "paths", "ntx", "nrx"]
    for k, v in (("sigma", None), ("seed", 1), ("in_format", pirip_amd.IN_CU8_CSDR), ("out_format", pirip_amd.IN_CU8_CSDR), ("device", -1)):
        assert sig.parameters[k].default == v, k
    assert inspect.signature(pirip_amd.HipAir.reset).parameters["n0"].default == 0
    for m in ("push", "set_sigma", "reset", "close"):
        assert callable(getattr(pirip_amd.HipAir, m)), m
    assert [f[0] for f in pirip_amd.AirPath._fields_] == ["rx", "tx", "delay", "offset_hz", "gain"]
    assert (pirip_amd.IN_CU8_CSDR, pirip_amd.IN_CF32) == (airref.U8, airref.CF32)
    assert os.access(os.path.join(ms.BIN, "air_channels"), os.X_OK)


def test_bound_is_the_arithmetic_of_its_derivation():
    e = airref.E
    rotated = 2 * np.pi * (1 + 2.0 ** -25) + 2 * np.sqrt(2.0) + 2
    assert 11.11 < rotated < 11.12                               # the first-order terms of a rotated path
    assert rotated + 0.88 <= 12.0 + 1e-12                        # what the 12 leaves for the second order
    assert 2 * e * 100 ** 2 * e < 0.01 * e                       # ... which needs far less, at (K + 12) <= 100
    x = np.array([[3 + 4j, 0], [1j, -2]], dtype=np.complex128)
    paths = [(0, 0, 0.5, 0, 0), (0, 1, -0.25, 1, 7), (1, 1, 2.0, 0, 0)]
    assert airref.amplitude(x, paths, 0) == 0.5 * 5 + 0.25 * 2 and airref.amplitude(x, paths, 1) == 4.0 and airref.amplitude(x, paths, 2) == 0.0
    assert airref.bound(x, paths, 0) == 14 * e * 3.0 and airref.bound(x, paths, 1) == 13 * e * 4.0 and airref.bound(x, paths, 2) == 0.0
    mag = np.array([0.0, 0.3])
    b = airref.bound(x, paths, 0, noise_mag=mag)
    assert np.array_equal(b, 14 * e * 3.0 + txref.NOISE_REL_BOUND * mag + e * (3.0 + mag))
    # a receiver with noise and no path: the noise's own bound and the sum's rounding
    assert np.array_equal(airref.bound(x, paths, 2, noise_mag=mag), txref.NOISE_REL_BOUND * mag + e * mag)
    assert airref.ring_size(0) == 64 and airref.ring_size(64) == 64 and airref.ring_size(65) == 128 and airref.ring_size(1 << 20) == 1 << 20
    assert airref.rings(sh.inputs(240000, "u8")[1], sh.NTX) == [8192, 512, 64]


def test_model_is_the_definition_on_a_case_worked_by_hand():
    Fs = 8
    x = np.array([[1, 2, 3, 4], [1j, 0, 0, 0]], dtype=np.complex128)
    paths = [(0, 0, 2.0, 1, 2), (0, 1, 1.0, 0, 0), (1, 0, 1.0, 3, -2)]
    # n = 6 .. 9: e^{j 2 pi 2 n / 8} = j^n
    y = airref.signal(x, Fs, paths, 0, 6)
    assert np.allclose(y, [1j, 2 * (1j ** 7) * 1, 2 * (1j ** 8) * 2, 2 * (1j ** 9) * 3])
    assert np.allclose(airref.signal(x, Fs, paths, 1, 6), [0, 0, 0, (1j ** -9) * 1])
    assert np.allclose(airref.signal(x, Fs, paths, 0, 6), airref.signal(x, Fs, paths, 0, 6 + 5 * Fs))
    assert not airref.noise(3, 0, 0, 4, 0.0).any()
    assert np.array_equal(airref.noise(3, 2, 10, 4, 0.5), txref.noise_f64(3, 2, np.arange(10, 14), 0.5))


def test_u8_to_u8_through_a_unit_path_is_the_identity_on_every_byte():
    b = np.arange(256)
    x = np.stack([b, b[::-1]], axis=-1).astype(np.uint8)[None]
    # the kernel's float32 steps: the conversion, fma(1, v, 0) = v, then product and sum rounded separately
    v = (b.astype(np.float64) / 127.5 - 1.0).astype(np.float32)
    q = np.clip(np.rint((np.float32(127.5) * v).astype(np.float32) + np.float32(127.5)), 0, 255)
    assert np.array_equal(q, b)
    # and the model's
    got, arg = airref.quantise_u8(airref.receive(airref.widen(x, airref.U8), 240000, [(0, 0, 1.0, 0, 0)], 0, 0))
    assert np.array_equal(got, x[0]) and np.abs(arg - np.rint(arg)).max() < 1e-4


def _cases():
    for Fs in sh.FSS:
        for in_fmt in ("u8", "cf32"):
            x, paths = sh.inputs(Fs, in_fmt)
            xw = airref.widen(x, sh.FMT[in_fmt])
            for n0 in sh.starts(Fs):
                for sigma in (None, sh.SIGMA):
                    yield Fs, in_fmt, xw, paths, n0, sigma


def test_every_u8_case_stays_clear_of_the_quantisers_ties():
    worst = 0.0
    for Fs, in_fmt, xw, paths, n0, sigma in _cases():
        for r in range(sh.NRX):
            K = len(airref.paths_of(paths, r))
            s = 0.0 if sigma is None else sigma[r]
            if not K and not s:
                continue                                         # all bytes 128: the argument is exactly 127.5 + 127.5 * 0, no tie
            nz = airref.noise(sh.SEED, r, n0, sh.N, s)
            y = airref.signal(xw, Fs, paths, r, n0) + nz
            b = airref.bound(xw, paths, r, np.abs(nz)) if s else airref.bound(xw, paths, r)
            _, v = airref.quantise_u8(y)
            share = float(airref.tie_window(v, b).mean())
            worst = max(worst, share)
            assert share <= 1e-3, (Fs, in_fmt, n0, r, share)
            if K:
                assert np.abs(y).max() > 100 * np.max(b), "the test signal should not vanish in the bound"
    print(f"largest share of components inside a tie window {worst:.2e}")


def _wraps(paths, ntx, n0, first_of_call):
    """does a call whose first sample is first_of_call (of the run that starts at n0) read a span of some ring across its wrap"""
    R = airref.rings(paths, ntx)
    a1 = n0 + first_of_call
    return any(d > 0 and first_of_call > 0 and (a1 - d) // R[tx] != (a1 - 1) // R[tx] for _, tx, _, d, _ in paths)


def test_shapes_reach_every_corner():
    assert sh.N > 3 * airref.TILE and sh.N % airref.TILE and sh.N % 8 and sum(sh.CALLS) == sh.N
    for Fs in sh.FSS:
        lay = sh.layout(Fs)
        delays = {d for _, _, d, _ in lay}
        assert {0, 1, 63, 64, 65, 4097} <= delays and max(delays) > airref.TILE and max(delays) < sh.CALLS[0] and max(delays) > sh.CALLS[1]
        per_rx = [[p for p in lay if p[0] == r] for r in range(sh.NRX)]
        assert [len(p) for p in per_rx] == [0, 1, 5, 4] and per_rx[1][0][3] == 0
        assert sorted(d for _, tx, d, _ in per_rx[2] if tx == 0) == [1, 65]
        assert {0, 1, -1, ms.edge(Fs), -ms.edge(Fs)} == {f for _, _, _, f in per_rx[2]}
        assert all(-Fs < 2 * f < Fs for _, _, _, f in lay)
        assert sh.starts(Fs) == [0, Fs - 5, 2 ** 31 + 3]
        x, paths = sh.inputs(Fs, "u8")
        assert all(abs(g) * 2 ** 12 != round(abs(g) * 2 ** 12) for _, _, g, _, _ in paths)        # never dyadic
        assert len(np.unique(x)) == 256
        # the second call reads across a ring's wrap at some start
        assert any(_wraps(paths, sh.NTX, n0, sh.CALLS[0]) for n0 in sh.starts(Fs)), Fs
    # cutting: every cut but the rest is shorter than the longest delay, and calls read across the wrap of both rings
    cp = sh.cut_paths(240000)
    assert max(p[3] for p in cp) > max(sh.CUTS) and sum(sh.CUTS) < sh.CUT_N and sh.CUT_N - sum(sh.CUTS) > airref.TILE
    assert airref.rings(cp, 2) == [256, 64] and 1 in sh.CUTS
    firsts = np.cumsum(sh.CUTS)
    assert any(_wraps(cp, 2, sh.CUT_START, int(f)) for f in firsts)
    assert {p[1] for p in cp if _wraps([p], 2, sh.CUT_START, int(firsts[-1]))} == {0, 1}


def test_clipping_case_exceeds_the_range():
    rng = np.random.default_rng(6)
    x = rng.integers(0, 256, (2, sh.CLIP_N, 2)).astype(np.uint8)
    y = airref.receive(airref.widen(x, airref.U8), 240000, sh.CLIP_PATHS, 0, 0)
    q, v = airref.quantise_u8(y)
    assert y.real.max() > 2 and y.real.min() < -2 and y.imag.max() > 2 and y.imag.min() < -2
    assert (v < -10).any() and (v > 265).any() and (q == 0).any() and (q == 255).any() and ((q > 0) & (q < 255)).any()


def loop_transmit_u8(oracle):
    """muxshapes.LOOP's transmit IQ as tests/test_mux_cpu.py builds it: txref -> muxref -> u8, int64 [n, 2], and the records and taps"""
    lp = ms.LOOP
    rec = ms.loop_records()
    syms = ms.loop_syms(rec)
    Ts = lp["mFs"] // lp["Rs"]
    z = np.stack([txref.mod_f64(syms[c], lp["f1"], lp["shift"], lp["mFs"], Ts) for c in range(4)]).astype(np.complex64)
    hb = np.zeros(79, dtype=np.float32)
    oracle.lib().oracle_firdes_lowpass_f_hamming(hb.ctypes.data, 79, 0.5 / lp["D"])
    h = np.float32(lp["D"]) * hb
    Q = muxref.q_of(79, lp["D"])
    zin = np.concatenate([np.zeros((4, Q - 1), np.complex64), z], axis=1)
    u8, _ = muxref.quantise_u8(muxref.mux(zin, h, lp["D"], lp["Fs"], lp["offsets"], ms.LOOP_GAINS, m0=-(Q - 1)))
    return u8, rec, hb


def decode_u8(oracle, u8, hb):
    """the reference chain on a wideband u8 stream: per LOOP channel the payloads of the frames that came out with RX_BITS"""
    lp = ms.LOOP
    code = oracle.parse_code_file(ms.CODE)
    out = []
    for fc in lp["offsets"]:
        y = chanref.channel(np.asarray(u8).astype(np.uint8), hb, lp["D"], lp["Fs"], fc)
        yf = np.stack([y.real, y.imag], axis=-1).astype(np.float32)
        o = oracle.OracleFsk(lp["mFs"], lp["Rs"], lp["M"], P=lp["P"], est_min=lp["est_min"], est_max=lp["est_max"])
        st, pl, _ = oracle.OracleLdpc(code, lp["M"]).rx(o.demod(yf, oracle.IN_CF32)["rx_filt"])
        out.append(pl[(st & txref.RX_BITS) != 0])
    return out


@pytest.mark.parametrize("leg", ["far", "leak"])
def test_both_legs_of_the_loop_decode_on_the_reference_chain(built_lib, oracle, leg):
    """The loop's transmit IQ through the model with the leg's gain, delay and offset and the loop's sigma, quantised, then through the
    reference chain: every frame of every channel comes out without a bit error."""
    lp = ms.LOOP
    u8, rec, hb = loop_transmit_u8(oracle)
    p = sh.FAR if leg == "far" else sh.LEAK
    y = airref.receive(airref.widen(u8[None].astype(np.uint8), airref.U8), lp["Fs"], [(0, 0, p["gain"], p["delay"], p["offset"])], 0, 0,
                       sigma=sh.LOOP_SIGMA, seed=sh.LOOP_SEED)
    q, v = airref.quantise_u8(y)
    clipped = float(((v < 0) | (v > 255)).mean())
    print(f"{leg}: share of components the ADC clips {clipped:.2e}")
    assert clipped < 1e-3                                            # four channels at full gain and 5 sigma of noise touch the rails, rarely
    kb = rec.shape[2] - 1
    for c, good in enumerate(decode_u8(oracle, q, hb)):
        assert good.shape[0] == lp["nframes"], (leg, c, good.shape[0])
        assert np.array_equal(good[:, :kb - 2], rec[c, :lp["nframes"], 1:kb - 1]), (leg, c)
