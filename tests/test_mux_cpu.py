"""include/pirip_hip.h section J (multiplexer) without a GPU: the library, the header, the binding and the CLI are there; the float64
statement the GPU tests hold the kernel to (tests/muxref.py) is linear interpolation for PIRIP_MUX_LINEAR and D times the decimator's
prototype for PIRIP_MUX_FIR; the shape table of tests/test_mux.py reaches the kernel's paths; and the float64 chain ALONE -- no device --
carries four FSK_LDPC channels through multiplexer, u8 quantiser, channelizer, demodulator and decoder with every CRC good."""
import inspect
import os
import subprocess

import numpy as np
import pytest

import chanref
import muxref
import muxshapes as ms
import txref

MUX_SYMBOLS = ("pirip_hip_mux_create", "pirip_hip_mux_destroy", "pirip_hip_mux_get_info", "pirip_hip_mux_taps", "pirip_hip_mux_nout",
               "pirip_hip_mux_batch")


def test_library_header_binding_and_cli(built_lib):
    import pirip_amd
    out = subprocess.run(["nm", "-D", "--defined-only", pirip_amd.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    hdr = open(os.path.join(ms.ROOT, "include", "pirip_hip.h")).read()
    assert "section J" in hdr
    for n in MUX_SYMBOLS:
        assert n in exported and hasattr(built_lib, n) and n + "(" in hdr, n
    sig = inspect.signature(pirip_amd.HipMux)
    assert list(sig.parameters)[:3] == ["Fs", "D", "offsets"]
    for k, v in (("outputs", None), ("gains", None), ("kind", pirip_amd.MUX_FIR), ("transition_bw", 0.05),
                 ("out_format", pirip_amd.IN_CU8_CSDR), ("device", -1)):
        assert sig.parameters[k].default == v, k
    assert (pirip_amd.MUX_FIR, pirip_amd.MUX_LINEAR) == (muxref.FIR, muxref.LINEAR) == (0, 1)
    assert inspect.signature(pirip_amd.HipMux.batch).parameters["m0"].default == 0
    for m in ("nout", "taps", "batch", "close"):
        assert callable(getattr(pirip_amd.HipMux, m)), m
    assert os.access(os.path.join(ms.BIN, "fsk_ldpc_tx_channels"), os.X_OK)


@pytest.mark.parametrize("D", [1, 2, 6, 45])
def test_linear_kind_is_linear_interpolation_delayed(D):
    """u[m D + p + D - 1] = (1 - p/D) z[m] + (p/D) z[m+1]: _interp of tests/test_rtl_fsk_cli.py, D - 1 samples late"""
    rng = np.random.default_rng(D)
    n_in = 40
    z = (rng.normal(size=n_in) + 1j * rng.normal(size=n_in)).astype(np.complex64)
    h = muxref.linear_taps(D)
    assert len(h) == max(1, 2 * D - 1) and muxref.q_of(len(h), D) == (1 if D == 1 else 2)
    got = muxref.mux(z[None], h, D, 240000 * D, [0], [1.0])
    Q = muxref.q_of(len(h), D)
    assert len(got) == muxref.nout(n_in, Q, D) == (n_in - Q + 1) * D
    # output j of the call has index (Q - 1) D + j of the interpolated row; t = index - (D - 1) = m D + p
    t = (Q - 1) * D + np.arange(len(got)) - (D - 1)
    m, p = t // D, t % D
    zz = np.concatenate([z.astype(np.complex128), [0.0]])
    want = (1.0 - p / D) * zz[m] + (p / D) * zz[m + 1]
    assert np.abs(got - want).max() < 1e-6                      # (the taps are floats: 1 - k/D rounded)
    assert (p[m + 1 == n_in] == 0).all()                        # the appended zero is never weighted


def test_fir_taps_are_D_times_the_decimators(oracle):
    """h = D h_B in float, h_B csdr's Hamming low-pass of cutoff 0.5 / D: the polyphase branches then have unity gain"""
    L = oracle.lib()
    for D, tbw in ((6, 0.05), (30, 0.05), (6, 0.0125), (1, 0.05)):
        n = L.oracle_firdes_filter_len(tbw)
        assert n == chanref.filter_len(tbw) == ms.taps_len(muxref.FIR, D, tbw)
        hb = np.zeros(n, dtype=np.float32)
        L.oracle_firdes_lowpass_f_hamming(hb.ctypes.data, n, 0.5 / D)
        h = np.float32(D) * hb
        assert abs(float(h.astype(np.float64).sum()) - D) < 1e-5 * D, D            # h_B sums to 1: the D branches have unity gain on average


def test_nout_arithmetic():
    assert muxref.q_of(79, 30) == 3 and muxref.q_of(79, 125) == 1 and muxref.q_of(319, 6) == 54 and muxref.q_of(1, 1) == 1
    assert muxref.nout(2, 3, 30) == 0 and muxref.nout(3, 3, 30) == 30 and muxref.nout(0, 1, 5) == 0 and muxref.nout(10, 1, 5) == 50
    z = np.ones((1, 5), dtype=np.complex64)
    assert len(muxref.mux(z, np.ones(79, np.float32), 30, 2400000, [0], [1.0])) == 90
    assert len(muxref.mux(z[:, :2], np.ones(79, np.float32), 30, 2400000, [0], [1.0])) == 0


def test_geometry_restates_the_host_rule():
    """the values mux_kernels.hip's constants give at shapes worked out by hand"""
    assert muxref.geometry(30, 79, 2) == (3, 30, 72, 8, 4096 + 8 * 8 * (90 + 72))
    assert muxref.geometry(1, 79, 2) == (79, 1, 2126, 3, 4096 + 8 * 3 * (79 + 2126))
    assert muxref.geometry(1, 79, 8) == (79, 1, 2126, 2, 16384 + 8 * 2 * (79 + 2126))
    assert muxref.geometry(45, 79, 2) == (2, 76, 48, 8, 4096 + 8 * 8 * (152 + 48))
    assert muxref.geometry(3807, 2 * 3807 - 1, 2) == (2, 3838, 3, 1, 65528) and muxref.geometry(3808, 2 * 3808 - 1, 2) is None
    assert muxref.geometry(3039, 2 * 3039 - 1, 8) == (2, 3070, 3, 1, 65528) and muxref.geometry(3040, 2 * 3040 - 1, 8) is None


def test_shape_table_reaches_every_path():
    Ds, Fss, ks, groups_cross, wrapped, q1, empty, unequal = set(), set(), set(), False, False, False, False, False
    for name, kind in ms.KINDS:
        Fs, D, tbw, offsets, outputs, noutputs, branch, m0 = ms.SHAPES[name]
        L = ms.taps_len(kind, D, tbw)
        for bs in (2, 8):
            g = muxref.geometry(D, L, bs)
            assert g is not None, (name, kind)
            Q, Dp, Mt, G, lds = g
            no = branch * D
            assert no > muxref.TILE and no % muxref.TILE and no % 8, (name, no)          # a full tile, a ragged one, a ragged 16-byte unit
            assert branch + Q - 1 <= 2400, name
            per_out = [len(c) for c in ms.channels_of(outputs, len(offsets), noutputs)]
            ks.update(per_out)
            groups_cross |= max(per_out) > G
            wrapped |= Dp != D
            q1 |= Q == 1
            empty |= 0 in per_out
            unequal |= len({k for k in per_out if k}) > 1
        Ds.add(D); Fss.add(Fs)
        assert all(-Fs < 2 * f < Fs for f in offsets)
    assert Ds == {1, 2, 6, 30, 45, 125} and Fss == {2400000, 240000, ms.FS24, ms.FS24 - 1}
    assert {1, 3, 8, 9} <= ks and groups_cross and wrapped and q1 and empty and unequal
    every = {f for s in ms.SHAPES.values() for f in s[3]}
    assert {0, 1, -1} <= every
    for Fs in (2400000, ms.FS24, ms.FS24 - 1):
        assert any(abs(f) == ms.edge(Fs) for s in ms.SHAPES.values() if s[0] == Fs for f in s[3]), Fs
    assert muxref.geometry(30, 79, 2)[3] == 8                                             # 9 channels at D = 30: a group of 8 and one of 1
    assert ms.taps_len(muxref.FIR, 6, 0.0125) == 319


def test_derived_bound_is_below_the_issues_and_signals_stand_above_it():
    for name, kind in ms.KINDS:
        Fs, D, tbw, offsets, outputs, noutputs, branch, m0 = ms.SHAPES[name]
        if kind == muxref.FIR:
            continue                                            # (the LINEAR taps need no device; the FIR case is asserted on the GPU)
        h = muxref.linear_taps(D)
        z, g = ms.inputs(name, branch + muxref.q_of(len(h), D) - 1)
        for chans in ms.channels_of(outputs, len(offsets), noutputs):
            if chans:
                b = muxref.bound(z[chans], h, D, g[chans])
                assert b <= muxref.issue_bound(z[chans], h, D, g[chans])
                w = muxref.mux(z[chans], h, D, Fs, [offsets[c] for c in chans], g[chans], m0)
                assert np.abs(w).max() > 100 * b, name


def test_float64_chain_alone_passes_the_loopback(oracle):
    """txref.mod_f64 bursts on four channels -> muxref -> quantise_u8 -> chanref.channel -> OracleFsk (complex float) -> OracleLdpc:
    every payload comes back with a good CRC. The GPU loopback of tests/test_mux.py uses exactly these records, gains and leads."""
    lp = ms.LOOP
    rec = ms.loop_records()
    syms = ms.loop_syms(rec)
    Ts = lp["mFs"] // lp["Rs"]
    z = np.stack([txref.mod_f64(syms[c], lp["f1"], lp["shift"], lp["mFs"], Ts) for c in range(4)]).astype(np.complex64)
    L = oracle.lib()
    hb = np.zeros(79, dtype=np.float32)
    L.oracle_firdes_lowpass_f_hamming(hb.ctypes.data, 79, 0.5 / lp["D"])
    h = np.float32(lp["D"]) * hb
    Q = muxref.q_of(79, lp["D"])
    zin = np.concatenate([np.zeros((4, Q - 1), np.complex64), z], axis=1)               # wideband sample 0 = modem sample 0
    w = muxref.mux(zin, h, lp["D"], lp["Fs"], lp["offsets"], ms.LOOP_GAINS, m0=-(Q - 1))
    assert len(w) == z.shape[1] * lp["D"]
    u8, v = muxref.quantise_u8(w)
    assert v.min() > 0 and v.max() < 255
    amp = 127.5 * 2 * ms.LOOP_GAINS
    assert (amp >= 20 - 1e-4).all() and (amp <= 30 + 1e-4).all()
    code = oracle.parse_code_file(ms.CODE)
    kb = code["k"] // 8
    for c, fc in enumerate(lp["offsets"]):
        y = chanref.channel(u8.astype(np.uint8), hb, lp["D"], lp["Fs"], fc)
        yf = np.stack([y.real, y.imag], axis=-1).astype(np.float32)
        o = oracle.OracleFsk(lp["mFs"], lp["Rs"], lp["M"], P=lp["P"], est_min=lp["est_min"], est_max=lp["est_max"])
        r = o.demod(yf, oracle.IN_CF32)
        st, pl, _ = oracle.OracleLdpc(code, lp["M"]).rx(r["rx_filt"])
        good = pl[(st & txref.RX_BITS) != 0]
        assert good.shape[0] == lp["nframes"], (c, good.shape[0])
        assert np.array_equal(good[:, :kb - 2], rec[c, :lp["nframes"], 1:kb - 1]), c
