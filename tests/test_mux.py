"""include/pirip_hip.h section J: the multiplexer (pirip_hip_mux_*, pirip_amd.HipMux) and the CLI fsk_ldpc_tx_channels.

Contract 1: every complex-float component within muxref.bound -- (2 K Q + K + 13) 2^-24 A, derived in DESIGN.md 4.10 from the
arithmetic, never above the (4 K Q + 16) 2^-24 A first stated for this stage -- of the float64 statement (tests/muxref.py) on the same
inputs, taps and gains; every u8 byte within one level of the quantised float64 value, and different from it only where the float64
argument lies within 127.5 bound + 2^-16 of a tie. Contract 2: blocks that overlap by Q - 1 inputs equal one shot, m0 equals m0 + Fs, an
output does not depend on the others, a sample-aligned row equals a 16-byte-aligned one -- bit for bit. Contract 3: what HipTx and HipMux
send, HipChan and the FSK_LDPC chain receive."""
import os
import subprocess

import numpy as np
import pytest

import muxref
import muxshapes as ms
import txref

pytestmark = pytest.mark.gpu

CANARY = 0xA5


def _run(mx, z, m0=0, in_pad=0, out_pad=0):
    """z complex64 [K, n_in] -> uint8 [noutputs, nout * bytes_per_sample] as stored. in_pad / out_pad: samples by which the first row is
    moved off its 16-byte alignment (the strides then are no multiple of 16 either). Every row is followed by canary bytes."""
    import torch
    K, n_in = z.shape
    bs = mx.bytes_per_sample
    no = mx.nout(n_in)
    in_stride = (n_in * 8 + 15) // 16 * 16 + (8 if in_pad else 0)
    buf = np.zeros(K * in_stride + 64, dtype=np.uint8)
    for c in range(K):
        buf[in_pad * 8 + c * in_stride: in_pad * 8 + c * in_stride + n_in * 8] = np.ascontiguousarray(z[c]).view(np.uint8)
    d_in = torch.from_numpy(buf).cuda()
    out_stride = (no * bs + 32 + 15) // 16 * 16 + (bs if out_pad else 0)
    d_out = torch.full((mx.noutputs * out_stride + 64,), CANARY, dtype=torch.uint8, device="cuda")
    assert d_in.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    mx.batch(d_in.data_ptr() + in_pad * 8, in_stride, n_in, d_out.data_ptr() + out_pad * bs, out_stride, m0=m0)
    torch.cuda.synchronize()
    o = d_out.cpu().numpy()
    assert (o[:out_pad * bs] == CANARY).all()
    rows = []
    for i in range(mx.noutputs):
        r = o[out_pad * bs + i * out_stride: out_pad * bs + (i + 1) * out_stride]
        assert (r[no * bs:] == CANARY).all(), f"output {i}: bytes stored past n_out"
        rows.append(r[:no * bs])
    assert (o[out_pad * bs + mx.noutputs * out_stride:] == CANARY).all()
    return np.stack(rows)


def _cf32(rows):
    v = np.ascontiguousarray(rows).view(np.float32).reshape(rows.shape[0], -1, 2).astype(np.float64)
    return v[..., 0] + 1j * v[..., 1]


def _u8(rows):
    return rows.reshape(rows.shape[0], -1, 2).astype(np.int64)


def _check_u8(got, want, b, tag):
    """the per-sample u8 rule; returns the share of components inside a tie window"""
    q, v = muxref.quantise_u8(want)
    d = np.abs(got - q)
    assert d.max(initial=0) <= 1, (tag, d.max())
    window = muxref.tie_window(v, b)
    assert not (d[~window] != 0).any(), (tag, int((d[~window] != 0).sum()))
    return float(window.mean()) if window.size else 0.0


@pytest.mark.parametrize("fmt", ["cf32", "u8"])
@pytest.mark.parametrize("name,kind", ms.KINDS, ids=[f"{s}-{'fir' if k == muxref.FIR else 'lin'}" for s, k in ms.KINDS])
def test_mux_matches_float64(built_lib, name, kind, fmt):
    import pirip_amd
    Fs, D, tbw, offsets, outputs, noutputs, branch, m0 = ms.SHAPES[name]
    mx = pirip_amd.HipMux(Fs, D, offsets, outputs=outputs, gains=None, kind=kind, transition_bw=tbw, noutputs=noutputs,
                          out_format=pirip_amd.IN_CF32 if fmt == "cf32" else pirip_amd.IN_CU8_CSDR)
    mx.close()
    n_in = branch + muxref.q_of(ms.taps_len(kind, D, tbw), D) - 1
    z, g = ms.inputs(name, n_in)
    mx = pirip_amd.HipMux(Fs, D, offsets, outputs=outputs, gains=g, kind=kind, transition_bw=tbw, noutputs=noutputs,
                          out_format=pirip_amd.IN_CF32 if fmt == "cf32" else pirip_amd.IN_CU8_CSDR)
    h = mx.taps()
    assert len(h) == mx.ntaps == ms.taps_len(kind, D, tbw) and mx.Q == muxref.q_of(len(h), D) and mx.ntaps_padded == mx.Q * D
    assert (mx.nchan, mx.noutputs, mx.bytes_per_sample) == (len(offsets), noutputs, 8 if fmt == "cf32" else 2)
    if kind == muxref.LINEAR:
        assert np.array_equal(h, muxref.linear_taps(D))
    else:
        assert np.array_equal(h, np.float32(D) * pirip_amd.HipDecim(D, transition_bw=tbw, out_s16=False).taps())
    assert mx.nout(n_in) == branch * D == muxref.nout(n_in, mx.Q, D)
    rows = _run(mx, z, m0=m0)
    got = _cf32(rows) if fmt == "cf32" else _u8(rows)
    for i, chans in enumerate(ms.channels_of(outputs, len(offsets), noutputs)):
        want = muxref.mux(z[chans], h, D, Fs, [offsets[c] for c in chans], g[chans], m0) if chans else np.zeros(branch * D, np.complex128)
        b = muxref.bound(z[chans], h, D, g[chans]) if chans else 0.0
        assert not chans or b <= muxref.issue_bound(z[chans], h, D, g[chans])
        if fmt == "cf32":
            e = max(np.abs(got[i].real - want.real).max(), np.abs(got[i].imag - want.imag).max())
            print(f"{name} kind {kind} output {i}: K {len(chans)} Q {mx.Q} largest error {e:.3e} bound {b:.3e} ratio {e / b if b else 0:.3f}")
            assert e <= b, (name, i, e, b)
            assert not chans or np.abs(want).max() > 100 * b, "the test signal should not vanish in the bound"
            if not chans:
                assert not rows[i].any()                                                 # an empty output: all zeros
        else:
            share = _check_u8(got[i], want, b, (name, i))
            print(f"{name} kind {kind} output {i}: K {len(chans)} share of components inside a tie window {share:.2e}")
            if not chans:
                assert (rows[i] == 128).all()                                            # an empty output: all bytes 128


def _handle(fmt="u8", kind=muxref.FIR, D=30, Fs=2400000, offsets=(-700003, 1, 0, 1159999), gains=(0.2, -0.15, 0.1, 0.25), **kw):
    import pirip_amd
    return pirip_amd.HipMux(Fs, D, list(offsets), gains=list(gains), kind=kind,
                            out_format=pirip_amd.IN_CF32 if fmt == "cf32" else pirip_amd.IN_CU8_CSDR, **kw)


def _noise(K, n, seed):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(K, n)) + 1j * rng.normal(size=(K, n))).astype(np.complex64)


@pytest.mark.parametrize("fmt", ["cf32", "u8"])
def test_edges(built_lib, fmt):
    """n_in = Q, Q - 1 and 0; rows aligned to the sample only equal 16-byte-aligned rows; negative and huge m0; nothing past n_out (the
    canaries of _run)"""
    mx = _handle(fmt)
    Q, D = mx.Q, mx.D
    z = _noise(4, 90, 1)
    assert mx.nout(Q) == D and mx.nout(Q - 1) == 0 and mx.nout(0) == 0
    assert _run(mx, z[:, :Q]).shape[1] == D * mx.bytes_per_sample
    assert _run(mx, z[:, :Q - 1]).shape[1] == 0 and _run(mx, z[:, :0]).shape[1] == 0
    h = mx.taps()
    for m0 in (0, -3, -2 ** 40 - 7):
        a = _run(mx, z, m0=m0)
        assert a.shape[1] == (90 - Q + 1) * D * mx.bytes_per_sample and (90 - Q + 1) * D > muxref.TILE
        for in_pad, out_pad in ((1, 0), (0, 1), (1, 1), (0, 3)):
            assert np.array_equal(_run(mx, z, m0=m0, in_pad=in_pad, out_pad=out_pad), a), (m0, in_pad, out_pad)
        want = muxref.mux(z, h, D, mx.Fs, mx.offsets, mx.gains, m0)
        b = muxref.bound(z, h, D, mx.gains)
        if fmt == "cf32":
            g = _cf32(a)[0]
            assert max(np.abs(g.real - want.real).max(), np.abs(g.imag - want.imag).max()) <= b, m0
        else:
            _check_u8(_u8(a)[0], want, b, m0)


def test_saturation(built_lib):
    mx = _handle("u8", gains=(3.0, -2.0, 4.0, 2.5))
    z = _noise(4, 80, 2)
    got = _u8(_run(mx, z))[0]
    want = muxref.mux(z, mx.taps(), mx.D, mx.Fs, mx.offsets, mx.gains)
    _check_u8(got, want, muxref.bound(z, mx.taps(), mx.D, mx.gains), "overdriven")
    q, v = muxref.quantise_u8(want)
    assert (v < -10).any() and (v > 265).any() and (got == 0).any() and (got == 255).any()
    assert (got[v < -1] == 0).all() and (got[v > 256] == 255).all()


@pytest.mark.parametrize("fmt,kind,D", [("u8", muxref.FIR, 30), ("cf32", muxref.FIR, 6), ("u8", muxref.LINEAR, 45), ("cf32", muxref.FIR, 1)])
def test_blocks_equal_one_shot_and_m0_plus_fs(built_lib, fmt, kind, D):
    Fs = 240000 * D if D > 1 else 2400000
    offs = [-(Fs // 2 - 1), 1, 0, Fs // 3 + 1, -7, 12345, -54321, Fs // 5, 99]           # 9 channels: two groups
    mx = _handle(fmt, kind=kind, D=D, Fs=Fs, offsets=offs, gains=[0.05 * (1 + c % 3) * (-1) ** c for c in range(9)])
    Q = mx.Q
    n_in = 2600 // D + 150 + Q
    z = _noise(9, n_in, 3 + D)
    base = -2 ** 33 - 11
    whole = _run(mx, z, m0=base)
    assert np.array_equal(_run(mx, z, m0=base + Fs), whole) and np.array_equal(_run(mx, z, m0=base - 5 * Fs), whole)
    assert not np.array_equal(_run(mx, z, m0=base + 1), whole)
    bs, nb = mx.bytes_per_sample, n_in - Q + 1
    splits = [0, 1, 37, nb // 3 + 1, nb // 2 + 5, nb - 1, nb]
    for k, (ja, jb) in enumerate(zip(splits[:-1], splits[1:])):
        part = _run(mx, z[:, ja: jb + Q - 1], m0=base + ja, in_pad=k % 2, out_pad=(k // 2) % 2)
        assert np.array_equal(part, whole[:, ja * D * bs: jb * D * bs]), (ja, jb)


def test_output_does_not_depend_on_the_other_outputs(built_lib):
    import pirip_amd
    Fs, D = 2400000, 30
    offs = [-700003, 1, 0, 1159999, -1, 5, 250000, 333333, -9, 77, 1000000]
    outs = [0, 1, 0, 2, 1, 0, 0, 2, 0, 1, 0]
    g = np.array([0.05 * (1 + c % 4) * (-1) ** c for c in range(11)], dtype=np.float32)
    z = _noise(11, 100, 9)
    full = _run(pirip_amd.HipMux(Fs, D, offs, outputs=outs, gains=g), z, m0=17)
    for i in range(3):
        sel = [c for c in range(11) if outs[c] == i]
        alone = _run(pirip_amd.HipMux(Fs, D, [offs[c] for c in sel], gains=g[sel]), z[sel], m0=17)
        assert np.array_equal(alone[0], full[i]), i
        # and in other company, at another output index
        other = _run(pirip_amd.HipMux(Fs, D, [5, 6] + [offs[c] for c in sel], outputs=[0, 2] + [1] * len(sel), gains=[1.0, 1.0] + list(g[sel])),
                     np.concatenate([z[:2], z[sel]]), m0=17)
        assert np.array_equal(other[1], full[i]), i


def test_limits_and_bad_arguments(built_lib):
    import torch
    import pirip_amd
    M = pirip_amd.HipMux

    def fails(code, fn, *a, **kw):
        with pytest.raises(pirip_amd.PiripError, match=rf"\({code}\)"):
            fn(*a, **kw)

    # PIRIP_ERR_UNSUPPORTED: both sides of the working-set rule (muxref.geometry) and of Fs = 2^24
    for bs, fmt, Dmax in ((2, pirip_amd.IN_CU8_CSDR, 3807), (8, pirip_amd.IN_CF32, 3039)):
        assert muxref.geometry(Dmax, 2 * Dmax - 1, bs) is not None and muxref.geometry(Dmax + 1, 2 * Dmax + 1, bs) is None
        fails(-6, M, 1 << 24, Dmax + 1, [0], kind=pirip_amd.MUX_LINEAR, out_format=fmt)
        mx = M(1 << 24, Dmax, [5], gains=[0.3], kind=pirip_amd.MUX_LINEAR, out_format=fmt)
        z = _noise(1, 3, Dmax)
        rows = _run(mx, z, m0=-1)
        want = muxref.mux(z, mx.taps(), Dmax, 1 << 24, [5], [0.3], -1)
        b = muxref.bound(z, mx.taps(), Dmax, mx.gains)
        if bs == 8:
            g = _cf32(rows)[0]
            assert max(np.abs(g.real - want.real).max(), np.abs(g.imag - want.imag).max()) <= b
        else:
            _check_u8(_u8(rows)[0], want, b, Dmax)
    # FIR at D = 6, u8: 4096 + 8 (6 Q + 342 + Q) <= 65536 up to Q = 1048, L = 6288; csdr's length rule gives 6271 and 6291 below
    assert muxref.geometry(6, 6271, 2) is not None and muxref.geometry(6, 6288, 2) is not None and muxref.geometry(6, 6291, 2) is None
    M(240000, 6, [0], transition_bw=4.0 / 6271.5).close()
    fails(-6, M, 240000, 6, [0], transition_bw=4.0 / 6290.5)
    M(1 << 24, 30, [0]).close()
    fails(-6, M, (1 << 24) + 1, 30, [0])
    # PIRIP_ERR_BAD_ARG
    fails(-1, M, 2400000, 30, [])                              # nchan < 1
    fails(-1, M, 2400000, 30, [0], noutputs=0)                 # noutputs < 1
    fails(-1, M, 2400000, 0, [0])                              # D < 1
    fails(-1, M, 2400000, 30, [0, 5], outputs=[0, -1])         # chan_output outside [0, noutputs)
    fails(-1, M, 2400000, 30, [0, 5], outputs=[0, 2], noutputs=2)
    fails(-1, M, 2400000, 30, [1200000])                       # offset at +Fs/2
    fails(-1, M, 2400000, 30, [-1200000])                      # offset at -Fs/2
    M(2400000, 30, [1199999, -1199999]).close()                # (just inside is fine)
    fails(-1, M, 2400000, 30, [0], gains=[float("nan")])
    fails(-1, M, 2400000, 30, [0], gains=[float("inf")])
    fails(-1, M, 2400000, 30, [0], kind=2)
    fails(-1, M, 2400000, 30, [0], out_format=pirip_amd.IN_CS16)
    mx = M(2400000, 30, [0, 1], outputs=[0, 1])
    cf = M(2400000, 30, [0], out_format=pirip_amd.IN_CF32)
    d_in = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(65536, dtype=torch.uint8, device="cuda")
    i, o = d_in.data_ptr(), d_out.data_ptr()
    fails(-1, mx.batch, i + 4, 800, 10, o, 8192)               # input not 8-byte aligned
    fails(-1, mx.batch, i, 804, 10, o, 8192)                   # input stride no multiple of 8
    fails(-1, mx.batch, i, 800, 10, o + 1, 8192)               # u8 output at an odd address
    fails(-1, mx.batch, i, 800, 10, o, 8191)
    fails(-1, cf.batch, i, 800, 10, o + 4, 8192)               # complex float output not 8-byte aligned
    fails(-1, cf.batch, i, 800, 10, o, 8196)
    fails(-1, mx.batch, i, 800, 10, o, 100)                    # rows of two outputs would overlap
    fails(-1, mx.batch, 0, 800, 10, o, 8192)
    fails(-1, mx.batch, i, 800, -1, o, 8192)
    mx.batch(i, 800, 10, o, 8192)
    torch.cuda.synchronize()


# ---- loopback: HipTx -> HipMux -> HipChan -> FSK_LDPC chain ----------------------------------------------------------------------------
def _sent(rec):
    lp = ms.LOOP
    return rec[:, :lp["nframes"], 1:-2]                          # the payloads apart from the CRC bytes


def _tx_rows(rec, Q, lead=None, gap=None):
    """HipTx on the loopback's records: complex float rows [4, Q - 1 + nmod] on the device with Q - 1 zeros in front, and nmod"""
    import torch
    import pirip_amd
    lp = ms.LOOP
    tx = pirip_amd.HipTx(ms.CODE, lp["mFs"], lp["Rs"], lp["M"], nstreams=4, f1=lp["f1"], shift=lp["shift"],
                         lead=lp["lead"] if lead is None else lead, gap=lp["tail"] if gap is None else gap)
    burst = tx.preamble_syms + lp["nframes"] * tx.frame_syms
    nsym = (max(lp["lead"]) if lead is None else lead) + burst + (lp["tail"] if gap is None else gap)
    nmod = nsym * tx.Ts
    rows = torch.zeros((4, Q - 1 + nmod, 2), dtype=torch.float32, device="cuda")
    d_rec = torch.from_numpy(rec).cuda()
    tx.records_to_iq(d_rec.data_ptr(), rec[0].size, rec.shape[1], nsym, rows.data_ptr() + (Q - 1) * 8, rows[0].numel() * 4,
                     out_format=pirip_amd.IN_CF32)
    torch.cuda.synchronize()
    return rows, nmod


def _rx_handles():
    import pirip_amd
    lp = ms.LOOP
    dem = pirip_amd.HipDemod(lp["mFs"], lp["Rs"], lp["M"], P=lp["P"], est_min=lp["est_min"], est_max=lp["est_max"], in_format=pirip_amd.IN_CF32,
                             nstreams=4)
    return dem, pirip_amd.HipLdpc(ms.CODE, lp["M"], nstreams=4), pirip_amd.HipChan(lp["Fs"], lp["D"], lp["offsets"])


def _assert_all_back(payloads, rec):
    want = _sent(rec)
    for c in range(4):
        got = payloads[c]
        assert got.shape[0] == ms.LOOP["nframes"], (c, got.shape[0])
        assert np.array_equal(got[:, :-2], want[c]), c


def test_loopback_on_the_device(built_lib):
    import torch
    import pirip_amd
    lp = ms.LOOP
    rec = ms.loop_records()
    mx = pirip_amd.HipMux(lp["Fs"], lp["D"], lp["offsets"], gains=ms.LOOP_GAINS)
    Q, D = mx.Q, lp["D"]
    rows, nmod = _tx_rows(rec, Q)
    # the device's modem rows are the float64 formula's, so these are the inputs of the CPU loopback
    syms = ms.loop_syms(rec)
    assert syms.shape[1] * (lp["mFs"] // lp["Rs"]) == nmod
    z64 = txref.mod_f64(syms[1], lp["f1"], lp["shift"], lp["mFs"], lp["mFs"] // lp["Rs"])
    zdev = rows[1, Q - 1:].cpu().numpy().astype(np.float64)
    assert np.abs(zdev[:, 0] - z64.real).max() <= txref.BOUND and np.abs(zdev[:, 1] - z64.imag).max() <= txref.BOUND
    n_in, n_wide = Q - 1 + nmod, nmod * D
    wide = torch.zeros(n_wide * 2, dtype=torch.uint8, device="cuda")
    mx.batch(rows.data_ptr(), n_in * 8, n_in, wide.data_ptr(), n_wide * 2, m0=-(Q - 1))
    # one shot: channelizer over the whole stream, one fused FSK_LDPC batch
    dem, ld, ch = _rx_handles()
    no = ch.nout(n_wide)
    mod = torch.zeros((4, no * 8), dtype=torch.uint8, device="cuda")
    ch.batch(wide.data_ptr(), n_wide * 2, n_wide, mod.data_ptr(), no * 8)
    R, nb = dem.max_frames_for(no), ld.data_bytes
    st = torch.zeros((4, R), dtype=torch.uint8, device="cuda")
    pl = torch.zeros((4, R, nb), dtype=torch.uint8, device="cuda")
    info = torch.zeros((4, R, 10), dtype=torch.int32, device="cuda")
    nfr = torch.zeros(4, dtype=torch.int32, device="cuda")
    cons = torch.zeros(4, dtype=torch.int64, device="cuda")
    ld.chain_batch(dem, mod.data_ptr(), no * 8, no, st.data_ptr(), pl.data_ptr(), info.data_ptr(), nfr.data_ptr(), cons.data_ptr(), R)
    torch.cuda.synchronize()
    s, p, nf = st.cpu().numpy(), pl.cpu().numpy(), nfr.cpu().numpy()
    _assert_all_back([p[c, :nf[c]][(s[c, :nf[c]] & pirip_amd.RX_BITS) != 0] for c in range(4)], rec)

    # block after block: the multiplexer with its Q - 1 overlap, the channelizer and the chain through HipRx(chan=...)
    Bm = 4000
    block = Bm * D
    dem2, ld2, ch2 = _rx_handles()
    rx = pirip_amd.HipRx(dem2, ldpc=ld2, chan=ch2, block=block)
    R = rx.max_frames
    outs = [[] for _ in range(4)]
    blk = torch.zeros(block * 2, dtype=torch.uint8, device="cuda")
    for k in range(nmod // Bm):
        mx.batch(rows.data_ptr() + k * Bm * 8, n_in * 8, Bm + Q - 1, blk.data_ptr(), block * 2, m0=k * Bm - (Q - 1))
        if k == 3:
            torch.cuda.synchronize()
            assert torch.equal(blk, wide[k * block * 2:(k + 1) * block * 2])             # blocks equal one shot, here too
        st = torch.zeros((4, R), dtype=torch.uint8, device="cuda")
        pl = torch.zeros((4, R, nb), dtype=torch.uint8, device="cuda")
        info = torch.zeros((4, R, 10), dtype=torch.int32, device="cuda")
        nfr = torch.zeros(4, dtype=torch.int32, device="cuda")
        rx.push(blk.data_ptr(), block * 2, d_status=st.data_ptr(), d_payload=pl.data_ptr(), d_info=info.data_ptr(), d_nframes=nfr.data_ptr())
        torch.cuda.synchronize()
        s, p, nf = st.cpu().numpy(), pl.cpu().numpy(), nfr.cpu().numpy()
        for c in range(4):
            outs[c] += [p[c, f] for f in range(nf[c]) if s[c, f] & pirip_amd.RX_BITS]
    _assert_all_back([np.array(o, dtype=np.uint8).reshape(-1, nb) for o in outs], rec)


@pytest.mark.parametrize("fmt", ["u8", "cf32"])
def test_cli_equals_python_and_feeds_rtl_fsk_channels(built_lib, tmp_path, fmt):
    import torch
    import pirip_amd
    lp = ms.LOOP
    rec = ms.loop_records(seed=22)
    prefix = str(tmp_path / "rec")
    for c in range(4):
        rec[c].tofile(f"{prefix}.{c}")
    lead, gap = 210, lp["tail"]
    out = str(tmp_path / "wide.iq")
    cmd = [os.path.join(ms.BIN, "fsk_ldpc_tx_channels"), "--code", ms.CODE, "-s", str(lp["Fs"]), "-a", str(lp["mFs"]), "-r", str(lp["Rs"]),
           "--f1", str(lp["f1"]), "--shift", str(lp["shift"]), "-c", ",".join(map(str, lp["offsets"])),
           "--gains", ",".join(f"{g:.9g}" for g in ms.LOOP_GAINS), "--format", fmt, "--packed", "--lead", str(lead), "--gap", str(gap),
           "-i", prefix, "-o", out]
    p = subprocess.run(cmd, capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    mx = pirip_amd.HipMux(lp["Fs"], lp["D"], lp["offsets"], gains=ms.LOOP_GAINS,
                          out_format=pirip_amd.IN_CF32 if fmt == "cf32" else pirip_amd.IN_CU8_CSDR)
    Q, bs = mx.Q, mx.bytes_per_sample
    rows, nmod = _tx_rows(rec, Q, lead=lead, gap=gap)
    n_wide = nmod * lp["D"]
    wide = torch.zeros(n_wide * bs, dtype=torch.uint8, device="cuda")
    mx.batch(rows.data_ptr(), (Q - 1 + nmod) * 8, Q - 1 + nmod, wide.data_ptr(), n_wide * bs, m0=-(Q - 1))
    torch.cuda.synchronize()
    got = np.fromfile(out, dtype=np.uint8)
    assert got.size == n_wide * bs and np.array_equal(got, wide.cpu().numpy())
    if fmt != "u8":
        return
    rxp = str(tmp_path / "ch")
    p = subprocess.run([os.path.join(ms.BIN, "rtl_fsk_channels"), "-s", str(lp["Fs"]), "-a", str(lp["mFs"]), "-r", str(lp["Rs"]),
                        "-c", ",".join(map(str, lp["offsets"])), "--code", ms.CODE, "-i", out, "-o", rxp, "-q"], capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    _assert_all_back([np.fromfile(f"{rxp}.{c}", dtype=np.uint8).reshape(-1, 32) for c in range(4)], rec)
