"""include/pirip_hip.h section H: the channelizer (pirip_hip_chan_*, pirip_amd.HipChan) and the streaming receiver behind it
(pirip_hip_rx_create_chan, pirip_amd.HipRx(chan=...)).

Contract 1: every complex-float component within 1e-5 * sum |h| of the float64 statement (tests/chanref.py) on the same bytes and taps,
s16 within one LSB -- a bound derived from the arithmetic (Lp float fma roundings plus the rotation), not fitted to what a GPU produced.
Contract 2: calls on overlapping windows and channel lists that differ in order, duplicates or company give the one-shot output bit for bit.
Contract 3: a channel at offset 0 is within the bound of section B's decimator."""
import os
import subprocess

import numpy as np
import pytest

import chanref
import sigutil

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "pirip_amd", "bin")

# (Fs, D, offsets, inputs, t0, n_out)
SHAPES = {
    # 2.4 MS/s / 30: negative, zero, 1 Hz, not multiples of the output rate, near +-(Fs/2 - Fs/(2D))
    "2M4_div30": (2400000, 30, [-700003, 0, 1, 123457, -250001, 1159999, -1159999, 333333], None, 0, 700),
    "1M8_div45": (1800000, 45, [0, 200000, -450001, 7, 859999], None, 0, 500),
    "240k_div6": (240000, 6, [0, 20000, -100001, 60001, 119999], None, 0, 2000),
    "3_inputs": (2400000, 30, [-300000, 250000, 0, 1, -1, 1000003, 77777], [2, 0, 2, 2, 1, 0, 2], 0, 600),
    "t0_odd": (2400000, 30, [-700003, 1, 1159999, 333333], None, 7, 600),
    "t0_above_2e31": (2400000, 30, [-700003, 1, 1159999, 333333], None, 2 ** 31 + 12345, 600),
}


def _run(ch, host, t0=0, in_pad=0):
    """host [W, n, 2] uint8 -> [K, nout] complex128 (cf32) or int64 [K, nout, 2] (s16); in_pad bytes of lead-in shift every capture's base"""
    import torch
    W, n = host.shape[0], host.shape[1]
    stride = 2 * n + in_pad + 2
    buf = torch.zeros(W * stride + 64, dtype=torch.uint8, device="cuda")
    flat = buf.cpu().numpy()
    for w in range(W):
        flat[in_pad + w * stride: in_pad + w * stride + 2 * n] = host[w].reshape(-1)
    buf.copy_(torch.from_numpy(flat))
    no = ch.nout(n)
    bps = ch.bytes_per_sample
    out = torch.zeros((ch.nchan, no * bps + 8), dtype=torch.uint8, device="cuda")
    ch.batch(buf.data_ptr() + in_pad, stride, n, out.data_ptr(), out.shape[1], t0=t0)
    torch.cuda.synchronize()
    o = out.cpu().numpy()[:, :no * bps]
    if ch.out_s16:
        return np.ascontiguousarray(o).view(np.int16).reshape(ch.nchan, no, 2).astype(np.int64)
    v = np.ascontiguousarray(o).view(np.float32).reshape(ch.nchan, no, 2).astype(np.float64)
    return v[..., 0] + 1j * v[..., 1]


@pytest.mark.parametrize("out_s16", [False, True])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_channelizer_matches_float64(built_lib, shape, out_s16):
    import pirip_amd
    Fs, D, offsets, inputs, t0, n_out = SHAPES[shape]
    ch = pirip_amd.HipChan(Fs, D, offsets, inputs=inputs, out_s16=out_s16)
    h = ch.taps()
    assert np.array_equal(h, pirip_amd.HipDecim(D, out_s16=False).taps())
    n = (n_out - 1) * D + ch.Lp + D - 1
    assert ch.nout(n) == n_out == chanref.nout(n, ch.Lp, D)
    rng = np.random.default_rng(sorted(SHAPES).index(shape))
    host = rng.integers(0, 256, (ch.ninputs, n, 2), dtype=np.uint8)
    got = _run(ch, host, t0=t0, in_pad=6)
    inp = [0] * len(offsets) if inputs is None else inputs
    b = chanref.bound(h)
    for c, (w, fc) in enumerate(zip(inp, offsets)):
        want = chanref.channel(host[w], h, D, Fs, fc, t0)
        if out_s16:
            d = np.abs(got[c] - chanref.to_s16(want))
            assert d.max() <= 1, (c, fc, d.max())
        else:
            e = max(np.abs(got[c].real - want.real).max(), np.abs(got[c].imag - want.imag).max())
            assert e <= b, (c, fc, e, b)
            assert np.abs(want).max() > 10 * b, "the test signal should not vanish in the bound"


def test_channelizer_blocks_equal_one_shot(built_lib):
    """consecutive overlapping windows (uneven split points, t0 advanced, capture bases at different alignments) give the one-shot
    output bit for bit"""
    import pirip_amd
    Fs, D = 2400000, 30
    offsets = [-700003, 0, 1, 123457, -250001, 1159999, -1159999, 333333, 5]
    ch = pirip_amd.HipChan(Fs, D, offsets, inputs=[0, 1, 0, 1, 0, 1, 0, 1, 1])
    n = 30 * 2000 + ch.Lp
    host = np.random.default_rng(3).integers(0, 256, (2, n, 2), dtype=np.uint8)
    t_base = 2 ** 33 + 1
    whole = _run(ch, host, t0=t_base)
    no = whole.shape[1]
    splits = [0, 1, 37, 256, 257, 900, 1500, 1999, no]
    for pad_i, (ja, jb) in enumerate(zip(splits[:-1], splits[1:])):
        part = host[:, ja * D: (jb - 1) * D + ch.Lp]
        got = _run(ch, part, t0=t_base + ja * D, in_pad=2 * (pad_i % 8))
        assert got.shape[1] == jb - ja
        assert np.array_equal(got.view(np.float64), whole[:, ja:jb].view(np.float64)), (ja, jb)


def test_channel_output_does_not_depend_on_the_other_channels(built_lib):
    import pirip_amd
    Fs, D = 1800000, 45
    offsets = [-500000, -1, 0, 3, 200001, 777777, -860000, 123, 45000, -45000, 9]
    base = pirip_amd.HipChan(Fs, D, offsets)
    n = 45 * 800 + base.Lp
    host = np.random.default_rng(4).integers(0, 256, (1, n, 2), dtype=np.uint8)
    ref = _run(base, host, t0=99)
    for sel in ([10, 3, 1, 7, 0], [2, 2, 2, 5, 5, 0, 9, 1, 4, 3, 6, 7, 8, 10, 10], [6], [4, 8]):
        ch = pirip_amd.HipChan(Fs, D, [offsets[i] for i in sel])
        got = _run(ch, host, t0=99)
        for k, i in enumerate(sel):
            assert np.array_equal(got[k].view(np.float64), ref[i].view(np.float64)), (sel, k, i)


@pytest.mark.parametrize("D", [6, 30, 45])
def test_offset_zero_matches_decimator(built_lib, D):
    import torch
    import pirip_amd
    ch = pirip_amd.HipChan(240000 * D // 6, D, [0])
    dec = pirip_amd.HipDecim(D, out_s16=False)
    n = D * 1500 + ch.Lp + 3
    host = np.random.default_rng(D).integers(0, 256, (1, n, 2), dtype=np.uint8)
    got = _run(ch, host)[0]
    dev = torch.from_numpy(host[0].reshape(-1).copy()).cuda()
    no = dec.nout(n)
    assert no == got.shape[0]
    out = torch.zeros(no * 2, dtype=torch.float32, device="cuda")
    dec.batch(dev.data_ptr(), 2 * n, n, out.data_ptr(), no * 8, 1)
    torch.cuda.synchronize()
    want = out.cpu().numpy().astype(np.float64).reshape(no, 2)
    b = chanref.bound(ch.taps())
    assert max(np.abs(got.real - want[:, 0]).max(), np.abs(got.imag - want[:, 1]).max()) <= b


# ---- end to end: one composite wideband capture, K FSK channels ----------------------------------------------------------------------
WIDE_FS, WIDE_D = 2400000, 30
WIDE_OFFSETS = [-875000, -625000, -375000, -125000, 125000, 375000, 625000, 875000]
MODEMS = {
    # rtl_fsk -a 80000 -r 10000: 2-FSK, tones 10 / 20 kHz above each channel's centre
    "2fsk": dict(Fs=80000, Rs=10000, M=2, P=8, f1=10000, shift=10000, est_min=5000, est_max=40000, mask=0),
    # 4-FSK at Rs = 5000 with a known tone spacing (--mask 5000)
    "4fsk": dict(Fs=80000, Rs=5000, M=4, P=8, f1=5000, shift=5000, est_min=2500, est_max=40000, mask=5000),
}


def _composite(mc, nsamp, seed, strong=3, amps=None, bits=None, offsets=WIDE_OFFSETS, Fs=WIDE_FS):
    """u8 [1, nsamp, 2]: one FSK signal per channel, each with its own bits; channel `strong` 20 dB above the others; and the tx bits"""
    rng = np.random.default_rng(seed)
    bps = 1 if mc["M"] == 2 else 2
    nsym = nsamp // (Fs // mc["Rs"]) + 2
    z = np.zeros(nsamp, dtype=np.complex128)
    tx = []
    for c, fc in enumerate(offsets):
        b = rng.integers(0, 2, nsym * bps).astype(np.uint8) if bits is None else bits[c % len(bits)]
        a = (amps[c] if amps else (60.0 if c == strong else 6.0))
        z += chanref.fsk_wideband(Fs, mc["Rs"], mc["M"], fc + mc["f1"], mc["shift"], b, nsamp, a, phase0=rng.uniform(0, 2 * np.pi))
        tx.append(b)
    return chanref.quantise_u8(z)[None], tx


def _demod(mc, nch, s16=False):
    import pirip_amd
    return pirip_amd.HipDemod(mc["Fs"], mc["Rs"], mc["M"], P=mc["P"], est_min=mc["est_min"], est_max=mc["est_max"], mask=mc["mask"],
                              in_format=pirip_amd.IN_CS16 if s16 else pirip_amd.IN_CF32, nstreams=nch)


def _one_shot(dem, d_in, stride, nsamp):
    """one demod_batch over every channel: per channel (bits, rx_filt, stats), frame counts, consumed"""
    import torch
    rows = dem.max_frames_for(nsamp)
    n = dem.nstreams
    bits = torch.zeros((n, rows, dem.Nbits), dtype=torch.uint8, device="cuda")
    filt = torch.zeros((n, rows, dem.M * dem.Nsym), dtype=torch.float32, device="cuda")
    stats = torch.zeros((n, rows, 10), dtype=torch.float32, device="cuda")
    nfr = torch.zeros(n, dtype=torch.int32, device="cuda")
    cons = torch.zeros(n, dtype=torch.int64, device="cuda")
    dem.demod_batch(d_in, stride, nsamp, bits.data_ptr(), rows * dem.Nbits, filt.data_ptr(), rows * dem.M * dem.Nsym, stats.data_ptr(),
                    rows * 10, nfr.data_ptr(), cons.data_ptr(), rows)
    torch.cuda.synchronize()
    nf = nfr.cpu().numpy()
    b, f, s = bits.cpu().numpy(), filt.cpu().numpy(), stats.cpu().numpy()
    return [(b[c, :nf[c]], f[c, :nf[c]], s[c, :nf[c]]) for c in range(n)], nf, cons.cpu().numpy()


def _channelize(ch, dev, stride, n):
    import torch
    no = ch.nout(n)
    bps = ch.bytes_per_sample
    mod = torch.zeros((ch.nchan, no * bps), dtype=torch.uint8, device="cuda")
    ch.batch(dev.data_ptr(), stride, n, mod.data_ptr(), no * bps)
    return mod, no, bps


@pytest.mark.parametrize("modem", list(MODEMS))
def test_end_to_end_channels_decode_their_own_bits(built_lib, modem):
    import torch
    import pirip_amd
    mc = MODEMS[modem]
    nsamp = WIDE_FS // 5                                    # 0.2 s: 2000 symbols per channel at 10 kBd
    host, tx = _composite(mc, nsamp, seed=11)
    dev = torch.from_numpy(host.reshape(-1).copy()).cuda()
    ch = pirip_amd.HipChan(WIDE_FS, WIDE_D, WIDE_OFFSETS)
    mod, no, bps = _channelize(ch, dev, 2 * nsamp, nsamp)
    dem = _demod(mc, len(WIDE_OFFSETS))
    got, nf, _ = _one_shot(dem, mod.data_ptr(), no * bps, no)
    for c in range(len(WIDE_OFFSETS)):
        rx = got[c][0].reshape(-1)
        assert nf[c] >= no // dem.N - 2
        err, nb = chanref.bit_errors(rx, tx[c], skip=2 * dem.Nbits)
        assert nb > 1000 and err == 0, (modem, c, err, nb)


@pytest.mark.parametrize("block_outputs", [1000, 777])
def test_stream_equals_one_shot(built_lib, block_outputs):
    """HipRx(chan=...) block after block: bits, soft magnitudes, statistics, frame counts and consumed samples of the one-shot
    channelizer followed by one demod_batch over the whole recording, bit for bit"""
    import torch
    import pirip_amd
    mc = MODEMS["2fsk"]
    block = WIDE_D * block_outputs
    K = 12
    n_raw = K * block
    host, _ = _composite(mc, n_raw, seed=5)
    dev = torch.from_numpy(host.reshape(-1).copy()).cuda()
    ch = pirip_amd.HipChan(WIDE_FS, WIDE_D, WIDE_OFFSETS)
    mod, no, bps = _channelize(ch, dev, 2 * n_raw, n_raw)
    dem_ref = _demod(mc, len(WIDE_OFFSETS))
    want, nf_want, cons_want = _one_shot(dem_ref, mod.data_ptr(), no * bps, no)
    dem = _demod(mc, len(WIDE_OFFSETS))
    rx = pirip_amd.HipRx(dem, chan=ch, block=block)
    assert rx.ninputs == 1
    R = rx.max_frames
    n = dem.nstreams
    bits = torch.zeros((K, n, R, dem.Nbits), dtype=torch.uint8, device="cuda")
    filt = torch.zeros((K, n, R, dem.M * dem.Nsym), dtype=torch.float32, device="cuda")
    stats = torch.zeros((K, n, R, 10), dtype=torch.float32, device="cuda")
    nfr = torch.zeros((K, n), dtype=torch.int32, device="cuda")
    for k in range(K):
        rx.push(dev.data_ptr() + k * block * 2, 2 * n_raw, bits[k].data_ptr(), R * dem.Nbits, filt[k].data_ptr(), R * dem.M * dem.Nsym,
                d_stats=stats[k].data_ptr(), stats_stride=R * 10, d_nframes=nfr[k].data_ptr())
    torch.cuda.synchronize()
    nf = nfr.cpu().numpy()
    b, f, s = bits.cpu().numpy(), filt.cpu().numpy(), stats.cpu().numpy()
    assert np.array_equal(nf.sum(axis=0), nf_want)
    for c in range(n):
        for arr, w in ((b, want[c][0]), (f, want[c][1]), (s, want[c][2])):
            g = np.concatenate([arr[k, c, :nf[k, c]] for k in range(K)])
            assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), c
    tot, backlog = rx.counters()
    assert np.array_equal(tot, cons_want) and np.array_equal(tot + backlog, np.full(n, no))
    # reset: t0 and the carries start again, the same outputs come out
    rx.reset()
    nfr2 = torch.zeros((K, n), dtype=torch.int32, device="cuda")
    bits2 = torch.zeros_like(bits)
    for k in range(K):
        rx.push(dev.data_ptr() + k * block * 2, 2 * n_raw, bits2[k].data_ptr(), R * dem.Nbits, d_nframes=nfr2[k].data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(nfr2, nfr) and torch.equal(bits2, bits)


# the deployed FSK_LDPC modem (rtl_fsk -a 40000 -r 1000 --code) on four channels of one 240 kS/s capture
LDPC_MODEM = dict(Fs=40000, Rs=1000, M=2, P=10, f1=1000, shift=2000, est_min=500, est_max=15000, mask=0)
LDPC_FS, LDPC_D, LDPC_OFFSETS = 240000, 6, [-90000, -30000, 30001, 90000]


def test_stream_fsk_ldpc_bursts_on_four_channels(built_lib):
    import torch
    import pirip_amd
    burst = sigutil.run_framer(["-m", "2", "--testframes", "3", "--bursts", "1", "--seq", "--source", "0x4", "/dev/zero", "-"])
    gap = np.zeros(40, dtype=np.uint8)
    bits = [np.concatenate([gap[:k * 8 + 8], burst, gap, gap, np.zeros(400, np.uint8)]) for k in range(4)]
    ts_w = LDPC_FS // LDPC_MODEM["Rs"]
    block = LDPC_D * 4000
    K = -(-(max(len(b) for b in bits) * ts_w) // block) + 1
    n_raw = K * block
    host, _ = _composite(LDPC_MODEM, n_raw, seed=8, amps=[20.0, 30.0, 20.0, 25.0], bits=bits, offsets=LDPC_OFFSETS, Fs=LDPC_FS)
    dev = torch.from_numpy(host.reshape(-1).copy()).cuda()
    ch = pirip_amd.HipChan(LDPC_FS, LDPC_D, LDPC_OFFSETS)
    nch = len(LDPC_OFFSETS)

    def handles():
        return _demod(LDPC_MODEM, nch), pirip_amd.HipLdpc(pirip_amd.STANDIN_CODE, 2, nstreams=nch)

    # one shot: channelizer over the whole capture, then one fused FSK_LDPC batch
    mod, no, bps = _channelize(ch, dev, 2 * n_raw, n_raw)
    dm, ld = handles()
    rows = dm.max_frames_for(no)
    nb = ld.data_bytes
    ref = [torch.zeros((nch, rows), dtype=torch.uint8, device="cuda"), torch.zeros((nch, rows, nb), dtype=torch.uint8, device="cuda"),
           torch.zeros((nch, rows, 10), dtype=torch.int32, device="cuda"), torch.zeros((nch, rows, 10), dtype=torch.float32, device="cuda"),
           torch.zeros(nch, dtype=torch.int32, device="cuda"), torch.zeros(nch, dtype=torch.int64, device="cuda")]
    ld.chain_batch(dm, mod.data_ptr(), no * bps, no, ref[0].data_ptr(), ref[1].data_ptr(), ref[2].data_ptr(), ref[4].data_ptr(),
                   ref[5].data_ptr(), rows, d_stats=ref[3].data_ptr(), stats_stride=rows * 10)
    torch.cuda.synchronize()
    nf_want = ref[4].cpu().numpy()
    want = [tuple(a[s, :nf_want[s]].cpu().numpy() for a in ref[:4]) for s in range(nch)]
    for s in range(nch):
        ok = (want[s][0] & pirip_amd.RX_BITS) != 0
        assert ok.sum() == 3, (s, ok.sum())
        assert (want[s][1][ok][:, 0] == 4).all() and sorted(want[s][1][ok][:, 1].tolist()) == sorted(set(want[s][1][ok][:, 1].tolist()))
    # streaming
    dm2, ld2 = handles()
    rx = pirip_amd.HipRx(dm2, ldpc=ld2, chan=ch, block=block)
    R = rx.max_frames
    out = [torch.zeros((K, nch, R), dtype=torch.uint8, device="cuda"), torch.zeros((K, nch, R, nb), dtype=torch.uint8, device="cuda"),
           torch.zeros((K, nch, R, 10), dtype=torch.int32, device="cuda"), torch.zeros((K, nch, R, 10), dtype=torch.float32, device="cuda"),
           torch.zeros((K, nch), dtype=torch.int32, device="cuda")]
    for k in range(K):
        rx.push(dev.data_ptr() + k * block * 2, 2 * n_raw, d_status=out[0][k].data_ptr(), d_payload=out[1][k].data_ptr(),
                d_info=out[2][k].data_ptr(), d_stats=out[3][k].data_ptr(), stats_stride=R * 10, d_nframes=out[4][k].data_ptr())
    torch.cuda.synchronize()
    nf = out[4].cpu().numpy()
    o = [a.cpu().numpy() for a in out[:4]]
    assert np.array_equal(nf.sum(axis=0), nf_want)
    for s in range(nch):
        for i in range(4):
            g = np.concatenate([o[i][k, s, :nf[k, s]] for k in range(K)])
            assert np.array_equal(g.view(np.uint8), want[s][i].view(np.uint8)), (s, i)


def test_bad_arguments(built_lib):
    import pirip_amd

    def bad(fn, *a, **kw):
        with pytest.raises(pirip_amd.PiripError, match=r"\(-1\)"):
            fn(*a, **kw)

    C = pirip_amd.HipChan
    bad(C, 2400000, 30, [1200000])                      # offset at +Fs/2
    bad(C, 2400000, 30, [-1200000])                     # offset at -Fs/2
    bad(C, 2400000, 30, [0, 5], inputs=[0, -1])         # chan_input out of range
    bad(C, 2400000, 30, [])                             # no channels
    bad(C, 2400000, 0, [0])                             # D < 1
    C(2400000, 30, [1199999, -1199999]).close()         # (just inside is fine)
    mc = MODEMS["2fsk"]
    ch = C(WIDE_FS, WIDE_D, WIDE_OFFSETS)
    bad(pirip_amd.HipRx, _demod(mc, 7), chan=ch, block=WIDE_D * 1000)                 # nstreams != nchan
    bad(pirip_amd.HipRx, _demod(mc, 8, s16=True), chan=ch, block=WIDE_D * 1000)       # s16 demodulator, complex-float channelizer
    bad(pirip_amd.HipRx, _demod(mc, 8), chan=ch, block=WIDE_D * 1000 + 1)             # block % D != 0
    bad(pirip_amd.HipRx, _demod(mc, 8), chan=C(WIDE_FS, WIDE_D, WIDE_OFFSETS, out_s16=True), block=WIDE_D * 1000)   # s16 out, cf32 in
    with pytest.raises(ValueError):
        pirip_amd.HipRx(_demod(mc, 8), dec=pirip_amd.HipDecim(WIDE_D, out_s16=False), chan=ch, block=WIDE_D * 1000)
    pirip_amd.HipRx(_demod(mc, 8), chan=ch, block=WIDE_D * 1000).close()
    pirip_amd.HipRx(_demod(mc, 8, s16=True), chan=C(WIDE_FS, WIDE_D, WIDE_OFFSETS, out_s16=True), block=WIDE_D * 1000).close()


# ---- the CLI: rtl_fsk_channels writes what the Python HipRx path computes ------------------------------------------------------------
def _rx_files(ch, dem, host, block, ldpc=None):
    """per channel: the bytes rtl_fsk_channels writes (bits one per byte, or with ldpc the payload of every CRC-ok frame)"""
    import torch
    import pirip_amd
    n_raw = host.shape[1]
    dev = torch.from_numpy(host.reshape(-1).copy()).cuda()
    rx = pirip_amd.HipRx(dem, ldpc=ldpc, chan=ch, block=block)
    R = rx.max_frames
    n = dem.nstreams
    outs = [bytearray() for _ in range(n)]
    nb = ldpc.data_bytes if ldpc is not None else 0
    for k in range(n_raw // block):
        nfr = torch.zeros(n, dtype=torch.int32, device="cuda")
        if ldpc is None:
            bits = torch.zeros((n, R, dem.Nbits), dtype=torch.uint8, device="cuda")
            rx.push(dev.data_ptr() + k * block * 2, 2 * n_raw, bits.data_ptr(), R * dem.Nbits, d_nframes=nfr.data_ptr())
            torch.cuda.synchronize()
            b, nf = bits.cpu().numpy(), nfr.cpu().numpy()
            for c in range(n):
                outs[c] += b[c, :nf[c]].tobytes()
        else:
            st = torch.zeros((n, R), dtype=torch.uint8, device="cuda")
            pl = torch.zeros((n, R, nb), dtype=torch.uint8, device="cuda")
            info = torch.zeros((n, R, 10), dtype=torch.int32, device="cuda")
            rx.push(dev.data_ptr() + k * block * 2, 2 * n_raw, d_status=st.data_ptr(), d_payload=pl.data_ptr(), d_info=info.data_ptr(),
                    d_nframes=nfr.data_ptr())
            torch.cuda.synchronize()
            s, p, nf = st.cpu().numpy(), pl.cpu().numpy(), nfr.cpu().numpy()
            for c in range(n):
                for f in range(nf[c]):
                    if s[c, f] & pirip_amd.RX_BITS:
                        outs[c] += p[c, f].tobytes()
    return [bytes(o) for o in outs]


@pytest.mark.parametrize("coded", [False, True])
def test_rtl_fsk_channels_cli_equals_python(built_lib, tmp_path, coded):
    import pirip_amd
    if coded:
        mc, Fs, D, offs = LDPC_MODEM, LDPC_FS, LDPC_D, LDPC_OFFSETS
        burst = sigutil.run_framer(["-m", "2", "--testframes", "3", "--bursts", "1", "--seq", "--source", "0x4", "/dev/zero", "-"])
        bits = [np.concatenate([np.zeros(8 * k + 8, np.uint8), burst, np.zeros(480, np.uint8)]) for k in range(4)]
        n_raw = (max(len(b) for b in bits) + 200) * (Fs // mc["Rs"])
        host, _ = _composite(mc, n_raw, seed=2, amps=[20.0, 30.0, 20.0, 25.0], bits=bits, offsets=offs, Fs=Fs)
    else:
        mc, Fs, D, offs = MODEMS["2fsk"], WIDE_FS, WIDE_D, WIDE_OFFSETS
        n_raw = Fs + Fs // 10
        host, _ = _composite(mc, n_raw, seed=9)
    iq = tmp_path / "wide.iq"
    host.reshape(-1).tofile(iq)
    prefix = str(tmp_path / "ch")
    cmd = [os.path.join(BIN, "rtl_fsk_channels"), "-s", str(Fs), "-a", str(mc["Fs"]), "-r", str(mc["Rs"]), "-c", ",".join(map(str, offs)),
           "-i", str(iq), "-o", prefix, "-q"]
    if coded:
        cmd += ["--code", pirip_amd.STANDIN_CODE]
    p = subprocess.run(cmd, capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()
    # the tool's block and modem settings, restated: Fs / 4 wideband samples per call rounded down to D, P as rtl_fsk picks it
    block = (Fs // 4) // D * D
    ch = pirip_amd.HipChan(Fs, D, offs)
    dem = _demod(dict(mc, est_min=mc["Rs"] // 2, est_max=mc["Fs"] // 2), len(offs))
    ldpc = pirip_amd.HipLdpc(pirip_amd.STANDIN_CODE, mc["M"], nstreams=len(offs)) if coded else None
    want = _rx_files(ch, dem, host[:, :n_raw // block * block], block, ldpc)
    for c in range(len(offs)):
        got = open(f"{prefix}.{c}", "rb").read()
        assert got == want[c], (c, len(got), len(want[c]))
        assert len(got) > (0 if not coded else 3 * 32 - 1)
