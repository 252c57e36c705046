"""include/pirip_hip.h section G: the streaming receiver (pirip_hip_rx_*, pirip_amd.HipRx).

A recording of many live channels -- each with its own timing offset and sample-clock error, so that every channel follows its own nin
sequence -- is fed block after block through the receiver and compared, bit for bit, with ONE batch call over the whole recording: same
kernels, same samples, same carried state, so bits, soft magnitudes, statistics rows, frame counts and consumed samples must be equal."""
import numpy as np
import pytest

import sigutil

pytestmark = pytest.mark.gpu


# rtl_fsk -r 1000 at 240 kS/s (the block kernel's Ts = 240 / Ndft = 4096 shape)
CFG_R1000 = dict(Fs=240000, Rs=1000, M=2, P=15, f1=11000, shift=2000, est_min=500, est_max=119000)
# rtl_fsk -a 40000 -r 1000 after the /6 front end: complex float, Ts = 40 (the services' modem)
CFG_TS40 = dict(Fs=40000, Rs=1000, M=2, P=10, f1=1000, shift=2000, est_min=500, est_max=15000)


def _channels(oracle, c, nch, nsamp, fmt, seed, noisy_db=8.0, ppm_max=1500.0, nbase=4, bits=None, tx_cfg=None):
    """[nch, nsamp, 2] samples: nbase modulated waveforms, channel s resampled at its own clock error (ppm) from its own start
    offset; every odd channel with AWGN at noisy_db. fmt: 'u8' (u8 IQ), 'cf32', 's16'."""
    tx = tx_cfg or c
    rng = np.random.default_rng(seed)
    ts = tx["Fs"] // tx["Rs"]
    need = int(nsamp * (1 + ppm_max * 1e-6)) + 4 * ts + 8
    nb = need // ts + 2
    nb *= 1 if tx["M"] == 2 else 2
    base = []
    for b in range(nbase):
        if bits is None:
            bb = rng.integers(0, 2, nb).astype(np.uint8)
        else:
            bb = np.resize(bits[b % len(bits)], nb) if len(bits[b % len(bits)]) < nb else bits[b % len(bits)]
        x = sigutil.mod_complex(oracle, tx, bb)
        if x.shape[0] < need:
            x = np.concatenate([x, np.zeros((need - x.shape[0], 2), np.float32)])
        base.append(x.astype(np.float64))
    ppm = np.linspace(-ppm_max, ppm_max, nch)
    out = np.zeros((nch, nsamp, 2), dtype={"u8": np.uint8, "cf32": np.float32, "s16": np.int16}[fmt])
    g = np.arange(need, dtype=np.float64)
    for s in range(nch):
        x = base[s % nbase]
        t = (s * 7 % ts) + 0.37 * s / nch + np.arange(nsamp) * (1.0 + ppm[s] * 1e-6)
        y = np.stack([np.interp(t, g, x[:need, 0]), np.interp(t, g, x[:need, 1])], axis=1).astype(np.float32)
        if noisy_db is not None and s % 2 == 1:
            y = sigutil.add_awgn(y, noisy_db, tx, rng)
        if fmt == "u8":
            out[s] = oracle.quantise_cu8(y, amp=20.0)
        elif fmt == "cf32":
            out[s] = y * np.float32(0.37)
        else:
            out[s] = np.clip(np.rint(y * 300.0), -32768, 32767)
    return out


def _demod(c, nch, fmt, **kw):
    import pirip_amd
    inf = {"u8": pirip_amd.IN_CU8_FSKDEMOD, "cf32": pirip_amd.IN_CF32, "s16": pirip_amd.IN_CS16}[fmt]
    return pirip_amd.HipDemod(c["Fs"], c["Rs"], c["M"], P=c["P"], est_min=c["est_min"], est_max=c["est_max"], in_format=inf, nstreams=nch, **kw)


def _outputs(dem, rows, calls=1):
    import torch
    n = dem.nstreams
    return (torch.zeros((calls, n, rows, dem.Nbits), dtype=torch.uint8, device="cuda"),
            torch.zeros((calls, n, rows, dem.M * dem.Nsym), dtype=torch.float32, device="cuda"),
            torch.zeros((calls, n, rows, 10), dtype=torch.float32, device="cuda"),
            torch.zeros((calls, n), dtype=torch.int32, device="cuda"))


def _gather(bits, filt, stats, nfr):
    """per channel: (bits, rx_filt, stats) of every call's valid rows, concatenated in call order"""
    b, f, s, n = bits.cpu().numpy(), filt.cpu().numpy(), stats.cpu().numpy(), nfr.cpu().numpy()
    out = []
    for ch in range(b.shape[1]):
        out.append(tuple(np.concatenate([a[k, ch, :n[k, ch]] for k in range(b.shape[0])]) for a in (b, f, s)))
    return out, n.sum(axis=0)


def _one_shot(dem, d_in, stride, nsamp):
    import torch
    rows = dem.max_frames_for(nsamp)
    bits, filt, stats, nfr = _outputs(dem, rows)
    cons = torch.zeros(dem.nstreams, dtype=torch.int64, device="cuda")
    dem.demod_batch(d_in, stride, nsamp, bits.data_ptr(), rows * dem.Nbits, filt.data_ptr(), rows * dem.M * dem.Nsym, stats.data_ptr(), rows * 10,
                    nfr.data_ptr(), cons.data_ptr(), rows)
    torch.cuda.synchronize()
    got, nf = _gather(bits, filt, stats, nfr)
    return got, nf, cons.cpu().numpy()


def _stream(rx, dem, d_in, stride, K, block, bps):
    """K blocks through rx.push (block k of channel s at d_in + s * stride + k * block * bps): no synchronisation until the end"""
    import torch
    R = rx.max_frames
    bits, filt, stats, nfr = _outputs(dem, R, K)
    for k in range(K):
        rx.push(d_in + k * block * bps, stride, bits[k].data_ptr(), R * dem.Nbits, filt[k].data_ptr(), R * dem.M * dem.Nsym,
                d_stats=stats[k].data_ptr(), stats_stride=R * 10, d_nframes=nfr[k].data_ptr())
    torch.cuda.synchronize()
    return _gather(bits, filt, stats, nfr)


def _assert_equal(got, want, nf_got, nf_want):
    assert np.array_equal(nf_got, nf_want), (nf_got, nf_want)
    for s, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g[0], w[0]), ("bits", s)
        assert np.array_equal(g[1].view(np.uint32), w[1].view(np.uint32)), ("rx_filt", s)
        assert np.array_equal(g[2].view(np.uint32), w[2].view(np.uint32)), ("stats", s)


SHAPES = {
    "cfg1_wave": (sigutil.CFG1, "u8", "wave", 64, 50),
    "cfg4_wave": (sigutil.CFG4, "u8", "wave", 64, 50),
    "r1000_block": (CFG_R1000, "u8", "block", 64, 42),
    "cfg1_general": (sigutil.CFG1, "u8", "general", 64, 42),
}


@pytest.mark.parametrize("blockname", ["min", "3N+17", "odd_large"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_stream_equals_one_shot(oracle, built_lib, monkeypatch, shape, blockname):
    import torch
    import pirip_amd
    c, fmt, kernel, nch, frames = SHAPES[shape]
    if kernel == "general":
        monkeypatch.setenv("PIRIP_FORCE_GENERAL", "1")
    dem_ref = _demod(c, nch, fmt)
    assert dem_ref.kernel() == kernel, dem_ref.kernel_name()
    N, nin_max = dem_ref.N, dem_ref.info.nin_max
    block = {"min": nin_max, "3N+17": 3 * N + 17, "odd_large": 7 * N + 331}[blockname]
    K = -(-frames * N // block)
    nsamp = K * block
    host = _channels(oracle, c, nch, nsamp, fmt, seed=sorted(SHAPES).index(shape))
    dev = torch.from_numpy(host).cuda()
    bps = host.itemsize * 2
    want, nf_want, cons_want = _one_shot(dem_ref, dev.data_ptr(), nsamp * bps, nsamp)
    assert nf_want.min() >= frames - 2
    dem = _demod(c, nch, fmt)
    rx = pirip_amd.HipRx(dem, block=block)
    got, nf_got = _stream(rx, dem, dev.data_ptr(), nsamp * bps, K, block, bps)
    tot, backlog = rx.counters()
    _assert_equal(got, want, nf_got, nf_want)
    assert np.array_equal(tot, cons_want)
    assert np.array_equal(tot + backlog, np.full(nch, nsamp)) and (backlog < nin_max).all()
    assert len(set(map(tuple, (s[2][:, 6] for s in want)))) > nch // 4, "the channels should follow their own nin sequences"


def test_stream_equals_one_shot_exact_kernel(oracle, built_lib, monkeypatch):
    import torch
    import pirip_amd
    monkeypatch.setenv("PIRIP_KERNEL", "exact")
    c, nch = sigutil.CFG1, 4
    dem_ref = _demod(c, nch, "u8")
    assert dem_ref.kernel() == "exact"
    block = 3 * dem_ref.N + 17
    K = 4
    nsamp = K * block
    host = _channels(oracle, c, nch, nsamp, "u8", seed=5)
    dev = torch.from_numpy(host).cuda()
    want, nf_want, cons_want = _one_shot(dem_ref, dev.data_ptr(), nsamp * 2, nsamp)
    dem = _demod(c, nch, "u8")
    rx = pirip_amd.HipRx(dem, block=block)
    got, nf_got = _stream(rx, dem, dev.data_ptr(), nsamp * 2, K, block, 2)
    _assert_equal(got, want, nf_got, nf_want)
    assert np.array_equal(rx.counters()[0], cons_want)


def test_stream_backlog_stays_below_nin_max(oracle, built_lib):
    import torch
    import pirip_amd
    c, nch, K = sigutil.CFG1, 16, 300
    dem = _demod(c, nch, "u8")
    nin_max = dem.info.nin_max
    block = nin_max                                        # the smallest block: the carries are largest relative to it
    host = _channels(oracle, c, nch, K * block, "u8", seed=11, ppm_max=3000.0)
    dev = torch.from_numpy(host).cuda()
    rx = pirip_amd.HipRx(dem, block=block)
    R = rx.max_frames
    bits, filt, stats, nfr = _outputs(dem, R)
    seen = set()
    for k in range(K):
        rx.push(dev.data_ptr() + k * block * 2, K * block * 2, bits[0].data_ptr(), R * dem.Nbits, d_nframes=nfr[0].data_ptr())
        tot, backlog = rx.counters()
        assert (backlog >= 0).all() and (backlog < nin_max).all(), (k, backlog)
        assert np.array_equal(tot + backlog, np.full(nch, (k + 1) * block)), k
        seen.update(backlog.tolist())
    assert len(seen) > 10


FRONT_ENDS = {
    # u8 IQ at 240 kS/s, /6 -> complex float -> Ts = 40 (rtl_fsk -a 40000 -r 1000)
    "div6_cf32": (6, False, CFG_TS40, "cf32", dict(CFG_TS40, Fs=240000, P=10), 16, 44, 0.05, None),
    # config 3: u8 IQ at 1.8 MS/s, /45 -> s16 -> Ts = 40 (the README.md:109 pipe)
    "div45_s16": (45, True, sigutil.CFG3, "s16", dict(sigutil.CFG3, Fs=1800000), 6, 41, 0.05, None),
}
# The receiver sizes its rows from the decimator's padded filter length Lp, D and output format: the shapes where a wrong one would
# show. D = 1 (every input sample is an output), and both paddings -- csdr's filter length L is always odd, so Lp == L does not occur:
# transition_bw 0.05 gives L = 79, Lp = L + 1, and 0.0975 gives L = 41, Lp = L + 3 -- for both output formats; a block of 4096 samples,
# three pushes.
FRONT_ENDS.update({f"div1_{fmt}_L{L}": (1, s16, sigutil.CFG1, fmt, sigutil.CFG1, 4, 10, tbw, (4096, 3))
                   for fmt, s16 in (("cf32", False), ("s16", True)) for tbw, L in ((0.05, 79), (0.0975, 41))})


@pytest.mark.parametrize("front", list(FRONT_ENDS))
def test_stream_front_end_equals_decimator_then_demod(oracle, built_lib, front):
    import torch
    import pirip_amd
    D, out_s16, c, fmt, tx, nch, frames, tbw, fixed = FRONT_ENDS[front]
    dec = pirip_amd.HipDecim(D, transition_bw=tbw, out_s16=out_s16)
    dem_ref = _demod(c, nch, fmt)
    N = dem_ref.N
    block, K = fixed or (D * (N + 301), -(-frames * N // (N + 301)))
    n_raw = K * block
    host = _channels(oracle, c, nch, n_raw, "u8", seed=D, tx_cfg=tx, nbase=2)
    dev = torch.from_numpy(host).cuda()
    # reference: the decimator over the whole recording in one buffer, then one batch call
    n_mod = dec.nout(n_raw)
    bps = 4 if out_s16 else 8
    mod = torch.zeros((nch, n_mod * bps), dtype=torch.uint8, device="cuda")
    dec.batch(dev.data_ptr(), n_raw * 2, n_raw, mod.data_ptr(), n_mod * bps, nch)
    want, nf_want, cons_want = _one_shot(dem_ref, mod.data_ptr(), n_mod * bps, n_mod)
    assert nf_want.min() >= frames - 3
    dem = _demod(c, nch, fmt)
    rx = pirip_amd.HipRx(dem, dec=dec, block=block)
    got, nf_got = _stream(rx, dem, dev.data_ptr(), n_raw * 2, K, block, 2)
    tot, backlog = rx.counters()
    _assert_equal(got, want, nf_got, nf_want)
    assert np.array_equal(tot, cons_want) and np.array_equal(tot + backlog, np.full(nch, n_mod))


def _bursts(M):
    """framer output (preamble, unique word, codeword) behind gaps of different lengths, one per base waveform (repeated to length)"""
    b = sigutil.run_framer(["-m", str(M), "--testframes", "3", "--bursts", "1", "--seq", "--source", "0x4", "/dev/zero", "-"])
    gap = np.zeros(40 * (1 if M == 2 else 2), dtype=np.uint8)
    return [np.concatenate([gap[:k * 8 + 8], b, gap, gap]) for k in range(4)]


CHAINS = {
    # config 4: 4-FSK, Ts = 24 / P = 8, u8 IQ of fsk_demod -d; ~3.5 dB Eb/N0 on the noisy half (near the stand-in code's FER knee)
    "cfg4": (None, sigutil.CFG4, "u8", sigutil.CFG4, 16, 3.5, 2400),
    # the deployed chain: u8 at 240 kS/s /6 -> complex float, 2-FSK Rs = 1000, P = 10
    "div6": (6, CFG_TS40, "cf32", dict(CFG_TS40, Fs=240000, P=10), 8, 5.0, 6 * 2000 + 6 * 77),
}


@pytest.mark.parametrize("split", [None, "2"])
@pytest.mark.parametrize("chain", list(CHAINS))
def test_stream_fsk_ldpc_records_equal_one_shot(oracle, built_lib, monkeypatch, chain, split):
    import torch
    import pirip_amd
    D, c, fmt, tx, nch, ebno, block = CHAINS[chain]
    if split:
        monkeypatch.setenv("PIRIP_CHAIN_SPLIT_MIN", split)
    M = c["M"]
    Ts = tx["Fs"] // tx["Rs"]
    bits = _bursts(M)
    per_call = 50 * Ts
    ncalls_total = max((len(bits[0]) // (1 if M == 2 else 2)) // 50 + 4, 60)
    K = -(-ncalls_total * per_call // block)
    n_in = K * block
    host = _channels(oracle, c, nch, n_in, "u8" if D else fmt, seed=31, noisy_db=ebno, ppm_max=300.0, bits=bits, tx_cfg=tx)
    dev = torch.from_numpy(host).cuda()
    dec = pirip_amd.HipDecim(D, out_s16=False) if D else None

    def handles():
        dm = _demod(c, nch, fmt)
        return dm, pirip_amd.HipLdpc(pirip_amd.STANDIN_CODE, M, nstreams=nch)

    # one batch over the whole recording (after the decimator over all of it in one buffer)
    dm, ld = handles()
    if dec:
        n_mod = dec.nout(n_in)
        mod = torch.zeros((nch, n_mod * 8), dtype=torch.uint8, device="cuda")
        dec.batch(dev.data_ptr(), n_in * 2, n_in, mod.data_ptr(), n_mod * 8, nch)
        src, stride, nsamp = mod.data_ptr(), n_mod * 8, n_mod
    else:
        src, stride, nsamp = dev.data_ptr(), n_in * 2, n_in
    rows = dm.max_frames_for(nsamp)
    nb = ld.data_bytes
    ref = [torch.zeros((nch, rows), dtype=torch.uint8, device="cuda"), torch.zeros((nch, rows, nb), dtype=torch.uint8, device="cuda"),
           torch.zeros((nch, rows, 10), dtype=torch.int32, device="cuda"), torch.zeros((nch, rows, 10), dtype=torch.float32, device="cuda"),
           torch.zeros(nch, dtype=torch.int32, device="cuda"), torch.zeros(nch, dtype=torch.int64, device="cuda")]
    ld.chain_batch(dm, src, stride, nsamp, ref[0].data_ptr(), ref[1].data_ptr(), ref[2].data_ptr(), ref[4].data_ptr(), ref[5].data_ptr(), rows,
                   d_stats=ref[3].data_ptr(), stats_stride=rows * 10)
    torch.cuda.synchronize()
    assert ld.last_path_fused()
    nf_want = ref[4].cpu().numpy()
    want = [tuple(a[s, :nf_want[s]].cpu().numpy() for a in ref[:4]) for s in range(nch)]
    assert sum(((w[0] & pirip_amd.RX_BITS) != 0).sum() for w in want) > 0, "some frames should decode"
    # the streaming receiver, block after block
    dm2, ld2 = handles()
    rx = pirip_amd.HipRx(dm2, ldpc=ld2, dec=dec, block=block)
    R = rx.max_frames
    out = [torch.zeros((K, nch, R), dtype=torch.uint8, device="cuda"), torch.zeros((K, nch, R, nb), dtype=torch.uint8, device="cuda"),
           torch.zeros((K, nch, R, 10), dtype=torch.int32, device="cuda"), torch.zeros((K, nch, R, 10), dtype=torch.float32, device="cuda"),
           torch.zeros((K, nch), dtype=torch.int32, device="cuda")]
    bps = 2 if (D or fmt == "u8") else 8
    for k in range(K):
        rx.push(dev.data_ptr() + k * block * bps, n_in * bps, d_status=out[0][k].data_ptr(), d_payload=out[1][k].data_ptr(),
                d_info=out[2][k].data_ptr(), d_stats=out[3][k].data_ptr(), stats_stride=R * 10, d_nframes=out[4][k].data_ptr())
    torch.cuda.synchronize()
    assert ld2.last_path_fused()
    nf = out[4].cpu().numpy()
    o = [a.cpu().numpy() for a in out[:4]]
    assert np.array_equal(nf.sum(axis=0), nf_want)
    for k in range(K):
        for s in range(nch):
            assert not o[0][k, s, nf[k, s]:].any() and (o[2][k, s, nf[k, s]:] == -1).all()
    for s in range(nch):
        for i in range(4):
            g = np.concatenate([o[i][k, s, :nf[k, s]] for k in range(K)])
            assert np.array_equal(g.view(np.uint8), want[s][i].view(np.uint8)), (s, i)
    assert np.array_equal(rx.counters()[0], ref[5].cpu().numpy())


def test_stream_process_does_not_synchronise(oracle, built_lib):
    import torch
    import pirip_amd
    if not hasattr(torch.cuda, "_sleep"):
        pytest.skip("torch.cuda._sleep is not available")
    c, nch = sigutil.CFG1, 8
    dem = _demod(c, nch, "u8")
    block = 3 * dem.N + 17
    host = _channels(oracle, c, nch, 3 * block, "u8", seed=3)
    dev = torch.from_numpy(host).cuda()
    stride = 3 * block * 2
    # three synchronised calls
    rx = pirip_amd.HipRx(dem, block=block)
    R = rx.max_frames
    want = _outputs(dem, R, 3)
    for k in range(3):
        rx.push(dev.data_ptr() + k * block * 2, stride, want[0][k].data_ptr(), R * dem.Nbits, want[1][k].data_ptr(), R * dem.M * dem.Nsym,
                d_stats=want[2][k].data_ptr(), stats_stride=R * 10, d_nframes=want[3][k].data_ptr())
        torch.cuda.synchronize()
    # the same three calls back to back behind a spin kernel, synchronised once
    dem2 = _demod(c, nch, "u8")
    rx2 = pirip_amd.HipRx(dem2, block=block)
    got = _outputs(dem2, R, 3)
    stream = torch.cuda.current_stream()
    torch.cuda.synchronize()
    torch.cuda._sleep(200_000_000)                         # ~0.1 s of spinning on the stream
    rx2.push(dev.data_ptr(), stride, got[0][0].data_ptr(), R * dem.Nbits, got[1][0].data_ptr(), R * dem.M * dem.Nsym,
             d_stats=got[2][0].data_ptr(), stats_stride=R * 10, d_nframes=got[3][0].data_ptr(), stream=stream.cuda_stream)
    assert not stream.query(), "pirip_hip_rx_push returned only after the work queued before it had finished"
    for k in (1, 2):
        rx2.push(dev.data_ptr() + k * block * 2, stride, got[0][k].data_ptr(), R * dem.Nbits, got[1][k].data_ptr(), R * dem.M * dem.Nsym,
                 d_stats=got[2][k].data_ptr(), stats_stride=R * 10, d_nframes=got[3][k].data_ptr(), stream=stream.cuda_stream)
    assert not stream.query()
    torch.cuda.synchronize()
    for a, b in zip(got, want):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_stream_zero_copy_process_equals_push(oracle, built_lib):
    """blocks written straight into pirip_hip_rx_input's landing zone (here by the device-side synthesiser), then process():
    the same outputs as push() from a buffer holding the same samples"""
    import torch
    import pirip_amd
    c, nch, K = sigutil.CFG1, 8, 6
    dem = _demod(c, nch, "u8")
    block = 2 * dem.N + 99
    rx = pirip_amd.HipRx(dem, block=block)
    R = rx.max_frames
    d_block, in_stride = rx.input()
    assert in_stride % 256 == 0 and d_block % 256 == 0
    # the whole recording, synthesised once into a plain buffer; the receiver's input gets each block the same way
    nsym = K * block // 24 + 2
    tx_bits = torch.from_numpy(np.random.default_rng(2).integers(0, 2, (nch, nsym)).astype(np.uint8)).cuda()
    full = torch.zeros((nch, K * block * 2), dtype=torch.uint8, device="cuda")
    f1 = [10000 + 50 * s for s in range(nch)]
    pirip_amd.binding.synth_cu8(c["Fs"], c["Rs"], c["M"], f1, 10000, tx_bits.data_ptr(), nsym, nsym, full.data_ptr(), K * block * 2, K * block,
                                amp=20.0, skip=[3 * s for s in range(nch)])
    got = _outputs(dem, R, K)
    for k in range(K):
        # (the synthesiser writes samples [k block, (k + 1) block) of each channel when it drops k block leading samples)
        pirip_amd.binding.synth_cu8(c["Fs"], c["Rs"], c["M"], f1, 10000, tx_bits.data_ptr(), nsym, nsym, d_block, in_stride, block,
                                    amp=20.0, skip=[3 * s + k * block for s in range(nch)])
        rx.process(got[0][k].data_ptr(), R * dem.Nbits, got[1][k].data_ptr(), R * dem.M * dem.Nsym, d_stats=got[2][k].data_ptr(),
                   stats_stride=R * 10, d_nframes=got[3][k].data_ptr())
    torch.cuda.synchronize()
    dem2 = _demod(c, nch, "u8")
    rx2 = pirip_amd.HipRx(dem2, block=block)
    want = _outputs(dem2, R, K)
    for k in range(K):
        rx2.push(full.data_ptr() + k * block * 2, K * block * 2, want[0][k].data_ptr(), R * dem.Nbits, want[1][k].data_ptr(), R * dem.M * dem.Nsym,
                 d_stats=want[2][k].data_ptr(), stats_stride=R * 10, d_nframes=want[3][k].data_ptr())
    torch.cuda.synchronize()
    assert int(want[3].sum()) > 0
    for a, b in zip(got, want):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_stream_reset_and_bad_arguments(oracle, built_lib):
    import torch
    import pirip_amd
    c, nch, K = sigutil.CFG1, 8, 5
    dem = _demod(c, nch, "u8")
    block = 3 * dem.N + 17
    host = _channels(oracle, c, nch, K * block, "u8", seed=21)
    dev = torch.from_numpy(host).cuda()
    rx = pirip_amd.HipRx(dem, block=block)
    first = _stream(rx, dem, dev.data_ptr(), K * block * 2, K, block, 2)
    rx.reset()
    assert not rx.counters()[0].any() and not rx.counters()[1].any()
    again = _stream(rx, dem, dev.data_ptr(), K * block * 2, K, block, 2)
    dem2 = _demod(c, nch, "u8")
    fresh = _stream(pirip_amd.HipRx(dem2, block=block), dem2, dev.data_ptr(), K * block * 2, K, block, 2)
    _assert_equal(again[0], fresh[0], again[1], fresh[1])
    _assert_equal(first[0], fresh[0], first[1], fresh[1])

    def bad(**kw):
        with pytest.raises(pirip_amd.PiripError, match=r"\(-1\)"):
            pirip_amd.HipRx(**kw)

    nin_max = dem.info.nin_max
    bad(dem=dem, block=nin_max - 1)                                          # below the minimum
    pirip_amd.HipRx(dem, block=nin_max).close()                              # (the minimum itself is fine)
    dem40 = _demod(CFG_TS40, nch, "cf32")
    dec6 = pirip_amd.HipDecim(6, out_s16=False)
    bad(dem=dem40, dec=dec6, block=6 * 3000 + 1)                             # block % D != 0
    bad(dem=dem40, dec=dec6, block=6 * 300)                                  # fewer than nin_max new samples per call
    bad(dem=dem40, dec=pirip_amd.HipDecim(6, out_s16=True), block=6 * 3000)  # s16 out, complex-float demodulator
    bad(dem=dem, dec=dec6, block=6 * 3000)                                   # a u8 demodulator behind a decimator
    pirip_amd.HipRx(dem40, dec=dec6, block=6 * 3000).close()
    code = pirip_amd.STANDIN_CODE
    bad(dem=dem, ldpc=pirip_amd.HipLdpc(code, 2, nstreams=nch + 1), block=block)   # nstreams
    bad(dem=dem, ldpc=pirip_amd.HipLdpc(code, 4, nstreams=nch), block=block)       # M
    bad(dem=dem, ldpc=pirip_amd.HipLdpc(code, 2, Nsym=100, nstreams=nch), block=block)   # Nsym
    pirip_amd.HipRx(dem, ldpc=pirip_amd.HipLdpc(code, 2, nstreams=nch), block=block).close()
