"""FSK_LDPC transmit on the device (include/pirip_hip.h section I): the framer against fsk_ldpc_framer byte for byte,
the modulator against its float64 statement (tests/txref.py), split calls, the float recursion, loopback into the receive chain, the CLI, the repeater's
record conversion against a replay of tx/frame_repeater.c."""
import os
import subprocess

import numpy as np
import pytest

import sigutil
import txref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "pirip_amd", "bin")
CODE = os.path.join(ROOT, "pirip_amd", "data", "standin_256_512_4.code")
RX_SYNC, RX_BITS = 2, 4
OFF = txref.OFF

# (Fs, Rs, M, first tones of the streams, shift): tones off the Fs / Ts grid so that the phases spread over the circle
# (tests/test_tx_cpu.py checks that the float64 formula alone meets few rounding ties on them)
MOD_SHAPES = [
    (240000, 10000, 2, [10037, 10000 + 137 * 3, 20011, -30000 + 41], 10000),
    (240000, 10000, 4, [10037, 9973, 50021, 12345], 10000),
    (100000, 10000, 2, [7001, 12007, 9413, 30011], 10000),          # Ts = 10: blocks of odd symbol counts are not 16-byte aligned
]


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [None, "rician"])
@pytest.mark.parametrize("M", [2, 4])
def test_framer_equals_fsk_ldpc_framer_byte_for_byte(built_lib, tmp_path, M, variant):
    import torch
    import pirip_amd
    code = CODE if variant is None else sigutil.code_variant(CODE, tmp_path, variant)
    rng = np.random.default_rng(100 + M)
    B, bps = 7, (1 if M == 2 else 2)
    lead = [0, 3, 10, 0, 65, 1, 130]
    gap = [40, 0, 7, 129, 64, 1, 300]
    tx = pirip_amd.HipTx(code, 240000, 10000, M, nstreams=B, f1=10000, shift=10000, lead=lead, gap=gap)
    kb = tx.data_bytes
    plans = [txref.burst_plan(rng, 1 + s % 4, 1 + (s * 5) % 7) for s in range(B)]
    plans[3] = [0, 1, 2, 2, 0, 7, 1, 0, 2]                           # a frame before any preamble, two ends in a row, an unknown control byte
    plans[5] = txref.burst_plan(rng, 30, 3)                          # more than 64 records: several rounds of the layout scan
    recs = [txref.records(rng, p, kb) for p in plans]
    max_rec = max(len(p) for p in plans)
    host = np.zeros((B, max_rec + 2, 1 + kb), dtype=np.uint8)
    host[:] = 1                                                      # records behind a stream's count must not be read as records
    for s in range(B):
        host[s, :len(plans[s])] = recs[s]
    nrec = np.array([len(p) for p in plans], dtype=np.int32)
    cap = tx.max_syms(max_rec)
    d_rec = torch.from_numpy(host).cuda()
    d_nrec = torch.from_numpy(nrec).cuda()
    syms = torch.full((B, cap + 5), 0xAA, dtype=torch.uint8, device="cuda")
    bits = torch.full((B, (cap + 5) * bps), 0xAA, dtype=torch.uint8, device="cuda")
    nsym = torch.zeros(B, dtype=torch.int32, device="cuda")
    tx.frame(d_rec.data_ptr(), host[0].size, max_rec, syms.data_ptr(), cap + 5, cap, d_nrec=d_nrec.data_ptr(), d_nsym=nsym.data_ptr(),
             d_bits=bits.data_ptr(), bits_stride=(cap + 5) * bps)
    torch.cuda.synchronize()
    syms, bits, nsym = syms.cpu().numpy(), bits.cpu().numpy(), nsym.cpu().numpy()
    for s in range(B):
        want = sigutil.run_framer(["-m", str(M), "--packed", "--gap", str(gap[s] * bps), "-", "-"], recs[s].tobytes(), code)
        want = np.concatenate([np.zeros(lead[s] * bps, dtype=np.uint8), want])
        assert nsym[s] * bps == want.size, (s, nsym[s], want.size)
        assert np.array_equal(bits[s, :want.size], want), s                                # the framer tool's output, exactly
        assert (bits[s, want.size:] == 0xAA).all() and (syms[s, nsym[s]:] == 0xAA).all()    # nothing written behind the row's end
        off = txref.carrier_mask(plans[s], lead[s], gap[s], tx.preamble_syms, tx.frame_syms)
        assert off.size == nsym[s]
        wsym = np.where(off, OFF, txref.bits_to_syms(want, M))
        assert np.array_equal(syms[s, :nsym[s]], wsym), s
    # a row too short for what the records can need is refused, not cut
    with pytest.raises(pirip_amd.PiripError):
        tx.frame(d_rec.data_ptr(), host[0].size, max_rec, torch.zeros((B, cap), dtype=torch.uint8, device="cuda").data_ptr(), cap - 1, cap - 1)


def _modulate(tx, syms, nsym_total, fmt, blocks=None, d_nsym=0, **kw):
    """syms: torch uint8 [B, >= nsym_total] on the device -> numpy rows, sent in `blocks` (symbol counts) or in one call"""
    import torch
    import pirip_amd
    B, Ts = syms.shape[0], tx.Ts
    bs = 2 if fmt == pirip_amd.IN_CU8_FSKDEMOD else 8
    out = torch.zeros((B, nsym_total * Ts * bs), dtype=torch.uint8, device="cuda")
    at = 0
    for n in (blocks or [nsym_total]):
        assert d_nsym == 0 or blocks is None
        tx.modulate(syms.data_ptr() + at, syms.shape[1], n, out.data_ptr() + at * Ts * bs, out.shape[1], out_format=fmt, d_nsym=d_nsym, **kw)
        at += n
    assert at == nsym_total
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    return o.reshape(B, -1, 2) if bs == 2 else o.view(np.float32).reshape(B, -1, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", MOD_SHAPES, ids=lambda s: "Fs%d-Rs%d-M%d" % s[:3])
def test_modulator_against_the_float64_formula(built_lib, shape):
    import torch
    import pirip_amd
    Fs, Rs, M, f1s, shift = shape
    Ts, B, nsym = Fs // Rs, len(f1s), 1500
    rng = np.random.default_rng(7 + M + Ts)
    host = rng.integers(0, M, (B, nsym)).astype(np.uint8)
    host[1, 100:160] = OFF
    host[2, :33] = OFF
    host[3, 700:] = OFF
    nvalid = np.array([nsym, nsym, nsym - 7, nsym], dtype=np.int32)           # stream 2: the last 7 symbols are off by its count
    tx = pirip_amd.HipTx(CODE, Fs, Rs, M, nstreams=B, f1=f1s, shift=shift)
    d = torch.from_numpy(host).cuda()
    d_nv = torch.from_numpy(nvalid).cuda()
    cf = _modulate(tx, d, nsym, pirip_amd.IN_CF32, d_nsym=d_nv.data_ptr())
    tx.reset()
    u8 = _modulate(tx, d, nsym, pirip_amd.IN_CU8_FSKDEMOD, d_nsym=d_nv.data_ptr(), amp=32.0)
    ties = total = 0
    for s in range(B):
        sy = host[s].copy()
        sy[nvalid[s]:] = OFF
        y = txref.mod_f64(sy, f1s[s], shift, Fs, Ts)
        err = max(float(np.max(np.abs(cf[s, :, 0] - y.real))), float(np.max(np.abs(cf[s, :, 1] - y.imag))))
        print(f"stream {s}: cf32 largest component error {err:.3e} (bound {txref.BOUND:.3e})")
        assert err <= txref.BOUND, (s, err)
        off = np.repeat(sy == OFF, Ts)
        assert not cf[s][off].any() and (u8[s][off] == 127).all()             # carrier off: zero signal
        q, v = txref.quantise(y, 32.0)
        diff = np.abs(u8[s].astype(np.int64) - q)
        assert diff.max() <= 1, (s, int(diff.max()))
        tie = txref.near_tie(v, 32.0)
        assert not (diff[~tie]).any(), (s, int(np.count_nonzero(diff[~tie])))
        ties += int(np.count_nonzero(tie)); total += tie.size
    print(f"samples within the bound of a rounding tie: {ties} of {total}")
    assert ties <= 1e-3 * total


@pytest.mark.gpu
@pytest.mark.parametrize("sigma", [0.0, 0.6])
@pytest.mark.parametrize("shape", MOD_SHAPES, ids=lambda s: "Fs%d-Rs%d-M%d" % s[:3])
def test_split_calls_and_reset_give_identical_bytes(built_lib, shape, sigma):
    import torch
    import pirip_amd
    Fs, Rs, M, f1s, shift = shape
    B, nsym = len(f1s), 1201
    rng = np.random.default_rng(11 + M)
    host = rng.integers(0, M, (B, nsym)).astype(np.uint8)
    host[0, 300:420] = OFF
    d = torch.from_numpy(host).cuda()
    tx = pirip_amd.HipTx(CODE, Fs, Rs, M, nstreams=B, f1=f1s, shift=shift)
    blocks = [7, 33, 1, 255, 256, 257, 391, 1]
    assert sum(blocks) == nsym
    for fmt in (pirip_amd.IN_CU8_FSKDEMOD, pirip_amd.IN_CF32):
        tx.reset()
        one = _modulate(tx, d, nsym, fmt, amp=20.0, sigma=sigma, seed=5)
        tx.reset()
        parts = _modulate(tx, d, nsym, fmt, blocks=blocks, amp=20.0, sigma=sigma, seed=5)
        assert np.array_equal(one.view(np.uint8), parts.view(np.uint8))
        tx.reset()
        again = _modulate(tx, d, nsym, fmt, amp=20.0, sigma=sigma, seed=5)
        assert np.array_equal(one.view(np.uint8), again.view(np.uint8))
        if sigma > 0:
            tx.reset()
            other = _modulate(tx, d, nsym, fmt, amp=20.0, sigma=sigma, seed=6)
            assert not np.array_equal(one.view(np.uint8), other.view(np.uint8))
            if fmt == pirip_amd.IN_CF32:                                      # the noise is sigma * N(0, 1) per component
                tx.reset()
                clean = _modulate(tx, d, nsym, fmt, amp=20.0, sigma=0.0, seed=5)
                n = (one - clean).astype(np.float64)
                assert abs(n.std() / sigma - 1.0) < 0.02 and abs(n.mean()) < 0.01
    # without a reset the phase runs on: the second row continues the first
    tx.reset()
    a = _modulate(tx, d, nsym, pirip_amd.IN_CF32)
    b = _modulate(tx, d, nsym, pirip_amd.IN_CF32)
    for s in range(B):
        _, _, p_end = txref.phase_ints(host[s], f1s[s], shift, Fs, Fs // Rs)
        y = txref.mod_f64(host[s], f1s[s], shift, Fs, Fs // Rs, p0=p_end)
        assert np.max(np.abs(b[s, :, 0] - y.real)) <= txref.BOUND and np.max(np.abs(b[s, :, 1] - y.imag)) <= txref.BOUND
    assert a.shape == b.shape


@pytest.mark.gpu
@pytest.mark.parametrize("M", [2, 4])
def test_one_burst_against_the_float_recursion(oracle, built_lib, M):
    """The CPU modulator (codec2's float recursion) and the exact-phase kernel send the same signal: the difference over one burst is the
    recursion's drift, recorded in DESIGN.md 4.9 -- asserted only to stay below half a u8 level at amp = 32."""
    import torch
    import pirip_amd
    cfg = dict(sigutil.CFG1, P=8) if M == 2 else sigutil.CFG4
    p = subprocess.run([os.path.join(BIN, "fsk_ldpc_framer"), "--code", CODE, "-m", str(M), "--testframes", "3", "--seq", "/dev/zero", "-"], capture_output=True)
    assert p.returncode == 0
    bits = np.frombuffer(p.stdout, dtype=np.uint8)
    bits = bits[:bits.size - bits.size % (50 * (1 if M == 2 else 2))]
    x = sigutil.mod_complex(oracle, cfg, bits)
    syms = txref.bits_to_syms(bits, M)
    tx = pirip_amd.HipTx(CODE, cfg["Fs"], cfg["Rs"], M, nstreams=1, f1=cfg["f1"], shift=cfg["shift"])
    y = _modulate(tx, torch.from_numpy(syms[None, :].copy()).cuda(), syms.size, pirip_amd.IN_CF32)[0]
    d = float(np.max(np.abs(x.astype(np.float64) - y.astype(np.float64))))
    print(f"M={M}: {y.shape[0]} samples, largest component difference to the float recursion {d:.3e}")
    assert d < 0.5 / 32.0


def _chain(dem, L, d_iq, nsamp):
    """IQ rows (torch uint8 [B, nsamp * 2]) -> per stream the payloads of its RX_BITS records"""
    import torch
    import pirip_amd
    B = d_iq.shape[0]
    maxf = dem.max_frames_for(nsamp)
    st = torch.zeros((B, maxf), dtype=torch.uint8, device="cuda")
    pl = torch.zeros((B, maxf, L.data_bytes), dtype=torch.uint8, device="cuda")
    inf = torch.zeros((B, maxf, pirip_amd.LDPC_INFO_PER_CALL), dtype=torch.int32, device="cuda")
    nfr = torch.zeros(B, dtype=torch.int32, device="cuda")
    cons = torch.zeros(B, dtype=torch.int64, device="cuda")
    L.chain_batch(dem, d_iq.data_ptr(), d_iq.shape[1], nsamp, st.data_ptr(), pl.data_ptr(), inf.data_ptr(), nfr.data_ptr(), cons.data_ptr(), maxf)
    torch.cuda.synchronize()
    st, pl, nfr = st.cpu().numpy(), pl.cpu().numpy(), nfr.cpu().numpy()
    return [pl[s, :nfr[s]][(st[s, :nfr[s]] & RX_BITS) != 0] for s in range(B)]


@pytest.mark.gpu
@pytest.mark.parametrize("M,P", [(4, 8), (2, 8)], ids=["config4", "2fsk"])
def test_loopback_into_the_receive_chain(oracle, built_lib, M, P):
    """HipTx -> pirip_hip_fsk_ldpc_rx_batch, every stream its own payloads. Noise-free: every frame comes back with its CRC. At Eb/N0 = 7 dB:
    nothing wrong is delivered, and the share of frames recovered is compared with the existing path's (fsk_ldpc_framer on the host ->
    pirip_hip_synth_cu8) on the same bits, seed and offsets: lower by at most three binomial standard deviations of the frame count."""
    import torch
    import pirip_amd
    Fs, Rs, f1, shift, amp = 240000, 10000, 10000, 10000, 14.0
    Ts, bps = Fs // Rs, (1 if M == 2 else 2)
    B, nfr, tail = 128, 3, 700
    rng = np.random.default_rng(900 + M)
    code = oracle.parse_code_file(CODE)
    crc = oracle.OracleLdpc(code, M).crc16
    # (200 symbols of silence in front: with 40 the receiver misses the first frame of some timing offsets noise-free -- on the existing
    # transmit path just the same; the chain tests of tests/test_ldpc.py lead with 167 and more)
    lead = [200 + s % 7 for s in range(B)]
    tx = pirip_amd.HipTx(CODE, Fs, Rs, M, nstreams=B, f1=f1, shift=shift, lead=lead, gap=tail)
    kb = tx.data_bytes
    ctl = [1] + [0] * (nfr - 1) + [2]
    host = np.stack([txref.records(rng, ctl, kb) for _ in range(B)])
    sent = host[:, :nfr, 1:].copy()
    for s in range(B):
        for f in range(nfr):
            c = crc(sent[s, f, :kb - 2])
            sent[s, f, kb - 2], sent[s, f, kb - 1] = c >> 8, c & 0xff
    assert len({sent[s, f].tobytes() for s in range(B) for f in range(nfr)}) == B * nfr
    burst = tx.preamble_syms + nfr * tx.frame_syms
    nsym = max(lead) + burst + tail
    nsamp = nsym * Ts
    d_rec = torch.from_numpy(host).cuda()
    iq = torch.zeros((B, nsamp * 2), dtype=torch.uint8, device="cuda")
    dem = pirip_amd.HipDemod(Fs, Rs, M, P=P, est_min=Rs // 2, est_max=min(Fs // 2 - Rs, 90000), in_format=pirip_amd.IN_CU8_FSKDEMOD, nstreams=B)
    L = pirip_amd.HipLdpc(CODE, M, nstreams=B)

    # noise-free
    tx.records_to_iq(d_rec.data_ptr(), host[0].size, len(ctl), nsym, iq.data_ptr(), nsamp * 2, amp=amp)
    got = _chain(dem, L, iq, nsamp)
    for s in range(B):
        assert got[s].shape[0] == nfr and np.array_equal(got[s], sent[s]), s

    # Eb/N0 = 7 dB
    sigma = float(np.sqrt(4.0 * Ts / np.log2(M) / (10 ** 0.7) / 2.0))
    seed = 77
    tx.reset(); dem.reset(); L.reset()
    tx.records_to_iq(d_rec.data_ptr(), host[0].size, len(ctl), nsym, iq.data_ptr(), nsamp * 2, amp=amp, sigma=sigma, seed=seed)
    got = _chain(dem, L, iq, nsamp)
    new = 0
    for s in range(B):
        ok = {sent[s, f].tobytes() for f in range(nfr)}
        assert all(g.tobytes() in ok for g in got[s]), s                      # nothing but what this stream sent
        new += len({g.tobytes() for g in got[s]})

    # the existing path: host framer, upload, pirip_hip_synth_cu8 for the burst; the silence around it spliced in on the host
    rows = np.zeros((B, nsamp, 2), dtype=np.uint8)
    bits = np.stack([sigutil.run_framer(["-m", str(M), "--packed", "--gap", "0", "-", "-"], host[s].tobytes(), CODE) for s in range(B)])
    assert bits.shape[1] == burst * bps
    d_bits = torch.from_numpy(bits).cuda()
    seg = torch.zeros((B, burst * Ts * 2), dtype=torch.uint8, device="cuda")
    pirip_amd.binding.synth_cu8(Fs, Rs, M, [f1] * B, shift, d_bits.data_ptr(), bits.shape[1], burst, seg.data_ptr(), burst * Ts * 2, burst * Ts,
                                amp=amp, sigma=sigma, seed=seed)
    torch.cuda.synchronize()
    seg = seg.cpu().numpy().reshape(B, -1, 2)
    nrng = np.random.default_rng(seed)
    for s in range(B):
        rows[s] = np.clip(np.rint(127.0 + amp * sigma * nrng.normal(size=(nsamp, 2))), 0, 255).astype(np.uint8)
        rows[s, lead[s] * Ts:lead[s] * Ts + burst * Ts] = seg[s]
    dem.reset(); L.reset()
    got_old = _chain(dem, L, torch.from_numpy(rows.reshape(B, -1)).cuda(), nsamp)
    old = sum(len({g.tobytes() for g in got_old[s]} & {sent[s, f].tobytes() for f in range(nfr)}) for s in range(B))
    N = B * nfr
    a, b = new / N, old / N
    pooled = (new + old) / (2.0 * N)
    sd = float(np.sqrt(pooled * (1.0 - pooled) / N))
    print(f"M={M}: frames recovered at 7 dB: HipTx {new}/{N} = {a:.4f}, host framer + synth_cu8 {old}/{N} = {b:.4f}, 3 sd = {3 * sd:.4f}")
    assert old > 0.5 * N                                                       # the operating point is one the receiver works at
    assert a >= b - 3.0 * sd


_repeater_replay = txref.repeater_replay


@pytest.mark.gpu
def test_repeater_record_conversion_equals_a_replay_of_frame_repeater(oracle, built_lib):
    """Records of a received multi-burst capture -> pirip_hip_tx_repeat_records (in two calls, cut inside a burst: the open burst waits in
    the handle) equal the replay of tx/frame_repeater.c; transmitted and received again, the payloads come back with the new source byte."""
    import torch
    import pirip_amd
    Fs, Rs, M, P, f1, shift, amp, src = 240000, 10000, 2, 8, 10000, 10000, 14.0, 0x7
    Ts, B, tail = Fs // Rs, 6, 700
    rng = np.random.default_rng(61)
    tx = pirip_amd.HipTx(CODE, Fs, Rs, M, nstreams=B, f1=f1, shift=shift, lead=[200 + 3 * s for s in range(B)], gap=tail)
    kb = tx.data_bytes
    plans = [[1, 0, 0, 2] + txref.burst_plan(rng, 1 + s % 2, 3) for s in range(B)]       # a first burst of three frames, then one or two more
    max_rec = max(len(p) for p in plans)
    host = np.zeros((B, max_rec, 1 + kb), dtype=np.uint8)
    for s in range(B):
        host[s, :len(plans[s])] = txref.records(rng, plans[s], kb)
    nrec = torch.tensor([len(p) for p in plans], dtype=torch.int32, device="cuda")
    nsym = tx.max_syms(max_rec)
    nsamp = nsym * Ts
    iq = torch.zeros((B, nsamp * 2), dtype=torch.uint8, device="cuda")
    tx.records_to_iq(torch.from_numpy(host).cuda().data_ptr(), host[0].size, max_rec, nsym, iq.data_ptr(), nsamp * 2, d_nrec=nrec.data_ptr(), amp=amp)
    dem = pirip_amd.HipDemod(Fs, Rs, M, P=P, est_min=Rs // 2, est_max=90000, in_format=pirip_amd.IN_CU8_FSKDEMOD, nstreams=B)
    L = pirip_amd.HipLdpc(CODE, M, nstreams=B)
    maxf = dem.max_frames_for(nsamp)
    st = torch.zeros((B, maxf), dtype=torch.uint8, device="cuda")
    pl = torch.zeros((B, maxf, kb), dtype=torch.uint8, device="cuda")
    inf = torch.zeros((B, maxf, pirip_amd.LDPC_INFO_PER_CALL), dtype=torch.int32, device="cuda")
    nfr = torch.zeros(B, dtype=torch.int32, device="cuda")
    cons = torch.zeros(B, dtype=torch.int64, device="cuda")
    L.chain_batch(dem, iq.data_ptr(), nsamp * 2, nsamp, st.data_ptr(), pl.data_ptr(), inf.data_ptr(), nfr.data_ptr(), cons.data_ptr(), maxf)
    torch.cuda.synchronize()
    hst, hpl, hnf = st.cpu().numpy(), pl.cpu().numpy(), nfr.cpu().numpy()
    want = [_repeater_replay(hst[s, :hnf[s]], hpl[s, :hnf[s]], src) for s in range(B)]
    nframes_sent = [sum(1 for c in p if c != 2) for p in plans]
    for s in range(B):
        assert (want[s][:, 0] != 2).sum() == nframes_sent[s] and (want[s][:, 0] == 2).sum() == sum(1 for c in plans[s] if c == 1), s
    # the conversion, cut at call c1 -- for every stream inside its first burst, after the first decoded frame
    c1 = 30
    assert all(((hst[s, :c1] & RX_BITS) != 0).any() and (hst[s, c1 - 1] & RX_SYNC) for s in range(B))
    got = [[] for _ in range(B)]
    for lo, hi in ((0, c1), (c1, maxf)):
        n = hi - lo
        cap = tx.repeat_max_records(n)
        out = torch.full((B, cap, 1 + kb), 0xEE, dtype=torch.uint8, device="cuda")
        cnt = torch.full((B,), -1, dtype=torch.int32, device="cuda")
        ncl = torch.clamp(nfr - lo, 0, n).to(torch.int32)
        tx.repeat_records(st.data_ptr() + lo, maxf, pl.data_ptr() + lo * kb, maxf * kb, n, src, out.data_ptr(), cap * (1 + kb), cap,
                          d_ncalls=ncl.data_ptr(), d_nrec=cnt.data_ptr())
        torch.cuda.synchronize()
        o, c = out.cpu().numpy(), cnt.cpu().numpy()
        for s in range(B):
            assert 0 <= c[s] <= cap and (o[s, c[s]:] == 0xEE).all(), s
            got[s].append(o[s, :c[s]])
    for s in range(B):
        assert got[s][0].shape[0] == 0                                        # nothing is written while the first burst is still coming in
        assert np.array_equal(np.concatenate(got[s]), want[s]), s
    # one call over everything gives the same (after a reset: no burst is open then anyway)
    tx.reset()
    cap = tx.repeat_max_records(maxf)
    out = torch.zeros((B, cap, 1 + kb), dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(B, dtype=torch.int32, device="cuda")
    tx.repeat_records(st.data_ptr(), maxf, pl.data_ptr(), maxf * kb, maxf, src, out.data_ptr(), cap * (1 + kb), cap, d_ncalls=nfr.data_ptr(), d_nrec=cnt.data_ptr())
    torch.cuda.synchronize()
    for s in range(B):
        assert np.array_equal(out[s, :int(cnt[s])].cpu().numpy(), want[s]), s
    # the repeated records on the air and back: every payload returns with the repeater's source byte
    tx.reset(); dem.reset(); L.reset()
    nsym2 = tx.max_syms(cap)
    iq2 = torch.zeros((B, nsym2 * Ts * 2), dtype=torch.uint8, device="cuda")
    tx.records_to_iq(out.data_ptr(), cap * (1 + kb), cap, nsym2, iq2.data_ptr(), nsym2 * Ts * 2, d_nrec=cnt.data_ptr(), amp=amp)
    back = _chain(dem, L, iq2, nsym2 * Ts)
    for s in range(B):
        sent = host[s, :len(plans[s])]
        sent = sent[sent[:, 0] != 2][:, 1:]
        assert back[s].shape[0] == sent.shape[0], s
        assert (back[s][:, 0] == src).all() and np.array_equal(back[s][:, 1:kb - 2], sent[:, 1:kb - 2]), s


@pytest.mark.gpu
def test_fsk_ldpc_tx_pipes_into_rtl_fsk(built_lib):
    """fsk_ldpc_tx --testframes 3 ... | rtl_fsk --code ... -b: three BITS records with the test frame's payload"""
    tx = subprocess.run([os.path.join(BIN, "fsk_ldpc_tx"), "--code", CODE, "--testframes", "3", "--seq", "--source", "0x3", "--lead", "60", "--gap", "900",
                         "240000", "10000", "10000", "10000", "/dev/zero", "-"], capture_output=True)
    assert tx.returncode == 0, tx.stderr
    assert len(tx.stdout) == 2 * 24 * (60 + 50 + 3 * 544 + 900)
    rx = subprocess.run([os.path.join(BIN, "rtl_fsk"), "-i", "-", "-", "-s", "240000", "-r", "10000", "--code", CODE, "-q", "-b"],
                        input=tx.stdout, capture_output=True)
    assert rx.returncode == 0, rx.stderr
    rec = np.frombuffer(rx.stdout, dtype=np.uint8).reshape(-1, 33)
    good = rec[(rec[:, 0] & RX_BITS) != 0]
    assert good.shape[0] == 3
    assert list(good[:, 1]) == [3, 3, 3] and list(good[:, 2]) == [1, 2, 3]
    fr = subprocess.run([os.path.join(BIN, "fsk_ldpc_framer"), "--code", CODE, "--testframes", "3", "--seq", "--source", "0x3", "/dev/zero", "-"], capture_output=True)
    bits = np.frombuffer(fr.stdout, dtype=np.uint8)
    for f in range(3):
        assert np.array_equal(good[f, 1:], np.packbits(bits[50 + f * 544 + 32:][:256]))
