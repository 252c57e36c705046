"""FSK_LDPC row: framer, LLR mapping, unique-word sync, LDPC decode, CRC16, the
`rtl_fsk --code ... -b` record stream.

What is pinned by /root/reference: frame layout and CRC placement (tx/rpitx_fsk.cpp:75-83,394-395), preamble (:313-336),
the burst-control byte protocol (:427-509), the status-byte record stream and its flags (tx/frame_repeater.c:55-62,71,80,88),
<= 15 iterations and the -v columns (README.md:200-212). The parity-check matrix, unique word and decoder arithmetic are
codec2's and absent: the code is a labelled stand-in (tools/make_standin_code.py) and GPU parity is against this repo's
oracle (oracle/ldpc_oracle.c, parity unpinned). External anchors used here: the CRC-16/CCITT-FALSE check value 0x29B1 of
"123456789", and a code-independent property: every emitted frame satisfies all parity checks."""
import os
import subprocess

import numpy as np
import pytest

import sigutil

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "pirip_amd", "bin")
CODE = os.path.join(ROOT, "pirip_amd", "data", "standin_256_512_4.code")
RX_SYNC, RX_BITS, RX_BIT_ERRORS = 2, 4, 8


def _bursts(ob, cfg, M, bursts, ebno_db, seed, silence=4000, amp=14.0):
    """bursts: list of bit arrays (framer output, preamble included). Returns u8 IQ with noise-only gaps, and sigma."""
    rng = np.random.default_rng(seed)
    ts = cfg["Fs"] // cfg["Rs"]
    segs = [np.zeros((silence + int(rng.integers(0, ts)), 2), dtype=np.float32)]
    for b in bursts:
        segs.append(sigutil.mod_complex(ob, cfg, b))
        segs.append(np.zeros((silence * 3, 2), dtype=np.float32))
    segs.append(np.zeros((silence * 2, 2), dtype=np.float32))     # the last frame's successor slot: the UW check there releases sync
    x = np.concatenate(segs)
    eb = 4.0 * ts / np.log2(M)                                  # fsk_mod_c output has |x|^2 = 4
    sigma = np.sqrt(eb / (10 ** (ebno_db / 10.0)) / 2.0)
    y = x + rng.normal(0.0, sigma, x.shape).astype(np.float32)
    return ob.quantise_cu8(y, amp=amp)


def _records(raw, nbytes):
    rec = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 1 + nbytes)
    return rec[:, 0], rec[:, 1:]


def test_code_file_framer_crc_and_parity_checks(oracle, built_lib):
    code = oracle.parse_code_file(CODE)
    assert code["n"] == 512 and code["k"] == 256 and len(code["rows"]) == 256 and code["uw"].size == 32
    o = oracle.OracleLdpc(code, 2)
    # public known-answer: CRC-16/CCITT-FALSE("123456789") = 0x29B1
    assert o.crc16(np.frombuffer(b"123456789", dtype=np.uint8)) == 0x29B1
    # test-frame mode of the Tx (rpitx_fsk.cpp:366-421): 2 bursts x 3 frames, source byte 0x5 and sequence numbers
    bits = sigutil.run_framer(["--testframes", "3", "--bursts", "2", "--source", "0x5", "--seq", "/dev/zero", "-"])
    pre, bpf = 50, 32 + 512
    assert bits.size == 2 * (pre + 3 * bpf)
    assert np.array_equal(bits[:8], [0, 0, 0, 1, 1, 0, 1, 1])        # preamble cycles symbols 0,1,2,3 (rpitx_fsk.cpp:329-335)
    H = np.zeros((256, 512), dtype=np.uint8)
    for r, cols in enumerate(code["rows"]):
        H[r, cols] = 1
    for b in range(2):
        for f in range(3):
            fr = bits[b * (pre + 3 * bpf) + pre + f * bpf:][:bpf]
            assert np.array_equal(fr[:32], code["uw"])
            cw = fr[32:]
            assert not (H.astype(np.int32) @ cw.astype(np.int32) % 2).any(), "emitted frame violates a parity check"
            by = np.packbits(cw[:256])
            assert by[0] == 0x5 and by[1] == f + 1
            assert o.crc16(by[:30]) == (int(by[30]) << 8 | int(by[31]))       # last 16 data bits = CRC of the first 30 bytes
    # burst-control protocol (rpitx_fsk.cpp:427-509) with packed input, as frame_repeater writes it (frame_repeater.c:92-104)
    rng = np.random.default_rng(1)
    pay = rng.integers(0, 256, (3, 32)).astype(np.uint8)
    rec = b"".join(bytes([bc]) + pay[i].tobytes() for i, bc in enumerate([1, 0, 0])) + bytes([2]) + bytes(32)
    bits2 = sigutil.run_framer(["--packed", "-", "-"], stdin=rec)
    assert bits2.size == pre + 3 * bpf
    for f in range(3):
        by = np.packbits(bits2[pre + f * bpf + 32:][:256])
        assert np.array_equal(by[:30], pay[f, :30])


def test_oracle_loopback_decodes_at_eight_percent_raw_ber(oracle, built_lib):
    """CPU plumbing of config 4's second half: framer -> fsk_mod -> AWGN (~8 % raw BER) -> oracle demod (soft) -> oracle
    FSK_LDPC rx: every frame of both bursts decodes with 0 coded errors, SYNC drops between bursts."""
    code = oracle.parse_code_file(CODE)
    c = dict(sigutil.CFG1, P=6)
    bits = sigutil.run_framer(["--testframes", "3", "--bursts", "1", "--seq", "/dev/zero", "-"])
    u8 = _bursts(oracle, c, 2, [bits, bits], ebno_db=5.6, seed=3)
    dem = oracle.OracleFsk(c["Fs"], c["Rs"], 2, P=6, est_min=500, est_max=25000)
    r = dem.demod(u8, oracle.IN_CU8_CSDR)
    rx = oracle.OracleLdpc(code, 2)
    status, payload, info = rx.rx(r["rx_filt"])
    got = payload[(status & RX_BITS) != 0]
    want = np.packbits(bits[50 + 32:][:256])
    raw = info[(status & RX_BITS) != 0, 8]
    print("frames delivered", got.shape[0], "of 6; raw errors per frame", raw, "iterations", info[(status & RX_BITS) != 0, 4])
    # With the recalled acquisition threshold (<= 5 of 32 unique-word errors) a false lock in the noise before a burst can
    # cost its first frame, and a frame with > ~10 % raw errors does not decode (README.md:210-212 reports 9 of 10 at this
    # operating point): what is delivered must be error free, and most frames must arrive.
    assert got.shape[0] >= 4
    assert all(np.array_equal(g[2:30], want[2:30]) for g in got)   # 0 coded errors (bytes 0,1: source / sequence; 30,31: CRC)
    assert raw.mean() > 20 and raw.mean() < 70                    # ~8 % of 512
    sync = (status & RX_SYNC) != 0
    assert sync.any() and not sync[-1]                             # sync is released after the last burst


DECODERS = ["auto", "bank"]      # PIRIP_LDPC_DECODER, read at handle creation: `bank` forces the persistent decoder with the bank-private
                                 # phi table (the choice for chip-filling batches) onto these small inputs too; same records either way


@pytest.mark.gpu
@pytest.mark.parametrize("decoder", DECODERS)
@pytest.mark.parametrize("llr_map", ["upstream", "rician"])
@pytest.mark.parametrize("M", [2, 4])
def test_gpu_llr_and_decoder_bit_exact_vs_oracle(oracle, built_lib, tmp_path, monkeypatch, M, llr_map, decoder):
    """(llr_map: the code file's key -- `upstream` = codec2's fsk_rx_filt_to_llrs as recalled, the default; `rician` = exact ln I0)"""
    import torch
    import pirip_amd
    monkeypatch.setenv("PIRIP_LDPC_DECODER", decoder)
    path = sigutil.code_variant(CODE, tmp_path, llr_map)
    code = oracle.parse_code_file(path)
    assert code["llr_map"] == llr_map and oracle.parse_code_file(CODE)["llr_map"] == "upstream"      # the shipped file runs the reference's mapping
    rng = np.random.default_rng(10 + M)
    o = oracle.OracleLdpc(code, M)
    h = pirip_amd.HipLdpc(path, M)
    # soft decisions like fsk_demod_sd's: Rician magnitudes at several SNRs, plus degenerate frames (all equal, zeros, huge)
    ncalls, nsym = 64, 50
    filt = np.zeros((ncalls, M, nsym), dtype=np.float32)
    for i in range(ncalls):
        snr = [0.5, 2.0, 6.0, 30.0][i % 4]
        sym = rng.integers(0, M, nsym)
        z = (rng.normal(size=(M, nsym)) + 1j * rng.normal(size=(M, nsym))) / np.sqrt(2)
        z[sym, np.arange(nsym)] += np.sqrt(snr)
        filt[i] = np.abs(z) * [1.0, 37.5, 1e-3, 900.0][(i // 4) % 4]
    filt[60] = 0.0; filt[61] = 1.0; filt[62] = 1e6
    d = torch.from_numpy(filt).cuda()
    out = torch.zeros((ncalls, o.Nbits), dtype=torch.float32, device="cuda")
    pirip_amd.binding._chk(h.L.pirip_hip_ldpc_llr(h.h, d.data_ptr(), ncalls, out.data_ptr(), 0), "llr")
    torch.cuda.synchronize()
    want = o.llr(filt)
    assert np.array_equal(out.cpu().numpy(), want), "LLR mapping differs from the oracle"
    # decoder: noisy codewords from easy to undecodable (BPSK-like LLRs), plus all-zero and saturated inputs
    H_rows = code["rows"]
    ncw = 96
    llr = np.zeros((ncw, 512), dtype=np.float32)
    for i in range(ncw):
        data = rng.integers(0, 2, 256).astype(np.uint8)
        par = np.zeros(256, dtype=np.uint8); prev = 0
        for p_, cols in enumerate(H_rows):
            prev = (int(data[[c_ for c_ in cols if c_ < 256]].sum()) + prev) & 1; par[p_] = prev
        cw = np.concatenate([data, par])
        sig = [0.55, 0.7, 0.8, 0.9, 1.0, 1.3][i % 6]
        y = (1.0 - 2.0 * cw) + rng.normal(0, sig, 512)
        llr[i] = np.clip(2.0 * y / sig ** 2, -24, 24)
    llr[90] = 0.0; llr[91] = 24.0; llr[92] = -24.0
    dl = torch.from_numpy(llr).cuda()
    bits = torch.zeros((ncw, 512), dtype=torch.uint8, device="cuda")
    ip = torch.zeros((ncw, 2), dtype=torch.int32, device="cuda")
    pirip_amd.binding._chk(h.L.pirip_hip_ldpc_decode_llr(h.h, dl.data_ptr(), ncw, bits.data_ptr(), ip.data_ptr(), 0), "decode")
    torch.cuda.synchronize()
    wb, wip = o.decode(llr)
    assert np.array_equal(ip.cpu().numpy(), wip), "iterations / parity-check counts differ"
    assert np.array_equal(bits.cpu().numpy(), wb), "decoded bits differ"
    it = wip[:90, 0]
    print("iterations histogram", np.bincount(it, minlength=16), "undecoded", int((wip[:90, 1] != 256).sum()))
    assert (wip[:90, 1] == 256).sum() > 40 and (wip[:90, 1] != 256).sum() > 3      # the sweep spans easy and undecodable words


@pytest.mark.gpu
@pytest.mark.parametrize("decoder", DECODERS)
@pytest.mark.parametrize("M,ebno", [(2, 5.6), (4, 5.5)])
def test_gpu_receiver_records_equal_oracle_on_the_same_soft_decisions(oracle, built_lib, monkeypatch, M, ebno, decoder):
    """Whole receiver (LLR -> sync FSM -> decode -> CRC) in chunks of calls: status, payload and the info columns equal the
    oracle's, fed with the same soft decisions (the GPU demodulator's)."""
    import pirip_amd
    monkeypatch.setenv("PIRIP_LDPC_DECODER", decoder)
    code = oracle.parse_code_file(CODE)
    c = dict(sigutil.CFG1 if M == 2 else sigutil.CFG4, P=6 if M == 2 else 8)
    bits = sigutil.run_framer(["-m", str(M), "--testframes", "3", "--bursts", "1", "--seq", "--source", "0x2", "/dev/zero", "-"])
    u8 = _bursts(oracle, c, M, [bits, bits[: (50 * M // 2) + 544], bits], ebno_db=ebno, seed=5 + M)
    dem = pirip_amd.HipDemod(c["Fs"], c["Rs"], M, P=c["P"], est_min=500, est_max=c["est_max"], in_format=pirip_amd.IN_CU8_CSDR, nstreams=1)
    r = dem.demod_host(u8)
    filt = r["rx_filt"]
    o = oracle.OracleLdpc(code, M)
    ws, wp, wi = o.rx(filt)
    h = pirip_amd.HipLdpc(CODE, M)
    gs, gp, gi = [], [], []
    pos = 0
    for n in (7, 1, 30, 64, 3, 10 ** 6):                        # uneven chunks: state and the two-frame history carry over
        blk = filt[pos:pos + n]
        if not len(blk):
            break
        s, p, i = h.rx_host(blk)
        gs.append(s); gp.append(p); gi.append(i); pos += n
    gs, gp, gi = np.concatenate(gs), np.concatenate(gp), np.concatenate(gi)
    assert np.array_equal(gs, ws), np.where(gs != ws)
    assert np.array_equal(gp, wp)
    assert np.array_equal(gi, wi), np.where(gi != wi)
    nb = ((ws & RX_BITS) != 0).sum()
    print("frames with CRC ok:", nb, "of 7; raw errors", wi[(ws & RX_BITS) != 0, 8], "iter", wi[(ws & RX_BITS) != 0, 4])
    assert nb >= 5                                                # (false locks in the gaps / > 10 % raw errors can cost a frame)


@pytest.mark.gpu
def test_rtl_fsk_code_records_drive_a_frame_repeater(oracle, built_lib):
    """`rtl_fsk ... --code NAME --filter A -q -b` (script/frame_repeater:36) on a file: the record stream is consumed the way
    tx/frame_repeater.c:55-104 consumes it (burst = first SYNC|BITS record until SYNC drops), payloads carry 0 coded errors
    at ~8 % raw BER, frames from the filtered source address are dropped, -v prints the reference's columns; without -b
    the payload bytes alone come out (README.md:297)."""
    c = dict(sigutil.CFG1, P=6)
    b_a = sigutil.run_framer(["--testframes", "3", "--seq", "--source", "0x1", "/dev/zero", "-"])
    b_b = sigutil.run_framer(["--testframes", "2", "--seq", "--source", "0x2", "/dev/zero", "-"])
    u8 = _bursts(oracle, c, 2, [b_a, b_b], ebno_db=5.6, seed=11)
    exe = os.path.join(BIN, "rtl_fsk")
    env = dict(os.environ, PIRIP_IQ_FILE="/dev/stdin", PIRIP_CODE_DIR=os.path.join(ROOT, "pirip_amd", "data"))
    # the reference's command line, IQ from the environment (no -i)
    p = subprocess.run([exe, "-g", "40", "-f", "144490000", "-", "-s", "240000", "-r", "10000", "--code", "standin_256_512_4",
                        "--filter", "0x2", "-q", "-b", "-v", "--testframes"], input=u8.tobytes(), capture_output=True, env=env)
    assert p.returncode == 0, p.stderr
    status, data = _records(p.stdout, 32)
    assert status.size > 60                                         # one record per demodulator call
    # frame_repeater's state machine
    bursts, cur, receiving = [], [], False
    for st, d in zip(status, data):
        if not receiving:
            if st == (RX_SYNC | RX_BITS):
                cur = [d]; receiving = True
        else:
            if st & RX_BITS:
                cur.append(d)
            if not (st & RX_SYNC):
                bursts.append(cur); receiving = False
    want = np.packbits(b_a[50 + 32:][:256])
    assert len(bursts) == 1 and len(bursts[0]) == 3                 # burst from 0x1 echoed, burst from 0x2 (our own address) filtered
    for i, d in enumerate(bursts[0]):
        assert d[0] == 0x1 and d[1] == i + 1 and np.array_equal(d[2:30], want[2:30])
    assert not data[(status & RX_BITS) == 0].any()                  # zeros when no frame
    lines = [ln for ln in p.stderr.decode().split("\n") if "rxst:" in ln]
    assert len(lines) == 5
    for key in ("nbits:", "state:", "uw_loc:", "uw_err:", "bad_uw:", "snrdB:", "eraw:", "ecdd:", "iter:", "pcc:", "rxst:"):
        assert key in lines[0]
    ecdd = [int(ln.split("ecdd:")[1].split()[0]) for ln in lines]
    eraw = [int(ln.split("eraw:")[1].split()[0]) for ln in lines]
    assert ecdd == [0] * 5 and 20 < np.mean(eraw) < 70
    # without -b and without the filter: payload bytes only
    p2 = subprocess.run([exe, "-i", "-", "-", "-s", "240000", "-r", "10000", "--code", os.path.join(ROOT, "pirip_amd", "data", "standin_256_512_4.code"), "-q"],
                        input=u8.tobytes(), capture_output=True)
    assert p2.returncode == 0, p2.stderr
    pay = np.frombuffer(p2.stdout, dtype=np.uint8).reshape(-1, 32)
    assert pay.shape[0] == 5 and list(pay[:, 0]) == [1, 1, 1, 2, 2]
    # an unknown code name is a data drop away, not a crash
    p3 = subprocess.run([exe, "-i", "-", "-", "--code", "H_256_512_4"], input=b"", capture_output=True)
    assert p3.returncode == 2 and b"PIRIP_CODE_DIR" in p3.stderr


@pytest.mark.gpu
def test_ldpc_batch_of_streams_on_device(oracle, built_lib):
    """Batch API: demodulator soft decisions of several streams go straight into pirip_hip_ldpc_rx_batch on the device."""
    import torch
    import pirip_amd
    c = dict(sigutil.CFG1, P=8)
    code = oracle.parse_code_file(CODE)
    B = 5
    streams, bits_tx = [], []
    for s in range(B):
        b = sigutil.run_framer(["--testframes", str(1 + s % 3), "--seq", "--source", hex(s + 1), "/dev/zero", "-"])
        bits_tx.append(b)
        streams.append(_bursts(oracle, c, 2, [b], ebno_db=9.0, seed=20 + s))
    nsamp = min(len(x) for x in streams)
    iq = np.stack([x[:nsamp] for x in streams])
    dev = torch.from_numpy(iq).cuda()
    h = pirip_amd.HipDemod(c["Fs"], c["Rs"], 2, P=8, est_min=500, est_max=25000, nstreams=B)
    maxf = h.max_frames_for(nsamp)
    filt = torch.zeros((B, maxf, 100), dtype=torch.float32, device="cuda")
    nfr = torch.zeros(B, dtype=torch.int32, device="cuda")
    cons = torch.zeros(B, dtype=torch.int64, device="cuda")
    h.demod_batch(dev.data_ptr(), nsamp * 2, nsamp, 0, 0, filt.data_ptr(), maxf * 100, 0, 0, nfr.data_ptr(), cons.data_ptr(), maxf, 0)
    L = pirip_amd.HipLdpc(pirip_amd.STANDIN_CODE, 2, nstreams=B)
    st = torch.zeros((B, maxf), dtype=torch.uint8, device="cuda")
    pl = torch.zeros((B, maxf, 32), dtype=torch.uint8, device="cuda")
    inf = torch.zeros((B, maxf, pirip_amd.LDPC_INFO_PER_CALL), dtype=torch.int32, device="cuda")
    L.rx_batch(filt.data_ptr(), maxf * 100, nfr.data_ptr(), maxf, st.data_ptr(), pl.data_ptr(), inf.data_ptr(), 0)
    torch.cuda.synchronize()
    st, pl, nfr_h = st.cpu().numpy(), pl.cpu().numpy(), nfr.cpu().numpy()
    filt_h = filt.cpu().numpy()
    for s in range(B):
        good = pl[s][(st[s] & RX_BITS) != 0]
        assert 1 <= good.shape[0] <= 1 + s % 3 and all(g[0] == s + 1 for g in good)      # (a false lock before the burst can cost a frame)
        o = oracle.OracleLdpc(code, 2)
        ws, wp, _ = o.rx(filt_h[s, :nfr_h[s]])
        assert np.array_equal(st[s, :nfr_h[s]], ws) and np.array_equal(pl[s, :nfr_h[s]], wp)


@pytest.mark.gpu
def test_ldpc_batches_with_ragged_call_counts_carry_state_like_the_oracle(oracle, built_lib):
    """Batch API under awkward shapes: call counts that are not multiples of the 32-call LLR tile, streams with fewer valid
    calls than the batch and none at all, three batches in a row (sync state and the two-frame history carry over). Calls beyond
    d_ncalls[s] are not demodulator output: the receiver must advance by the VALID calls only -- the oracle is fed just those,
    back to back, as upstream's receiver would be -- and report status 0 / zero payload / info -1 for the rest."""
    import torch
    import pirip_amd
    code = oracle.parse_code_file(CODE)
    c = dict(sigutil.CFG4, P=8)
    M, per = 4, 200
    bits = sigutil.run_framer(["-m", "4", "--testframes", "4", "--bursts", "1", "--seq", "--source", "0x3", "/dev/zero", "-"])
    u8 = _bursts(oracle, c, M, [bits, bits, bits, bits], ebno_db=6.0, seed=31)
    dem = pirip_amd.HipDemod(c["Fs"], c["Rs"], M, P=8, est_min=500, est_max=c["est_max"], in_format=pirip_amd.IN_CU8_CSDR, nstreams=1)
    filt = dem.demod_host(u8)["rx_filt"].reshape(-1, per)
    n1, n2, n3 = 37, 29, 33                                        # three batches of calls, none a multiple of 32
    assert filt.shape[0] >= n1 + n2 + n3 + 9
    B = 4
    valid1 = np.array([37, 17, 0, 37], dtype=np.int32)              # stream 1 runs out early, stream 2 has nothing in batch 1
    valid2 = np.array([29, 29, 20, 0], dtype=np.int32)
    valid3 = np.array([33, 31, 33, 12], dtype=np.int32)
    offs = [0, 3, 9, 1]                                             # every stream starts somewhere else in the recording
    rows = lambda s, a, n: filt[offs[s] + a: offs[s] + a + n]
    L = pirip_amd.HipLdpc(pirip_amd.STANDIN_CODE, M, nstreams=B)
    got = [[], [], [], []]
    want_in = [[], [], [], []]
    consumed = [0] * B
    for ncalls, valid in ((n1, valid1), (n2, valid2), (n3, valid3)):
        host = np.zeros((B, ncalls, per), dtype=np.float32)
        for s in range(B):
            v = int(valid[s])
            host[s, :v] = rows(s, consumed[s], v)
            host[s, v:] = 123.0                                   # must not be read: calls beyond d_ncalls[s] do not exist
            want_in[s].append(rows(s, consumed[s], v))
            consumed[s] += v
        d = torch.from_numpy(host).cuda()
        dv = torch.from_numpy(valid).cuda()
        st = torch.zeros((B, ncalls), dtype=torch.uint8, device="cuda")
        pl = torch.zeros((B, ncalls, 32), dtype=torch.uint8, device="cuda")
        inf = torch.zeros((B, ncalls, pirip_amd.LDPC_INFO_PER_CALL), dtype=torch.int32, device="cuda")
        L.rx_batch(d.data_ptr(), ncalls * per, dv.data_ptr(), ncalls, st.data_ptr(), pl.data_ptr(), inf.data_ptr(), 0)
        torch.cuda.synchronize()
        for s in range(B):
            v = int(valid[s])
            gs_, gp_, gi_ = st[s].cpu().numpy(), pl[s].cpu().numpy(), inf[s].cpu().numpy()
            assert not gs_[v:].any() and not gp_[v:].any() and (gi_[v:] == -1).all(), (s, v)
            got[s].append((gs_[:v], gp_[:v], gi_[:v]))
    nok = 0
    for s in range(B):
        o = oracle.OracleLdpc(code, M)
        ws, wp, wi = o.rx(np.concatenate(want_in[s]))
        gs = np.concatenate([g[0] for g in got[s]]); gp = np.concatenate([g[1] for g in got[s]]); gi = np.concatenate([g[2] for g in got[s]])
        assert np.array_equal(gs, ws), (s, np.where(gs != ws))
        assert np.array_equal(gp, wp), s
        assert np.array_equal(gi, wi), (s, np.where(gi != wi))
        nok += int(((ws & RX_BITS) != 0).sum())
    assert nok >= 8                                                 # frames were decoded along the way, across the batch boundaries


@pytest.mark.gpu
@pytest.mark.parametrize("M,Nsym", [(2, 7), (2, 33), (4, 33), (2, 136), (4, 68), (4, 136), (2, 272), (4, 272), (2, 300), (4, 50)])
def test_unique_word_search_under_awkward_call_sizes(oracle, built_lib, M, Nsym):
    """The unique-word search shares a bit position's error count between the overlapping windows of consecutive calls (chunks of
    Nbits, bpf / Nbits whole chunks + a head of bpf % Nbits positions per window): call sizes that do not divide a frame, divide it
    exactly (bpf = 544 = 4 x 136 = 2 x 272), equal it, are tiny, or exceed half of it; noisy soft decisions with three frames in
    them and long stretches of noise only (the receiver searching, info[2] = the best window's errors); fed in uneven chunks.
    status / payload / info equal the oracle's."""
    import pirip_amd
    code = oracle.parse_code_file(CODE)
    Nbits = Nsym * (1 if M == 2 else 2)
    bits = sigutil.run_framer(["-m", str(M), "--testframes", "3", "--bursts", "1", "--seq", "--source", "0x4", "/dev/zero", "-"])
    rng = np.random.default_rng(100 * M + Nsym)
    lead = rng.integers(0, 2, 977, dtype=np.uint8)
    allbits = np.concatenate([lead, np.frombuffer(bits, dtype=np.uint8), rng.integers(0, 2, 1500, dtype=np.uint8)])
    bps = 1 if M == 2 else 2
    nsym = allbits.size // bps
    sym = allbits[:nsym * bps].reshape(nsym, bps)
    sym = sym[:, 0] if M == 2 else sym[:, 0] * 2 + sym[:, 1]
    ncalls = nsym // Nsym
    sym = sym[:ncalls * Nsym].reshape(ncalls, Nsym)
    esn0 = bps * 10 ** (6.5 / 10.0)
    z = (rng.normal(size=(ncalls, M, Nsym)) + 1j * rng.normal(size=(ncalls, M, Nsym))) / np.sqrt(2)
    ci, si = np.meshgrid(np.arange(ncalls), np.arange(Nsym), indexing="ij")
    z[ci, sym, si] += np.sqrt(esn0)
    filt = (np.abs(z) * 0.37).astype(np.float32).reshape(ncalls, M * Nsym)
    ws, wp, wi = oracle.OracleLdpc(code, M, Nsym=Nsym).rx(filt)
    h = pirip_amd.HipLdpc(CODE, M, Nsym=Nsym)
    gs, gp, gi = [], [], []
    pos = 0
    for n in (1, 5, 59, 2, 113, 10 ** 6):                        # (57 calls = one workgroup of the search: cross it)
        blk = filt[pos:pos + n]
        if not len(blk):
            break
        s_, p_, i_ = h.rx_host(blk)
        gs.append(s_); gp.append(p_); gi.append(i_); pos += n
    gs, gp, gi = np.concatenate(gs), np.concatenate(gp), np.concatenate(gi)
    assert np.array_equal(gs, ws), np.where(gs != ws)
    assert np.array_equal(gp, wp)
    assert np.array_equal(gi, wi), np.where(gi != wi)
    assert ((ws & RX_BITS) != 0).sum() >= 2


from ldpcshapes import _write_random_code      # the repeat-accumulate code writer, shared with test_ldpc_decoders.py


@pytest.mark.gpu
@pytest.mark.parametrize("decoder", DECODERS)
@pytest.mark.parametrize("n,k,wcol", [(200, 104, 3), (136, 104, 3), (600, 296, 3)])
def test_other_code_shapes_take_the_generic_paths(oracle, built_lib, tmp_path, monkeypatch, n, k, wcol, decoder):
    """Nothing in the receiver is specific to the (512,256) stand-in: a (200,104) code whose two-frame window is not a whole
    number of 32-bit words (the hard-decision words then come from their own kernel) and a (136,104) code with check rows of
    degree > 8 (the decoder's two-pass check loop) give the oracle's records, payloads and info columns, through chunked
    single-stream calls. A (600,296) code has more check rows (304) than the generic decoder keeps in registers and none of
    weight > 8: its check pass reads the rows' edge lists from LDS; it has no fast layout, so both decoder settings reach it."""
    import pirip_amd
    monkeypatch.setenv("PIRIP_LDPC_DECODER", decoder)       # ((200,104): row weight 7-8, the decoders' wider build; (136,104) fits neither fast one)
    path = str(tmp_path / "test.code")
    maxdeg = _write_random_code(path, n, k, wcol, seed=n)
    assert (maxdeg > 8) == (n == 136)
    code = oracle.parse_code_file(path)
    c = dict(sigutil.CFG1, P=6)
    p = subprocess.run([os.path.join(BIN, "fsk_ldpc_framer"), "--code", path, "--testframes", "6", "--seq", "--source", "0x5", "/dev/zero", "-"],
                       capture_output=True)
    assert p.returncode == 0, p.stderr
    bits = np.frombuffer(p.stdout, dtype=np.uint8)
    u8 = _bursts(oracle, c, 2, [bits, bits], ebno_db=9.0, seed=n + 1)
    dem = pirip_amd.HipDemod(c["Fs"], c["Rs"], 2, P=6, est_min=500, est_max=c["est_max"], in_format=pirip_amd.IN_CU8_CSDR, nstreams=1)
    filt = dem.demod_host(u8)["rx_filt"]
    o = oracle.OracleLdpc(code, 2)
    ws, wp, wi = o.rx(filt)
    h = pirip_amd.HipLdpc(path, 2)
    gs, gp, gi = [], [], []
    pos = 0
    for nn in (5, 33, 2, 10 ** 6):
        blk = filt[pos:pos + nn]
        if not len(blk):
            break
        s, pl, i = h.rx_host(blk)
        gs.append(s); gp.append(pl); gi.append(i); pos += nn
    gs, gp, gi = np.concatenate(gs), np.concatenate(gp), np.concatenate(gi)
    assert np.array_equal(gs, ws), np.where(gs != ws)
    assert np.array_equal(gp, wp)
    assert np.array_equal(gi, wi), np.where(gi != wi)
    assert ((ws & RX_BITS) != 0).sum() >= 6


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [
    # Fs, Rs, M, P, input format name, mask spacing, fused hand-over expected
    (240000, 10000, 4, 8, "u8d", 0, True),         # BASELINE config 4: 4-FSK Fs=240k Rs=10k + LDPC
    (240000, 10000, 2, 6, "csdr", 0, True),        # rtl_fsk --code at the default rates
    (100000, 10000, 2, 10, "cf32", 0, True),       # rtl_fsk -a 100000 -r 10000 --code (README.md:196)
    (200000, 10000, 4, 10, "cf32", 10000, True),   # rtl_fsk -a 200000 -r 10000 -m 4 --code --mask 10000 (README.md:262)
    (40000, 1000, 2, 10, "cf32", 0, True),         # the services' modem (script/ping:47, script/frame_repeater:36)
    (100000, 10000, 2, 10, "cf32tiny", 0, True),   # the same shape at 1e-17 of the amplitude: |f|^2 below 2^-96, the hand-over's sqrtf / IEEE-quotient path
    (240000, 10000, 2, 12, "u8d", 0, False),       # no wave instance: magnitudes through the work buffer, same records
    (240000, 1000, 2, 15, "csdr", 0, False),       # rtl_fsk -r 1000 --code: the block instance, not soft-capable -- the unfused route as well
    (240000, 1000, 4, 15, "u8d", 2000, False),     # ... 4-FSK with the mask estimator, `-d` format
    (240000, 10000, 4, 8, "u8d", 0, True, "rician"),     # the same two shapes with the code file's llr_map key set to the exact
    (240000, 10000, 2, 6, "csdr", 0, True, "rician"),    # Rician mapping (every other row: the default, codec2's as recalled)
], ids=lambda s: "Fs%d-M%d-P%d-%s-mask%d%s" % (s[0], s[2], s[3], s[4], s[5], "-" + s[7] if len(s) > 7 else ""))
@pytest.mark.parametrize("decoder", DECODERS)
def test_fused_demod_to_ldpc_chain_equals_oracle_on_the_same_magnitudes(oracle, built_lib, tmp_path, monkeypatch, shape, decoder):
    """pirip_hip_fsk_ldpc_rx_batch (IQ -> records in one call): where the demodulator's instance writes the bit LLRs and hard-decision
    words itself, the records must be exactly what the oracle's receiver makes of the soft magnitudes the same demodulator
    hands out on the unfused path -- several streams at different timing offsets, two batches (demodulator state, the
    two-frame soft-bit history and the sync state carry over), ragged frame counts at the batch boundary."""
    import torch
    import pirip_amd
    if decoder != "auto" and (len(shape) > 7 or shape[3] not in (8, 6)):
        pytest.skip("the forced decoder runs on the two command-line shapes of the coded mode")
    monkeypatch.setenv("PIRIP_LDPC_DECODER", decoder)
    Fs, Rs, M, P, fmtname, mask, want_fused = shape[:7]
    code_path = sigutil.code_variant(CODE, tmp_path, shape[7]) if len(shape) > 7 else pirip_amd.STANDIN_CODE
    code = oracle.parse_code_file(code_path)
    c = dict(Fs=Fs, Rs=Rs, M=M, P=P, f1=Rs if Rs == 1000 else 10000, shift=mask if mask else (2 * Rs if Rs == 1000 else 10000))
    Ts = Fs // Rs
    fmt_h, conv, bps = {
        "csdr": (pirip_amd.IN_CU8_CSDR, lambda x: oracle.quantise_cu8(x, amp=14.0), 2),
        "u8d": (pirip_amd.IN_CU8_FSKDEMOD, lambda x: oracle.quantise_cu8(x, amp=14.0), 2),
        "cf32": (pirip_amd.IN_CF32, lambda x: np.ascontiguousarray(x * np.float32(0.37)), 8),
        "cf32tiny": (pirip_amd.IN_CF32, lambda x: np.ascontiguousarray(x * np.float32(1e-17)), 8),
    }[fmtname]
    bits = sigutil.run_framer(["-m", str(M), "--testframes", "3", "--bursts", "1", "--seq", "--source", "0x4", "/dev/zero", "-"])
    rng = np.random.default_rng(77 + P + M)
    gap = 40 * Ts
    segs = [np.zeros((gap, 2), dtype=np.float32)]
    for _ in range(3):
        segs += [sigutil.mod_complex(oracle, c, bits), np.zeros((3 * gap, 2), dtype=np.float32)]
    segs.append(np.zeros((600 * Ts, 2), dtype=np.float32))
    x = np.concatenate(segs)
    eb = 4.0 * Ts / np.log2(M)
    x = (x + rng.normal(0.0, np.sqrt(eb / (10 ** (6.5 / 10.0)) / 2.0), x.shape)).astype(np.float32)      # ~ 6 % raw BER: the decoder iterates
    B = 5
    offs = [0, 7, Ts + 3, 2 * Ts - 1, 5]
    n1 = (x.shape[0] - 3 * Ts) // 2 + 11                           # batch 1 ends mid-frame; the carry goes in front of batch 2
    est_max = min(Fs // 2 - Rs, 90000)
    per = M * 50

    def streams(a, b):
        return np.stack([conv(x[o + a:o + b]) for o in offs])

    # reference: unfused demodulator (soft magnitudes out) per stream over the same two batches -> oracle receiver
    want = []
    for s in range(B):
        dem = pirip_amd.HipDemod(Fs, Rs, M, P=P, est_min=Rs // 2, est_max=est_max, mask=mask, in_format=fmt_h, nstreams=1)
        o = oracle.OracleLdpc(code, M)
        r1 = dem.demod_host(conv(x[offs[s]:offs[s] + n1]))
        tail0 = offs[s] + r1["consumed"]
        r2 = dem.demod_host(conv(x[tail0:offs[s] + x.shape[0] - 3 * Ts]))
        want.append((r1["nframes"], r2["nframes"], o.rx(np.concatenate([r1["rx_filt"], r2["rx_filt"]]))))
    # fused chain, all streams at once. Batch 2 starts at each stream's own consumed position: re-present the tails
    dem = pirip_amd.HipDemod(Fs, Rs, M, P=P, est_min=Rs // 2, est_max=est_max, mask=mask, in_format=fmt_h, nstreams=B)
    L = pirip_amd.HipLdpc(code_path, M, nstreams=B)
    got = [[], [], [], [], []]
    cons_prev = np.zeros(B, dtype=np.int64)
    for batch in range(2):
        if batch == 0:
            host = streams(0, n1)
        else:
            m = min(x.shape[0] - 3 * Ts - int(cons_prev[s]) for s in range(B))
            host = np.stack([conv(x[offs[s] + int(cons_prev[s]):offs[s] + int(cons_prev[s]) + m]) for s in range(B)])
        nsamp = host.shape[1]
        d = torch.from_numpy(host).cuda()
        maxf = dem.max_frames_for(nsamp)
        st = torch.zeros((B, maxf), dtype=torch.uint8, device="cuda")
        pl = torch.zeros((B, maxf, 32), dtype=torch.uint8, device="cuda")
        inf = torch.zeros((B, maxf, pirip_amd.LDPC_INFO_PER_CALL), dtype=torch.int32, device="cuda")
        nfr = torch.zeros(B, dtype=torch.int32, device="cuda")
        cons = torch.zeros(B, dtype=torch.int64, device="cuda")
        L.chain_batch(dem, d.data_ptr(), nsamp * bps, nsamp, st.data_ptr(), pl.data_ptr(), inf.data_ptr(), nfr.data_ptr(), cons.data_ptr(), maxf)
        torch.cuda.synchronize()
        assert L.last_path_fused() == want_fused, shape
        nf = nfr.cpu().numpy()
        for s in range(B):
            v = int(nf[s])
            got[s].append((st[s, :v].cpu().numpy(), pl[s, :v].cpu().numpy(), inf[s, :v].cpu().numpy()))
            assert not st[s, v:].any() and (inf[s, v:] == -1).all()
        cons_prev += cons.cpu().numpy()
    nok = 0
    for s in range(B):
        n1f, n2f, (ws, wp, wi) = want[s]
        gs = np.concatenate([g[0] for g in got[s]]); gp = np.concatenate([g[1] for g in got[s]]); gi = np.concatenate([g[2] for g in got[s]])
        n = min(len(gs), len(ws))
        assert len(got[s][0][0]) == n1f and abs(len(gs) - len(ws)) <= 1, (s, len(gs), len(ws))      # (batch 2 is cut to the shortest stream)
        assert np.array_equal(gs[:n], ws[:n]), (s, np.where(gs[:n] != ws[:n]))
        assert np.array_equal(gp[:n], wp[:n]), s
        assert np.array_equal(gi[:n], wi[:n]), (s, np.where(gi[:n] != wi[:n]))
        nok += int(((ws[:n] & RX_BITS) != 0).sum())
        assert (wi[:n][(ws[:n] & RX_BITS) != 0, 4] > 1).any() or s > 0 or fmtname == "cf32tiny"    # the decoder worked (iterations > 1)
    # (at 1e-17 of the amplitude the 1e-12 in the noise estimate drowns the frame's SNR: soft bits near zero, nothing decodes -- equal records all the same)
    assert nok >= 5 * B or fmtname == "cf32tiny"


@pytest.mark.gpu
@pytest.mark.parametrize("M,ebno", [(2, 6.0), (4, 6.0)])
def test_freedv_api_c_program_records_equal_rtl_fsk_and_the_oracle_chain(oracle, built_lib, tmp_path, M, ebno):
    """a coded receive loop written against libcodec2's FreeDV names (tests/cprog/rtl_fsk_coded_like_upstream.c:
    freedv_open_advanced(FREEDV_MODE_FSK_LDPC) / freedv_nin / freedv_rawdatacomprx / freedv_get_rx_status), compiled as plain C
    against include/pirip_hip.h, linked to libpirip_hip.so. Its `-b` records (status byte + k/8 data bytes per demodulator call,
    tx/frame_repeater.c:55-62) must be byte for byte those of `pirip_amd/bin/rtl_fsk --code ... -b` on the same file and those of
    the oracle chain (CPU demodulator -> mirror receiver) -- three receivers, three demodulator kernels (the shim's handle takes
    complex float: any-configuration kernel; the tool's takes the bytes: wave instance, fused hand-over)."""
    import pirip_amd
    exe = str(tmp_path / "rtl_coded")
    libdir = os.path.dirname(pirip_amd.lib_path())
    subprocess.check_call(["gcc", "-std=gnu11", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cprog", "rtl_fsk_coded_like_upstream.c"), "-L", libdir, "-lpirip_hip",
                           "-Wl,-rpath," + libdir, "-lm"])
    code = oracle.parse_code_file(CODE)
    c = dict(sigutil.CFG1 if M == 2 else sigutil.CFG4, P=6)                 # Ts = 24 -> P = 6: the FSK_LDPC oversample rule
    bits = sigutil.run_framer(["-m", str(M), "--testframes", "4", "--bursts", "1", "--seq", "--source", "0x3", "/dev/zero", "-"])
    u8 = _bursts(oracle, c, M, [bits, bits], ebno_db=ebno, seed=90 + M)
    lo, hi = 5000, c["est_max"]
    p = subprocess.run([exe, CODE, str(M), "240000", "10000", str(lo), str(hi), "v"], input=u8.tobytes(), capture_output=True)
    assert p.returncode == 0, p.stderr[-2000:]
    nb = code["k"] // 8
    st_c, pl_c = _records(p.stdout, nb)
    # the repo's own rtl_fsk on the same bytes (README.md:184's shape + -b)
    t = subprocess.run([os.path.join(BIN, "rtl_fsk"), "-s", "240000", "-r", "10000", "-m", str(M), "-l", str(lo), "-U", str(hi), "--code", CODE, "-q", "-b",
                        "-"], input=u8.tobytes(), capture_output=True, env=dict(os.environ, PIRIP_IQ_FILE="/dev/stdin"))
    assert t.returncode == 0, t.stderr[-2000:]
    st_t, pl_t = _records(t.stdout, nb)
    # oracle chain
    r = oracle.OracleFsk(c["Fs"], c["Rs"], M, P=6, est_min=lo, est_max=hi).demod(u8, oracle.IN_CU8_CSDR)
    st_o, pl_o, info_o = oracle.OracleLdpc(code, M).rx(r["rx_filt"])
    pl_o = np.where(((st_o & RX_BITS) != 0)[:, None], pl_o, 0)            # -b: zeros when no frame
    n = len(st_o)
    assert len(st_c) == n and len(st_t) >= n - 1
    good = int(((st_o & RX_BITS) != 0).sum())
    assert good >= 6, good
    assert np.array_equal(st_c, st_o) and np.array_equal(pl_c, pl_o), np.where(st_c != st_o)
    m = min(n, len(st_t))
    assert np.array_equal(st_t[:m], st_o[:m]) and np.array_equal(pl_t[:m], pl_o[:m])
    # freedv_set_verbose(2): one line per decoded frame with the reference's columns (README.md:200-208)
    vl = [ln for ln in p.stderr.decode().split("\n") if " uw_loc: " in ln]
    assert len(vl) == int((info_o[:, 6] >= 0).sum()) and all(" iter: " in ln and " rxst: " in ln for ln in vl)
    assert sum(" ecdd:   0 " in ln for ln in vl) >= good - 1                # test frames: the payload is the known one (bytes 0,1: source, sequence)


# ---- the independent CPU receiver (oracle/ldpc_independent.c): what the product's precision choices are measured against ----
def test_recalled_logbesseli0_tracks_ln_i0(oracle):
    """The five segments of CML / codec2's logbesseli0 as recalled [UPSTREAM-RECALLED] against ln I0 itself (scipy): a
    mis-remembered coefficient would miss by far more than these fit errors."""
    from scipy.special import ive
    code = oracle.parse_code_file(CODE)
    d = oracle.IndepLdpc(code, 2, mode=2)
    xs = np.linspace(0.0, 60.0, 6001)
    true = np.log(ive(0, xs)) + xs
    mine = np.array([d.l.indep_ln_i0(float(x)) for x in xs])
    rec = np.array([d.l.indep_logbesseli0_recalled(float(x)) for x in xs])
    assert np.abs(mine - true).max() < 1e-6                       # the independent receiver's own ln I0 is exact
    for lo, hi, bound in ((0, 1, 0.0015), (1, 2, 0.002), (2, 5, 0.012), (5, 20, 0.035), (20, 60.01, 0.065)):
        m = (xs >= lo) & (xs < hi)
        assert np.abs(rec - true)[m].max() < bound, (lo, hi, np.abs(rec - true)[m].max())


def _llr_bar(llr_map, li):
    """(live mask, tolerance) of product-arithmetic LLRs against the independent receiver's li.
    rician: the product clamps at +-24; table ln I0 (1/8 steps, linear; beyond x = 32 continued with slope 1 where the true slope is
    1 - 1/2x: up to 0.4 % of a large LLR) + binary16 rounding (2^-11 relative).
    upstream: the same polynomial on both sides (float32 here, float32 there), argument formed as k |r| instead of
    2 SNR sqrt(r^2 / v^2), wave-order instead of serial frame sums (last float bits), binary16 rounding; clamp at +-1000."""
    if llr_map == "rician":
        return np.abs(li) < 23.0, 0.02 + np.abs(li) * 0.005
    return np.abs(li) < 990.0, 0.005 + np.abs(li) * 0.001


def _llr_check(llr_map, lm, li):
    live, tol = _llr_bar(llr_map, li)
    over = (np.abs(lm - li) > tol) & live
    if llr_map == "upstream":
        # logbesseli0's five pieces do not meet (jumps of 0.003 / 0.012 / 0.038 / 0.067 at x = 1, 2, 5, 20): an argument within a float
        # ulp of a break point can fall on the other side of it in the other evaluation order -- allowed for 1 value in 10^4, within the jump
        assert over.sum() <= max(1, lm.size // 10000) and np.all(np.abs(lm - li)[over] <= 0.07 + tol[over]), (int(over.sum()), float(np.abs(lm - li)[live].max()))
    else:
        assert not over.any(), float(np.abs(lm - li)[live].max())


@pytest.mark.parametrize("llr_map", ["upstream", "rician"])
@pytest.mark.parametrize("M,ebno", [(2, 6.5), (4, 6.5)])
def test_independent_receiver_agrees_with_the_mirror_oracle(oracle, built_lib, M, ebno, llr_map):
    """CPU only: the mirror oracle (binary16 soft bits, wave-order sums, table phi / ln I0 -- the kernel's arithmetic) against the
    independent receiver (float32, serial sums, exact ln I0, double sum-product) on the same soft decisions. LLRs within a stated
    tolerance, every frame delivered by one delivered by the other with the same bytes, iteration counts within one."""
    code = oracle.parse_code_file(CODE)
    c = dict(sigutil.CFG1 if M == 2 else sigutil.CFG4, P=6 if M == 2 else 8)
    bits = sigutil.run_framer(["-m", str(M), "--testframes", "5", "--bursts", "1", "--seq", "--source", "0x2", "/dev/zero", "-"])
    u8 = _bursts(oracle, c, M, [bits, bits], ebno_db=ebno, seed=40 + M)
    r = oracle.OracleFsk(c["Fs"], c["Rs"], M, P=c["P"], est_min=500, est_max=c["est_max"]).demod(u8, oracle.IN_CU8_CSDR)
    mir, ind = oracle.OracleLdpc(code, M, llr_map=llr_map), oracle.IndepLdpc(code, M, mode=3 if llr_map == "upstream" else 1)
    lm, li = mir.llr(r["rx_filt"]), ind.llr(r["rx_filt"])
    _llr_check(llr_map, lm, li)
    assert np.all(np.sign(lm[np.abs(li) > 0.1]) == np.sign(li[np.abs(li) > 0.1]))
    sm, pm, im = mir.rx(r["rx_filt"])
    si, pi, ii = ind.rx(r["rx_filt"])
    okm, oki = (sm & RX_BITS) != 0, (si & RX_BITS) != 0
    assert okm.sum() >= 8 and np.array_equal(okm, oki)
    assert np.array_equal(pm[okm], pi[oki])
    assert np.abs(im[okm, 4] - ii[oki, 4]).max() <= 1, (im[okm, 4], ii[oki, 4])
    assert np.array_equal(im[:, :4], ii[:, :4])                   # sync state, UW position / errors / misses: call for call


@pytest.mark.gpu
@pytest.mark.parametrize("llr_map", ["upstream", "rician"])
@pytest.mark.parametrize("M,ebno", [(2, 6.5), (4, 6.5)])
def test_gpu_receiver_against_the_independent_float32_receiver(oracle, built_lib, tmp_path, M, ebno, llr_map):
    """the GPU against a checker that does NOT share its arithmetic. LLRs (pirip_hip_ldpc_llr) within a
    stated tolerance of float32 / exact-ln-I0 LLRs; decoded payloads, status bytes and sync columns equal; iterations within one."""
    import torch
    import pirip_amd
    code = oracle.parse_code_file(CODE)
    c = dict(sigutil.CFG1 if M == 2 else sigutil.CFG4, P=6 if M == 2 else 8)
    bits = sigutil.run_framer(["-m", str(M), "--testframes", "5", "--bursts", "1", "--seq", "--source", "0x2", "/dev/zero", "-"])
    u8 = _bursts(oracle, c, M, [bits, bits, bits], ebno_db=ebno, seed=50 + M)
    dem = pirip_amd.HipDemod(c["Fs"], c["Rs"], M, P=c["P"], est_min=500, est_max=c["est_max"], in_format=pirip_amd.IN_CU8_CSDR, nstreams=1)
    filt = dem.demod_host(u8)["rx_filt"]
    ind = oracle.IndepLdpc(code, M, mode=3 if llr_map == "upstream" else 1)      # the product's default against the RECALLED codec2 mapping (and phi0 range)
    h = pirip_amd.HipLdpc(sigutil.code_variant(CODE, tmp_path, llr_map), M)
    d = torch.from_numpy(np.ascontiguousarray(filt)).cuda()
    out = torch.zeros((filt.shape[0], ind.Nbits), dtype=torch.float32, device="cuda")
    pirip_amd.binding._chk(h.L.pirip_hip_ldpc_llr(h.h, d.data_ptr(), filt.shape[0], out.data_ptr(), 0), "llr")
    torch.cuda.synchronize()
    lg, li = out.cpu().numpy(), ind.llr(filt)
    _llr_check(llr_map, lg, li)                                   # see the CPU test above for where the bars come from
    gs, gp, gi = h.rx_host(filt)
    si, pi, ii = ind.rx(filt)
    okg, oki = (gs & RX_BITS) != 0, (si & RX_BITS) != 0
    assert okg.sum() >= 12 and np.array_equal(gs, si)
    assert np.array_equal(gp[okg], pi[oki])
    assert np.abs(gi[okg, 4] - ii[oki, 4]).max() <= 1
    assert np.array_equal(gi[:, :4], ii[:, :4])


@pytest.mark.gpu
def test_chain_in_groups_on_prioritised_streams_writes_the_same_records(oracle, built_lib):
    """pirip_hip_fsk_ldpc_rx_batch_groups: five channels as groups of 3 + 2 (own handle pairs, own HIP streams inside the library, fork /
    join around the caller's stream), two batches in a row (state carries per group): every record equals what ONE handle pair over
    the five channels writes with pirip_hip_fsk_ldpc_rx_batch."""
    import torch
    import pirip_amd
    c = dict(sigutil.CFG4, P=8)
    M = 4
    bits = sigutil.run_framer(["-m", "4", "--testframes", "3", "--bursts", "1", "--seq", "--source", "0x5", "/dev/zero", "-"])
    u8 = _bursts(oracle, c, M, [bits, bits, bits], ebno_db=6.5, seed=41)
    B, nsamp = 5, 2 * ((u8.shape[0] - 40) // 4)
    host = np.stack([u8[3 * s: 3 * s + 2 * nsamp] for s in range(B)])                     # every channel its own start offset
    mk = lambda n: (pirip_amd.HipDemod(c["Fs"], c["Rs"], M, P=8, est_min=500, est_max=c["est_max"], in_format=pirip_amd.IN_CU8_CSDR, nstreams=n),
                    pirip_amd.HipLdpc(pirip_amd.STANDIN_CODE, M, nstreams=n))
    d1, l1 = mk(B)
    (da, la), (db, lb) = mk(3), mk(2)
    maxf = d1.max_frames_for(nsamp)
    out = lambda n: (torch.zeros((n, maxf), dtype=torch.uint8, device="cuda"), torch.zeros((n, maxf, 32), dtype=torch.uint8, device="cuda"),
                     torch.zeros((n, maxf, pirip_amd.LDPC_INFO_PER_CALL), dtype=torch.int32, device="cuda"),
                     torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int64, device="cuda"))
    ok = 0
    for half in range(2):
        dev = torch.from_numpy(np.ascontiguousarray(host[:, half * nsamp:(half + 1) * nsamp])).cuda()
        s1, p1, i1, n1, c1 = out(B)
        l1.chain_batch(d1, dev.data_ptr(), nsamp * 2, nsamp, s1.data_ptr(), p1.data_ptr(), i1.data_ptr(), n1.data_ptr(), c1.data_ptr(), maxf)
        s2, p2, i2, n2, c2 = out(B)
        pirip_amd.HipLdpc.chain_batch_groups(
            [(la, da, dev[0].data_ptr(), s2[0].data_ptr(), p2[0].data_ptr(), i2[0].data_ptr(), n2[0:].data_ptr(), c2[0:].data_ptr()),
             (lb, db, dev[3].data_ptr(), s2[3].data_ptr(), p2[3].data_ptr(), i2[3].data_ptr(), n2[3:].data_ptr(), c2[3:].data_ptr())],
            nsamp * 2, nsamp, maxf)
        torch.cuda.synchronize()
        assert torch.equal(n1, n2) and torch.equal(c1, c2)
        assert torch.equal(s1, s2) and torch.equal(p1, p2) and torch.equal(i1, i2)
        ok += int(((s1 & RX_BITS) != 0).sum())
    assert ok >= 5


@pytest.mark.gpu
def test_chain_split_into_two_stream_ranges_writes_the_same_records(oracle, built_lib, monkeypatch):
    """pirip_hip_fsk_ldpc_rx_batch runs a big batch as two ranges of streams on two internal HIP streams (from 4096 streams; the
    threshold is moved down here): seven channels, two batches in a row, split 4 + 3 against not split at all -- records, frame and
    sample counts identical, and the state that carries to the second batch with them."""
    import torch
    import pirip_amd
    c = dict(sigutil.CFG4, P=8)
    M, B = 4, 7
    bits = sigutil.run_framer(["-m", "4", "--testframes", "3", "--bursts", "1", "--seq", "--source", "0x6", "/dev/zero", "-"])
    u8 = _bursts(oracle, c, M, [bits, bits, bits], ebno_db=6.5, seed=43)
    nsamp = 2 * ((u8.shape[0] - 60) // 4)
    host = np.stack([u8[5 * s: 5 * s + 2 * nsamp] for s in range(B)])
    res = {}
    # split: the default (two ranges, the first one's decode beside the second one's demodulator on the small decoder); bank: both ranges on the
    # persistent decoder; low: the first range's decode on the lowest-priority internal stream; three / four ranges: the experiment knob
    for mode, env, eighths, overlap in (("split", "2", None, None), ("bank", "2", None, "off"), ("low", "2", None, "fast-low"), ("three", "2", "3,6", "fast"),
                                        ("four", "2", "2,4,6", None), ("whole", "0", None, None)):
        monkeypatch.setenv("PIRIP_CHAIN_SPLIT_MIN", env)
        for name, val in (("PIRIP_CHAIN_SPLIT_EIGHTHS", eighths), ("PIRIP_CHAIN_OVERLAP_DECODER", overlap)):     # (both read at create)
            if val: monkeypatch.setenv(name, val)
            else: monkeypatch.delenv(name, raising=False)
        d = pirip_amd.HipDemod(c["Fs"], c["Rs"], M, P=8, est_min=500, est_max=c["est_max"], in_format=pirip_amd.IN_CU8_CSDR, nstreams=B)
        l = pirip_amd.HipLdpc(pirip_amd.STANDIN_CODE, M, nstreams=B)
        maxf = d.max_frames_for(nsamp)
        got = []
        for half in range(2):
            dev = torch.from_numpy(np.ascontiguousarray(host[:, half * nsamp:(half + 1) * nsamp])).cuda()
            st = torch.zeros((B, maxf), dtype=torch.uint8, device="cuda"); pl = torch.zeros((B, maxf, 32), dtype=torch.uint8, device="cuda")
            inf = torch.zeros((B, maxf, pirip_amd.LDPC_INFO_PER_CALL), dtype=torch.int32, device="cuda")
            nf = torch.zeros(B, dtype=torch.int32, device="cuda"); cons = torch.zeros(B, dtype=torch.int64, device="cuda")
            stats = torch.zeros((B, maxf, pirip_amd.STATS_PER_FRAME), dtype=torch.float32, device="cuda")
            l.chain_batch(d, dev.data_ptr(), nsamp * 2, nsamp, st.data_ptr(), pl.data_ptr(), inf.data_ptr(), nf.data_ptr(), cons.data_ptr(), maxf,
                          d_stats=stats.data_ptr(), stats_stride=maxf * pirip_amd.STATS_PER_FRAME)
            torch.cuda.synchronize()
            assert l.last_path_fused()
            got.append([t.cpu().numpy() for t in (st, pl, inf, nf, cons, stats)])
        res[mode] = got
    for mode in ("split", "bank", "low", "three", "four"):
        for a, b in zip(res[mode], res["whole"]):
            for x, y in zip(a, b):
                assert np.array_equal(x.view(np.uint8) if x.dtype == np.float32 else x, y.view(np.uint8) if y.dtype == np.float32 else y), mode
    assert int(((res["whole"][0][0] & RX_BITS) != 0).sum() + ((res["whole"][1][0] & RX_BITS) != 0).sum()) >= 7


def _chain_outputs(torch, pirip_amd, B, maxf):
    return (torch.zeros((B, maxf), dtype=torch.uint8, device="cuda"), torch.zeros((B, maxf, 32), dtype=torch.uint8, device="cuda"),
            torch.zeros((B, maxf, pirip_amd.LDPC_INFO_PER_CALL), dtype=torch.int32, device="cuda"),
            torch.zeros(B, dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.int64, device="cuda"))


@pytest.mark.gpu
@pytest.mark.parametrize("which", [0, 1])
def test_chain_split_joins_the_callers_stream_when_a_range_fails(oracle, built_lib, monkeypatch, which):
    """A split call whose first / second range reports an error after the fork (PIRIP_CHAIN_TEST_FAIL, read at create: the hook
    of this test) still joins both internal streams back into the caller's: the error comes back, and a healthy receiver
    enqueued on the same HIP stream right behind it -- no synchronisation in between -- writes exactly the records it writes
    alone. The failing handle can be called again (its streams and events are the handle's, made once) and destroyed."""
    import torch
    import pirip_amd
    c = dict(sigutil.CFG4, P=8)
    M, B = 4, 7
    bits = sigutil.run_framer(["-m", "4", "--testframes", "3", "--bursts", "1", "--seq", "--source", "0x7", "/dev/zero", "-"])
    u8 = _bursts(oracle, c, M, [bits, bits], ebno_db=6.5, seed=47)
    nsamp = (u8.shape[0] - 60) // 2
    host = np.stack([u8[5 * s: 5 * s + nsamp] for s in range(B)])
    dev = torch.from_numpy(np.ascontiguousarray(host)).cuda()
    mk = lambda: (pirip_amd.HipDemod(c["Fs"], c["Rs"], M, P=8, est_min=500, est_max=c["est_max"], in_format=pirip_amd.IN_CU8_CSDR, nstreams=B),
                  pirip_amd.HipLdpc(pirip_amd.STANDIN_CODE, M, nstreams=B))
    monkeypatch.setenv("PIRIP_CHAIN_SPLIT_MIN", "2")
    d_ref, l_ref = mk()
    d_ok, l_ok = mk()
    monkeypatch.setenv("PIRIP_CHAIN_TEST_FAIL", str(which))
    d_bad, l_bad = mk()
    monkeypatch.delenv("PIRIP_CHAIN_TEST_FAIL")
    maxf = d_ref.max_frames_for(nsamp)
    ref = _chain_outputs(torch, pirip_amd, B, maxf)
    l_ref.chain_batch(d_ref, dev.data_ptr(), nsamp * 2, nsamp, ref[0].data_ptr(), ref[1].data_ptr(), ref[2].data_ptr(), ref[3].data_ptr(), ref[4].data_ptr(), maxf)
    torch.cuda.synchronize()
    assert int(((ref[0] & RX_BITS) != 0).sum()) >= 7
    s = torch.cuda.Stream()
    junk = _chain_outputs(torch, pirip_amd, B, maxf)
    got = _chain_outputs(torch, pirip_amd, B, maxf)
    torch.cuda.synchronize()
    for _ in range(2):
        with pytest.raises(pirip_amd.binding.PiripError):
            l_bad.chain_batch(d_bad, dev.data_ptr(), nsamp * 2, nsamp, junk[0].data_ptr(), junk[1].data_ptr(), junk[2].data_ptr(), junk[3].data_ptr(), junk[4].data_ptr(),
                              maxf, stream=s.cuda_stream)
    l_ok.chain_batch(d_ok, dev.data_ptr(), nsamp * 2, nsamp, got[0].data_ptr(), got[1].data_ptr(), got[2].data_ptr(), got[3].data_ptr(), got[4].data_ptr(), maxf,
                     stream=s.cuda_stream)
    s.synchronize()
    torch.cuda.synchronize()                                     # (whatever the failed calls did launch has drained too)
    for a, b in zip(got, ref):
        assert torch.equal(a, b)
    del l_bad, d_bad


@pytest.mark.gpu
def test_two_chain_receivers_of_4096_streams_on_two_hip_streams_concurrently(oracle, built_lib):
    """Two (demodulator, FSK_LDPC receiver) pairs of 4096 streams each -- enough for each call to split into its two stream ranges on
    ITS OWN internal HIP streams -- enqueued on two caller streams without synchronisation, three rounds: each writes the records
    it writes alone on the default stream (the persistent decoder serves both: 4096 x ~10 frames fill the chip)."""
    import torch
    import pirip_amd
    c = dict(sigutil.CFG4, P=8)
    M, B = 4, 4096
    outs = []
    pairs = []
    data = []
    for k, (seed, ebno) in enumerate(((51, 6.0), (53, 4.5))):
        bits = sigutil.run_framer(["-m", "4", "--testframes", "3", "--bursts", "1", "--seq", "--source", hex(8 + k), "/dev/zero", "-"])
        u8 = _bursts(oracle, c, M, [bits, bits], ebno_db=ebno, seed=seed)
        nsamp = u8.shape[0] - 64
        d = torch.from_numpy(u8).cuda()
        dev = torch.empty((B, nsamp, 2), dtype=torch.uint8, device="cuda")
        for o in range(16):
            dev[o::16] = d[3 * o: 3 * o + nsamp].unsqueeze(0)
        data.append((dev, nsamp))
        pairs.append((pirip_amd.HipDemod(c["Fs"], c["Rs"], M, P=8, est_min=500, est_max=c["est_max"], in_format=pirip_amd.IN_CU8_CSDR, nstreams=B),
                      pirip_amd.HipLdpc(pirip_amd.STANDIN_CODE, M, nstreams=B)))
    ref = []
    for (dm, ld), (dev, nsamp) in zip(pairs, data):
        maxf = dm.max_frames_for(nsamp)
        o = _chain_outputs(torch, pirip_amd, B, maxf)
        ld.chain_batch(dm, dev.data_ptr(), nsamp * 2, nsamp, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), o[4].data_ptr(), maxf)
        torch.cuda.synchronize()
        ref.append([t.clone() for t in o])
        assert int(((o[0] & RX_BITS) != 0).sum()) >= B                       # frames decode on every stream
        outs.append(o)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for _ in range(3):
        for (dm, ld), (dev, nsamp), o, s in zip(pairs, data, outs, streams):
            dm.reset(s.cuda_stream); ld.reset(s.cuda_stream)
            for t in o[:3]:
                with torch.cuda.stream(s):
                    t.zero_()
            ld.chain_batch(dm, dev.data_ptr(), nsamp * 2, nsamp, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), o[4].data_ptr(),
                           dm.max_frames_for(nsamp), stream=s.cuda_stream)
    torch.cuda.synchronize()
    for o, r in zip(outs, ref):
        for a, b in zip(o, r):
            assert torch.equal(a, b)
