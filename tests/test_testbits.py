"""include/pirip_hip.h section L: the test-frame counter on the device (pirip_hip_tbits_*, pirip_amd.HipTestBits) and
rtl_fsk_channels --put-test-bits. Every comparison is exact integer equality with the numpy reference (tests/tbitsref.py), which
tests/test_testbits_cpu.py holds to the CPU counter and whose inputs (tests/tbitsshapes.py) it shows to reach their cases."""
import os
import subprocess

import numpy as np
import pytest

import chanref
import sigutil
import tbitsref
import tbitsshapes as ts

pytestmark = pytest.mark.gpu

BIN = tbitsref.BIN


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _padded(rows, extra=3):
    """the rows on the device inside a larger allocation: the stride per stream is larger than the stream's rows"""
    import torch
    n, maxf, rb = rows.shape
    buf = torch.full((n, maxf + extra, rb), 0xA5, dtype=torch.uint8, device="cuda")
    buf[:, :maxf] = _dev(rows)
    return buf[:, :maxf]


def _push_calls(tb, rows, nframes, splits, packed, row_bits):
    """the rows as consecutive calls of splits[k] rows; stream s has nframes[s] rows in all (None: every row)"""
    import torch
    n, maxf = rows.shape[0], rows.shape[1]
    data = tbitsref.pack_rows(rows, pad=1) if packed else rows
    r0 = 0
    for k in splits:
        part = _padded(data[:, r0:r0 + k]) if k else torch.zeros((n, 0, data.shape[2]), dtype=torch.uint8, device="cuda")
        nf = None if nframes is None else _dev((np.clip(nframes, 0, maxf) - r0).clip(0, k).astype(np.int32))
        tb.push(part, nframes=nf, row_bits=row_bits, packed=packed)
        r0 += k
    assert r0 == maxf


def _assert_counters(tb, want, what=""):
    got = tb.counters()
    for k in tbitsref.NAMES:
        assert np.array_equal(got[k], want[k]), (what, k, got[k][:8], want[k][:8])


@pytest.mark.parametrize("packed", [False, True], ids=["bytes", "packed"])
def test_synthetic_rows(built_lib, packed):
    import pirip_amd
    rows, S = ts.syn_rows(), ts.SYN
    nf = S["nframes"]
    tb = pirip_amd.HipTestBits(nstreams=5)
    for splits in ([S["max_frames"]], ts.SYN_SPLITS):
        tb.reset()
        _push_calls(tb, rows, nf, splits, packed, S["row_bits"])
        _assert_counters(tb, ts.syn_want(tuple(nf)), splits)
    # no row counts: every stream has max_frames rows
    tb.reset()
    _push_calls(tb, rows, None, [S["max_frames"]], packed, S["row_bits"])
    _assert_counters(tb, ts.syn_want((9,) * 5), "nframes None")
    # row counts below 0 and above max_frames are clamped
    tb.reset()
    data = tbitsref.pack_rows(rows, pad=1) if packed else rows
    tb.push(_padded(data), nframes=_dev(np.array([-3, 1, 2, 7, 12], dtype=np.int32)), row_bits=S["row_bits"], packed=packed)
    _assert_counters(tb, ts.syn_want(tuple(nf)), "clamped")
    assert tb.counters_device() != 0            # (where a caller that stays on the device reads the same numbers)
    tb.close()


@pytest.mark.parametrize("F,thresh,e,valid", ts.LIMIT_CASES)
def test_errors_exactly_at_the_limit(built_lib, F, thresh, e, valid):
    import pirip_amd
    bits = ts.limit_bits(F, e)
    tb = pirip_amd.HipTestBits(framesize=F, valid_thresh=thresh, nstreams=1)
    tb.push(_dev(bits.reshape(1, 2, F)))
    got = tb.counters()
    assert (got["packets"][0], got["bits"][0], got["errors"][0], got["pushed"][0]) == ((1, F, e, 2 * F) if valid else (0, 0, 0, 2 * F))
    tb.close()


@pytest.mark.parametrize("F", ts.SWEEP_F)
def test_frame_size_sweep(built_lib, F):
    import pirip_amd
    bits, want = ts.sweep_bits(F), ts.sweep_want(F)
    tb = pirip_amd.HipTestBits(framesize=F, valid_thresh=ts.sweep_thresh(F), frame=ts.sweep_frame(F), nstreams=bits.shape[0])
    for rb in ts.SWEEP_ROW_BITS:
        rows = bits.reshape(bits.shape[0], -1, rb)
        nrows = rows.shape[1]
        tb.reset()
        _push_calls(tb, rows, None, [nrows], False, rb)
        _assert_counters(tb, want, (F, rb, "bytes"))
        tb.reset()
        _push_calls(tb, rows, None, [nrows // 3, nrows - nrows // 3], True, rb)
        _assert_counters(tb, want, (F, rb, "packed, two calls"))
    tb.close()


def test_frame_size_limit(built_lib):
    import pirip_amd
    with pytest.raises(pirip_amd.PiripError, match=r"\(-6\)"):
        pirip_amd.HipTestBits(framesize=4097, frame=np.zeros(4097, dtype=np.uint8))
    pirip_amd.HipTestBits(framesize=4096, frame=np.zeros(4096, dtype=np.uint8)).close()


def test_grid_edges(built_lib):
    import pirip_amd
    # more streams than a wave has lanes
    rows = ts.many_streams()
    tb = pirip_amd.HipTestBits(nstreams=300)
    tb.push(_dev(rows))
    _assert_counters(tb, ts.want_of("many"), "300 streams")
    tb.close()
    # one stream over many tiles, bytes and packed
    rows = ts.long_stream()
    tb = pirip_amd.HipTestBits(nstreams=1)
    for packed in (False, True):
        tb.reset()
        _push_calls(tb, rows, None, [rows.shape[1]], packed, 50)
        _assert_counters(tb, ts.want_of("long"), ("3000 rows", packed))
    tb.close()
    # the history survives 200 calls of one row
    rows = rows[:, :600].reshape(3, 200, 50)
    tb = pirip_amd.HipTestBits(nstreams=3)
    d = _dev(rows)
    for r in range(200):
        tb.push(d[:, r:r + 1])
    _assert_counters(tb, ts.want_of("calls200"), "200 calls")
    tb.close()


def test_reset_gives_the_created_state(built_lib):
    import pirip_amd
    rows, S = ts.syn_rows(), ts.SYN
    tb = pirip_amd.HipTestBits(nstreams=5)
    tb.set_payload(ts.REC_DB)
    st, pl, info, nc = ts.crafted_records(pirip_amd.testframe_payload(8 * ts.REC_DB))
    tb.push(_dev(rows[:, :4]))                  # an odd number of calls, history in the middle of a frame
    tb.push_records(_dev(np.tile(st, (2, 1))[:5]), _dev(np.tile(pl, (2, 1, 1))[:5]), _dev(np.tile(info, (2, 1, 1))[:5]))
    assert tb.counters()["pushed"].sum() > 0 and tb.record_counters()["crc_ok"].sum() > 0
    tb.reset()
    assert all(not v.any() for v in tb.counters().values()) and all(not v.any() for v in tb.record_counters().values())
    _push_calls(tb, rows, S["nframes"], [S["max_frames"]], False, S["row_bits"])
    _assert_counters(tb, ts.syn_want(tuple(S["nframes"])), "after reset")
    tb.close()


# ---- behind the real receiver -------------------------------------------------------------------------------------------------------
NSTREAMS, NFRAMES = 4, 40
AMP = 14.0
SIGMA = float(np.sqrt(4.0 * 24 / (10 ** 0.75) / 2.0))          # Eb/N0 = 7.5 dB at 24 samples per symbol: a few per cent raw bit errors


def _test_signal(oracle, sigma):
    """u8 IQ [4, nsamp * 2] on the device: the test frames, every stream from its own timing offset"""
    import torch
    from pirip_amd.binding import synth_cu8
    c = sigutil.CFG1
    ts_ = c["Fs"] // c["Rs"]
    nsym = NFRAMES * 50 + 60
    bits = oracle.get_test_bits(nsym)
    nsamp = NFRAMES * 50 * ts_
    d_bits = _dev(bits)
    out = torch.zeros((NSTREAMS, nsamp * 2), dtype=torch.uint8, device="cuda")
    synth_cu8(c["Fs"], c["Rs"], c["M"], [c["f1"]] * NSTREAMS, c["shift"], d_bits.data_ptr(), 0, nsym, out.data_ptr(), nsamp * 2, nsamp,
              amp=AMP, sigma=sigma, seed=5, skip=[0, 7, 13, 22], stream=torch.cuda.current_stream().cuda_stream)
    return out, nsamp


def _want_of_bits(bits, nf, row_bits):
    """the reference on downloaded bit rows [n, rows, bytes] (one bit per byte, or packed)"""
    rows = bits if bits.shape[2] == row_bits else np.unpackbits(bits, axis=-1)[..., :row_bits]
    return tbitsref.count_streams(rows, nf, ts.default_frame(), 0.1)


@pytest.mark.parametrize("packed", [False, True], ids=["bytes", "packed"])
@pytest.mark.parametrize("noisy", [False, True], ids=["clean", "noisy"])
def test_behind_the_demodulator(oracle, built_lib, noisy, packed):
    """synth_cu8 -> HipDemod (the wave kernel) -> HipTestBits on one HIP stream, nothing synchronised in between"""
    import torch
    import pirip_amd
    c = sigutil.CFG1
    iq, nsamp = _test_signal(oracle, SIGMA if noisy else 0.0)
    dem = pirip_amd.HipDemod(c["Fs"], c["Rs"], c["M"], P=c["P"], est_min=c["est_min"], est_max=c["est_max"], nstreams=NSTREAMS)
    assert dem.kernel() == "wave"
    if packed:
        dem.set_bit_packing(True)
    rb = (dem.Nbits + 7) // 8 if packed else dem.Nbits
    rows = dem.max_frames_for(nsamp)
    bits = torch.zeros((NSTREAMS, rows, rb), dtype=torch.uint8, device="cuda")
    nfr = torch.zeros(NSTREAMS, dtype=torch.int32, device="cuda")
    tb = pirip_amd.HipTestBits(nstreams=NSTREAMS)
    st = torch.cuda.current_stream().cuda_stream
    dem.demod_batch(iq.data_ptr(), nsamp * 2, nsamp, bits.data_ptr(), rows * rb, d_nframes=nfr.data_ptr(), max_frames=rows, stream=st)
    tb.push(bits, nframes=nfr, row_bits=dem.Nbits, packed=packed, stream=st)
    got = tb.counters()
    nf = nfr.cpu().numpy()
    want = _want_of_bits(bits.cpu().numpy(), nf, dem.Nbits)
    print(f"noisy={noisy} packed={packed}: frames {nf}, packets {want['packets']}, errors {want['errors']} in {want['bits']} bits")
    for k in tbitsref.NAMES:
        assert np.array_equal(got[k], want[k]), (k, got[k], want[k])
    assert (nf >= NFRAMES - 2).all() and (want["packets"] > 0).all()
    assert (want["errors"].sum() > 0) == noisy
    tb.close()


def test_behind_the_streaming_receiver(oracle, built_lib):
    """the same signal through HipRx in 3 blocks, a push behind every block"""
    import torch
    import pirip_amd
    c = sigutil.CFG1
    iq, nsamp = _test_signal(oracle, SIGMA)
    dem = pirip_amd.HipDemod(c["Fs"], c["Rs"], c["M"], P=c["P"], est_min=c["est_min"], est_max=c["est_max"], nstreams=NSTREAMS)
    block = nsamp // 3
    rx = pirip_amd.HipRx(dem, block=block)
    R = rx.max_frames
    bits = torch.zeros((3, NSTREAMS, R, dem.Nbits), dtype=torch.uint8, device="cuda")
    nfr = torch.zeros((3, NSTREAMS), dtype=torch.int32, device="cuda")
    tb = pirip_amd.HipTestBits(nstreams=NSTREAMS)
    for k in range(3):
        rx.push(iq.data_ptr() + k * block * 2, nsamp * 2, bits[k].data_ptr(), R * dem.Nbits, d_nframes=nfr[k].data_ptr())
        tb.push(bits[k], nframes=nfr[k], stream=0)
    got = tb.counters()
    b, nf = bits.cpu().numpy(), nfr.cpu().numpy()
    ref = [tbitsref.Counter(ts.default_frame()) for _ in range(NSTREAMS)]
    for k in range(3):
        for s in range(NSTREAMS):
            ref[s].push(b[k, s, :nf[k, s]])
    for k in tbitsref.NAMES:
        assert np.array_equal(got[k], [r.counters()[k] for r in ref]), k
    assert (got["packets"] > 0).all() and got["errors"].sum() > 0 and (nf.sum(axis=0) >= NFRAMES - 3).all()
    tb.close()


# ---- records ------------------------------------------------------------------------------------------------------------------------
def _assert_records(tb, want, what=""):
    got = tb.record_counters()
    for k in tbitsref.REC_NAMES:
        assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])


def test_crafted_records(built_lib):
    import pirip_amd
    want_pl = pirip_amd.testframe_payload(8 * ts.REC_DB)
    st, pl, info, nc = ts.crafted_records(want_pl)
    tb = pirip_amd.HipTestBits(nstreams=3)
    with pytest.raises(pirip_amd.PiripError, match=r"\(-1\)"):
        tb.push_records(_dev(st), _dev(pl), _dev(info))                                # no payload set yet
    tb.set_payload(ts.REC_DB)
    tb.push_records(_dev(st), _dev(pl), _dev(info), ncalls=_dev(nc))
    _assert_records(tb, tbitsref.record_tally(st, pl, info, nc, want_pl), "clamped ncalls")
    tb.reset()
    tb.push_records(_dev(st), _dev(pl), _dev(info))
    tb.push_records(_dev(st), _dev(pl), _dev(info), ncalls=_dev(np.array([0, 1, 2], dtype=np.int32)))
    a, b = tbitsref.record_tally(st, pl, info, [6, 6, 6], want_pl), tbitsref.record_tally(st, pl, info, [0, 1, 2], want_pl)
    _assert_records(tb, {k: a[k] + b[k] for k in a}, "two calls")
    # a payload of the caller's own
    own = np.arange(ts.REC_DB, dtype=np.uint8)
    tb.reset()
    tb.set_payload(ts.REC_DB, own)
    tb.push_records(_dev(st), _dev(pl), _dev(info))
    _assert_records(tb, tbitsref.record_tally(st, pl, info, [6, 6, 6], own), "own payload")
    tb.close()


def test_records_of_a_test_frame_burst(oracle, built_lib):
    """HipTx sends a burst of test frames, pirip_hip_fsk_ldpc_rx_batch receives it, the tally runs behind it on the same HIP stream"""
    import torch
    import pirip_amd
    CODE = pirip_amd.STANDIN_CODE
    Fs, Rs, M, f1, shift, nfr, B = 240000, 10000, 2, 10000, 10000, 3, 4
    Ts = Fs // Rs
    lead = [200 + s for s in range(B)]
    tx = pirip_amd.HipTx(CODE, Fs, Rs, M, nstreams=B, f1=f1, shift=shift, lead=lead, gap=700)
    kb = tx.data_bytes
    rec = np.zeros((B, nfr + 1, 1 + kb), dtype=np.uint8)
    rec[:, :, 0] = [1] + [0] * (nfr - 1) + [2]
    rec[:, :nfr, 1:] = pirip_amd.testframe_payload(8 * kb)
    for s in range(B):
        rec[s, :nfr, 1], rec[s, :nfr, 2] = 0x10 + s, np.arange(1, nfr + 1)              # source and sequence bytes: not compared
    nsym = max(lead) + tx.preamble_syms + nfr * tx.frame_syms + 700
    nsamp = nsym * Ts
    iq = torch.zeros((B, nsamp * 2), dtype=torch.uint8, device="cuda")
    dem = pirip_amd.HipDemod(Fs, Rs, M, P=8, est_min=Rs // 2, est_max=90000, nstreams=B)
    L = pirip_amd.HipLdpc(CODE, M, nstreams=B)
    maxf = dem.max_frames_for(nsamp)
    st = torch.zeros((B, maxf), dtype=torch.uint8, device="cuda")
    pl = torch.zeros((B, maxf, L.data_bytes), dtype=torch.uint8, device="cuda")
    info = torch.zeros((B, maxf, pirip_amd.LDPC_INFO_PER_CALL), dtype=torch.int32, device="cuda")
    nf = torch.zeros(B, dtype=torch.int32, device="cuda")
    cons = torch.zeros(B, dtype=torch.int64, device="cuda")
    tb = pirip_amd.HipTestBits(nstreams=B)
    tb.set_payload(kb)
    d_rec = _dev(rec)
    tx.records_to_iq(d_rec.data_ptr(), rec[0].size, nfr + 1, nsym, iq.data_ptr(), nsamp * 2, amp=14.0)
    L.chain_batch(dem, iq.data_ptr(), nsamp * 2, nsamp, st.data_ptr(), pl.data_ptr(), info.data_ptr(), nf.data_ptr(), cons.data_ptr(), maxf)
    tb.push_records(st, pl, info, ncalls=nf, stream=0)
    got = tb.record_counters()
    want = tbitsref.record_tally(st.cpu().numpy(), pl.cpu().numpy(), info.cpu().numpy(), nf.cpu().numpy(), pirip_amd.testframe_payload(8 * kb))
    _assert_records(tb, want, "burst")
    assert (got["frames"] > 0).all() and (got["crc_ok"] == nfr).all() and got["errors"][got["frames"] == got["crc_ok"]].sum() == 0
    tb.close()


# ---- the CLI ------------------------------------------------------------------------------------------------------------------------
def test_rtl_fsk_channels_put_test_bits(oracle, built_lib, tmp_path):
    """rtl_fsk_channels --put-test-bits on a 2-channel capture: per channel the line fsk_put_test_bits ends with on that channel's file,
    and its PASS rule for the exit code"""
    Fs, D, offs = 2400000, 30, [-375000, 375000]
    mFs, Rs, f1, shift = 80000, 10000, 10000, 10000
    n_raw = Fs // 2 + Fs // 10                                   # two blocks of a quarter second
    nsym = n_raw // (Fs // Rs) + 2
    bits = oracle.get_test_bits(nsym)
    rng = np.random.default_rng(71)
    z = np.zeros(n_raw, dtype=np.complex128)
    for c, fc in enumerate(offs):
        z += chanref.fsk_wideband(Fs, Rs, 2, fc + f1, shift, np.roll(bits, -17 * c), n_raw, 8.0, phase0=rng.uniform(0, 2 * np.pi))
    # Eb/N0 about 10 dB in each channel (64 * 8 samples per symbol at the modem rate against 2 * 27^2 / 30): a few bit errors
    z += rng.normal(0, 27.0, n_raw) + 1j * rng.normal(0, 27.0, n_raw)
    iq = tmp_path / "wide.iq"
    chanref.quantise_u8(z).reshape(-1).tofile(iq)
    prefix = str(tmp_path / "ch")
    base = [os.path.join(BIN, "rtl_fsk_channels"), "-s", str(Fs), "-a", str(mFs), "-r", str(Rs), "-c", ",".join(map(str, offs)), "-i", str(iq),
            "-o", prefix, "-q", "--put-test-bits", "-b", "0.2"]
    p = subprocess.run(base + ["-p", "20"], capture_output=True, timeout=300)
    lines = [ln for ln in p.stderr.decode().split("\n") if "BER" in ln]
    assert len(lines) == 2, p.stderr.decode()
    packets = []
    for c in range(2):
        chan_bits = np.fromfile(f"{prefix}.{c}", dtype=np.uint8)
        line, (pk, nb, ne), _ = tbitsref.put_test_bits_tool(chan_bits)
        assert lines[c] == f"{c}: {line}", (lines[c], line)
        assert pk > 20 and nb == 100 * pk
        packets.append(pk)
    assert p.returncode == 0, p.stderr.decode()
    # a packet count only one channel reaches, or none: FAIL
    q = subprocess.run(base + ["-p", str(max(packets) + 1)], capture_output=True, timeout=300)
    assert q.returncode == 1 and [ln for ln in q.stderr.decode().split("\n") if "BER" in ln] == lines
