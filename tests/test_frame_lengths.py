"""The general demodulator against the oracle at frame lengths other than the 50 symbols every instance is compiled for. Nsym is a
public parameter (pirip_fsk_params.Nsym, fsk_create_hbr, fsk_demod --nsym, HipDemod(Nsym=)); any value but 50 lands on
fsk_demod_general.hip, where the frame length picks the thread count, the register read-ahead, the LDS layout, direct input and the
number of estimator FFTs. The rows, the paths they take and the input conditions are proven without a GPU in test_frame_lengths_cpu.py;
here each row runs on the device. Every tolerance is tests/parity.py's, scaled by its one rule (N / 2400 for long frames)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import nsymshapes as ns
import sigutil
from demodrun import host_chunks, same_results, same_words, stream_state
from parity import RX_FILT_TOL, TIMING_TOL, _compare, oracle_Sf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "pirip_amd", "bin")

_ref = {}


def _reference(oracle, r, ebno=None):
    """(input buffer, oracle result, the oracle object afterwards) of a row: computed once, shared, left unchanged"""
    key = (r.name, ebno)
    if key not in _ref:
        buf, _ = ns.signal(oracle, sigutil, r, ebno_db=ebno)
        o = ns.oracle_for(oracle, r)
        _ref[key] = (buf, o.demod(buf, ns.formats(oracle, None, r)[0]), o)
    return _ref[key]


def _tol(r):
    return RX_FILT_TOL * max(1.0, ns.dims(r)["N"] / 2400.0)


def _handle(r, nstreams=1):
    import pirip_amd
    from oracle import binding as ob
    c = ns.config(r)
    return pirip_amd.HipDemod(r.Fs, r.Rs, r.M, P=r.P, Nsym=r.Nsym, est_min=c["est_min"], est_max=c["est_max"],
                              in_format=ns.formats(ob, pirip_amd, r)[1], nstreams=nstreams)


# ---- 1. parity on every row ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", ns.DEVICE_ROWS, ids=lambda r: r.name)
def test_every_frame_length_row_equals_the_oracle_one_shot_and_in_ragged_chunks(oracle, built_lib, r):
    """Clean and at Eb/N0 = 9 dB, in one call and in three ragged host calls: frame count, consumed samples, tone estimates, the nin
    sequence, the smoothed spectrum left behind and (clean) every bit exactly; soft magnitudes, timing, SNR within the project's
    tolerances. The handle reports the general kernel at the row's frame length."""
    for ebno in (None, 9.0):
        buf, ro, o = _reference(oracle, r, ebno)
        n = buf.shape[0]
        h = _handle(r)
        name = h.kernel_name()
        assert h.kernel() == "general" and "general" in name and f"Nsym={r.Nsym}," in name, name
        rh = h.demod_host(buf)
        Sf = h.get_Sf(0)
        h.close()
        print(f"{r.name} Eb/N0 {ebno}: {ro['nframes']} frames, rx_filt err {sigutil.rel_err(rh['rx_filt'], ro['rx_filt']) if rh['nframes'] == ro['nframes'] else 'n/a'}, "
              f"timing err {np.abs(rh['stats'][:, 4] - ro['stats'][:, 4]).max() if rh['nframes'] == ro['nframes'] else 'n/a'}")
        nfl = _compare(ro, rh, tol=_tol(r), allow_near_tie_flips=ebno is not None, M=r.M)
        # the smoothed spectrum after the last frame: one FFT more or fewer in any frame shows here even where the peaks stay put
        same_words(Sf, oracle_Sf(oracle, o, ns.dims(r)["Ndft"]), "Sf")
        h = _handle(r)
        rc = host_chunks(h, buf, [n // 3 + 17, (2 * n) // 3 + 5])
        h.close()
        assert _compare(ro, rc, tol=_tol(r), allow_near_tie_flips=ebno is not None, M=r.M) == nfl
        same_results(rc, rh, "chunked against one-shot")


# ---- 2. frames where no FFT fits ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ns.DEGENERATE)
def test_frames_too_short_for_an_estimator_fft(oracle, built_lib, name):
    """Sf is never updated: the peak search of a zero spectrum gives bin 0 = -Fs / 2 for every tone, all tones are down-converted alike,
    the strict > of the decision keeps every bit 0; timing and nin still run and equal the oracle's."""
    r = ns.BY_NAME[name]
    buf, ro, _ = _reference(oracle, r)
    h = _handle(r)
    rh = h.demod_host(buf)
    assert rh["nframes"] == ro["nframes"] > 0 and rh["consumed"] == ro["consumed"]
    assert (rh["stats"][:, :r.M] == -r.Fs / 2).all() and np.array_equal(rh["stats"][:, :4], ro["stats"][:, :4])
    assert not h.get_Sf(0).any()
    assert not rh["bits"].any() and not ro["bits"].any()
    assert np.array_equal(rh["stats"][:, 6], ro["stats"][:, 6])
    h.close()


# ---- 3. dispatch ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,Nsym", [("wave", 49), ("wave", 51), ("block", 49), ("block", 51)])
def test_neighbours_of_the_compiled_length_leave_the_specialised_instances(oracle, built_lib, monkeypatch, shape, Nsym):
    import pirip_amd
    c = dict(sigutil.CFG1, f1=10000, shift=10000) if shape == "wave" else dict(Fs=240000, Rs=1000, M=2, P=15, f1=11000, shift=2000, est_min=500, est_max=25000)
    mk = lambda n: pirip_amd.HipDemod(c["Fs"], c["Rs"], c["M"], P=c["P"], Nsym=n, est_min=c["est_min"], est_max=c["est_max"], nstreams=1)
    monkeypatch.delenv("PIRIP_KERNEL", raising=False); monkeypatch.delenv("PIRIP_FORCE_GENERAL", raising=False)
    h50 = mk(50)
    assert h50.kernel() == shape
    h50.close()
    h = mk(Nsym)
    assert h.kernel() == "general" and f"Nsym={Nsym}," in h.kernel_name()
    with pytest.raises(pirip_amd.PiripError):
        h.set_estimator_band_only(True)
    rng = np.random.default_rng(Nsym)
    Ts = c["Fs"] // c["Rs"]
    x = sigutil.mod_complex(oracle, c, rng.integers(0, 2, 22 * Nsym).astype(np.uint8))[Ts // 3:]
    u8 = oracle.quantise_cu8(x, amp=20.0)
    rh = h.demod_host(u8)
    h.close()
    monkeypatch.setenv("PIRIP_KERNEL", "general")
    hg = mk(Nsym)
    rg = hg.demod_host(u8)
    hg.close()
    same_results(rh, rg, "PIRIP_KERNEL=general")
    o = oracle.OracleFsk(c["Fs"], c["Rs"], c["M"], P=c["P"], Nsym=Nsym, est_min=c["est_min"], est_max=c["est_max"])
    ro = o.demod(u8, oracle.IN_CU8_FSKDEMOD)
    assert ro["nframes"] >= 20
    _compare(ro, rh, tol=RX_FILT_TOL * max(1.0, Ts * Nsym / 2400.0))


# ---- 4. batch -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ts24_p8_s16_n20", "ts24_n127"])
def test_five_streams_at_their_own_offsets_and_an_odd_stride(oracle, built_lib, name):
    """pirip_hip_demod_batch on the 64-thread and the wide shape: each stream starts at its own sample of the recording, rows are laid
    out at a stride that is no round number; every stream equals its own oracle replay."""
    import torch
    import pirip_amd
    r = ns.BY_NAME[name]
    buf, _, _ = _reference(oracle, r, 9.0)
    B, d = 5, ns.dims(r)
    offs = [0, 7, d["Ts"] // 2 + 1, 2 * d["Ts"] + 3, 5 * d["Ts"] - 1]
    nsamp = min(buf.shape[0] - max(offs), 24 * d["N"])
    host = [np.ascontiguousarray(buf[o:o + nsamp]) for o in offs]
    bps = host[0].itemsize * 2
    stride = nsamp * bps + 3 * bps
    flat = np.zeros(B * stride + 64, dtype=np.uint8)
    for s in range(B):
        flat[s * stride:s * stride + nsamp * bps] = host[s].view(np.uint8).reshape(-1)
    dev = torch.from_numpy(flat).cuda()
    h = _handle(r, nstreams=B)
    maxf, nb, nf_ = h.max_frames_for(nsamp), h.Nbits, r.M * r.Nsym
    bits = torch.zeros((B, maxf, nb), dtype=torch.uint8, device="cuda")
    filt = torch.zeros((B, maxf, nf_), dtype=torch.float32, device="cuda")
    stats = torch.zeros((B, maxf, pirip_amd.STATS_PER_FRAME), dtype=torch.float32, device="cuda")
    nfr = torch.zeros(B, dtype=torch.int32, device="cuda"); cons = torch.zeros(B, dtype=torch.int64, device="cuda")
    h.demod_batch(dev.data_ptr(), stride, nsamp, bits.data_ptr(), maxf * nb, filt.data_ptr(), maxf * nf_, stats.data_ptr(),
                  maxf * pirip_amd.STATS_PER_FRAME, nfr.data_ptr(), cons.data_ptr(), maxf, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    h.close()
    for s in range(B):
        ro = ns.oracle_for(oracle, r).demod(host[s], ns.formats(oracle, None, r)[0])
        k = int(nfr[s])
        rh = {"nframes": k, "consumed": int(cons[s]), "bits": bits[s, :k].cpu().numpy(), "rx_filt": filt[s, :k].cpu().numpy(),
              "stats": stats[s, :k].cpu().numpy()}
        assert ro["nframes"] >= 20
        _compare(ro, rh, tol=_tol(r), allow_near_tie_flips=True, M=r.M)


# ---- 5. packed bits -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ts24_n11", "ts24_4fsk_f32_n21", "ts24_n127", "ts24_p8_s16_n20", "ts24_n8"])
def test_packed_bits_equal_packbits_and_pad_with_zeros(oracle, built_lib, name):
    """Nbits = 11, 42, 127 (no multiple of 8), 20 on a shape whose down-converted samples share the FFT work array with the staged bits,
    and the aliasing Nsym = 8 shape: the packed row is numpy.packbits of the unpacked twin's, the last byte's padding bits are zero."""
    r = ns.BY_NAME[name]
    buf, ro, _ = _reference(oracle, r, None if name in ns.DEGENERATE else 9.0)
    h = _handle(r)
    ref = h.demod_host(buf)["bits"]
    h.close()
    hp = _handle(r)
    hp.set_bit_packing(True)
    got = hp.demod_host(buf)["bits"]
    hp.close()
    nb = ns.dims(r)["Nbits"]
    assert ref.shape == (ro["nframes"], nb) and got.shape == (ro["nframes"], (nb + 7) // 8)
    if name not in ns.DEGENERATE:
        assert 0.3 < ref.mean() < 0.7                          # (a row of zeros would pack to zeros whatever the packing does)
    pad = 8 * got.shape[1] - nb
    assert not (got[:, -1] & ((1 << pad) - 1)).any(), "padding bits set"
    assert np.array_equal(got, np.packbits(ref, axis=1))


# ---- 6. max_frames stop and resume ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ts24_n127", "ts24_p8_n342"])
def test_stop_after_three_frames_resume_and_reset(oracle, built_lib, name):
    """pirip_hip_demod_batch with max_frames = 3, then the unconsumed rest: together one shot, word for word. The read-ahead row holds
    the fourth frame in registers when the kernel stops; the direct-input row reads global memory at the resumed position. The stream
    scalars after the stopped call are the oracle's after three frames; reset gives a created stream."""
    import torch
    import pirip_amd
    r = ns.BY_NAME[name]
    buf, ro, _ = _reference(oracle, r)
    d = ns.dims(r)
    nsamp, bps = buf.shape[0], buf.itemsize * 2
    dev = torch.from_numpy(buf).cuda()
    h = _handle(r)
    created = stream_state(h).copy()
    maxf, nb, nf_ = h.max_frames_for(nsamp), h.Nbits, r.M * r.Nsym
    st = torch.cuda.current_stream().cuda_stream

    def call(ptr, n, limit):
        bits = torch.zeros((maxf, nb), dtype=torch.uint8, device="cuda")
        filt = torch.zeros((maxf, nf_), dtype=torch.float32, device="cuda")
        stats = torch.zeros((maxf, pirip_amd.STATS_PER_FRAME), dtype=torch.float32, device="cuda")
        nfr = torch.zeros(1, dtype=torch.int32, device="cuda"); cons = torch.zeros(1, dtype=torch.int64, device="cuda")
        h.demod_batch(ptr, n * bps, n, bits.data_ptr(), maxf * nb, filt.data_ptr(), maxf * nf_, stats.data_ptr(), maxf * pirip_amd.STATS_PER_FRAME,
                      nfr.data_ptr(), cons.data_ptr(), limit, st)
        torch.cuda.synchronize()
        k = int(nfr[0])
        return {"nframes": k, "consumed": int(cons[0]), "bits": bits[:k].cpu().numpy(), "rx_filt": filt[:k].cpu().numpy(), "stats": stats[:k].cpu().numpy()}

    a = call(dev.data_ptr(), nsamp, 3)
    assert a["nframes"] == 3 and a["consumed"] == d["N"] + int(ro["stats"][:2, 6].sum())
    s3 = stream_state(h)
    sf = s3.view(np.float32)
    assert int(s3.view(np.int32)[0]) == int(ro["stats"][2, 6])                                  # nin the fourth frame will take
    assert np.array_equal(sf[7:11], ro["stats"][2, :4])                                          # tone estimates
    assert abs(sf[1] - ro["stats"][2, 4]) < TIMING_TOL * max(1.0, _tol(r) / RX_FILT_TOL)
    assert np.array_equal(s3[[1, 2, 4, 11, 12]], a["stats"][2, [4, 7, 5, 8, 9]].view(np.uint32))   # ... and the third row's own words
    b = call(dev.data_ptr() + a["consumed"] * bps, nsamp - a["consumed"], maxf)
    both = {"nframes": a["nframes"] + b["nframes"], "consumed": a["consumed"] + b["consumed"],
            **{k: np.concatenate([a[k], b[k]]) for k in ("bits", "rx_filt", "stats")}}
    _compare(ro, both, tol=_tol(r), M=r.M)
    h.reset()
    torch.cuda.synchronize()
    assert np.array_equal(stream_state(h), created) and not h.get_Sf(0).any()
    one = call(dev.data_ptr(), nsamp, maxf)
    same_results(both, one, "stopped + resumed against one shot after reset")
    h.close()


# ---- 7. the every-frame-exact kernel --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,packed", [("ts24_n11", False), ("ts24_4fsk_f32_n21", False), ("ts40_4fsk_f32_n30", False), ("ts24_n8", True),
                                         ("ts24_p8_s16_n20", True)])
def test_exact_kernel_is_the_oracle_bit_for_bit_at_other_frame_lengths(oracle, built_lib, monkeypatch, name, packed):
    """PIRIP_KERNEL=exact under 7 dB noise: bits, soft magnitudes and every per-frame statistic (tone estimates, timing, SNRest, nin, ppm
    -- the division by Nsym -- signal and noise power) word for word, as test_exact_kernel_equals_the_oracle_bit_for_bit_under_noise
    asserts at 50 symbols. With bit packing at Nsym = 8, Ts = 24 the staged bits share LDS with the FFT work array AND with the rows of
    per-symbol powers the serial sums read: those rows once started at the same address and overwrote the bits before they were packed."""
    monkeypatch.setenv("PIRIP_KERNEL", "exact")
    r = ns.BY_NAME[name]
    buf, _ = ns.signal(oracle, sigutil, r, ebno_db=7.0)
    ro = ns.oracle_for(oracle, r).demod(buf, ns.formats(oracle, None, r)[0])
    h = _handle(r)
    assert h.kernel() == "exact" and f"Nsym={r.Nsym}," in h.kernel_name()
    if packed:
        h.set_bit_packing(True)
    n = buf.shape[0]
    rh = host_chunks(h, buf, [n // 3 + 17, (2 * n) // 3 + 5])
    h.close()
    assert rh["nframes"] == ro["nframes"] >= 14 and rh["consumed"] == ro["consumed"]
    if name not in ns.DEGENERATE:
        assert 0.3 < ro["bits"].mean() < 0.7
    want = np.packbits(ro["bits"], axis=1) if packed else ro["bits"]
    assert np.array_equal(rh["bits"], want), ("bits", int((rh["bits"] != want).sum()))
    assert np.array_equal(rh["rx_filt"].view(np.uint32), ro["rx_filt"].view(np.uint32)), "soft magnitudes"
    assert np.array_equal(rh["stats"][:, :10].view(np.uint32), ro["stats"][:, :10].view(np.uint32)), \
        np.argwhere(rh["stats"][:, :10].view(np.uint32) != ro["stats"][:, :10].view(np.uint32))[:6].tolist()


# ---- 8. eye diagram and Sf ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ts24_n11", "ts24_4fsk_f32_n21", "ts24_n8"])
def test_eye_diagram_and_spectrum_of_short_frames(oracle, built_lib, name):
    """MODEM_STATS.rx_eye of the latest frame: rows, points and values are the oracle's at eleven- and 21-symbol frames; at eight symbols
    the frame's window sums hold three of the four traces per tone and both sides cut the diagram to them. The smoothed spectrum read
    back from the handle is the oracle's, bit for bit."""
    r = ns.BY_NAME[name]
    buf, _ = ns.signal(oracle, sigutil, r, ebno_db=None if name in ns.DEGENERATE else 12.0)
    o = ns.oracle_for(oracle, r)
    ro = o.demod(buf, ns.formats(oracle, None, r)[0])
    h = _handle(r)
    h.enable_eye()
    rh = h.demod_host(buf)
    assert rh["nframes"] == ro["nframes"] > 0 and np.array_equal(rh["stats"][:, :4], ro["stats"][:, :4])
    eo_raw, eh_raw = o.eye(normalise=False), h.eye(normalise=False)
    assert eh_raw.shape == eo_raw.shape == ns.eye_shape(r)
    assert eo_raw.max() > 0 and np.abs(eh_raw - eo_raw).max() <= RX_FILT_TOL * eo_raw.max()
    eo, eh = o.eye(), h.eye()
    assert eh.max() == 1.0 and np.abs(eh - eo).max() <= 2 * RX_FILT_TOL
    Sf_o = oracle_Sf(oracle, o, ns.dims(r)["Ndft"])
    assert (Sf_o.any()) == (name not in ns.DEGENERATE)
    same_words(h.get_Sf(0), Sf_o, "Sf")
    h.close()


# ---- 9. limits ------------------------------------------------------------------------------------------------------------------------
def test_frame_lengths_the_library_refuses_and_the_capture_route(oracle, built_lib):
    import pirip_amd
    import test_capture as tc
    from pirip_amd.binding import FskParams
    L = built_lib
    r = ns.BY_NAME["ts24_4fsk_f32_n400"]
    c = ns.config(r)

    def create(nsym):
        p = FskParams(r.Fs, r.Rs, r.M, r.P, nsym, c["est_min"], c["est_max"], 0, 100, pirip_amd.IN_CF32)
        hh = C.c_void_p()
        rc = L.pirip_hip_create(C.byref(p), 1, -1, C.byref(hh))
        if rc == 0:
            L.pirip_hip_destroy(hh)
        return rc
    assert create(400) == -6                                   # PIRIP_ERR_UNSUPPORTED: 208 880 bytes of LDS
    assert create(0) == -2 and create(-3) == -2                # PIRIP_ERR_BAD_CONFIG
    assert create(21) == 0
    # a capture on a handle off the compiled frame length: the sequential route, equal to the read loop
    r = ns.BY_NAME["ts40_4fsk_f32_n30"]
    buf, ro, _ = _reference(oracle, r, 9.0)
    hs = _handle(r)
    seq = hs.demod_host(buf)
    hs.close()
    hc = _handle(r, nstreams=8)
    cap, reps = tc._capture(pirip_amd, hc, buf)
    hc.close()
    assert [(p["segments"], p["segment_frames"], p["passes"]) for p in reps] == [(1, 0, 1)]
    tc._same(cap, seq, "capture")
    _compare(ro, cap, tol=_tol(r), allow_near_tie_flips=True, M=r.M)


# ---- 10. IQ to records ----------------------------------------------------------------------------------------------------------------
def test_iq_to_records_at_34_symbols_per_call(oracle, built_lib):
    """pirip_hip_fsk_ldpc_rx_batch with demodulator and receiver both at Nsym = 34 (4-FSK: 68 bits per call, no divisor of the frame):
    the records equal what the oracle's receiver makes of the unfused demodulator's soft magnitudes, over the unfused route (the
    fused hand-over belongs to the 50-symbol wave instances)."""
    import torch
    import pirip_amd as A
    M, P, Nsym = 4, 8, 34
    code = oracle.parse_code_file(A.STANDIN_CODE)
    c = dict(Fs=240000, Rs=10000, M=M, P=P, f1=10000, shift=10000)
    fr = subprocess.run([os.path.join(BIN, "fsk_ldpc_framer"), "--code", A.STANDIN_CODE, "-m", str(M), "--testframes", "2", "--bursts", "1", "--seq",
                         "--source", "0x5", "/dev/zero", "-"], capture_output=True, check=True).stdout
    bits = np.frombuffer(fr, dtype=np.uint8)
    rng = np.random.default_rng(34)
    z = lambda n: np.zeros((n, 2), dtype=np.float32)
    x = np.concatenate([z(1700), sigutil.mod_complex(oracle, c, bits), z(5003), sigutil.mod_complex(oracle, c, bits), z(14400)])
    sigma = np.sqrt(4.0 * 24 / np.log2(M) / (10 ** (8.0 / 10.0)) / 2.0)
    B, offs = 3, [0, 13, 40]
    nsamp = x.shape[0] - 48
    host = np.stack([oracle.quantise_cu8(x[o:o + nsamp] + rng.normal(0.0, sigma, (nsamp, 2)).astype(np.float32), amp=14.0) for o in offs])
    mk = lambda n: A.HipDemod(240000, 10000, M, P=P, Nsym=Nsym, est_min=500, est_max=60000, in_format=A.IN_CU8_FSKDEMOD, nstreams=n)
    want = []
    for s in range(B):
        dem = mk(1)
        want.append(oracle.OracleLdpc(code, M, Nsym=Nsym).rx(dem.demod_host(host[s])["rx_filt"]))
        dem.close()
    dem, ld = mk(B), A.HipLdpc(A.STANDIN_CODE, M, Nsym=Nsym, nstreams=B)
    d = torch.from_numpy(host).cuda()
    maxf = dem.max_frames_for(nsamp)
    st = torch.zeros((B, maxf), dtype=torch.uint8, device="cuda"); pl = torch.zeros((B, maxf, 32), dtype=torch.uint8, device="cuda")
    inf = torch.zeros((B, maxf, A.LDPC_INFO_PER_CALL), dtype=torch.int32, device="cuda")
    nfr = torch.zeros(B, dtype=torch.int32, device="cuda"); cons = torch.zeros(B, dtype=torch.int64, device="cuda")
    ld.chain_batch(dem, d.data_ptr(), nsamp * 2, nsamp, st.data_ptr(), pl.data_ptr(), inf.data_ptr(), nfr.data_ptr(), cons.data_ptr(), maxf)
    torch.cuda.synchronize()
    assert not ld.last_path_fused()
    nf, st, pl, inf = nfr.cpu().numpy(), st.cpu().numpy(), pl.cpu().numpy(), inf.cpu().numpy()
    ld.close(); dem.close()
    for s in range(B):
        ws, wp, wi = want[s]
        v = int(nf[s])
        assert v == len(ws) > 30 and ((ws & A.RX_BITS) != 0).sum() >= 2, (s, v, len(ws))
        assert np.array_equal(st[s, :v], ws) and np.array_equal(pl[s, :v], wp) and np.array_equal(inf[s, :v], wi), s


# ---- 11. CLI --------------------------------------------------------------------------------------------------------------------------
def test_cli_fsk_demod_nsym_matches_oracle_cli(oracle, built_lib):
    r = ns.BY_NAME["ts24_n49"]
    raw = _reference(oracle, r)[0][:40000].tobytes()
    argv = ["--fsk_lower", "500", "--fsk_upper", "25000", "-d", "-p", "24", "--nsym", "30", "2", "240000", "10000", "-", "-"]
    po = subprocess.run([os.path.join(ROOT, "oracle", "build", "fsk_demod_oracle")] + argv, input=raw, capture_output=True)
    ph = subprocess.run([os.path.join(BIN, "fsk_demod")] + argv, input=raw, capture_output=True)
    assert po.returncode == 0 and ph.returncode == 0, ph.stderr
    assert ph.stdout == po.stdout and len(ph.stdout) % 30 == 0 and len(ph.stdout) >= 30 * 50 and 0.3 < np.frombuffer(ph.stdout, dtype=np.uint8).mean() < 0.7
