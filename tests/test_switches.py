"""Every opt-in arithmetic and tuning switch, launched (tests/switchshapes.py holds the table, the rows and the restated launch rules;
tests/test_switches_cpu.py proves without a GPU that the rows reach what they claim and that the arithmetic rows tell their arithmetics
apart). No tolerance is introduced here: a switch either has an arithmetic restated exactly on the CPU -- the fused FFT multiply, the
decimator's two fma tap loops -- or must not change an output word; the demodulator comparisons are tests/parity.py's _compare as it is.

  PIRIP_FFT_FMA            the fused instance of the headline shape: Sf bit for bit the fused oracle's, everything else under _compare
  PIRIP_DECIM_FMA / set_arith, PIRIP_DECIM_LUT, PIRIP_DECIM_TPW (and the walk of several tiles per workgroup it stands in front of)
  PIRIP_GENERAL_THREADS    every accepted thread count of the general kernel against the oracle
  PIRIP_BLOCK_STAGGER, PIRIP_CAPTURE_REPLICAS, PIRIP_CAPTURE_PIN_FRAMES, PIRIP_LAYOUT_TRIES      no output word moves
  PIRIP_EST_BAND, PIRIP_EXACT0                              the env forms equal the API forms
  PIRIP_CSDR_BLOCKS, PIRIP_FSK_DEMOD_FRAMES, PIRIP_FSK_DEMOD_SLOTS      the tools' output bytes do not depend on how they cut their input"""
import os
import subprocess

import numpy as np
import pytest

import blockshapes as bs
import ldpcshapes as ls
import nsymshapes as ns
import sigutil
import switchshapes as ss
from demodrun import host_chunks, make_handle, same_results, same_words, stream_state, words
from parity import RX_FILT_TOL, _compare, oracle_Sf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "pirip_amd", "bin")
ERR_UNSUPPORTED = -6
_memo = {}


def _once(key, make):
    """a reference computed once, shared, left unchanged"""
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


# ======== the fused FFT multiply ===========================================================================================================
def _cfg1_handle(nstreams=1):
    return make_handle(sigutil.CFG1, nstreams)


def _fused_oracle(oracle, name, first_frame_unfused=True, n=None):
    return _once(("fft", name, first_frame_unfused, n),
                 lambda: ss.oracle_fft_run(oracle, sigutil, ss.fft_input(oracle, sigutil, name)[:n], True, first_frame_unfused))


def _compare_fused(name, ro, rh):
    if name.startswith("awgn"):
        nflips = _compare(ro, rh, allow_near_tie_flips=True)
        print(f"{name}: {nflips} near-tie bit flips of {ro['bits'].size}")
        assert nflips <= 5
    else:
        _compare(ro, rh)


@pytest.mark.parametrize("name", ss.FFT_INPUTS)
def test_fused_fft_multiply_equals_the_fused_oracle(oracle, built_lib, monkeypatch, name):
    """One stream of the headline shape under PIRIP_FFT_FMA=1, in one call and in three ragged calls: the smoothed spectrum is the fused
    oracle's bit for bit, everything else holds under _compare. Frame 0 comes from the exact prologue, which runs in the general kernel's
    unfused body: the oracle's replay turns its switch on after frame 0."""
    monkeypatch.setenv("PIRIP_FFT_FMA", "1")
    u8 = ss.fft_input(oracle, sigutil, name)
    ro, Sf_o = _fused_oracle(oracle, name)
    h = _cfg1_handle()
    assert h.kernel() == "wave" and "fused FFT multiply" in h.kernel_name(), h.kernel_name()
    rh = h.demod_host(u8)
    _compare_fused(name, ro, rh)
    same_words(h.get_Sf(0), Sf_o, (name, "Sf, one call"))
    h = _cfg1_handle()
    n = u8.shape[0]
    rc = host_chunks(h, u8, (n // 3 + 17, (2 * n) // 3 + 5))
    _compare_fused(name, ro, rc)
    same_words(h.get_Sf(0), Sf_o, (name, "Sf, three calls"))
    same_results(rc, rh, (name, "three calls against one"))


def test_fused_fft_multiply_five_streams(oracle, built_lib, monkeypatch):
    """five streams: one full workgroup of four and a partial one, each stream its own oracle run"""
    import torch
    import pirip_amd
    monkeypatch.setenv("PIRIP_FFT_FMA", "1")
    streams = [ss.fft_input(oracle, sigutil, nm) for nm in ss.FFT_BATCH]
    B, nsamp = len(streams), min(x.shape[0] for x in streams)
    dev = torch.from_numpy(np.stack([x[:nsamp] for x in streams])).cuda()
    h = _cfg1_handle(B)
    assert "fused FFT multiply" in h.kernel_name()
    maxf = h.max_frames_for(nsamp)
    bits = torch.zeros((B, maxf, h.Nbits), dtype=torch.uint8, device="cuda")
    filt = torch.zeros((B, maxf, 100), dtype=torch.float32, device="cuda")
    stats = torch.zeros((B, maxf, pirip_amd.STATS_PER_FRAME), dtype=torch.float32, device="cuda")
    nfr = torch.zeros(B, dtype=torch.int32, device="cuda")
    cons = torch.zeros(B, dtype=torch.int64, device="cuda")
    h.demod_batch(dev.data_ptr(), nsamp * 2, nsamp, bits.data_ptr(), maxf * h.Nbits, filt.data_ptr(), maxf * 100, stats.data_ptr(),
                  maxf * pirip_amd.STATS_PER_FRAME, nfr.data_ptr(), cons.data_ptr(), maxf, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for s, nm in enumerate(ss.FFT_BATCH):
        ro, Sf_o = _fused_oracle(oracle, nm, n=nsamp)
        k = int(nfr[s])
        rh = {"nframes": k, "consumed": int(cons[s]), "bits": bits[s, :k].cpu().numpy(), "rx_filt": filt[s, :k].cpu().numpy(),
              "stats": stats[s, :k].cpu().numpy()}
        _compare_fused(nm, ro, rh)
        same_words(h.get_Sf(s), Sf_o, (nm, "Sf of stream %d" % s))


def test_fused_fft_multiply_without_the_exact_prologue(oracle, built_lib, monkeypatch):
    """set_exact_first_frame(False): frame 0 comes from the fused instance too -- the one case where it starts a created stream -- so the
    oracle is fused from the start. Frame 0 keeps the tolerance contract of the prologue-off runs elsewhere (3 x RX_FILT_TOL of the peak
    on its soft magnitudes) with its tone estimates, nin and (noise-free) bits exact; frames 1 .. go through _compare unchanged. Sf is
    the fused oracle's bit for bit after the whole run and after frame 0 alone, where a fused first frame still shows."""
    monkeypatch.setenv("PIRIP_FFT_FMA", "1")
    u8 = ss.fft_input(oracle, sigutil, "clean")
    ro, Sf_o = _fused_oracle(oracle, "clean", first_frame_unfused=False)
    h = _cfg1_handle()
    h.set_exact_first_frame(False)
    assert "fused FFT multiply" in h.kernel_name()
    rh = h.demod_host(u8)
    assert rh["nframes"] == ro["nframes"] >= 100 and rh["consumed"] == ro["consumed"]
    err0 = sigutil.rel_err(rh["rx_filt"][0], ro["rx_filt"][0])             # (relative to frame 0's own peak)
    print(f"frame 0 without the prologue: rx_filt error {err0:.2e} of its peak (bar {3 * RX_FILT_TOL:g})")
    assert err0 < 3 * RX_FILT_TOL
    same_words(rh["stats"][0, :4], ro["stats"][0, :4], "tone estimates of frame 0")
    assert rh["stats"][0, 6] == ro["stats"][0, 6] and np.array_equal(rh["bits"][0], ro["bits"][0])
    n0 = 1200                                               # (frame 0 of a created stream takes nin = N samples)
    rest = lambda r: dict({k: r[k][1:] for k in ("bits", "rx_filt", "stats")}, nframes=r["nframes"] - 1, consumed=r["consumed"] - n0,
                          **({"timing_cond": r["timing_cond"][1:]} if "timing_cond" in r else {}))
    _compare(rest(ro), rest(rh))
    same_words(h.get_Sf(0), Sf_o, "Sf, fused from frame 0")
    h1 = _cfg1_handle()
    h1.set_exact_first_frame(False)
    r1 = h1.demod_host(u8[:1200])
    assert r1["nframes"] == 1 and r1["consumed"] == 1200
    same_words(h1.get_Sf(0), ss.oracle_fft_run(oracle, sigutil, u8[:1200], True)[1], "Sf after frame 0 alone")


def test_fused_switch_changes_nothing_without_a_fused_instance(oracle, built_lib, monkeypatch):
    """4-FSK has no fused instance: under PIRIP_FFT_FMA=1 the name says nothing of it and every output word is the plain handle's"""
    import pirip_amd
    c = sigutil.CFG4
    u8 = sigutil.make_u8_stream(oracle, c, 12000, seed=5, ebno_db=9.0, random_bits=True, amp=14.0)[0]
    mk = lambda: make_handle(c)
    monkeypatch.delenv("PIRIP_FFT_FMA", raising=False)
    h0 = mk()
    r0 = h0.demod_host(u8)
    monkeypatch.setenv("PIRIP_FFT_FMA", "1")
    h1 = mk()
    assert h1.kernel() == "wave" and h1.kernel_name() == h0.kernel_name() and "fused" not in h1.kernel_name()
    r1 = h1.demod_host(u8)
    assert r0["nframes"] >= 100
    same_results(r1, r0, "4-FSK under PIRIP_FFT_FMA=1")
    same_words(h1.get_Sf(0), h0.get_Sf(0), "Sf")


# ======== the decimator ====================================================================================================================
def _decimate(dec, dev, off, stride, n_in, B, s16, fill=12345):
    """one pirip_hip_decim_batch call on B streams `stride` bytes apart from byte `off` of dev -> [B, n_out, 2] on the host"""
    import torch
    n_out = dec.nout(n_in)
    out = torch.full((B, n_out, 2), fill, dtype=torch.int16 if s16 else torch.float32, device="cuda")
    dec.batch(dev.data_ptr() + off, stride, n_in, out.data_ptr(), n_out * (4 if s16 else 8), B, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _stream(host, off, stride, n_in, s):
    return np.ascontiguousarray(host[off + s * stride: off + s * stride + 2 * n_in]).reshape(n_in, 2)


@pytest.mark.parametrize("form", ["env", "api"])
@pytest.mark.parametrize("D,tbw,kernel", ss.ARITH_ROWS)
def test_decimator_opt_in_arithmetics_are_their_formulas_bit_for_bit(oracle, built_lib, monkeypatch, D, tbw, kernel, form):
    """PIRIP_DECIM_FMA=1 | 2 at create and pirip_hip_decim_set_arith(1 | 2), f32 and s16 outputs, three streams at 2-byte aligned
    addresses: every output word is oracle_fir_decimate_cc_arith's for the mode -- which also shows that the convert-once kernels of
    D = 45 and D = 6 stepped aside. (The bytes are switchshapes.arith_host's: on them the three modes differ in f32 and in s16 words,
    test_switches_cpu.py; truncation leaves the s16 rows one or two such words per row against mode 0, the f32 rows thousands.) Then the same bytes at an odd stride: the middle stream starts on an odd address, takes the table
    loop whatever the mode and equals the exact oracle; its even neighbours keep the mode's arithmetic."""
    import torch
    import pirip_amd
    n_in, B, off = ss.arith_n_in(D), ss.ARITH_STREAMS, ss.ARITH_OFF
    strides = ss.arith_strides(D)
    host = ss.arith_host(D)
    dev = torch.from_numpy(host).cuda()
    for mode in (1, 2):
        for s16 in (False, True):
            if form == "env":
                monkeypatch.setenv("PIRIP_DECIM_FMA", str(mode))
                dec = pirip_amd.HipDecim(D, tbw, out_s16=s16)
            else:
                monkeypatch.delenv("PIRIP_DECIM_FMA", raising=False)
                dec = pirip_amd.HipDecim(D, tbw, out_s16=s16)
                assert dec.get_arith() == 0
                dec.set_arith(mode)
            assert dec.get_arith() == mode
            for layout, stride in strides.items():
                got = _decimate(dec, dev, off, stride, n_in, B, s16)
                for s in range(B):
                    m = 0 if (off + s * stride) % 2 else mode
                    want = _once(("arith", D, layout, s, m, s16), lambda: oracle.decim_u8(ss.arith_stream(host, D, layout, s), D, tbw, mode=m, out_s16=s16))
                    same_words(got[s], want, (D, form, "mode %d" % mode, "s16" if s16 else "f32", layout, "stream %d in arithmetic %d" % (s, m)))
            dec.close()


@pytest.mark.parametrize("D,tile", ss.LUT_ROWS)
def test_decimator_table_conversion_is_the_exact_oracle(oracle, built_lib, monkeypatch, D, tile):
    """PIRIP_DECIM_LUT at create: every output converts its samples through the 256-entry table (no convert-once kernel, no arithmetic
    conversion), at aligned and at odd addresses, f32 and s16: the exact oracle bit for bit. The table path has one arithmetic."""
    import torch
    import pirip_amd
    monkeypatch.setenv("PIRIP_DECIM_LUT", "1")
    n_in, B = ss.arith_n_in(D), ss.ARITH_STREAMS
    stride = 2 * n_in + 6
    host = ss.random_bytes(1000 + D, 2 + B * stride + 64)
    dev = torch.from_numpy(host).cuda()
    for s16 in (False, True):
        dec = pirip_amd.HipDecim(D, 0.05, out_s16=s16)
        for mode in (1, 2):
            with pytest.raises(pirip_amd.PiripError, match=r"\(%d\)" % ERR_UNSUPPORTED):
                dec.set_arith(mode)
        assert dec.get_arith() == 0
        for off in (2, 1):
            got = _decimate(dec, dev, off, stride, n_in, B, s16)
            for s in range(B):
                want = _once(("lut", D, off, s, s16), lambda: oracle.decim_u8(_stream(host, off, stride, n_in, s), D, 0.05, mode=0, out_s16=s16))
                same_words(got[s], want, (D, "s16" if s16 else "f32", "offset %d" % off, "stream %d" % s))
        dec.close()


@pytest.mark.parametrize("r", ss.WALK_ROWS, ids=lambda r: r.name)
def test_decimator_multi_tile_walk(oracle, built_lib, monkeypatch, r):
    """Calls large enough for a workgroup to walk several tiles, re-staging its window between them (the path production-sized calls
    take; everything else in the suite has a few streams of a few tiles and one tile per workgroup): distinct random bytes per stream,
    s16 output, ragged even strides. Every stream word for word the same call under PIRIP_DECIM_TPW=1, and the exact oracle."""
    import torch
    import pirip_amd
    monkeypatch.delenv("PIRIP_DECIM_TPW", raising=False)
    plan = ss.decim_plan(r.D)
    n_in, B = ss.walk_n_in(r, plan), r.nstreams
    stride = 2 * n_in + r.pad
    host = ss.random_bytes(7000 + r.D, r.base + B * stride + 64)
    dev = torch.from_numpy(host).cuda()
    dec = pirip_amd.HipDecim(r.D, 0.05, out_s16=True)
    n_out = dec.nout(n_in)
    assert n_out == ss.decim_launch(plan, n_in, B)["n_out"]
    st = torch.cuda.current_stream().cuda_stream
    outs = []
    for tpw in (None, "1"):
        if tpw:
            monkeypatch.setenv("PIRIP_DECIM_TPW", tpw)
        o = torch.full((B, n_out + 1, 2), 12345, dtype=torch.int16, device="cuda")           # (one spare row per stream: must stay untouched)
        dec.batch(dev.data_ptr() + r.base, stride, n_in, o.data_ptr(), (n_out + 1) * 4, B, st)
        torch.cuda.synchronize()
        outs.append(o)
    walk, single = outs
    assert bool((walk[:, n_out] == 12345).all()) and bool((single[:, n_out] == 12345).all()), "a row past a stream's outputs was written"
    if not torch.equal(walk, single):
        bad = torch.nonzero((walk != single).any(2))
        raise AssertionError((r.name, "%d outputs differ from the one-tile-per-workgroup call" % len(bad), "first (stream, output):", bad[:4].tolist()))
    sel = ss.walk_oracle_streams(r, plan)
    got = walk[torch.tensor(sel, device="cuda"), :n_out].cpu().numpy()
    for i, s in enumerate(sel):
        want = oracle.decim_u8(_stream(host, r.base, stride, n_in, s), r.D, 0.05, mode=0, out_s16=True)
        if not np.array_equal(got[i], want):
            bad = np.argwhere((got[i] != want).any(1)).reshape(-1)
            raise AssertionError((r.name, "stream %d: %d outputs differ from the oracle, first at" % (s, len(bad)), bad[:4].tolist(),
                                  "tiles", (bad[:4] // r.tile).tolist()))
    print(f"{r.name}: {B} streams x {n_out} outputs, {len(sel)} streams held to the oracle")


# ======== the general kernel's thread count ================================================================================================
GENERAL_THREADS = (64, 128, 192, 256, 320, 384, 448, 512)
THREAD_ROWS = [next(r for r in ns.DEVICE_ROWS if r.threads == nt and r.ffts > 0) for nt in (64, 128, 256, 512)]


def _general_run(r, buf, monkeypatch, value):
    """one demod_host call of a created handle under PIRIP_GENERAL_THREADS=value (None: unset) -> result, Sf, the 14 state words"""
    import test_frame_lengths as fl
    if value is None:
        monkeypatch.delenv("PIRIP_GENERAL_THREADS", raising=False)
    else:
        monkeypatch.setenv("PIRIP_GENERAL_THREADS", value)
    h = fl._handle(r)
    assert h.kernel() == "general"
    rh = h.demod_host(buf)
    Sf, st = h.get_Sf(0), stream_state(h)
    h.close()
    return rh, Sf, st


def _state_is_the_last_frames(st, rh, what):
    """pirip_stream_state after a call repeats the last frame's statistics: norm_rx_timing, ppm, SNRest, f_est[4], rx_sig_pow, rx_nse_pow"""
    last = rh["stats"][-1]
    same_words(st.view(np.float32)[[1, 2, 4, 7, 8, 9, 10, 11, 12]], last[[4, 7, 5, 0, 1, 2, 3, 8, 9]], (what, "state against the last stats row"))


@pytest.mark.parametrize("r", THREAD_ROWS, ids=lambda r: "%s_default%d" % (r.name, r.threads))
def test_general_kernel_thread_counts_equal_the_oracle(oracle, built_lib, monkeypatch, r):
    """PIRIP_GENERAL_THREADS = 64 ... 512 in steps of a wave on one row per default thread count (which also crosses from
    fsk_demod_general_kernel, up to 256, to the wide kernel): the body strides every loop by blockDim.x and sums its per-wave partials in a
    plain loop over blockDim.x / 64, so every multiple of 64 is a supported launch. Each count is held to the oracle like the default
    launch: frame and sample counts, tone estimates, nin sequence, clean bits and Sf exact, the rest under _compare; the stream state
    left behind is the last frame's statistics, its nin and tone estimates the default launch's words. The row's own default count, set
    explicitly, gives every word of the unset launch. The other counts are not compared with it word for word -- the workgroup sums and
    the down-conversion's runs are cut by the thread count, another rounding of the same sums -- but at 9 dB at least one of them must
    differ from it in a soft-magnitude word: that the switch reaches the launch is observed, not assumed."""
    import test_frame_lengths as fl
    for ebno in (None, 9.0):
        buf, ro, o = fl._reference(oracle, r, ebno)
        Sf_o = oracle_Sf(oracle, o, ns.dims(r)["Ndft"])
        base, base_Sf, base_st = _general_run(r, buf, monkeypatch, None)
        _compare(ro, base, tol=fl._tol(r), allow_near_tie_flips=ebno is not None, M=r.M)
        differ = {}
        for nt in GENERAL_THREADS:
            rh, Sf, st = _general_run(r, buf, monkeypatch, str(nt))
            _compare(ro, rh, tol=fl._tol(r), allow_near_tie_flips=ebno is not None, M=r.M)
            same_words(Sf, Sf_o, (r.name, ebno, nt, "Sf"))
            _state_is_the_last_frames(st, rh, (r.name, ebno, nt))
            same_words(st[[0, 7, 8, 9, 10]], base_st[[0, 7, 8, 9, 10]], (r.name, ebno, nt, "nin and tone estimates of the state"))
            if nt == r.threads:
                same_results(rh, base, (r.name, ebno, "the default count set explicitly"))
                same_words(st, base_st, (r.name, ebno, nt, "stream state"))
            else:
                differ[nt] = int((words(rh["rx_filt"]) != words(base["rx_filt"])).sum())
        print(f"{r.name} Eb/N0 {ebno}: rx_filt words that differ from the default launch ({r.threads} threads), by thread count: {differ}")
        if ebno is not None:
            assert any(differ.values()), differ


@pytest.mark.parametrize("r", [r for r in THREAD_ROWS if r.threads != 128], ids=lambda r: "%s_default%d" % (r.name, r.threads))
def test_general_kernel_refused_thread_counts_keep_the_default(oracle, built_lib, monkeypatch, r):
    """A value that is no whole number of waves from 64 to 512 threads is ignored: the launch is the shape's default one, every output
    and state word equal to the unset launch's -- on rows whose default is not 128 threads, and where 128 threads is seen to give other
    words, so a parser that fell back to a fixed count would not pass."""
    import test_frame_lengths as fl
    buf, ro, o = fl._reference(oracle, r, 9.0)
    base, base_Sf, base_st = _general_run(r, buf, monkeypatch, None)
    other = _general_run(r, buf, monkeypatch, "128")[0]
    assert (words(other["rx_filt"]) != words(base["rx_filt"])).any(), "128 threads and the default count give the same words on this row"
    for value in ("100", "63", "576", "0", "-128", "wide", ""):
        rh, Sf, st = _general_run(r, buf, monkeypatch, value)
        same_results(rh, base, (r.name, "PIRIP_GENERAL_THREADS=%r" % value))
        same_words(st, base_st, (r.name, value, "stream state"))
        same_words(Sf, base_Sf, (r.name, value, "Sf"))


# ======== switches that move no output word ==================================================================================================
@pytest.mark.parametrize("stagger", ["3", "6"])
def test_block_stagger_changes_no_output_word(oracle, built_lib, monkeypatch, stagger):
    """PIRIP_BLOCK_STAGGER: each wave of the block kernel sleeps before its first frame. Three streams of one row; outputs, counts, stream
    state and Sf equal the default launch's, and the default's equal the oracle's (so two equally wrong launches cannot pass)."""
    import pirip_amd
    import test_block_demod as tb
    name = "m2_csdr_peak"
    M, fmt, mask, off = bs.ROWS[name]
    streams = [bs.noisy_stream(oracle, M, fmt, 600, 4000 + s, off + 37 * s, 9.0 if s != 1 else None) for s in range(3)]

    def run():
        h = bs.handle_of(pirip_amd, M, fmt, mask, nstreams=3)
        assert h.kernel() == "block"
        rows = h.max_frames_for(min(x.shape[0] for x in streams))
        res = tb.Batch(h, streams, rows).run(rows).fetch()
        return res, [tb._state(h, s) for s in range(3)]

    monkeypatch.delenv("PIRIP_BLOCK_STAGGER", raising=False)
    base, base_state = _once(("stagger base",), run)
    monkeypatch.setenv("PIRIP_BLOCK_STAGGER", stagger)
    got, got_state = run()
    nsamp = min(x.shape[0] for x in streams)
    for s in range(3):
        assert base[s]["nframes"] >= 10 and base[s]["untouched"] and got[s]["untouched"]
        same_results(got[s], base[s], (stagger, "stream %d" % s))
        same_words(got_state[s][0], base_state[s][0], (stagger, s, "stream state"))
        same_words(got_state[s][1], base_state[s][1], (stagger, s, "Sf"))
        ro = _once(("stagger oracle", s), lambda: bs.oracle_of(oracle, M, mask).demod(streams[s][:nsamp], bs.fmt_of(oracle, fmt)))
        _compare(ro, base[s], tol=tb.TOL, allow_near_tie_flips=s != 1, M=M)


def _capture_cases():
    import test_capture as tc
    want = ("headline noisy", "headline +50 ppm", "Ts = 40 s16 (Ndft 512)")
    return [c for c in tc.CASES if c[0] in want]


@pytest.mark.parametrize("switch,value", [("PIRIP_CAPTURE_REPLICAS", v) for v in ("1", "3", "15")] + [("PIRIP_CAPTURE_PIN_FRAMES", v) for v in ("0", "1", "100")])
@pytest.mark.parametrize("case", _capture_cases(), ids=lambda c: c[0])
def test_capture_replicas_and_pinned_frames_change_no_output_word(oracle, built_lib, monkeypatch, case, switch, value):
    """How many speculative replicas a segment gets and how many warm-up frames run with nin pinned only change how fast the capture's
    repair converges: outputs, counts, the state left behind and Sf equal the sequential read loop's, on the frame-parallel route. Rows
    of test_capture.CASES: the headline shape at 6 dB, with a sample-clock offset, and Ts = 40 with s16 input. Pass counts are printed."""
    import pirip_amd
    import test_capture as tc
    name, cfg, fmt, mask, nbits, ppm, ebno, slots, segf, pieces = case
    fmt_h = {"u8": pirip_amd.IN_CU8_FSKDEMOD, "s16": pirip_amd.IN_CS16}[fmt]
    buf = _once(("capture input", name), lambda: tc._signal(oracle, cfg, nbits, seed=len(name), ppm=ppm, ebno_db=ebno, offset=5, fmt=fmt))

    def read_loop():
        hs = tc._mk(pirip_amd, cfg, fmt_h, 1, mask)
        seq = hs.demod_host(buf)
        assert hs.kernel() == "wave"
        return seq, tc._state(hs)

    seq, (sc_s, sf_s) = _once(("capture read loop", name), read_loop)
    monkeypatch.setenv("PIRIP_CAPTURE_SEG_FRAMES", str(segf))
    monkeypatch.setenv(switch, value)
    hc = tc._mk(pirip_amd, cfg, fmt_h, slots, mask)
    cap, reps = tc._capture(pirip_amd, hc, buf, pieces)
    print(name, switch, value, reps)
    tc._same(cap, seq, (name, switch, value))
    sc_c, sf_c = tc._state(hc)
    same_words(sf_c, sf_s, (name, switch, value, "Sf"))
    same_words(sc_c, sc_s, (name, switch, value, "stream state"))
    assert all(rp["segments"] >= 3 for rp in reps), reps


@pytest.mark.parametrize("decoder", ["fast", "bank"])
@pytest.mark.parametrize("name", [ls.SHIPPED, "unbalanced7"])
def test_ldpc_storage_layouts_decode_the_same_words(oracle, built_lib, tmp_path, monkeypatch, name, decoder):
    """PIRIP_LAYOUT_TRIES = 0 (the identity layout with its bank conflicts), 1000 and the default search, one code of each row-weight
    build (6 and 8) under the fast and the persistent decoder: the layout moves where variables and rows are stored, not the slot order
    inside a row or the edge order inside a variable, so no float sum changes its order -- codeword bits, iterations and parity counts are
    equal across layouts and each equals the oracle's. The layouts are told apart by their bank conflicts."""
    import test_ldpc_decoders as td
    code, path = td._code(oracle, tmp_path, name)
    assert ls.launch_path(code, decoder, 64, 1, 256)["build"] == (6 if name == ls.SHIPPED else 8)
    cw, llr, easy = ls.matrix_words(name, code)
    wb, wip = td._oracle_decode(oracle, ("matrix", name), code, llr)
    got, conflicts = {}, {}
    for tries in (None, "0", "1000"):
        if tries is None:
            monkeypatch.delenv("PIRIP_LAYOUT_TRIES", raising=False)
        else:
            monkeypatch.setenv("PIRIP_LAYOUT_TRIES", tries)
        h = td._handle(monkeypatch, decoder, path)
        conflicts[tries] = h.layout_conflicts()
        got[tries] = td._decode(h, llr)
        td._assert_equal(got[tries][0], got[tries][1], wb, wip, (name, decoder, "PIRIP_LAYOUT_TRIES", tries))
    print(name, decoder, "bank conflicts per iteration (identity, in use):", conflicts)
    ident = conflicts["0"][0]
    assert ident > 0 and conflicts["0"] == (ident, ident), conflicts
    assert conflicts[None][0] == ident and conflicts["1000"][0] == ident
    assert conflicts[None][1] <= conflicts["1000"][1] < ident, conflicts
    for tries in ("0", "1000"):
        assert np.array_equal(got[tries][0], got[None][0]) and np.array_equal(got[tries][1], got[None][1]), tries


# ======== env forms of two API switches ======================================================================================================
def test_env_forms_equal_the_api_forms(oracle, built_lib, monkeypatch):
    """PIRIP_EST_BAND=1 is pirip_hip_set_estimator_band_only(1) and PIRIP_EXACT0=0 is pirip_hip_set_exact_first_frame(0) for programs
    that only call create (the command-line tools): the same kernel and the same output words as the handle that made the call."""
    import pirip_amd
    u8 = ss.fft_input(oracle, sigutil, "awgn9")
    monkeypatch.delenv("PIRIP_EST_BAND", raising=False); monkeypatch.delenv("PIRIP_EXACT0", raising=False)
    plain = _cfg1_handle()
    r_plain = plain.demod_host(u8)
    api = _cfg1_handle()
    api.set_estimator_band_only(True)
    r_api = api.demod_host(u8)
    monkeypatch.setenv("PIRIP_EST_BAND", "1")
    c = sigutil.CFG1                      # (created bare: make_handle holds a handle to what its shape says, and this one's estimator comes from the environment)
    env = pirip_amd.HipDemod(c["Fs"], c["Rs"], c["M"], P=c["P"], est_min=c["est_min"], est_max=c["est_max"], in_format=0, nstreams=1)
    monkeypatch.delenv("PIRIP_EST_BAND")
    assert env.kernel_name() == api.kernel_name() != plain.kernel_name() and "band-only estimator" in env.kernel_name(), env.kernel_name()
    r_env = env.demod_host(u8)
    assert r_env["nframes"] >= 100
    same_results(r_env, r_api, "PIRIP_EST_BAND=1 against set_estimator_band_only")
    same_words(env.get_Sf(0), api.get_Sf(0), "Sf, band-only")
    same_results(r_env, r_plain, "the band-only estimator against the full one")          # (its own contract: outputs unchanged)

    api = _cfg1_handle()
    api.set_exact_first_frame(False)
    r_api = api.demod_host(u8)
    monkeypatch.setenv("PIRIP_EXACT0", "0")
    env = _cfg1_handle()
    monkeypatch.delenv("PIRIP_EXACT0")
    r_env = env.demod_host(u8)
    same_results(r_env, r_api, "PIRIP_EXACT0=0 against set_exact_first_frame(0)")
    same_words(env.get_Sf(0), api.get_Sf(0), "Sf, no prologue")
    # the switch does something on this input: without the prologue frame 0 is the wave kernel's rounding of the soft magnitudes
    assert not np.array_equal(words(r_api["rx_filt"][0]), words(r_plain["rx_filt"][0]))
    monkeypatch.setenv("PIRIP_EXACT0", "1")
    env = _cfg1_handle()
    same_results(env.demod_host(u8), r_plain, "PIRIP_EXACT0=1 against the default")


# ======== the tools' call sizes ================================================================================================================
CSDR_D, CSDR_BUF = 45, 16384
CSDR_SKIP = ((CSDR_BUF - 80) // CSDR_D + 1) * CSDR_D          # samples one block advances by
CSDR_INPUTS = {"less than one block": CSDR_BUF - 1, "exactly two block advances": CSDR_BUF + 2 * CSDR_SKIP,
               "five advances and a partial block": CSDR_BUF + 5 * CSDR_SKIP + 7000}


@pytest.mark.parametrize("K", ["1", "2", "1000"])
def test_csdr_tool_block_count_changes_no_output_byte(oracle, built_lib, K):
    """`csdr fir_decimate_cc 45` replays csdr's block loop PIRIP_CSDR_BLOCKS blocks per GPU call: one block per call, two, and more than
    the input holds. stdout is oracle_csdr_fir_decimate_stream's bytes whatever K is -- nothing for an input shorter than a block, the
    trailing partial block dropped."""
    for what, n in CSDR_INPUTS.items():
        def make():
            x = np.zeros((n, 2), dtype=np.float32)
            u8 = ss.random_bytes(n, 2 * n)
            oracle.lib().oracle_convert_u8_f(u8.ctypes.data, x.ctypes.data, 2 * n)
            out = np.zeros((n // CSDR_D + 2, 2), dtype=np.float32)
            k = oracle.lib().oracle_csdr_fir_decimate_stream(x.ctypes.data, n, out.ctypes.data, out.shape[0], CSDR_D, 0.05, CSDR_BUF)
            return x.tobytes(), out[:k].tobytes()
        raw, want = _once(("csdr", what), make)
        p = subprocess.run([os.path.join(BIN, "csdr"), "fir_decimate_cc", str(CSDR_D)], input=raw, capture_output=True,
                           env=dict(os.environ, PIRIP_CSDR_BLOCKS=K))
        assert p.returncode == 0, p.stderr
        blocks = (n - CSDR_BUF) // CSDR_SKIP + 1 if n >= CSDR_BUF else 0
        assert len(want) == 8 * blocks * (CSDR_SKIP // CSDR_D), (what, len(want))
        assert p.stdout == want, (what, K, len(p.stdout), len(want))


def _fsk_demod_input(oracle, tmp_path_factory):
    def make():
        import test_capture as tc
        buf = tc._signal(oracle, sigutil.CFG1, 30000, seed=31, ppm=40e-6, ebno_db=8.0)
        src = tmp_path_factory.mktemp("switches") / "in.u8"
        buf.tofile(src)
        argv = [os.path.join(BIN, "fsk_demod"), "-d", "-p", "24", "2", "240000", "10000"]
        env = {k: v for k, v in os.environ.items() if not k.startswith("PIRIP_FSK_DEMOD_")}
        p = subprocess.run(argv + ["-", "-"], input=src.read_bytes(), capture_output=True, env=env)
        assert p.returncode == 0 and len(p.stdout) >= 25000, p.stderr
        return src, argv, env, p.stdout
    return _once(("fsk_demod input",), make)


@pytest.mark.parametrize("switch,value,source", [("PIRIP_FSK_DEMOD_FRAMES", "1", "pipe"), ("PIRIP_FSK_DEMOD_FRAMES", "1", "file"),
                                                 ("PIRIP_FSK_DEMOD_FRAMES", "7", "pipe"), ("PIRIP_FSK_DEMOD_FRAMES", "7", "file"),
                                                 ("PIRIP_FSK_DEMOD_SLOTS", "3", "file"), ("PIRIP_FSK_DEMOD_SLOTS", "4", "file"),
                                                 ("PIRIP_FSK_DEMOD_SLOTS", "64", "file")])
def test_fsk_demod_tool_call_sizes_change_no_output_byte(oracle, built_lib, tmp_path, tmp_path_factory, switch, value, source):
    """PIRIP_FSK_DEMOD_FRAMES (frames per read-loop call; it also keeps a file off the capture route) and PIRIP_FSK_DEMOD_SLOTS (the
    capture's stream slots: 3 leaves too few for segments, 4 the fewest that has them, 64): the bits on stdout are the default run's."""
    src, argv, env, want = _fsk_demod_input(oracle, tmp_path_factory)
    env = dict(env, **{switch: value}, PIRIP_FSK_DEMOD_REPORT="1")
    if source == "pipe":
        p = subprocess.run(argv + ["-", "-"], input=src.read_bytes(), capture_output=True, env=env)
        got = p.stdout
    else:
        out = tmp_path / "out.bits"
        p = subprocess.run(argv + [str(src), str(out)], capture_output=True, env=env)
        got = out.read_bytes() if p.returncode == 0 else b""
    assert p.returncode == 0, p.stderr
    assert got == want, (switch, value, source, len(got), len(want))
    if switch == "PIRIP_FSK_DEMOD_SLOTS":
        assert b"capture:" in p.stderr, p.stderr
        assert (b" 1 segments of 0 frames" in p.stderr) == (value == "3"), p.stderr
    else:
        assert b"capture:" not in p.stderr
