"""The workgroup-per-stream demodulator (pirip_amd/csrc/fsk_demod_block.hip: `rtl_fsk -r 1000` at 240 kS/s, Ts = 240, P = 15, Ndft = 4096)
against the oracle on every path it can take: all eight template instances, state carried through ragged chunks, every start offset of a
symbol (where the correlator changes from last frame's oscillator to this frame's), a sustained clock offset in both directions, the
packed-bit epilogue, what a call leaves outside its outputs, the scalar state of a call without a stats output, every 16-byte residue of the
sample loads, reset, burst mode, run-time estimator limits, the capture entry point and two handles at once.

Bar: frame and sample counts, tone estimates, the nin sequence, bits and Sf exact; soft magnitudes within
RX_FILT_TOL x N / 2400 = 5e-4 of the peak; two runs of the same kernel on the same samples equal bit for bit. The inputs are those of
tests/blockshapes.py; tests/test_block_demod_cpu.py shows on the oracle alone that they reach the paths named here."""
import numpy as np
import pytest

import blockshapes as bs
from demodrun import host_chunks, same_results, same_words, scalars, stream_state
from parity import RX_FILT_TOL, _compare

pytestmark = pytest.mark.gpu

TOL = 5 * RX_FILT_TOL            # RX_FILT_TOL x N / 2400
FILL = 0xA5
NFILT = bs.NSYM                  # soft magnitudes per tone and frame


def _state(h, s=0):
    """the 13 words of stream s's pirip_stream_state and its Sf"""
    return stream_state(h, s), h.get_Sf(s)


class Batch:
    """One pirip_hip_demod_batch call on device arrays that were filled with 0xA5: B streams of the same length at in_stride bytes from
    byte `base` of one buffer; every stream's output row block holds `rows` frames and `pad` more elements than that."""

    def __init__(self, h, streams, rows, in_pad=2, base=0, pad=(5, 3, 7), frame_bytes=None):
        import torch
        self.h, self.B, self.rows, self.pad = h, len(streams), rows, pad
        self.nsamp = min(x.shape[0] for x in streams)
        self.in_stride = 2 * self.nsamp + in_pad
        flat = np.full(base + self.B * self.in_stride + 64, 0x7F, dtype=np.uint8)
        for s, x in enumerate(streams):
            flat[base + s * self.in_stride: base + s * self.in_stride + 2 * self.nsamp] = x[:self.nsamp].reshape(-1)
        self.dev, self.base = torch.from_numpy(flat).cuda(), base
        assert self.dev.data_ptr() % 16 == 0
        self.fb = frame_bytes if frame_bytes is not None else h.Nbits
        self.width = (rows * self.fb + pad[0], rows * h.M * NFILT + pad[1], rows * 10 + pad[2])       # elements per stream: bits, filt, stats
        mk = lambda n: torch.full((self.B, n), FILL, dtype=torch.uint8, device="cuda")
        self.bits, self.filt, self.stats = mk(self.width[0]), mk(4 * self.width[1]), mk(4 * self.width[2])
        self.nfr, self.cons = mk(4).view(torch.int32), mk(8).view(torch.int64)

    def run(self, max_frames, want_filt=True, want_stats=True, stream=0):
        self.h.demod_batch(self.dev.data_ptr() + self.base, self.in_stride, self.nsamp, self.bits.data_ptr(), self.width[0],
                           self.filt.data_ptr() if want_filt else 0, self.width[1], self.stats.data_ptr() if want_stats else 0, self.width[2],
                           self.nfr.data_ptr(), self.cons.data_ptr(), max_frames, stream)
        return self

    def fetch(self):
        """per stream: the result, and whether everything outside its nframes rows still holds the fill"""
        import torch
        torch.cuda.synchronize()
        bits, filt, stats = self.bits.cpu().numpy(), self.filt.cpu().numpy(), self.stats.cpu().numpy()
        nfr, cons = self.nfr.cpu().numpy().reshape(-1), self.cons.cpu().numpy().reshape(-1)
        out = []
        for s in range(self.B):
            n = int(nfr[s])
            assert 0 <= n <= self.rows, n
            nb, nf, ns = n * self.fb, 4 * n * self.h.M * NFILT, 4 * n * 10
            out.append({"nframes": n, "consumed": int(cons[s]), "bits": bits[s, :nb].reshape(n, self.fb).copy(),
                        "rx_filt": filt[s, :nf].copy().view(np.float32).reshape(n, self.h.M * NFILT),
                        "stats": stats[s, :ns].copy().view(np.float32).reshape(n, 10),
                        "untouched": bool((bits[s, nb:] == FILL).all() and (filt[s, nf:] == FILL).all() and (stats[s, ns:] == FILL).all())})
        return out


# ---- a ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(bs.ROWS))
def test_every_instance_one_shot_and_ragged_chunks_equal_the_oracle(oracle, built_lib, name):
    """Each of the eight instances on a noise-free stream and one at 9 dB, 31 frames from the row's start offset: one call, then ragged
    chunks of 1 ... 40000 samples (the raw tail, the trailer and Sf saved and reloaded through the fftshift index at every call). Both equal
    the oracle, Sf bit for bit after both, and the chunked run equals the one-shot run of the same kernel in every output word."""
    import pirip_amd
    M, fmt, mask, _ = bs.ROWS[name]
    for noisy, u8 in enumerate(bs.row_streams(oracle, name)):
        o = bs.oracle_of(oracle, M, mask)
        ro = o.demod(u8, bs.fmt_of(oracle, fmt))
        Sf_o = bs.oracle_Sf(oracle, o)
        assert ro["nframes"] >= 30
        h1 = bs.handle_of(pirip_amd, M, fmt, mask)
        assert h1.kernel() == "block" and ("mask" in h1.kernel_name()) == bool(mask) and ("M=%d," % M) in h1.kernel_name() \
            and ("u8 csdr" if fmt == "csdr" else "u8 -d") in h1.kernel_name(), h1.kernel_name()
        r1 = h1.demod_host(u8)
        nflips = _compare(ro, r1, tol=TOL, allow_near_tie_flips=bool(noisy), M=M)
        same_words(h1.get_Sf(0), Sf_o, (name, noisy, "Sf after one shot"))
        h2 = bs.handle_of(pirip_amd, M, fmt, mask)
        cuts = [int(c) for c in np.cumsum(bs.chunk_sizes(sorted(bs.ROWS).index(name) + 10 * noisy, u8.shape[0])) if c < u8.shape[0]]
        ncalls = len(cuts) + 1
        r2 = host_chunks(h2, u8, cuts)
        assert ncalls >= 3
        _compare(ro, r2, tol=TOL, allow_near_tie_flips=bool(noisy), M=M)
        same_words(h2.get_Sf(0), Sf_o, (name, noisy, "Sf after chunks"))
        same_results(r2, r1, (name, noisy, "chunks against one shot"))
        same_words(_state(h2)[0], _state(h1)[0], (name, noisy, "stream state"))
        print(f"{name} {'9 dB' if noisy else 'clean'}: {ro['nframes']} frames, {ncalls} chunks, {nflips} near-tie flips, "
              f"rx_filt error {np.abs(r1['rx_filt'].astype(np.float64) - ro['rx_filt']).max() / np.abs(ro['rx_filt']).max():.2e} of the peak (bar {TOL:g})")


# ---- b ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [2, 4])
@pytest.mark.parametrize("fmt", ["u8d", "csdr"])
def test_all_240_start_offsets_in_one_batch(oracle, built_lib, fmt, M):
    """Every timing phase of a symbol: stream `off` starts `off` samples into the same noise-free recording, so the first new sample of a
    frame -- where one thread of the correlator changes oscillators in the middle of a 16-sample step -- falls on every thread / step /
    position the three nin values allow, and all three nin values occur. 240 streams, 5 frames each, one launch, at a stride that is only
    sample-aligned. No stream is exempt from an exact nin sequence (tests/test_block_demod_cpu.py: none comes near the threshold)."""
    import pirip_amd
    want = bs.sweep_oracle(oracle, M, fmt)
    h = bs.handle_of(pirip_amd, M, fmt, nstreams=bs.TS)
    assert h.kernel() == "block"
    b = Batch(h, [bs.sweep_stream(oracle, M, fmt, off) for off in range(bs.TS)], rows=bs.SWEEP_FRAMES + 2)
    got = b.run(bs.SWEEP_FRAMES + 2).fetch()
    worst = 0.0
    for off in range(bs.TS):
        ro, rh = want[off], got[off]
        assert rh["nframes"] == bs.SWEEP_FRAMES and rh["untouched"], off
        try:
            _compare(ro, rh, tol=TOL, M=M)
        except AssertionError as e:
            raise AssertionError(f"start offset {off}: {e}") from e
        same_words(h.get_Sf(off), ro["Sf"], ("Sf of start offset", off))
        worst = max(worst, float(np.abs(rh["rx_filt"].astype(np.float64) - ro["rx_filt"]).max() / np.abs(ro["rx_filt"]).max()))
    print(f"{fmt} M = {M}: 240 start offsets, largest rx_filt error {worst:.2e} of the peak (bar {TOL:g})")


# ---- c ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,fmt", [(2, "csdr"), (4, "u8d")])
@pytest.mark.parametrize("ppm", [bs.CLOCK_PPM, -bs.CLOCK_PPM])
def test_sustained_clock_offset(oracle, built_lib, ppm, M, fmt):
    """A sample clock off by +-300 ppm for 39 frames: the timing estimate walks to the threshold and nin steps twice, short frames on the
    fast clock and long ones on the slow clock."""
    import pirip_amd
    u8 = bs.clock_stream(oracle, M, fmt, ppm)
    o = bs.oracle_of(oracle, M)
    ro = o.demod(u8, bs.fmt_of(oracle, fmt))
    assert bs.clock_counts_ok(ro, ppm), ro["stats"][:, 6]
    h = bs.handle_of(pirip_amd, M, fmt)
    assert h.kernel() == "block"
    _compare(ro, h.demod_host(u8), tol=TOL, M=M)
    same_words(h.get_Sf(0), bs.oracle_Sf(oracle, o), "Sf")


# ---- d ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", bs.PACKED_ROWS)
def test_packed_bits_equal_packbits_of_the_unpacked_twin(oracle, built_lib, name):
    """pirip_hip_set_bit_packing on this kernel (two ballots, a bit reverse for 2-FSK, nibble interleaving for 4-FSK): 7 / 13 bytes per frame
    equal to numpy.packbits of what a twin handle without packing writes, every other output word the twin's, and nothing written past the
    frames' bytes."""
    import pirip_amd
    M, fmt, mask, _ = bs.ROWS[name]
    streams = bs.packed_streams(oracle, name)
    fb = {2: 7, 4: 13}[M]
    hp, ht = bs.handle_of(pirip_amd, M, fmt, mask, nstreams=2), bs.handle_of(pirip_amd, M, fmt, mask, nstreams=2)
    assert hp.kernel() == "block" and ht.kernel() == "block"
    hp.set_bit_packing(True)
    rows = hp.max_frames_for(streams[0].shape[0]) + 1
    bt = Batch(ht, streams, rows)
    packed, twin = Batch(hp, streams, rows, frame_bytes=fb).run(rows).fetch(), bt.run(rows).fetch()
    for s in range(2):
        assert twin[s]["nframes"] >= 10 and twin[s]["bits"].max() == 1 and twin[s]["untouched"] and packed[s]["untouched"]
        assert packed[s]["nframes"] == twin[s]["nframes"] and packed[s]["consumed"] == twin[s]["consumed"]
        assert packed[s]["bits"].shape == (twin[s]["nframes"], fb)
        same_words(packed[s]["bits"], np.packbits(twin[s]["bits"], axis=1), (name, s, "packed bits"))
        same_words(packed[s]["rx_filt"], twin[s]["rx_filt"], (name, s, "rx_filt"))
        same_words(packed[s]["stats"], twin[s]["stats"], (name, s, "stats"))
    # ... and the twin is not wrong in the same way: its first stream against the oracle
    _compare(bs.oracle_of(oracle, M, mask).demod(streams[0][:bt.nsamp], bs.fmt_of(oracle, fmt)), twin[0], tol=TOL, allow_near_tie_flips=True, M=M)


# ---- e ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,fmt", [(2, "u8d"), (4, "csdr")])
def test_a_call_stopped_by_max_frames_writes_its_frames_and_nothing_else(oracle, built_lib, M, fmt):
    """Three streams whose second frames are short, long and nominal, stopped after three frames with two more in the buffer: three
    different consumed counts, rows 3 and 4 of every output and the padding behind each stream's rows keep their fill."""
    import pirip_amd
    offs = (bs.OFF_SHORT, bs.OFF_LONG, bs.OFF_EVEN)
    h = bs.handle_of(pirip_amd, M, fmt, nstreams=3)
    assert h.kernel() == "block"
    got = Batch(h, [bs.sweep_stream(oracle, M, fmt, o) for o in offs], rows=5).run(3).fetch()
    want = bs.sweep_oracle(oracle, M, fmt)
    assert len({g["consumed"] for g in got}) == 3
    for g, o in zip(got, offs):
        ro = {k: (v[:3] if isinstance(v, np.ndarray) and k != "Sf" else v) for k, v in want[o].items()}
        ro["nframes"], ro["consumed"] = 3, int(bs.N + want[o]["stats"][:2, 6].sum())
        assert g["nframes"] == 3 and g["untouched"], (o, g["nframes"], g["untouched"])
        _compare(ro, g, tol=TOL, M=M)


# ---- f ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", bs.SCALAR_ROWS)
@pytest.mark.parametrize("ending", ["samples run out", "max_frames reached"])
def test_stream_scalars_after_a_call_without_stats_output(oracle, built_lib, ending, name):
    """SNRest / EbNodB / v_est are computed on observable frames only: those whose stats row is written, and the last frame of a call --
    last because max_frames is reached or because the next frame does not fit. A call without a stats output must leave the scalars a
    call with one leaves, and they are the last stats row."""
    import pirip_amd
    M, fmt, mask, _ = bs.ROWS[name]
    u8 = bs.scalar_stream(oracle, name)
    rows = bs.handle_of(pirip_amd, M, fmt, mask).max_frames_for(u8.shape[0])
    maxf = bs.SCALAR_MAX_FRAMES if ending == "max_frames reached" else rows
    out = []
    for want_stats in (True, False):
        h = bs.handle_of(pirip_amd, M, fmt, mask)
        assert h.kernel() == "block"
        r = Batch(h, [u8], rows).run(maxf, want_filt=False, want_stats=want_stats).fetch()[0]
        assert r["untouched"]
        out.append((r, scalars(h), _state(h)[0]))
    (r1, sc1, st1), (r2, sc2, st2) = out
    assert r1["nframes"] == r2["nframes"] >= 5 and r1["consumed"] == r2["consumed"]
    assert (r1["nframes"] == bs.SCALAR_MAX_FRAMES and u8.shape[0] - r1["consumed"] > bs.N + bs.Q) if ending == "max_frames reached" \
        else u8.shape[0] - r1["consumed"] < bs.N - bs.Q
    same_words(r1["bits"], r2["bits"], "bits")
    assert r2["stats"].shape == (r1["nframes"], 10) and (r2["stats"].view(np.uint8) == FILL).all()       # no stats asked for, none written
    same_words(sc1, sc2, "scalars with and without the stats output")
    # (the rest of the state too, but for word 3, snr_est: a running average over the observable frames -- every frame with a stats output, the
    #  call's last one without, as include/pirip_hip.h says of pirip_stream_state)
    keep = [i for i in range(13) if i != 3]          # (the 13 words of the structure: all the library writes)
    same_words(st1[keep], st2[keep], "stream state with and without the stats output")
    last = r1["stats"][-1]
    same_words(sc1[[0, 1, 4, 5, 7]], last[[0, 1, 4, 5, 7]], "scalars against the last stats row")
    assert sc1[6] == last[6] and sc1[5] > 1.0


# ---- g ---------------------------------------------------------------------------------------------------------------------------------
def test_sample_loads_at_every_16_byte_residue(oracle, built_lib):
    """The correlator reads its new samples as 16-byte pieces at the alignment of a sample (2 bytes). Eight streams with the same samples, a
    stream length that is a multiple of 16 bytes and a stride 2 bytes longer: stream s starts at byte residue 2 s of 16; and the whole
    batch moved by 2, 6 and 14 bytes. Every stream of every run gives stream 0's words, and those are the oracle's."""
    import pirip_amd
    M, fmt = 2, "u8d"
    nsamp = bs.SWEEP_LEN - bs.SWEEP_LEN % 8
    assert (2 * nsamp) % 16 == 0
    u8 = bs.sweep_stream(oracle, M, fmt, bs.OFF_LONG)[:nsamp]
    ref = None
    for base in (0, 2, 6, 14):
        h = bs.handle_of(pirip_amd, M, fmt, nstreams=8)
        assert h.kernel() == "block"
        b = Batch(h, [u8] * 8, rows=bs.SWEEP_FRAMES + 1, in_pad=2, base=base)
        assert sorted((base + s * b.in_stride) % 16 for s in range(8)) == [0, 2, 4, 6, 8, 10, 12, 14]
        got = b.run(bs.SWEEP_FRAMES + 1).fetch()
        ref = ref or (got[0], h.get_Sf(0))
        for s in range(8):
            assert got[s]["untouched"]
            same_results(got[s], ref[0], ("base", base, "stream", s))
            same_words(h.get_Sf(s), ref[1], ("Sf, base", base, "stream", s))
    ro = bs.sweep_oracle(oracle, M, fmt)[bs.OFF_LONG]
    assert (ro["stats"][:, 6] == bs.N + bs.Q).any()
    _compare(ro, ref[0], tol=TOL, M=M)
    same_words(ref[1], ro["Sf"], "Sf")


# ---- h ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", bs.PAIR_ROWS)
def test_reset_gives_a_created_stream(oracle, built_lib, name):
    """pirip_hip_reset after a recording: the trailer is back at nin = 0 (no integrator memory: old positions contribute zeros), Sf at zero,
    and the next recording comes out as from a new handle -- outputs, Sf and stream state, word for word. The same on a batch of three,
    reset on a HIP stream of its own between two calls. (The handle has one reset, for all of its streams.)"""
    import torch
    import pirip_amd
    M, fmt, mask, _ = bs.ROWS[name]
    A, B = bs.pair_streams(oracle, name)
    h, fresh = bs.handle_of(pirip_amd, M, fmt, mask), bs.handle_of(pirip_amd, M, fmt, mask)
    assert h.kernel() == "block"
    ra = h.demod_host(A)
    assert ra["nframes"] >= 10 and h.get_Sf(0).max() > 0
    h.reset()
    assert h.kernel() == "block" and not h.get_Sf(0).any()
    rb, rf = h.demod_host(B), fresh.demod_host(B)
    same_results(rb, rf, (name, "after reset against a new handle"))
    for x, y, what in zip(_state(h), _state(fresh), ("stream state", "Sf")):
        same_words(x, y, (name, what))
    same_words(scalars(h), scalars(fresh), (name, "scalars"))
    _compare(bs.oracle_of(oracle, M, mask).demod(B, bs.fmt_of(oracle, fmt)), rb, tol=TOL, M=M)       # (B is the noise-free one)
    # a batch of three: A, then reset on another HIP stream, then B with each stream a different 0 / 16 / 33 samples in
    hb, twin = bs.handle_of(pirip_amd, M, fmt, mask, nstreams=3), bs.handle_of(pirip_amd, M, fmt, mask, nstreams=3)
    rows = hb.max_frames_for(A.shape[0])
    Batch(hb, [A[k:] for k in (0, 16, 33)], rows).run(rows).fetch()
    side = torch.cuda.Stream()
    hb.reset(side.cuda_stream)
    second = [B[k:] for k in (0, 16, 33)]
    bq = Batch(hb, second, rows)
    torch.cuda.synchronize()                   # (its arrays were filled on the default stream)
    got = bq.run(rows, stream=side.cuda_stream).fetch()
    want = Batch(twin, second, rows).run(rows).fetch()
    for s in range(3):
        assert got[s]["nframes"] >= 10 and got[s]["untouched"]
        same_results(got[s], want[s], (name, "batch after reset, stream", s))
        for x, y, what in zip(_state(hb, s), _state(twin, s), ("stream state", "Sf")):
            same_words(x, y, (name, what, s))


# ---- i ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,fmt", [(2, "csdr"), (4, "u8d")])
def test_burst_mode_pins_nin(oracle, built_lib, M, fmt):
    """fsk_enable_burst_mode() on a stream whose first timing estimate lies beyond -0.25 (start offset OFF_SHORT of the sweep: without burst
    mode its second frame is short): nin stays N in every frame."""
    import pirip_amd
    u8 = bs.sweep_base(oracle, M, fmt)[bs.OFF_SHORT:]
    assert (bs.sweep_oracle(oracle, M, fmt)[bs.OFF_SHORT]["stats"][:, 6] != bs.N).any()
    o, h = bs.oracle_of(oracle, M), bs.handle_of(pirip_amd, M, fmt)
    o.enable_burst_mode(); h.set_burst_mode(True)
    assert h.kernel() == "block"
    ro, rh = o.demod(u8, bs.fmt_of(oracle, fmt)), h.demod_host(u8)
    assert ro["nframes"] >= 5 and (ro["stats"][:, 6] == bs.N).all() and (np.abs(ro["stats"][:, 4]) > 0.25).any()
    _compare(ro, rh, tol=TOL, M=M)
    same_words(h.get_Sf(0), bs.oracle_Sf(oracle, o), "Sf")


def test_estimator_limits_set_on_the_live_handle(oracle, built_lib):
    """pirip_hip_set_freq_est_limits(500, 12000) after create: still the block instance, the words of a handle created with that range and
    the oracle's with it -- and not those of the default range (the upper tone lies outside the new one)."""
    import pirip_amd
    M, fmt = 2, "csdr"
    u8 = bs.limits_stream(oracle)
    h, made, default = bs.handle_of(pirip_amd, M, fmt), bs.handle_of(pirip_amd, M, fmt, est_min=bs.LIMITS[0], est_max=bs.LIMITS[1]), \
        bs.handle_of(pirip_amd, M, fmt)
    assert h.set_freq_est_limits(*bs.LIMITS) == 0
    assert h.kernel() == "block" and made.kernel() == "block"
    r, rm, rd = h.demod_host(u8), made.demod_host(u8), default.demod_host(u8)
    same_results(r, rm, "limits set against limits at create")
    same_words(h.get_Sf(0), made.get_Sf(0), "Sf")
    o = bs.oracle_of(oracle, M, est_min=bs.LIMITS[0], est_max=bs.LIMITS[1])
    _compare(o.demod(u8, bs.fmt_of(oracle, fmt)), r, tol=TOL, allow_near_tie_flips=True, M=M)
    same_words(h.get_Sf(0), bs.oracle_Sf(oracle, o), "Sf against the oracle")
    assert rd["nframes"] == r["nframes"] and not np.array_equal(rd["stats"][:, :2], r["stats"][:, :2])


# ---- j ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nstreams", [1, 4])
@pytest.mark.parametrize("pieces", [1, 3])
def test_capture_on_a_block_handle_equals_the_read_loop(oracle, built_lib, pieces, nstreams):
    """pirip_hip_demod_capture on this kernel takes its sequential route (one segment) on stream slot 0, whole or in three pieces: the
    read loop's words -- bits, rx_filt, stats with the ppm column, counts, the state left behind and Sf."""
    import pirip_amd
    from test_capture import _capture
    M, fmt, mask, _ = bs.ROWS[bs.CAPTURE_ROW]
    u8 = np.array(bs.capture_stream(oracle))           # (a writable copy: the capture helper hands it to torch)
    hs, hc = bs.handle_of(pirip_amd, M, fmt, mask), bs.handle_of(pirip_amd, M, fmt, mask, nstreams=nstreams)
    assert hs.kernel() == "block" and hc.kernel() == "block"
    seq = hs.demod_host(u8)
    assert seq["nframes"] == 25
    cap, reports = _capture(pirip_amd, hc, u8, pieces)
    assert len(reports) == pieces and all(r["segments"] == 1 and r["passes"] == 1 for r in reports), reports
    same_results(cap, seq, "capture against the read loop")
    for x, y, what in zip(_state(hc), _state(hs), ("stream state", "Sf")):
        same_words(x, y, what)
    same_words(scalars(hc), scalars(hs), "scalars")
    _compare(bs.oracle_of(oracle, M, mask).demod(u8, bs.fmt_of(oracle, fmt)), cap, tol=TOL, allow_near_tie_flips=True, M=M)


# ---- k ---------------------------------------------------------------------------------------------------------------------------------
def test_two_block_handles_on_two_hip_streams_at_once(oracle, built_lib):
    """A 2-FSK and a 4-FSK mask handle, eight streams of ten frames each, enqueued on two HIP streams without a synchronisation in
    between: each gives the words it gives alone."""
    import torch
    import pirip_amd
    jobs = []
    for name in bs.PAIR_ROWS:
        M, fmt, mask, _ = bs.ROWS[name]
        streams = bs.pair_streams(oracle, name, 8)
        h = bs.handle_of(pirip_amd, M, fmt, mask, nstreams=8)
        assert h.kernel() == "block"
        rows = h.max_frames_for(min(x.shape[0] for x in streams))
        alone = Batch(h, streams, rows).run(rows).fetch()
        assert all(r["nframes"] >= 10 and r["untouched"] for r in alone)
        h.reset()
        jobs.append((name, h, Batch(h, streams, rows), rows, alone, torch.cuda.Stream()))
    torch.cuda.synchronize()
    for name, h, b, rows, alone, st in jobs:
        b.run(rows, stream=st.cuda_stream)
    for name, h, b, rows, alone, st in jobs:
        for s, (g, w) in enumerate(zip(b.fetch(), alone)):
            assert g["untouched"]
            same_results(g, w, (name, "stream", s))
