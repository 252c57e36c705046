"""The wave kernel keeps frame-invariant work out of its frame loop: the correlator's per-lane start phasors are
reused while a stream's tone rows repeat and nin == N (anything else -- a call's first frame, the frame behind the exact prologue,
ninp == 0, a tone-bin change, nin or ninp != N -- rebuilds them), the peak search tests its range once per call, and the wave arg-max
reads the winner's index from the one lane that holds the maximum (ties fall back to the smallest-index reduction).

Every case runs 5 streams (a partial workgroup) of about ten frames and compares, per stream,
  * bits, per-frame stats, rx_filt, Sf, the stream scalars and `consumed` with the oracle (tests/parity.py's rules), and
  * every word of every output with the same library whose cache misses on every frame (PIRIP_FRAME_CACHE=0, read at create time).
"""
import numpy as np
import pytest

import sigutil
from demodrun import make_handle, make_oracle, run_calls, same_results
from parity import _compare, oracle_Sf

pytestmark = pytest.mark.gpu

CFG1_P8 = dict(sigutil.CFG1, P=8)
# "mask": the comb estimator at that tone spacing (its tone rows and phase steps are both functions of the comb position, the cache's key)
SHAPES = {"2fsk_p24": sigutil.CFG1, "2fsk_p8": CFG1_P8, "4fsk_p8": sigutil.CFG4,
          "2fsk_p8_mask": dict(CFG1_P8, mask=10000), "4fsk_p8_mask": dict(sigutil.CFG4, mask=10000)}
BIN_HZ = 937.5                      # Fs / Ndft of every shape here
NFRAMES = 13                        # frames of input per stream (the runs stop a few frames short: F below)
PPM = 2500e-6


def mixed_batch(oracle, c):
    """[steady, mover, steady on other bins, clock offset, steady at another timing phase]: each wave's cache key is its own. The mover's
    tones go one FFT bin up in the middle of the call, and back; the sample clock runs fast, then slow: the timing estimate crosses
    -1/4 and +1/4 symbol, nin takes N - Ts/4 and N + Ts/4"""
    return sigutil.mixed_batch(oracle, c, NFRAMES, (4, 4, NFRAMES - 7), lambda n: np.where(np.arange(n) < n // 3, 1.0 + PPM, 1.0 - PPM))


def run(c, host, F, per_call=None, cache=True, exact0=True, est=None, monkeypatch=None, reset_first=False):
    """All B streams until every stream has made F frames, per_call frames per call (None: one call), on a handle created with the frame
    cache on or off. Returns per-stream outputs and state."""
    import torch
    monkeypatch.setenv("PIRIP_FRAME_CACHE", "1" if cache else "0")
    lo, hi = est or (c["est_min"], c["est_max"])
    h = make_handle(c, host.shape[0], est_min=lo, est_max=hi)
    assert h.kernel() == "wave"
    if not exact0:
        h.set_exact_first_frame(False)
    if reset_first:
        # a used handle, then reset: the state a created handle starts from (ninp == 0)
        st = torch.cuda.current_stream().cuda_stream
        dev = torch.from_numpy(host).cuda()
        h.demod_batch(dev.data_ptr(), host.shape[1] * 2, host.shape[1], 0, 0, 0, 0, 0, 0, 0, 0, 3, st)
        h.reset(st)
    k = per_call or F
    res = run_calls(h, host, [min(k, F - done) for done in range(0, F, k)])
    h.close()
    return res


def against_oracle(oracle, c, host, res, est=None):
    """Each stream against its own oracle run over exactly the samples the device consumed. Returns the oracle results."""
    ros = []
    for s, rh in enumerate(res):
        o = make_oracle(oracle, c, est)
        ro = o.demod(host[s, :rh["consumed"]], oracle.IN_CU8_FSKDEMOD)
        _compare(ro, rh, M=c["M"])
        assert np.array_equal(rh["Sf"], oracle_Sf(oracle, o)), s
        # the stream scalars are the last frame's stats row (f_est, timing, SNRest, nin, ppm), which _compare has just held to the oracle's
        last = rh["stats"][-1]
        assert np.array_equal(rh["scalars"][[0, 1, 2, 3, 4, 5, 7]], last[[0, 1, 2, 3, 4, 5, 7]]) and rh["scalars"][6] == last[6] == o.nin(), s
        ros.append(ro)
    return ros


def frames_for(oracle, c, host, est=None):
    """F: one frame fewer than the shortest oracle run, so that every stream has the samples for F frames in every call pattern"""
    return min(make_oracle(oracle, c, est).demod(host[s], oracle.IN_CU8_FSKDEMOD, want_filt=False)["nframes"] for s in range(host.shape[0])) - 1


@pytest.fixture(scope="module")
def batches(oracle):
    return {name: mixed_batch(oracle, c) for name, c in SHAPES.items()}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_steady_moving_tones_and_nin_steps_hit_and_miss_alike(oracle, built_lib, batches, monkeypatch, shape):
    """Cases 1-3 in one batch: steady streams (hits from the second frame on), a stream whose tones move one bin and back (a miss at
    either move, hits in between) beside streams that stay, and a stream whose nin takes N - Ts/4 and N + Ts/4."""
    c, host = SHAPES[shape], batches[shape]
    F = frames_for(oracle, c, host)
    assert 8 <= F <= 12
    hit = run(c, host, F, monkeypatch=monkeypatch)
    ros = against_oracle(oracle, c, host, hit)
    # the input does what the case needs (the oracle's own per-frame stats): stream 0 keeps its bins, stream 1 moves and comes back,
    # stream 3 sees both nin steps
    N, Q = c["Fs"] // c["Rs"] * 50, c["Fs"] // c["Rs"] // 4
    f0, f1 = ros[0]["stats"][2:, 0], ros[1]["stats"][:, 0]
    assert (f0 == f0[0]).all()
    moves = np.flatnonzero(np.diff(f1) != 0)
    assert len(moves) >= 2 and moves[0] >= 2 and f1[-1] == f1[moves[0]], f1
    nin = ros[3]["stats"][:, 6]
    assert (nin == N - Q).any() and (nin == N + Q).any() and (nin == N).any(), nin
    same_results(hit, run(c, host, F, cache=False, monkeypatch=monkeypatch), "cache off")


@pytest.mark.parametrize("shape,per_call", [("2fsk_p24", 1), ("2fsk_p24", 2), ("2fsk_p24", 3), ("2fsk_p8", 2), ("4fsk_p8", 3), ("2fsk_p8_mask", 2), ("4fsk_p8_mask", 1)])
def test_cache_does_not_survive_a_call_boundary(oracle, built_lib, batches, monkeypatch, shape, per_call):
    """Case 4: the same input as one call and as calls of 1, 2 and 3 frames: a call's first frame rebuilds the start state."""
    c, host = SHAPES[shape], batches[shape]
    F = frames_for(oracle, c, host)
    one = run(c, host, F, monkeypatch=monkeypatch)
    parts = run(c, host, F, per_call=per_call, monkeypatch=monkeypatch)
    same_results(one, parts, f"calls of {per_call}")
    against_oracle(oracle, c, host, parts)
    same_results(parts, run(c, host, F, per_call=per_call, cache=False, monkeypatch=monkeypatch), "cache off")


@pytest.mark.parametrize("exact0", [True, False])
def test_first_call_after_reset_with_and_without_the_exact_prologue(oracle, built_lib, batches, monkeypatch, exact0):
    """Case 5: ninp == 0 in the first frame the wave kernel sees -- frame 1 behind the exact prologue, frame 0 without it -- on a
    created handle and on a used one after reset."""
    c, host = SHAPES["2fsk_p24"], batches["2fsk_p24"]
    F = frames_for(oracle, c, host)
    fresh = run(c, host, F, exact0=exact0, monkeypatch=monkeypatch)
    against_oracle(oracle, c, host, fresh)
    same_results(fresh, run(c, host, F, exact0=exact0, reset_first=True, monkeypatch=monkeypatch), "after reset")
    same_results(fresh, run(c, host, F, exact0=exact0, cache=False, monkeypatch=monkeypatch), "cache off")


def test_all_neutral_input_takes_the_tie_path(oracle, built_lib, monkeypatch):
    """Case 6: every Sf equal (zero), best == 0 on every lane: all 64 lanes hold the maximum, the arg-max falls back to the
    smallest-index reduction."""
    c = sigutil.CFG1
    host = np.full((5, 10 * 1200 + 700, 2), 127, dtype=np.uint8)
    F = frames_for(oracle, c, host)
    hit = run(c, host, F, monkeypatch=monkeypatch)
    for s, ro in enumerate(against_oracle(oracle, c, host, hit)):
        # (nothing exceeds best = 0: both tones end on index 0 of the shifted spectrum, -Fs/2)
        assert not hit[s]["Sf"].any() and (ro["stats"][:, :2] == -c["Fs"] / 2).all() and (hit[s]["stats"][:, :2] == -c["Fs"] / 2).all()
    same_results(hit, run(c, host, F, cache=False, monkeypatch=monkeypatch), "cache off")


def test_bit_equal_maxima_in_two_lanes_smaller_bin_wins(oracle, built_lib, monkeypatch):
    """Case 7: a REAL input (Q at the neutral byte: converted to exactly 0) has a spectrum mirrored about DC, and kiss_fft's dataflow keeps
    the mirror exact in float32 (conjugate twiddles, sign-symmetric rounding): Sf[128 - k] == Sf[128 + k] bit for bit, in different lanes
    (checked below on the oracle's own Sf). The lower tone sits three bins above DC and the search range reaches down to -4 kHz, so the
    lower tone's peak is held by bins 125 and 131 alike; codec2 takes the first, the smaller bin, whose blanking (8 bins
    either side) removes the other: the lower tone estimate must be NEGATIVE, -2812.5 Hz. (The upper tone's mirror is outside the search
    range; with both tones mirrored inside it -- the first input tried -- every symbol decision of the later frames is an exact tie in
    the oracle itself, and bits cannot be compared.)"""
    c = dict(sigutil.CFG1, f1=2812)
    est = (-4000, 25000)
    rows = []
    for s in range(5):
        x = sigutil.mod_frames(oracle, c, NFRAMES + 1, 40 + s)
        x[:, 1] = 0.0
        rows.append(oracle.quantise_cu8(x)[5 * s:])
    n = min(r.shape[0] for r in rows)
    host = np.stack([r[:n] for r in rows])
    assert (host[:, :, 1] == 127).all()
    F = frames_for(oracle, c, host, est)
    hit = run(c, host, F, est=est, monkeypatch=monkeypatch)
    for s, ro in enumerate(against_oracle(oracle, c, host, hit, est=est)):
        Sf = hit[s]["Sf"]                                      # (the oracle's, bit for bit: against_oracle)
        assert np.array_equal(Sf[1:128][::-1].view(np.uint32), Sf[129:].view(np.uint32)), "the oracle's Sf is not mirrored exactly"
        assert Sf[125] == Sf[131] == Sf[118:139].max()         # the lower tone's peak sits in two bins, both inside the search range
        assert (ro["stats"][2:, 0] == -3 * BIN_HZ).all() and (ro["stats"][2:, 1] > 0).all(), ro["stats"][:, :2]
        assert np.array_equal(hit[s]["stats"][:, :2], ro["stats"][:, :2])
    same_results(hit, run(c, host, F, est=est, cache=False, monkeypatch=monkeypatch), "cache off")
