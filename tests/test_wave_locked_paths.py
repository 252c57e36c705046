"""What a locked receiver's frames skip in the wave kernel ("locked paths"): on a frame-cache hit the correlator branches
round its oscillator-switch selects, and a call whose search range reaches only bin slots 0 and 1 searches those two. With the test
hook PIRIP_FRAME_CACHE=0 (read at create time) every frame runs the selecting correlator and the four-slot search: the two settings
must agree word for word, and either must agree with the oracle.

Every case runs 5 streams (4 per workgroup: the last one partial) of about twelve frames. Compared between the hook settings: bits,
rx_filt, every stats column, Sf, the stream scalars, pirip_stream_state and `consumed` -- and the same again with the input handed over in
ragged calls, which is how the state block a call leaves behind (raw tail, tone rows, last frame's length: no accessor of its own) shows.
The instances that have not taken the locked paths run the same code under both settings apart from the frame cache itself; they are
here so that taking them later is tested from the start.
"""
import numpy as np
import pytest

import sigutil
from demodrun import make_handle, make_oracle, run_calls, same_results
from parity import _compare, oracle_Sf

pytestmark = pytest.mark.gpu

NFRAMES = 14
U8D, CSDR, CF32 = 0, 1, 3          # pirip_amd.IN_* == oracle.IN_*


def shape(Fs, M, P, fmt, est_max, band=False, f1=10000, shift=10000):
    return dict(Fs=Fs, Rs=10000, M=M, P=P, f1=f1, shift=shift, est_min=500, est_max=est_max, fmt=fmt, band=band)


SHAPES = {
    "headline_u8": shape(240000, 2, 24, U8D, 25000),
    "csdr_u8": shape(240000, 2, 24, CSDR, 25000),
    "4fsk_p8": shape(240000, 4, 8, U8D, 60000),
    "ts20_f32": shape(200000, 2, 10, CF32, 90000),         # NFFT = 6: a partial second FFT batch
    "ts18_f32": shape(180000, 2, 9, CF32, 80000),
    "band_only": shape(240000, 2, 24, U8D, 25000, band=True),
}


def mixed_batch(oracle, c):
    """the mover's tones go one FFT bin up half-way through; the sample clock is 2500 ppm fast"""
    h = (NFRAMES + 1) // 2
    return sigutil.mixed_batch(oracle, c, NFRAMES, (h, NFRAMES + 1 - h), lambda n: np.full(n, 1.0 + 2500.0 * 1e-6))


def run(c, host, calls, cache, monkeypatch, limits=None):
    """run_calls on a wave handle created with the frame cache on or off. limits[i] (when given and not None):
    pirip_hip_set_freq_est_limits before call i. Returns per-stream results."""
    monkeypatch.setenv("PIRIP_FRAME_CACHE", "1" if cache else "0")
    h = make_handle(c, host.shape[0])
    assert h.kernel() == "wave"

    def set_limits(i, h):
        if limits and limits[i]:
            assert h.set_freq_est_limits(*limits[i]) == 0
    res = run_calls(h, host, calls, before_call=set_limits)
    h.close()
    return res


def against_oracle(oracle, c, host, res, limits=None, calls=None):
    """Each stream against its own oracle run over exactly the samples the device consumed (the search range changed where the device's was).
    Returns the oracle's stats per stream."""
    ros = []
    for s, rh in enumerate(res):
        o = make_oracle(oracle, c)
        if limits and calls:
            parts, pos = [], 0
            for i, k in enumerate(calls):
                if limits[i]:
                    o.l.oracle_fsk_set_freq_est_limits(o.h, *limits[i])
                got = {"bits": [], "rx_filt": [], "stats": []}
                for _ in range(k):                          # frame by frame: exactly k frames under this range
                    r = o.demod(host[s, pos:pos + o.nin()], c["fmt"])
                    assert r["nframes"] == 1
                    pos += r["consumed"]
                    for key in got:
                        got[key].append(r[key])
                parts.append(got)
            ro = {"nframes": sum(calls), "consumed": pos, **{key: np.concatenate([np.concatenate(p[key]) for p in parts]) for key in ("bits", "rx_filt", "stats")}}
        else:
            ro = o.demod(host[s, :rh["consumed"]], c["fmt"])
        _compare(ro, rh, M=c["M"])
        assert np.array_equal(rh["stats"][:, :4], ro["stats"][:, :4]), s           # f_est frame by frame
        lo_hi = slice(128, 160) if c["band"] else slice(0, 256)
        assert np.array_equal(rh["Sf"][lo_hi], oracle_Sf(oracle, o)[lo_hi]), s
        ros.append(ro["stats"])
    return ros


def frames_for(oracle, c, host):
    return min(make_oracle(oracle, c).demod(host[s], c["fmt"], want_filt=False)["nframes"] for s in range(host.shape[0])) - 1


@pytest.fixture(scope="module")
def batches(oracle):
    return {name: mixed_batch(oracle, c) for name, c in SHAPES.items()}


@pytest.mark.parametrize("name", list(SHAPES))
def test_hook_off_equals_hook_on_equals_oracle(oracle, built_lib, batches, monkeypatch, name):
    c, host = SHAPES[name], batches[name]
    F = frames_for(oracle, c, host)
    assert 10 <= F <= 13
    on = run(c, host, [F], True, monkeypatch)
    st = against_oracle(oracle, c, host, on)
    N, Q = c["Fs"] // c["Rs"] * 50, c["Fs"] // c["Rs"] // 4
    assert (st[0][2:, 0] == st[0][2, 0]).all() and (np.diff(st[1][:, 0]) != 0).any()      # stream 0 stays on its bins, stream 1 moves
    assert (st[3][:, 6] == N - Q).any() and (st[3][:, 6] == N).any()                       # stream 3 steps nin between hit frames
    same_results(on, run(c, host, [F], False, monkeypatch), "hook off")
    ragged = [3, 1, F - 6, 2]
    same_results(on, run(c, host, ragged, True, monkeypatch), "ragged calls")
    same_results(on, run(c, host, ragged, False, monkeypatch), "ragged calls, hook off")


# (est_min, est_max, f1, shift): the tones stay inside the range (checked on the oracle's f_est below); live slot sets by
# tests/test_wave_locked_paths_cpu.py's rule
RANGES = {
    "slots_01": (500, 25000, 10000, 10000),
    "slot_0": (500, 14000, 2000, 10000),
    "slot_1": (16000, 29000, 17000, 10000),
    "slots_012": (500, 45000, 10000, 28000),
    "slots_0123": (500, 60000, 20000, 35000),
}


def _range_batch(oracle, c):
    return sigutil.batch(oracle, c, [sigutil.mod_frames(oracle, c, NFRAMES + 1, 30 + s)[5 * s:] for s in range(5)])


@pytest.mark.parametrize("name", list(RANGES))
def test_search_range_set_on_the_live_handle(oracle, built_lib, monkeypatch, name):
    lo, hi, f1, shift = RANGES[name]
    c = dict(SHAPES["headline_u8"], f1=f1, shift=shift)
    host = _range_batch(oracle, c)
    F = 11
    limits = [(lo, hi)]
    on = run(c, host, [F], True, monkeypatch, limits=limits)
    st = against_oracle(oracle, c, host, on, limits=limits, calls=[F])
    top_slot = max(int(ch) for ch in name.split("_")[1])
    for s in range(5):
        # the oracle finds two tones inside the range from the third frame on, the lower near f1 and the upper in the highest slot the case names
        f = st[s][2:, :2]
        assert (f >= lo).all() and (f < hi).all() and (np.abs(f[:, 0] - f1) <= 1875).all(), (s, f)
        assert (((np.rint(f[:, 1] / 937.5).astype(int) >> 4) & 3) == top_slot).all(), (s, f)
    same_results(on, run(c, host, [F], False, monkeypatch, limits=limits), "hook off")


def test_search_range_changes_between_two_calls(oracle, built_lib, monkeypatch):
    """slots {0, 1} in the first call, {0, 1, 2} in the second, back in the third: which search runs is decided per call"""
    c = dict(SHAPES["headline_u8"], f1=10000, shift=10000)
    host = _range_batch(oracle, c)
    calls, limits = [4, 4, 3], [(500, 25000), (500, 40000), (2000, 28000)]
    on = run(c, host, calls, True, monkeypatch, limits=limits)
    against_oracle(oracle, c, host, on, limits=limits, calls=calls)
    same_results(on, run(c, host, calls, False, monkeypatch, limits=limits), "hook off")


@pytest.mark.parametrize("name", ["headline_u8", "4fsk_p8"])
def test_hit_path_exits_in_the_middle_of_a_call(oracle, built_lib, monkeypatch, name):
    """+ 300 and - 300 ppm of sample-clock offset: nin = N + Ts/4 or N - Ts/4 frames fall between runs of hit frames; one stream's tones
    move by a bin half-way. One-shot and in ragged calls against the oracle, then word for word between the hook settings."""
    c = SHAPES[name]
    long_frames = 2 * NFRAMES
    rows = []
    for s, ppm in enumerate([300.0, -300.0, 300.0, -300.0]):
        x = sigutil.mod_complex(oracle, c, np.random.default_rng(50 + s).integers(0, 2, long_frames * sigutil.frame_bits(c)).astype(np.uint8))
        # a start phase near the nin threshold, so that the slow drift (0.36 samples per frame) crosses it inside the run
        rows.append(sigutil.resample_steps(x, np.full(x.shape[0], 1.0 + ppm * 1e-6))[(6 if ppm > 0 else 17) + s:])
    rows.append(sigutil.mover(oracle, c, 60, (NFRAMES, NFRAMES)))
    host = sigutil.batch(oracle, c, rows)
    F = frames_for(oracle, c, host)
    assert 22 <= F <= 27
    on = run(c, host, [F], True, monkeypatch)
    st = against_oracle(oracle, c, host, on)
    N = c["Fs"] // c["Rs"] * 50
    stepped = [s for s in range(4) if ((st[s][:, 6] != N).any() and (st[s][2:, 6] == N).sum() >= 6)]
    assert len(stepped) >= 2, [st[s][:, 6].tolist() for s in range(4)]      # nin steps between runs of N-sample (hit) frames
    assert (np.diff(st[4][:, 0]) != 0).any()
    ragged = [5, 1, 2, F - 11, 3]
    parts = run(c, host, ragged, True, monkeypatch)
    same_results(on, parts, "ragged calls")
    same_results(on, run(c, host, [F], False, monkeypatch), "hook off")
    same_results(parts, run(c, host, ragged, False, monkeypatch), "ragged calls, hook off")
