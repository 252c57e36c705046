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
import ctypes as C

import numpy as np
import pytest

import sigutil
from parity import _compare, _oracle_field_Sf

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


def _nbits(c):
    return 50 * (1 if c["M"] == 2 else 2)


def _bin_hz(c):
    return c["Fs"] / 256.0


def _mod(oracle, c, nframes, seed, tone_bins=0):
    bits = np.random.default_rng(seed).integers(0, 2, nframes * _nbits(c)).astype(np.uint8)
    return sigutil.mod_complex(oracle, c, bits, f1=c["f1"] + int(round(tone_bins * _bin_hz(c))))


def _conv(oracle, c, x):
    if c["fmt"] == CF32:
        return np.ascontiguousarray(x.astype(np.float32) * np.float32(0.37))
    return oracle.quantise_cu8(x)


def _resample(x, step):
    """x read at positions 0, step[0], step[0] + step[1], ... (linear interpolation)"""
    t = np.concatenate([[0.0], np.cumsum(step)[:-1]])
    t = t[t < x.shape[0] - 2]
    i0 = np.floor(t).astype(int); fr = (t - i0)[:, None].astype(np.float32)
    return ((1 - fr) * x[i0] + fr * x[i0 + 1]).astype(np.float32)


def clock_offset(oracle, c, seed, ppm):
    x = _mod(oracle, c, NFRAMES + 2, seed)
    return _resample(x, np.full(x.shape[0], 1.0 + ppm * 1e-6))


def mover(oracle, c, seed):
    """tones one FFT bin up half-way through"""
    h = (NFRAMES + 1) // 2
    return np.concatenate([_mod(oracle, c, h, seed), _mod(oracle, c, NFRAMES + 1 - h, seed + 1, tone_bins=1)])[3:]


def batch(oracle, c, rows):
    rows = [_conv(oracle, c, r) for r in rows]
    n = min(r.shape[0] for r in rows)
    return np.stack([r[:n] for r in rows])


def mixed_batch(oracle, c):
    return batch(oracle, c, [_mod(oracle, c, NFRAMES + 1, 1), mover(oracle, c, 10), _mod(oracle, c, NFRAMES + 1, 2, tone_bins=-1)[7:],
                             clock_offset(oracle, c, 20, 2500.0), _mod(oracle, c, NFRAMES + 1, 3, tone_bins=2)[17:]])


def _oracle(oracle, c, est=None):
    lo, hi = est or (c["est_min"], c["est_max"])
    return oracle.OracleFsk(c["Fs"], c["Rs"], c["M"], P=c["P"], est_min=lo, est_max=hi)


def _oracle_Sf(oracle, o):
    return np.ctypeslib.as_array(C.cast(_oracle_field_Sf(oracle, o), C.POINTER(C.c_float)), shape=(256,)).copy()


def run(c, host, calls, cache, monkeypatch, limits=None):
    """All B streams through pirip_hip_demod_batch, calls[i] frames in call i; every stream's unconsumed samples are presented again
    from its own position. limits[i] (when given and not None): pirip_hip_set_freq_est_limits before call i. Returns per-stream results."""
    import torch
    import pirip_amd
    monkeypatch.setenv("PIRIP_FRAME_CACHE", "1" if cache else "0")
    B, L = host.shape[0], host.shape[1]
    bps = host.dtype.itemsize * 2
    h = pirip_amd.HipDemod(c["Fs"], c["Rs"], c["M"], P=c["P"], est_min=c["est_min"], est_max=c["est_max"], in_format=c["fmt"], nstreams=B)
    if c["band"]:
        h.set_estimator_band_only(True)
    assert h.kernel() == "wave" and ("band-only" in h.kernel_name()) == c["band"]
    st = torch.cuda.current_stream().cuda_stream
    nb, nf = h.Nbits, c["M"] * 50
    pos = np.zeros(B, dtype=np.int64)
    out = {k: [[] for _ in range(B)] for k in ("bits", "rx_filt", "stats")}
    for i, k in enumerate(calls):
        if limits and limits[i]:
            assert h.set_freq_est_limits(*limits[i]) == 0
        n = int(L - pos.max())
        dev = torch.from_numpy(np.stack([host[s, pos[s]:pos[s] + n] for s in range(B)])).cuda()
        bits = torch.zeros((B, k, nb), dtype=torch.uint8, device="cuda")
        filt = torch.zeros((B, k, nf), dtype=torch.float32, device="cuda")
        stats = torch.zeros((B, k, pirip_amd.STATS_PER_FRAME), dtype=torch.float32, device="cuda")
        nfr = torch.zeros(B, dtype=torch.int32, device="cuda"); cons = torch.zeros(B, dtype=torch.int64, device="cuda")
        h.demod_batch(dev.data_ptr(), n * bps, n, bits.data_ptr(), k * nb, filt.data_ptr(), k * nf, stats.data_ptr(),
                      k * pirip_amd.STATS_PER_FRAME, nfr.data_ptr(), cons.data_ptr(), k, st)
        torch.cuda.synchronize()
        assert (nfr.cpu().numpy() == k).all(), (nfr, k, i)
        for s in range(B):
            out["bits"][s].append(bits[s].cpu().numpy()); out["rx_filt"][s].append(filt[s].cpu().numpy()); out["stats"][s].append(stats[s].cpu().numpy())
        pos += cons.cpu().numpy()
    res = []
    for s in range(B):
        sc = np.zeros(8, dtype=np.float32)
        assert h.L.pirip_hip_get_scalars(h.h, s, sc.ctypes.data) == 0
        res.append({"nframes": sum(calls), "consumed": int(pos[s]), "Sf": h.get_Sf(s), "scalars": sc,
                    "state": np.frombuffer(h.stream_state(s), dtype=np.uint32),
                    **{k: np.concatenate(out[k][s]) for k in out}})
    h.close()
    return res


def same_words(a, b, what):
    for s, (x, y) in enumerate(zip(a, b)):
        assert x["consumed"] == y["consumed"], (what, s)
        for k in ("bits", "rx_filt", "stats", "Sf", "scalars", "state"):
            assert np.array_equal(x[k].view(np.uint8 if x[k].dtype == np.uint8 else np.uint32),
                                  y[k].view(np.uint8 if y[k].dtype == np.uint8 else np.uint32)), (what, s, k)


def against_oracle(oracle, c, host, res, limits=None, calls=None):
    """Each stream against its own oracle run over exactly the samples the device consumed (the search range changed where the device's was).
    Returns the oracle's stats per stream."""
    ros = []
    for s, rh in enumerate(res):
        o = _oracle(oracle, c)
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
        assert np.array_equal(rh["Sf"][lo_hi], _oracle_Sf(oracle, o)[lo_hi]), s
        ros.append(ro["stats"])
    return ros


def frames_for(oracle, c, host):
    return min(_oracle(oracle, c).demod(host[s], c["fmt"], want_filt=False)["nframes"] for s in range(host.shape[0])) - 1


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
    same_words(on, run(c, host, [F], False, monkeypatch), "hook off")
    ragged = [3, 1, F - 6, 2]
    same_words(on, run(c, host, ragged, True, monkeypatch), "ragged calls")
    same_words(on, run(c, host, ragged, False, monkeypatch), "ragged calls, hook off")


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
    return batch(oracle, c, [_mod(oracle, c, NFRAMES + 1, 30 + s)[5 * s:] for s in range(5)])


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
    same_words(on, run(c, host, [F], False, monkeypatch, limits=limits), "hook off")


def test_search_range_changes_between_two_calls(oracle, built_lib, monkeypatch):
    """slots {0, 1} in the first call, {0, 1, 2} in the second, back in the third: which search runs is decided per call"""
    c = dict(SHAPES["headline_u8"], f1=10000, shift=10000)
    host = _range_batch(oracle, c)
    calls, limits = [4, 4, 3], [(500, 25000), (500, 40000), (2000, 28000)]
    on = run(c, host, calls, True, monkeypatch, limits=limits)
    against_oracle(oracle, c, host, on, limits=limits, calls=calls)
    same_words(on, run(c, host, calls, False, monkeypatch, limits=limits), "hook off")


@pytest.mark.parametrize("name", ["headline_u8", "4fsk_p8"])
def test_hit_path_exits_in_the_middle_of_a_call(oracle, built_lib, monkeypatch, name):
    """+ 300 and - 300 ppm of sample-clock offset: nin = N + Ts/4 or N - Ts/4 frames fall between runs of hit frames; one stream's tones
    move by a bin half-way. One-shot and in ragged calls against the oracle, then word for word between the hook settings."""
    c = SHAPES[name]
    long_frames = 2 * NFRAMES
    rows = []
    for s, ppm in enumerate([300.0, -300.0, 300.0, -300.0]):
        x = sigutil.mod_complex(oracle, c, np.random.default_rng(50 + s).integers(0, 2, long_frames * _nbits(c)).astype(np.uint8))
        # a start phase near the nin threshold, so that the slow drift (0.36 samples per frame) crosses it inside the run
        rows.append(_resample(x, np.full(x.shape[0], 1.0 + ppm * 1e-6))[(6 if ppm > 0 else 17) + s:])
    rows.append(np.concatenate([_mod(oracle, c, NFRAMES, 60), _mod(oracle, c, NFRAMES, 61, tone_bins=1)])[3:])
    host = batch(oracle, c, rows)
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
    same_words(on, parts, "ragged calls")
    same_words(on, run(c, host, [F], False, monkeypatch), "hook off")
    same_words(parts, run(c, host, ragged, False, monkeypatch), "ragged calls, hook off")
