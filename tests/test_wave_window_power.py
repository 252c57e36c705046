"""The wave kernel's packed window powers and the ppm smoother's constant divide on the device ("packed window powers").

Inputs: tests/wpshapes.py -- 6 streams (a full workgroup of four and a partial one) of 12 frames, noise-free at start offsets 0, 5, 11,
17, 23 and 20 samples (floor(rx_timing) negative, zero and positive: both select branches), at 9 dB, and 40 frames at + 300 / - 300 ppm
(nin steps in both directions, timing falls and rises: the ppm smoother's dividend has both signs).
tests/test_wave_window_power_cpu.py shows on the oracle alone that no frame's timing is within 5e-4 symbols of a nin threshold or the
wrap, so the nin sequence is demanded exactly of every stream.

On every instance the predicate wave_packed_power_instance enables (the `fsk_demod -p 24` instance and its band-only twin, which must
also agree with each other word for word):
  * bits equal the oracle's (noise-free: exactly; 9 dB: tests/parity.py's near-tie rule), f_est frame by frame and Sf are bit-identical,
    nin is exact, timing / rx_filt / SNR / signal and noise power within parity._compare's bounds. ppm has no bound of its own there: it
    is a convex combination of 1e6 d / Nsym with d the difference of two timing estimates, each within TIMING_TOL of the oracle's, so
    it is held to 2 TIMING_TOL 1e6 / Nsym = 2 ppm;
  * one call equals ragged calls word for word; PIRIP_FRAME_CACHE=0 -- the hook that also sends appm through the IEEE divide --
    equals the default word for word (the ppm column in particular); packed bit output equals the unpacked bits.
On instances outside the predicate every output word is what the library computed before the change: the sha256 values below were
taken from a build of the parent commit (13c6425) on an MI355X over exactly these batches.
"""
import hashlib

import numpy as np
import pytest

import wpshapes as wp
from demodrun import make_handle, make_oracle, run_calls, same_results
from parity import TIMING_TOL, _compare, oracle_Sf

pytestmark = pytest.mark.gpu

# sha256 over consumed, bits, rx_filt, stats, Sf, scalars and stream state of all six streams (digest()), parent build
PARENT_SHA256 = {
    ("csdr_u8", "clean"): "18c2b8671cc94b9a587929a7700c7ddbb2681f8c4e84ec6f1e8fc8fc21267c63",
    ("csdr_u8", "drifting"): "77e9e4d14035779370382e9e55428cc771a450a34e6aec92876db5176e4b44bd",
    ("4fsk_p8", "clean"): "c0e04b707e27d8490db02593bdca488f5c609d974d4cdf1db7f42e500a9eb243",
}


@pytest.fixture(scope="module")
def batches(oracle):
    shapes = {**wp.PACKED, **wp.UNCHANGED}
    return {(name, case): make(oracle, shapes[name]) for name in shapes for case, make in wp.CASES.items()
            if name in wp.PACKED or (name, case) in PARENT_SHA256}


def run(c, host, calls, cache, monkeypatch):
    """run_calls on a wave handle created with the frame cache on or off"""
    monkeypatch.setenv("PIRIP_FRAME_CACHE", "1" if cache else "0")
    h = make_handle(c, host.shape[0])
    assert h.kernel() == "wave"
    res = run_calls(h, host, calls)
    h.close()
    return res


def frames_of(case):
    return wp.PPM_FRAMES if case == "drifting" else wp.CLEAN_FRAMES


def digest(res):
    h = hashlib.sha256()
    for r in res:
        h.update(np.int64(r["consumed"]).tobytes())
        for k in ("bits", "rx_filt", "stats", "Sf", "scalars", "state"):
            h.update(np.ascontiguousarray(r[k]).tobytes())
        # (the values above were taken when the state was read into 14 words, the last of them never written by the library: the
        #  structure's 13 words are followed by that zero word here so that they stand)
        assert r["state"].nbytes == 52
        h.update(bytes(4))
    return h.hexdigest()


def check_against_oracle(oracle, c, host, res, noisy):
    for s, rh in enumerate(res):
        o = make_oracle(oracle, c)
        ro = o.demod(host[s, :rh["consumed"]], c["fmt"])
        flips = _compare(ro, rh, allow_near_tie_flips=noisy, M=c["M"])       # exact: frames, consumed, f_est, nin, (noise-free) bits
        band = slice(128, 160) if c["band"] else slice(0, 256)               # (band-only: Sf is kept for FFT bins 0 .. 31)
        assert np.array_equal(rh["Sf"][band], oracle_Sf(oracle, o)[band]), s
        dp = np.abs(rh["stats"][:, 7].astype(np.float64) - ro["stats"][:, 7].astype(np.float64))
        print(f"stream {s}: timing max diff {np.abs(rh['stats'][:, 4] - ro['stats'][:, 4]).max():.2e} symbols, ppm max diff {dp.max():.2e}, "
              f"near-tie bit flips {flips}")
        assert (dp <= 2.0 * TIMING_TOL * 1e6 / wp.NSYM).all(), (s, dp.max())


@pytest.mark.parametrize("case", list(wp.CASES))
@pytest.mark.parametrize("name", list(wp.PACKED))
def test_packed_instance_against_the_oracle_and_itself(oracle, built_lib, batches, monkeypatch, name, case):
    c, host = wp.PACKED[name], batches[name, case]
    F = frames_of(case)
    one = run(c, host, [F], True, monkeypatch)
    check_against_oracle(oracle, c, host, one, noisy=case == "noisy")
    N, Q = c["Fs"] // c["Rs"] * wp.NSYM, c["Fs"] // c["Rs"] // 4
    if case == "drifting":
        nin = [r["stats"][:, 6] for r in one]
        assert any((n == N + Q).any() for n in nin) and any((n == N - Q).any() for n in nin)
        d = np.concatenate([np.diff(r["stats"][:, 4]) for r in one])
        assert (d < 0).sum() >= 20 and (d > 0).sum() >= 20                   # dividends of both signs reach the divide
    ragged = [3, 1, F - 6, 2]
    same_results(one, run(c, host, ragged, True, monkeypatch), "ragged calls")
    hook = run(c, host, [F], False, monkeypatch)
    same_results(one, hook, "frame cache off, IEEE divide")
    for s in range(len(one)):
        assert np.array_equal(one[s]["stats"][:, 7].view(np.uint32), hook[s]["stats"][:, 7].view(np.uint32)), s
    same_results(hook, run(c, host, ragged, False, monkeypatch), "ragged calls, frame cache off")


def test_band_only_twin_computes_the_full_instances_words(oracle, built_lib, batches, monkeypatch):
    """both are packed-power instances: every output word but Sf outside the band is the same"""
    for case in ("clean", "drifting"):
        full = run(wp.PACKED["headline_u8"], batches["headline_u8", case], [frames_of(case)], True, monkeypatch)
        band = run(wp.PACKED["band_only"], batches["band_only", case], [frames_of(case)], True, monkeypatch)
        same_results(full, band, case, keys=("bits", "rx_filt", "stats"))


@pytest.mark.parametrize("name", list(wp.PACKED))
def test_packed_bit_output_equals_unpacked(oracle, built_lib, batches, name):
    import torch
    c, host = wp.PACKED[name], batches[name, "clean"]
    B, n, F = host.shape[0], host.shape[1], wp.CLEAN_FRAMES
    dev = torch.from_numpy(host).cuda()
    out = []
    for packed in (False, True):
        h = make_handle(c, B)
        h.set_bit_packing(packed)
        fb = (h.Nbits + 7) // 8 if packed else h.Nbits
        bits = torch.zeros((B, F, fb), dtype=torch.uint8, device="cuda")
        nfr = torch.zeros(B, dtype=torch.int32, device="cuda"); cons = torch.zeros(B, dtype=torch.int64, device="cuda")
        h.demod_batch(dev.data_ptr(), n * 2, n, bits.data_ptr(), F * fb, 0, 0, 0, 0, nfr.data_ptr(), cons.data_ptr(), F,
                      torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert (nfr.cpu().numpy() == F).all()
        out.append(bits.cpu().numpy())
        h.close()
    assert np.array_equal(np.unpackbits(out[1], axis=2)[:, :, :out[0].shape[2]], out[0])


@pytest.mark.parametrize("name, case", list(PARENT_SHA256))
def test_instances_outside_the_predicate_compute_the_parents_words(oracle, built_lib, batches, monkeypatch, name, case):
    c, host = wp.UNCHANGED[name], batches[name, case]
    assert digest(run(c, host, [frames_of(case)], True, monkeypatch)) == PARENT_SHA256[name, case]
