"""The frame-length rows of tests/nsymshapes.py on the oracle and on the restated path rules alone (no GPU): each row takes the path
its comment claims, the oracle demodulates it, and the clean input keeps away from what would make a device comparison test rounding
instead of the kernel (a timing estimate at a nin threshold, an ill-conditioned timing sum)."""
import numpy as np
import pytest

import nsymshapes as ns
import sigutil

_cache = {}


def _clean(oracle, r):
    """(buffer, transmitted bits, oracle result) of a row's clean input: computed once, shared, left unchanged"""
    if r.name not in _cache:
        buf, bits = ns.signal(oracle, sigutil, r)
        fo, _ = ns.formats(oracle, None, r)
        _cache[r.name] = (buf, bits, ns.oracle_for(oracle, r).demod(buf, fo))
    return _cache[r.name]


@pytest.mark.parametrize("r", ns.ROWS, ids=lambda r: r.name)
def test_row_takes_the_path_its_comment_claims(r):
    p = ns.path(r)
    assert p["lds_fits"] == r.lds_fits
    if not r.lds_fits:
        assert p["lds"] == 128 + 208880
        return
    assert (p["threads"], p["pre"], p["alias"], p["ffts"], p["direct"]) == (r.threads, r.pre, r.alias, r.ffts, r.direct), p
    assert (r.name in ns.DEGENERATE) == (p["ffts"] == 0)


def test_rows_cover_every_path_the_frame_length_selects():
    paths = [ns.path(r) for r in ns.DEVICE_ROWS]
    assert {p["threads"] for p in paths} == {64, 128, 256, 512}
    for nt in (64, 128, 512):
        assert {p["pre"] for p in paths if p["threads"] == nt} == {True, False}, nt
    assert {(p["alias"], p["ffts"] == 0) for p in paths} == {(True, True), (True, False), (False, True), (False, False)}
    assert {p["direct"] for p in paths} == {True, False}
    assert any(p["threads"] == 512 and p["alias"] for p in paths)
    # the staged / direct threshold from both sides, the first frame length with an FFT from both sides, the compiled length's neighbours
    assert {340, 342} <= {r.Nsym for r in ns.ROWS} and {10, 11} <= {r.Nsym for r in ns.ROWS} and {49, 51} <= {r.Nsym for r in ns.ROWS}
    # nin one step either side of N changes the FFT count at Nsym = 128, and only there among the Ts = 24 rows up to it
    r = ns.BY_NAME["ts24_s16_n128"]; d = ns.dims(r)
    assert [ns.numffts(d, d["N"] + k * d["nin_step"]) for k in (-1, 0, 1)] == [22, 23, 23]
    # excluded by construction: frame lengths that leave nin moving on a timing sum of condition 1e-6 (Nsym 1, 2 at Ts = 24; 5 at Ts = 80)
    assert not [r for r in ns.ROWS if (r.Fs // r.Rs, r.Nsym) in ((24, 1), (24, 2), (80, 5))]
    # the eye diagram: Nsym = 11 at P = 24 is the shortest frame but two that still holds all four traces per tone; Nsym = 8 holds three
    assert ns.eye_shape(ns.BY_NAME["ts24_n11"]) == (8, 48) and ns.eye_shape(ns.BY_NAME["ts24_4fsk_f32_n21"]) == (8, 16)
    assert ns.eye_shape(ns.BY_NAME["ts24_n8"]) == (6, 48) and ns.eye_shape(ns.BY_NAME["ts24_n49"]) == (8, 48)


@pytest.mark.parametrize("r", ns.DEVICE_ROWS, ids=lambda r: r.name)
def test_oracle_demodulates_the_row_and_the_clean_input_is_well_conditioned(oracle, r):
    buf, bits, ro = _clean(oracle, r)
    d = ns.dims(r)
    assert ro["nframes"] >= ns.nframes(r) and ro["bits"].shape == (ro["nframes"], d["Nbits"])
    assert np.isfinite(ro["stats"]).all() and np.isfinite(ro["rx_filt"]).all()
    nin = ro["stats"][:, 6]
    assert set(np.unique(nin)) <= {d["N"] - d["nin_step"], d["N"], d["N"] + d["nin_step"]}
    # a device comparison must not hang on the last bit of a timing estimate: away from the nin thresholds, the sum well conditioned
    t = ro["stats"][:, 4]
    assert np.abs(np.abs(t) - 0.25).min() >= 0.01, float(np.abs(np.abs(t) - 0.25).min())
    assert ro["timing_cond"].min() >= 0.005, float(ro["timing_cond"].min())
    if r.name in ns.DEGENERATE:
        # no FFT ever runs: the peak search of an all-zero spectrum finds bin 0 for every tone, equal tones never beat tone 0
        assert (ro["stats"][:, :r.M] == -r.Fs / 2).all() and not ro["bits"].any()
        return
    # the transmitted bits, from the fifth frame on (the estimator has settled; the first decision of the recording is a partial symbol)
    rx = ro["bits"][4:].ravel()
    lags = [k for k in range(0, 6 * d["Nbits"] + 1) if np.array_equal(bits[k:k + len(rx)], rx)]
    assert len(lags) == 1, lags


def test_nin_moves_in_the_row_whose_fft_count_depends_on_it(oracle):
    r = ns.BY_NAME["ts24_s16_n128"]
    d = ns.dims(r)
    nin = _clean(oracle, r)[2]["stats"][:, 6]
    consumed = np.concatenate([[d["N"]], nin[:-1]])            # (a frame consumes the nin the frame before it asked for)
    assert len({ns.numffts(d, int(n)) for n in consumed}) == 2, np.unique(consumed)
