"""On the oracle alone, no GPU: the inputs of tests/test_block_demod.py (tests/blockshapes.py) reach the paths they claim -- every nin value
at known start offsets of the 240-offset sweep and under a sustained clock offset, no timing estimate near enough to the +-0.25 threshold for
two float32 evaluation orders to fall on different sides of it, and as many frames per stream as each device test states."""
import numpy as np
import pytest

import blockshapes as bs
from parity import TIMING_TOL

MARGIN = 5 * TIMING_TOL          # 2.5e-4 symbols


@pytest.mark.parametrize("M", [2, 4])
@pytest.mark.parametrize("fmt", ["u8d", "csdr"])
def test_offset_sweep_takes_every_nin_and_stays_clear_of_the_threshold(oracle, fmt, M):
    res = bs.sweep_oracle(oracle, M, fmt)
    assert len(res) == bs.TS and all(r["nframes"] == bs.SWEEP_FRAMES for r in res)
    nin = np.array([r["stats"][:, 6] for r in res])
    dist = np.abs(np.abs(np.array([r["stats"][:, 4] for r in res], dtype=np.float64)) - 0.25)
    print(f"offset sweep {fmt} M = {M}: smallest distance of |norm_rx_timing| to 0.25 over {dist.size} frames: {dist.min():.3e} "
          f"(stream {int(dist.min(axis=1).argmin())}); nin values {sorted(int(v) for v in set(nin.reshape(-1)))}")
    assert set(nin.reshape(-1).astype(int)) == set(bs.NINS)
    assert dist.min() > MARGIN, dist.min()
    # the offsets the table names: a short frame, a long frame, neither
    assert (nin[bs.OFF_SHORT] == bs.N - bs.Q).any() and not (nin[bs.OFF_SHORT] == bs.N + bs.Q).any()
    assert (nin[bs.OFF_LONG] == bs.N + bs.Q).any() and not (nin[bs.OFF_LONG] == bs.N - bs.Q).any()
    assert (nin[bs.OFF_EVEN] == bs.N).all()
    # ... within the canary test's three frames, so that its three streams consume three different sample counts
    cons3 = {int(bs.N + nin[o][:2].sum()) for o in (bs.OFF_SHORT, bs.OFF_LONG, bs.OFF_EVEN)}
    assert len(cons3) == 3, cons3


@pytest.mark.parametrize("M", [2, 4])
@pytest.mark.parametrize("fmt", ["u8d", "csdr"])
def test_clock_offset_takes_short_and_long_frames(oracle, fmt, M):
    for ppm, want in ((bs.CLOCK_PPM, bs.N - bs.Q), (-bs.CLOCK_PPM, bs.N + bs.Q)):
        r = bs.oracle_of(oracle, M).demod(bs.clock_stream(oracle, M, fmt, ppm), bs.fmt_of(oracle, fmt))
        nin = r["stats"][:, 6]
        print(f"{fmt} M = {M} {ppm * 1e6:+.0f} ppm: {int((nin == want).sum())} of {r['nframes']} frames with nin = {want}")
        assert bs.clock_counts_ok(r, ppm)
        assert np.abs(np.abs(r["stats"][:, 4].astype(np.float64)) - 0.25).min() > MARGIN


@pytest.mark.parametrize("name", sorted(bs.ROWS))
def test_every_row_has_the_frames_its_device_tests_ask_for(oracle, name):
    M, fmt, mask, off = bs.ROWS[name]
    f = bs.fmt_of(oracle, fmt)
    for u8 in bs.row_streams(oracle, name):
        assert bs.oracle_of(oracle, M, mask).demod(u8, f, want_filt=False)["nframes"] >= 30
    if name in bs.PACKED_ROWS:
        for u8 in bs.packed_streams(oracle, name):
            assert bs.oracle_of(oracle, M, mask).demod(u8, f, want_filt=False)["nframes"] >= 10
    if name in bs.SCALAR_ROWS:
        n = bs.oracle_of(oracle, M, mask).demod(bs.scalar_stream(oracle, name), f, want_filt=False)["nframes"]
        assert n > bs.SCALAR_MAX_FRAMES >= 5          # the max_frames arm stops with samples left
    if name in bs.PAIR_ROWS:
        for u8 in bs.pair_streams(oracle, name):
            assert bs.oracle_of(oracle, M, mask).demod(u8, f, want_filt=False)["nframes"] >= 10
    if name == bs.CAPTURE_ROW:
        assert bs.oracle_of(oracle, M, mask).demod(bs.capture_stream(oracle), f, want_filt=False)["nframes"] == 25


def test_burst_mode_and_estimator_limit_inputs(oracle):
    """The burst-mode stream leaves nin = N without burst mode and keeps |timing| above 0.25 with it; the narrowed estimator range moves a
    tone estimate."""
    M, fmt = 2, "csdr"
    u8 = bs.sweep_base(oracle, M, fmt)[bs.OFF_SHORT:]
    free = bs.oracle_of(oracle, M).demod(u8, bs.fmt_of(oracle, fmt))
    ob = bs.oracle_of(oracle, M); ob.enable_burst_mode()
    burst = ob.demod(u8, bs.fmt_of(oracle, fmt))
    assert (free["stats"][:, 6] != bs.N).any()
    assert burst["nframes"] >= 5 and (burst["stats"][:, 6] == bs.N).all() and (np.abs(burst["stats"][:, 4]) > 0.25).any()
    u8 = bs.limits_stream(oracle)
    wide = bs.oracle_of(oracle, M).demod(u8, bs.fmt_of(oracle, fmt))
    narrow = bs.oracle_of(oracle, M, est_min=bs.LIMITS[0], est_max=bs.LIMITS[1]).demod(u8, bs.fmt_of(oracle, fmt))
    assert wide["nframes"] == narrow["nframes"] >= 5 and not np.array_equal(wide["stats"][:, :2], narrow["stats"][:, :2])
