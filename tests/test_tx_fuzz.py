"""A fixed slice of tools/fuzz_parity.py's transmit draws: 150 seeds of tx_one (code shape, M, Fs / Rs, tones, lead / gap, record plan, call
split, format, sigma), each through the framer checks of tests/test_tx_shapes.py and the modulator / noise checks against tests/txref.py.
The draw's tie filter (float64 formula only) is checked on the CPU to discard at most 10 % of the draws."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
SEEDS = range(7300000, 7300150)


def test_tie_filter_discards_at_most_a_tenth_of_the_draws():
    import fuzz_parity
    draws = [fuzz_parity.tx_draw(seed) for seed in SEEDS]
    discarded = sum(d for _, d in draws)
    print(f"{discarded} discarded for {len(draws)} kept")
    assert discarded <= 0.10 * (len(draws) + discarded)
    cfgs = [c for c, _ in draws]
    assert {(c["n"], c["k"]) for c in cfgs} == {(136, 104), (200, 104), (600, 296), (512, 256)}
    assert {c["M"] for c in cfgs} == {2, 4} and {c["fmt"] for c in cfgs} == {"cf32", "u8"} and any(c["Ts"] < 8 for c in cfgs)
    assert any(c["sigma"] > 0 for c in cfgs) and any(c["sigma"] == 0 for c in cfgs) and any(c["Fs"] == 1 << 24 for c in cfgs)


@pytest.mark.gpu
def test_one_hundred_and_fifty_random_transmit_draws_have_nothing_failed(oracle, built_lib):
    import fuzz_parity
    import pirip_amd
    res = [(seed, fuzz_parity.tx_one(seed, oracle, pirip_amd)) for seed in SEEDS]
    fails = [(seed, r[1]) for seed, r in res if r[0] != "exact"]
    assert not fails, fails[:3]
    info = [r[1] for _, r in res]
    assert {i["shape"] for i in info} == {(136, 104), (200, 104), (600, 296), (512, 256)}
    assert {i["M"] for i in info} == {2, 4} and {i["fmt"] for i in info} == {"cf32", "u8"} and any(i["Ts"] < 8 for i in info)
