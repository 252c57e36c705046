"""The wave kernel's peak search over live bin slots only, checked by enumeration without a GPU.

A lane of the Ndft = 256 estimator owns four Sf bins, slots b = 0 .. 3: FFT bin (lane & 15) + 16 b + 64 (lane >> 4), at index
(bin + 128) & 255 of the shifted spectrum (`own_sfi` in pirip_amd/csrc/fsk_demod_wave.hip). Per call every lane forms `in_range`, bit b
set when its slot-b index lies in [est_st, est_en); the kernel then searches slots 0 and 1 only when no lane has a bit above 1 set.
Restated here in plain Python: for every (est_st, est_en) over the 256 bins

  * the set of live slots by a closed rule on the range -- slot b is live iff the range holds an index whose FFT bin has
    (bin >> 4) & 3 == b -- equals the union over the 64 lanes of their in_range bits, and
  * the two-slot search sees every in-range bin exactly when that set is inside {0, 1}; the reference's 500 .. 25000 Hz range
    at Fs = 240 kHz (fsk_est_range: indices 128 .. 153) is such a call, so are the other ranges the GPU tests name.
"""
import numpy as np

NDFT, NLIVE = 256, 2


def own_sfi(lane, b):
    return (((lane & 15) + 16 * b + 64 * (lane >> 4)) + NDFT // 2) & (NDFT - 1)


def lane_in_range(lane, st, en):
    return sum(1 << b for b in range(4) if st <= own_sfi(lane, b) < en)


def est_range(Fs, est_min, est_max):
    """fsk_est_range (pirip_amd/csrc/fsk_plan.cpp): C integer division truncates towards zero"""
    st = max(int(est_min * NDFT / Fs) + NDFT // 2, 0)
    en = min(int(est_max * NDFT / Fs) + NDFT // 2, NDFT)
    return st, en


def live_by_rule(st, en):
    return {(((i - NDFT // 2) & (NDFT - 1)) >> 4) & 3 for i in range(st, en)}


def test_every_bin_has_one_owner_slot():
    owners = sorted(own_sfi(lane, b) for lane in range(64) for b in range(4))
    assert owners == list(range(NDFT))


def test_live_slot_set_equals_union_of_lane_flags_for_every_range():
    # the union over the 64 lanes for EVERY pair: flags[en][lane][slot] = st <= index < en
    idx = np.array([[own_sfi(lane, b) for b in range(4)] for lane in range(64)])          # [lane][slot]
    for st in range(NDFT + 1):
        en = np.arange(st, NDFT + 1)[:, None, None]
        flags = (idx[None] >= st) & (idx[None] < en)                                     # [en][lane][slot]
        union = flags.any(axis=1)                                                        # [en][slot]
        rule = np.zeros_like(union)
        for k, e in enumerate(range(st, NDFT + 1)):
            for b in live_by_rule(st, e):
                rule[k, b] = True
        assert np.array_equal(union, rule), st


def test_two_slot_search_sees_every_in_range_bin_exactly_when_the_high_slots_are_dead():
    for st in range(NDFT + 1):
        for en in range(st, NDFT + 1, 3):
            flags = [lane_in_range(lane, st, en) for lane in range(64)]
            two = not any(f >> NLIVE for f in flags)                                     # the kernel's test: __any((in_range >> 2) != 0) is false
            in_range = set(range(st, en))
            seen_by_two = {own_sfi(lane, b) for lane in range(64) for b in range(NLIVE) if flags[lane] >> b & 1}
            assert two == (live_by_rule(st, en) <= {0, 1})
            if two:
                assert seen_by_two == in_range, (st, en)
            else:
                assert seen_by_two < in_range, (st, en)


def test_ranges_the_gpu_tests_name():
    Fs = 240000
    assert est_range(Fs, 500, 25000) == (128, 154) and live_by_rule(128, 154) == {0, 1}     # the reference's range: FFT bins 0 .. 25
    assert live_by_rule(*est_range(Fs, 500, 14000)) == {0}
    assert live_by_rule(*est_range(Fs, 16000, 29000)) == {1}
    assert live_by_rule(*est_range(Fs, 500, 40000)) == {0, 1, 2} and live_by_rule(*est_range(Fs, 500, 45000)) == {0, 1, 2}
    assert live_by_rule(*est_range(Fs, 500, 60000)) == {0, 1, 2, 3}
    assert live_by_rule(*est_range(Fs, -30000, 29000)) == {0, 1, 2, 3}                      # negative frequencies: FFT bins 224 .. 255
    assert live_by_rule(*est_range(Fs, 0, 0 + 1)) == set()                                  # an empty range: nothing competes in either search
