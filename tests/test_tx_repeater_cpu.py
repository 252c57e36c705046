"""The repeater's record conversion without a device: tests/txref.py's replay of tx/frame_repeater.c against what the reference's own
program wrote (tests/golden/repeater_cases.npz, made by oracle/build_ref_repeater.sh + oracle/make_repeater_golden.py), what the
fixture covers, and the two entry points' exports and no-device refusals. tests/test_tx_repeater.py runs the kernel over the same cases."""
import ctypes as C
import os

import numpy as np

import txref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYNC, BITS = txref.RX_SYNC, txref.RX_BITS


def _burst_lengths(out):
    """frames per burst of a Tx record stream 1 0 ... 0 2"""
    ends = np.flatnonzero(out[:, 0] == 2)
    return np.diff(np.concatenate([[-1], ends])) - 1


def test_replay_equals_the_recorded_output_of_frame_repeater_byte_for_byte():
    cases = txref.repeater_cases()
    assert len(cases) > 300 and {c["kb"] for c in cases} == {13, 32, 37} and len({c["source"] for c in cases}) >= 3
    for c in cases:
        got = txref.repeater_replay(c["status"], c["payload"], c["source"])
        assert got.shape == c["out"].shape and np.array_equal(got, c["out"]), c["name"]


def test_fixture_drives_every_branch_of_the_state_machine():
    cases = txref.repeater_cases()
    seen, lengths = set(), []
    hit = dict(start_refused_with_bit_errors=0, append_and_flush=0, flush_plain=0, sync_only_in_burst=0, errored_frame_taken=0, open_at_end=0,
               end_then_open=0)
    for c in cases:
        st, out = c["status"], c["out"]
        seen |= set(int(v) for v in st)
        lengths += list(_burst_lengths(out))
        assert (out[out[:, 0] != 2][:, 1] == c["source"]).all() and not out[out[:, 0] == 2][:, 1:].any(), c["name"]
        rec, closed = False, 0
        for v in st:
            if not rec:
                hit["start_refused_with_bit_errors"] += v == 0xE
                hit["end_then_open"] += v == 6 and closed > 0
                rec = v == 6
            else:
                hit["append_and_flush"] += bool(v & BITS) and not (v & SYNC)
                hit["flush_plain"] += not (v & BITS) and not (v & SYNC)
                hit["sync_only_in_burst"] += not (v & BITS) and bool(v & SYNC)
                hit["errored_frame_taken"] += v == 0xE
                rec = bool(v & SYNC)
                closed += not rec
        hit["open_at_end"] += rec
    assert seen >= {0, 2, 4, 6, 8, 0xA, 0xC, 0xE, 1}, seen
    assert all(n > 0 for n in hit.values()), hit
    lengths = np.array(lengths)
    assert lengths.min() == 1 and lengths.max() == txref.REPEAT_MAX_FRAMES          # no burst above 100: the program asserts there
    assert np.count_nonzero(lengths == 100) >= 3 and np.count_nonzero((lengths > 20) & (lengths < 100)) >= 10
    print(f"{len(cases)} cases, {sum(c['status'].size for c in cases)} records, {lengths.size} bursts, branch counts {hit}")


def test_an_open_burst_at_the_end_of_input_writes_nothing():
    cases = {(c["name"], c["kb"]): c for c in txref.repeater_cases()}
    for kb in (13, 32, 37):
        assert cases[("burst open at the end of input: nothing written", kb)]["out"].shape == (0, 1 + kb)
        assert cases[("a single 6 left open", kb)]["out"].shape == (0, 1 + kb)
        c = cases[("a burst, then one left open", kb)]
        assert list(c["out"][:, 0]) == [1, 0, 2]                                    # the first burst only
        assert np.array_equal(c["out"][:2, 2:], c["payload"][:2, 1:])
    # and in the replay, for every case: cutting the records behind the last one without SYNC changes nothing
    for c in cases.values():
        st = c["status"]
        drop = np.flatnonzero((st & SYNC) == 0)
        last = int(drop[-1]) + 1 if drop.size else 0
        assert np.array_equal(txref.repeater_replay(st[:last], c["payload"][:last], c["source"]), c["out"]), c["name"]


def test_the_library_exports_the_record_conversion_and_refuses_bad_arguments_without_a_device(built_lib):
    hdr = open(os.path.join(ROOT, "include", "pirip_hip.h")).read()
    for name in ("pirip_hip_tx_repeat_records", "pirip_hip_tx_repeat_max_records"):
        assert name + "(" in hdr and hasattr(built_lib, name), name
    assert "#define PIRIP_TX_REPEAT_MAX_FRAMES 100" in hdr
    mx, rr = built_lib.pirip_hip_tx_repeat_max_records, built_lib.pirip_hip_tx_repeat_records
    assert mx(None, 10) == 0 and mx(None, -1) == 0
    buf = (C.c_uint8 * 64)()
    p = C.cast(buf, C.c_void_p)
    assert rr(None, p, 64, p, 64, None, 1, 7, p, 64, 1, None, None) == -1           # PIRIP_ERR_BAD_ARG: no handle
