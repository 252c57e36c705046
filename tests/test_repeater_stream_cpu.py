"""tests/rptref.py, the host model of the streaming repeater (include/pirip_hip.h section M), pinned on the CPU before
tests/test_repeater_stream.py relies on it: with nothing in the way its offered records are frame_repeater's own output (the fixture of
tests/test_tx_repeater_cpu.py), however the records are cut into calls, and its schedules reach every corner of the intake and the offer."""
import numpy as np

import rptref
import txref

PRE, FRAME = 50, 544                          # the stand-in code with 2-FSK: preamble and frame in symbols
EMITTING = 43                                 # of the selected fixture cases, those whose output holds a burst


def _cat(offered, t, kb=rptref.KB):
    parts = [o[t] for o in offered]
    return np.concatenate(parts) if parts else np.zeros((0, 1 + kb), np.uint8)


def test_fixture_selection():
    cases = rptref.fixture_streams()
    assert len(cases) >= 60
    assert all(c["kb"] == 32 and c["status"].size <= 60 for c in cases)
    assert sum(1 for c in cases if c["out"].shape[0] > 0) == EMITTING
    assert max(b.shape[0] - 1 for c in cases for b in rptref._bursts(c["out"])) <= 12


def test_offered_records_equal_the_replay_in_one_call_and_in_pieces():
    cases = rptref.fixture_streams()
    by_name = {s["name"]: s for s in rptref.schedules(PRE, FRAME)}
    for name in ("fixture_one_call", "fixture_pieces"):
        s = by_name[name]
        assert s["filter"] is None and s["holdoff"] == 0 and s["route"] == list(range(len(cases)))
        offered, m = rptref.run(s, PRE, FRAME)
        for t, c in enumerate(cases):
            want = txref.repeater_replay(c["status"], c["payload"], s["source"])
            fix = c["out"].copy()
            fix[fix[:, 0] != 2, 1] = s["source"]                     # the program's own output with this schedule's source byte
            assert np.array_equal(want, fix), c["name"]
            got = _cat(offered, t)
            assert got.shape == want.shape and np.array_equal(got, want), (name, c["name"])
        cnt = m.counters()
        assert not cnt["dropped"].any() and not cnt["pending"].any() and not cnt["unrouted"].any() and not cnt["filtered"].any()
        assert int((cnt["bursts_out"] > 0).sum()) == EMITTING
    pieces = by_name["fixture_pieces"]["calls"]
    sizes = {len(st) for call in pieces for st, _ in call}
    assert 0 in sizes and 1 in sizes and max(sizes) > 1              # empty pieces, pieces of one record, larger ones


def test_cutting_changes_nothing_at_any_cut():
    """one channel of the fixture, every way of cutting it in two"""
    c = max(rptref.fixture_streams(), key=lambda c: c["out"].shape[0])
    want = txref.repeater_replay(c["status"], c["payload"], 7)
    n = c["status"].size
    for cut in range(n + 1):
        calls = [[(c["status"][:cut], c["payload"][:cut])], [(c["status"][cut:], c["payload"][cut:])]]
        s = dict(calls=calls, route=[0], ntx=1, source=7, filter=None, holdoff=0, max_burst=100, pending=64, queue_syms=10 ** 6, S=3)
        offered, _ = rptref.run(s, PRE, FRAME)
        assert np.array_equal(_cat(offered, 0), want), cut


def test_the_schedules_reach_every_corner():
    ev, cnt = {}, {}
    for s in rptref.schedules(PRE, FRAME):
        _, m = rptref.run(s, PRE, FRAME)
        ev[s["name"]], cnt[s["name"]] = m.ev, m.counters()
        assert s["pending"] >= s["max_burst"] + 1
        assert s["queue_syms"] >= rptref.burst_cost(s["max_burst"], PRE, FRAME, rptref.GAP_SYMS)
    c1, c3 = "corners_holdoff1", "corners_holdoff3"
    for name in ("corners_holdoff0", c1, c3):
        e, c = ev[name], cnt[name]
        assert e["filtered_first"] >= 1                              # a filtered first frame: no burst starts
        assert e["filtered_middle"] >= 1                             # a filtered middle frame
        assert c["filtered"].sum() == e["filtered_first"] + e["filtered_middle"]
        assert e["max_open_calls"] > 3                               # a burst open across more than 3 calls
        assert 2 in e["blocked"]                                     # head-of-line blocking on a full queue that clears two calls later
        assert e["drop_while_waiting"] >= 1 and c["dropped"].sum() >= 1     # a burst dropped on a full ring while an earlier one waits
        assert c["unrouted"].sum() >= 1                              # an unrouted channel
        assert e["cut"] >= 1                                         # a burst cut at max_burst
        assert e["wraps"] >= 1                                       # a ring wrap
        assert c["pending"].sum() >= 1                               # and something still waits at the end
    assert 1 in ev[c1]["waits"] and 3 in ev[c3]["waits"]             # a hold-off wait of 1 and of 3 calls
    assert ev["fixture_one_call"]["max_bursts_per_offer"] >= 2       # two bursts offered in one call
    assert ev["fixture_pieces"]["max_open_calls"] > 3
    assert 2 in ev["fixture_permuted"]["waits"]


def test_a_filtered_first_frame_starts_no_burst_and_a_filtered_middle_frame_is_left_out():
    rng = np.random.default_rng(3)
    B, E = rptref.BITS | rptref.SYNC, 0
    st, pl = rptref._frames(rng, [B, B, E, B, B, B, E], {0: 9, 4: 9})
    s = dict(calls=[[(st, pl)]], route=[0], ntx=1, source=9, filter=9, holdoff=0, max_burst=100, pending=16, queue_syms=10 ** 6, S=3)
    offered, m = rptref.run(s, PRE, FRAME)
    got = offered[0][0]
    # the first burst starts at its second frame; the second loses its middle frame
    assert got[:, 0].tolist() == [1, 2, 1, 0, 2]
    assert np.array_equal(got[0, 2:], pl[1, 1:]) and np.array_equal(got[2, 2:], pl[3, 1:]) and np.array_equal(got[3, 2:], pl[5, 1:])
    assert (got[[0, 2, 3], 1] == 9).all() and m.counters()["filtered"].tolist() == [2]
