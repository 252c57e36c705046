"""tests/txsref.py's schedules reach the queue paths tests/test_txs.py relies on (no GPU): from the model alone, every shape's schedule
has a refused send, an underrun enclosed in a burst's gap, a ring wrap and a call that starts inside a frame; and the shapes have the
filter lengths and history depths they are named for."""
import numpy as np
import pytest

import chanref
import muxref
import txsref


@pytest.mark.parametrize("name", sorted(txsref.SHAPES))
def test_schedule_reaches_every_queue_path(name):
    sh = txsref.SHAPES[name]
    plans, lens, tags, cap = txsref.shape_plans(name)
    steps = txsref.make_schedule(plans, lens, tags, sh["S"], cap)
    m = txsref.replay(steps, plans, lens, tags, None, sh["S"], cap)
    K = len(plans)
    assert m.refused.sum() >= 1 and (m.refused > 0).all()
    assert m.gap_underruns >= K                         # every channel runs dry behind a gap and sends again
    assert m.wraps >= 1
    assert m.mid_frame_starts >= 1
    assert (m.sent == [sum(l) for l in lens]).all() and not m.queued().any()
    assert (m.sent + m.underrun == m.calls * sh["S"]).all()
    tl = m.timelines()
    assert tl.shape == (K, m.calls * sh["S"])
    assert sum(1 for s in steps if s[0] == "P") == m.calls < 1500


@pytest.mark.parametrize("name", sorted(txsref.SHAPES))
def test_shapes_have_the_history_they_are_named_for(name):
    sh = txsref.SHAPES[name]
    L = chanref.filter_len(sh["tbw"]) if sh["kind"] == txsref.FIR else 2 * sh["D"] - 1
    Q = muxref.q_of(L, sh["D"])
    mFs = sh["Fs"] // sh["D"]
    Ts = mFs // sh["Rs"]
    assert sh["Fs"] % sh["D"] == 0 and mFs % sh["Rs"] == 0
    assert Q == sh["Q"] and -(-(Q - 1) // Ts) == sh["H"]
    for f1 in sh["f1"]:
        assert all(abs(f1 + m * sh["shift"]) < mFs // 2 for m in range(sh["M"]))
    assert muxref.geometry(sh["D"], L, 2) is not None and muxref.geometry(sh["D"], L, 8) is not None


def test_shapes_cover_the_cases():
    S = txsref.SHAPES
    assert {s["H"] for s in S.values()} >= {0, 1, 2, 10}
    assert {s["S"] for s in S.values()} >= {1, 3}
    assert {s["M"] for s in S.values()} == {2, 4}
    assert any(s["S"] * s["D"] * (s["Fs"] // s["D"] // s["Rs"]) > muxref.TILE for s in S.values())              # a block crosses a tile
    assert any(len(s["f1"]) == 9 and s["outputs"] is None for s in S.values())                                   # two staging groups
    assert any(s["outputs"] and s["noutputs"] > len(set(s["outputs"])) for s in S.values())                       # an empty output
    assert any(f < 0 for s in S.values() for f in s["f1"]) and any(s["pad"] for s in S.values())


def test_model_all_or_nothing_and_counters():
    m = txsref.Model(1, 4, 10)
    sy = lambda n, v=1: (np.full(n, v, np.uint8), np.full(n, txsref.FRAME, np.int8), np.arange(n))
    assert m.send([sy(7)])[0] and not m.send([sy(4)])[0] and m.refused[0] == 1 and m.queued()[0] == 7
    assert m.process()[0] == 4 and m.send([sy(7, 2)])[0] and m.wraps == 1 and m.queued()[0] == 10
    assert [int(m.process()[0]) for _ in range(4)] == [4, 4, 2, 0]
    assert m.sent[0] == 14 and m.underrun[0] == 6
    assert m.timelines()[0].tolist() == [1] * 7 + [2] * 7 + [txsref.OFF] * 6


def test_cli_policy_sends_everything_with_a_queue_of_one_burst():
    """two bursts of 10 symbols, 4 per block, a queue of 10: the second burst waits until the queue is empty, the channel underruns, and
    the run is longer than ceil(20 / 4) blocks -- an end counted in symbols alone would drop the last two"""
    plans = [[2, 2]]
    lens = [txsref.record_lens(plans[0], 0, 0, 10)]
    tags = [txsref.record_tags(plans[0], 0, 0, 10)]
    steps = txsref.cli_schedule(plans, lens, tags, 4, 10)
    m = txsref.replay(steps, plans, lens, tags, None, 4, 10)
    assert m.sent[0] == 20 and not m.queued().any() and m.calls == 6 and m.underrun[0] == 4 and m.refused[0] == 3
    # with the largest burst plus S no queue runs dry before its input ends
    steps = txsref.cli_schedule(plans, lens, tags, 4, 14)
    m = txsref.replay(steps, plans, lens, tags, None, 4, 14)
    assert m.sent[0] == 20 and m.calls == 5 and m.underrun[0] == 0
