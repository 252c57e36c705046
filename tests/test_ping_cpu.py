"""include/pirip_hip.h section N without a GPU: the host model tests/pingref.py that tests/test_ping.py holds the device to. Its burst
records are what fsk_ldpc_framer --testframes sends, and its tables reach the corners they claim."""
import numpy as np
import pytest

import pingref
import rptref
import sigutil

MODEM = {2: (50, 544), 4: (100, 272)}         # preamble and frame of the stand-in code, in symbols
GAP = 64


@pytest.mark.parametrize("M", [2, 4])
@pytest.mark.parametrize("frames", [1, 3])
@pytest.mark.parametrize("seq", [False, True])
def test_burst_records_are_the_framers_test_frames(built_lib, M, frames, seq):
    import pirip_amd
    source = 0xA7
    rec = pingref.burst_records(pirip_amd.testframe_payload(8 * pingref.KB), frames, source, seq)
    assert rec.shape == (frames + 1, 1 + pingref.KB) and rec[:, 0].tolist() == [1] + [0] * (frames - 1) + [2]
    got = sigutil.run_framer(["-m", str(M), "--packed", "--gap", "7", "-", "-"], rec.tobytes())
    want = sigutil.run_framer(["-m", str(M), "--testframes", str(frames), "--bursts", "1", "--source", hex(source), "--gap", "7"] + (["--seq"] if seq else []) +
                   ["/dev/zero", "-"])
    assert got.size == want.size > 0 and np.array_equal(got, want)
    if seq:
        assert rec[:frames, 2].tolist() == list(range(1, frames + 1))


def _want():
    import pirip_amd
    return pirip_amd.testframe_payload(8 * pingref.KB)


def test_log_model_on_hand_made_rows(built_lib):
    want = _want()
    calls = pingref.log_calls(want)
    m = pingref.run_log(calls, want)
    ev = m.ev
    assert ev["filtered"] > 0 and ev["crc_fail"] > 0 and ev["empty_calls"] >= 3
    assert frozenset({pingref.N0 - pingref.STEP, pingref.N0, pingref.N0 + pingref.STEP}) in ev["nins_in_one_call"]
    assert ev["wraps"] > 0 and ev["call_larger_than_ring"] > 0
    assert sorted({max(len(c[0]) for c in call) for call in calls})[-2:] == [65, 130] and ev["max_rows"] == 130
    assert [65 > pingref.CHUNK, 130 > 2 * pingref.CHUNK] == [True, True]
    # the first call by hand. Channel 0: row 1 is filtered, row 2 decoded with a bad CRC; the clock counts every row
    m1 = pingref.run_log(calls[:1], want)
    st, pl, info, stats = calls[0][0]
    assert m1.c["filtered"][0] >= 1 and m1.c["crc_fail"][0] >= 1
    clock = pingref.N0 + np.concatenate([[0], np.cumsum(stats[:-1, 6].astype(np.int64))])
    for e in m1.log(0):
        f = int(e["row"])
        assert st[f] & pingref.BITS and pl[f, 0] != pingref.FILT and e["t_samples"] == clock[f] and e["call"] == 0
        assert e["S"].tobytes() == stats[f, 8].tobytes() and e["N"].tobytes() == stats[f, 9].tobytes()
        assert (e["source"], e["seq"], e["status"]) == (pl[f, 0], pl[f, 1], st[f])
    assert [int(e["row"]) for e in m1.log(0)] == [f for f in range(len(st)) if st[f] & pingref.BITS and pl[f, 0] != pingref.FILT]
    # channel 2: three rows of nin N - STEP, N, N + STEP: the second row's time is N0 + (N0 - STEP)
    assert m1.samples[2] == 3 * pingref.N0 - pingref.STEP and m1.next_nin[2] == pingref.N0 + pingref.STEP
    # the ring keeps the newest entries, lost counts the others; bit errors are those of every logged row
    for c in range(3):
        assert len(m.log(c)) == min(len(m.entries[c]), pingref.LOG_ENTRIES)
        assert m.c["lost"][c] == len(m.entries[c]) - len(m.log(c)) and m.c["frames"][c] == len(m.entries[c])
        assert m.c["bit_errors"][c] == sum(int(e["ecdd"]) for e in m.entries[c])
    assert m.c["lost"][0] > 0 and m.c["bit_errors"].sum() > 0
    assert len(m.log(0, 3)) == 3 and m.log(0, 3).tobytes() == m.log(0)[-3:].tobytes()
    # some special float made it into the ring, so that "bit for bit" is looked at
    kept = np.concatenate([m.log(c) for c in range(3)])
    assert np.isin(kept["S"].view(np.uint32), pingref.SPECIAL.view(np.uint32)).any()
    # the same rows cut into other calls: the same entries but for call and row, the same counters
    m2 = pingref.run_log(pingref.recut(calls, 3), want)
    for c in range(3):
        assert pingref.same_but_call_and_row(m.log(c), m2.log(c)) and len(m.entries[c]) == len(m2.entries[c])
    assert all(np.array_equal(m.c[k], m2.c[k]) for k in m.c)
    assert any(m.log(c)["call"].tolist() != m2.log(c)["call"].tolist() for c in range(3))


@pytest.mark.parametrize("M", [2, 4])
def test_schedule_model(built_lib, M):
    pre, frame = MODEM[M]
    burst = pingref.burst_records(_want(), 3, 1, True)
    cost = rptref.burst_cost(3, pre, frame, GAP)
    sch = {s["name"]: s for s in pingref.schedules(pre, frame, GAP)}
    # staggered first calls: a channel's first burst goes out in its first call and then every period calls
    s = sch["staggered"]
    offered, m = pingref.run_schedule(s, burst)
    for t in range(4):
        sent = [n for n in range(s["calls"]) if len(offered[n][t])]
        assert sent[0] == s["first_call"][t] and all(b - a == s["period"] for a, b in zip(sent, sent[1:])) and len(sent) >= 2
        assert all(np.array_equal(offered[n][t], burst) for n in sent)
    assert not m.c["skipped"].any() and len(set(s["first_call"])) == 4
    # the cut-off: two bursts per channel although more were due
    s = sch["cutoff"]
    offered, m = pingref.run_schedule(s, burst)
    assert m.c["bursts_sent"].tolist() == [2] * 4 and m.c["frames_sent"].tolist() == [6] * 4 and not m.c["skipped"].any()
    assert all((s["calls"] - 1 - f) // s["period"] + 1 > 2 for f in s["first_call"])
    # a queue of one burst, a period shorter than a burst: due bursts are skipped, and none is retried before its next due call
    s = sch["tight"]
    assert s["queue_syms"] == cost and s["period"] * s["S"] < cost
    offered, m = pingref.run_schedule(s, burst)
    assert (m.c["skipped"] > 0).all() and (m.c["bursts_sent"] >= 2).all()
    for t in range(4):
        assert all(n % s["period"] == 0 for n in range(s["calls"]) if len(offered[n][t]))
    assert np.array_equal(m.c["bursts_sent"] + m.c["skipped"], np.full(4, (s["calls"] - 1) // s["period"] + 1))
