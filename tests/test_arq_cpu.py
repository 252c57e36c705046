"""include/pirip_hip.h section S without a GPU: the host model tests/arqref.py that tests/test_arq.py holds the device to. Its tables and
sessions reach every counter and every branch of the rules; under seeded loss both directions deliver every segment once and in order --
the preconditions of the GPU test, shown on the model alone --; a one-way link breaks the session after exactly max_tries transmissions;
the sequence byte wraps with segments held across the wrap. Also: an ACK's bytes by hand, pirip_amd/csrc/arq_device.hpp against the
model's functions in a stand-alone program (built once more with the host sanitizers), the structures' layouts, and the library's refusal
of NULL handles."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import arqref as ar
import pktref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACKLEN = 20


def _finished(pair, ta, tb):
    """both directions delivered every segment exactly once, in order, and every segment is acknowledged"""
    for nd, peer, sent in ((pair.a, pair.b, ta), (pair.b, pair.a, tb)):
        for t, s in enumerate(nd.sess):
            assert [b for _, b in peer.sess[t].out] == sent[t], t
            assert [int(e["seq"]) for e, _ in peer.sess[t].out] == list(range(len(sent[t])))
            assert s.snd_una == s.sub_nxt == len(sent[t]) and not s.broken
    return pair.a.counters(), pair.b.counters()


@pytest.fixture(scope="module")
def runs():
    """every session of the GPU test on the model alone, once: name -> (pair or node, ...)"""
    out = {}
    for seed in ar.LOSS_SEEDS:
        for fec in (None, (4, 50)):
            pair, ta, tb, K = ar.loss_pair(seed, fec)
            ar.run_pair(pair, ta, tb, K)
            out["loss", seed, fec] = (pair, ta, tb)
    pair, ta, tb, K = ar.broken_pair()
    ar.run_pair(pair, ta, tb, K)
    out["broken"] = (pair, ta, tb)
    pair, ta, tb, K = ar.wrap_pair()
    ar.run_pair(pair, ta, tb, K, per_call=16)
    out["wrap"] = (pair, ta, tb)
    pair, ta, tb, K = ar.tight_pair()
    ar.run_pair(pair, ta, tb, K)
    out["tight"] = (pair, ta, tb)
    chans = ar.rule_streams(ACKLEN)
    out["rules"] = ar.run_rules(pktref.cut(chans, 1, 7))[0]
    out["overrun"] = ar.run_rules(pktref.one_call(chans), ring_entries=2)[0]
    return out


def test_sizes_and_an_ack_by_hand():
    assert (pktref.cap(ar.KB), pktref.max_packet(ar.KB, 5), ar.ack_len(ar.KB, 5)) == (24, 116, ACKLEN)
    assert ar.ack_len(16, 1) == 6 and ar.ack_len(18, 1) == 6 and ar.ack_len(19, 1) == 7      # cap 8, 10, 11; max_packet 4, 6, 7
    # base 2, segments 3 and 6 held: bits 0 and 3; filler byte q = (31 * 2 + 73 q + 0x5A) & 0xFF = (152 + 73 q) & 0xFF
    want = bytes([0xA0, 0x02, 0x09, 0x00, 0x00, 0x00,
                  0x4E, 0x97, 0xE0, 0x29, 0x72, 0xBB, 0x04, 0x4D, 0x96, 0xDF, 0x28, 0x71, 0xBA, 0x03])
    assert ar.ack_bytes(2, 0b1001, 20) == want and len(want) == 20
    assert ar.ack_bytes(258, 1 << 31, 6) == bytes([0xA0, 0x02, 0, 0, 0, 0x80])
    assert ar.data_bytes(300, b"ab") == bytes([0xD0, 44, 0x61, 0x62])
    # an ACK is one fragment filled up to its CRC-32: no zero padding in the frame
    rec = pktref.segment(want, 1, 2, 0, ar.KB, 5)
    assert rec.shape[0] == 2 and rec[0, 6] == 24


def test_the_sequence_byte_by_hand():
    W = 4
    assert ar.data_class(7, 7, W) == (ar.IN_ORDER, 0) and ar.data_class(8, 7, W) == (ar.AHEAD, 1) and ar.data_class(10, 7, W) == (ar.AHEAD, 3)
    assert ar.data_class(11, 7, W)[0] == ar.OUTSIDE and ar.data_class(6, 7, W)[0] == ar.OLD and ar.data_class(3, 7, W)[0] == ar.OLD
    assert ar.data_class(2, 7, W)[0] == ar.OUTSIDE
    assert ar.data_class(1, 254 + 256, W) == (ar.AHEAD, 3) and ar.data_class(254, 257, W)[0] == ar.OLD     # across the wrap
    assert ar.data_class(255, 0, W)[0] == ar.OUTSIDE and ar.data_class(255, 1, W)[0] == ar.OUTSIDE and ar.data_class(0, 1, W)[0] == ar.OLD
    assert ar.data_class(254, 258, 32)[0] == ar.OLD and ar.data_class(225, 257, 32)[0] == ar.OLD and ar.data_class(224, 257, 32)[0] == ar.OUTSIDE
    assert ar.ack_advance(5, 3, 7) == 2 and ar.ack_advance(7, 3, 7) == 4 and ar.ack_advance(8, 3, 7) == -1 and ar.ack_advance(2, 3, 7) == -1
    assert ar.ack_advance(1, 255, 259) == 2 and ar.ack_advance(3, 3, 3) == 0 and ar.ack_advance(4, 3, 3) == -1


def test_the_tables_and_sessions_reach_every_counter_and_branch(runs):
    ev = dict.fromkeys(ar.EVENTS, 0)
    counters = dict.fromkeys(ar.SENDER_COUNTERS + ar.RECEIVER_COUNTERS, 0)
    nodes = [runs["rules"], runs["overrun"]] + [nd for k, v in runs.items() if k not in ("rules", "overrun") for nd in (v[0].a, v[0].b)]
    # a bad length, a full ring and a broken session at submit
    pair = runs["broken"][0]
    assert pair.a.submit([[b"x"]] * 4) == [0] * 4
    full = ar.node(1, 2, ar.LINK_S, ar.LINK_RTO)
    assert full.submit([[b"x"] * 9, [b""], [bytes(115)], [bytes(114), b"y"]]) == [8, 0, 0, 2]
    for nd in nodes + [full]:
        for k, v in nd.ev.items():
            ev[k] += v
        for k, v in nd.counters().items():
            counters[k] += int(v.sum())
    assert all(v > 0 for v in ev.values()), [k for k, v in ev.items() if not v]
    assert all(v > 0 for v in counters.values()), [k for k, v in counters.items() if not v]
    # channel 0 of the tables by hand
    c = runs["rules"].counters()
    assert [int(c[k][0]) for k in ("delivered", "duplicate", "outside", "stale", "alien", "stranger", "malformed", "acked")] == [14, 4, 3, 2, 3, 2, 2, 4]
    s = runs["rules"].sess[0]
    assert s.state() == dict(sub_nxt=4, snd_nxt=4, snd_una=4, rcv_nxt=14, held=0, ack_pending=s.ack_pending)
    ent, data = s.delivered()
    assert ent["seq"].tolist() == [10, 11, 12, 13] and int(c["lost"][0]) == 10 and len(set(ent["call"].tolist())) == 1
    assert runs["rules"].sess[2].c["delivered"] == 3 and runs["rules"].sess[2].c["alien"] == 3       # peer -1: whoever answers
    assert runs["rules"].sess[1].rcv_nxt == 280 and runs["rules"].ev["held_across_wrap"] + runs["wrap"][0].b.ev["held_across_wrap"] > 0
    assert runs["overrun"].counters()["overrun"][1] > 0 and not runs["rules"].counters()["overrun"].any()


@pytest.mark.parametrize("how", ["one_call", "between_fragments", "seed2"])
def test_the_same_rows_cut_into_other_calls_give_the_same_receiver(runs, how):
    chans = ar.rule_streams(ACKLEN)
    calls = {"one_call": pktref.one_call, "between_fragments": pktref.between_fragments, "seed2": lambda c: pktref.cut(c, 2, 9)}[how](chans)
    nd, ref = ar.run_rules(calls)[0], runs["rules"]
    for k in ar.RECEIVER_COUNTERS + ("acked",):
        assert np.array_equal(nd.counters()[k], ref.counters()[k]), k
    for a, b in zip(nd.sess, ref.sess):
        assert {k: v for k, v in a.state().items() if k != "ack_pending"} == {k: v for k, v in b.state().items() if k != "ack_pending"}
        (ea, ba), (eb, bb) = a.delivered(), b.delivered()
        assert ba == bb and ea["seq"].tolist() == eb["seq"].tolist() and ea["length"].tolist() == eb["length"].tolist()
    assert nd.sess[1].delivered()[0]["call"].tolist() != ref.sess[1].delivered()[0]["call"].tolist() or how == "between_fragments"


@pytest.mark.parametrize("fec", [None, (4, 50)], ids=["plain", "fec"])
@pytest.mark.parametrize("seed", ar.LOSS_SEEDS)
def test_under_seeded_loss_every_segment_arrives_once_and_in_order(runs, seed, fec):
    pair, ta, tb = runs["loss", seed, fec]
    a, b = _finished(pair, ta, tb)
    lost = sum(pair.loss.lost(d, k, c, 0, 0) for d in (0, 1) for k in range(100) for c in range(4))
    assert 0.2 < lost / 800 < 0.4                                        # about 30 % of the bursts
    for k in ("retransmitted", "duplicate", "deferred", "acks_sent"):
        assert a[k].sum() + b[k].sum() > 0, k
    assert a["sent"].tolist() == [ar.LOSS_SEGMENTS] * 4 and a["acked"].tolist() == [ar.LOSS_SEGMENTS] * 4 and not a["waiting"].any()
    assert not a["inflight"].any() and not a["lost"].any() and not a["overrun"].any()


def test_a_full_pending_ring_defers_what_was_staged(runs):
    pair, ta, tb = runs["tight"]
    a, b = _finished(pair, ta, tb)
    assert a["deferred"].min() > 0 and a["retransmitted"].min() > 0 and b["duplicate"].min() > 0 and not a["refused"].any()
    assert all(pair.a.ev[k] > 0 for k in ("commit_untaken_ack", "commit_untaken_again", "commit_untaken_new"))


def test_a_one_way_link_breaks_the_session_after_max_tries_transmissions(runs):
    pair, ta, tb = runs["broken"]
    a, b = pair.a.counters(), pair.b.counters()
    assert a["broken"].tolist() == [1] * 4 and b["broken"].tolist() == [1] * 4
    # every segment in flight was sent max_tries times, no more; nothing of A's arrived, everything of B's did, unacknowledged
    assert (a["sent"] + a["retransmitted"]).tolist() == [3 * ar.BROKEN_TRIES] * 4 and a["sent"].tolist() == [3] * 4
    assert all(s.tries[:3] == [ar.BROKEN_TRIES] * 3 for s in pair.a.sess)
    assert not b["delivered"].any() and a["delivered"].tolist() == [3] * 4 and not b["acked"].any() and a["acks_sent"].min() > 0
    assert a["refused"].tolist() == [1] * 4                              # the submit after the break (the test above made it)
    # the break falls on the call at which the last transmission is overdue
    solo = ar.node(1, 2, ar.LINK_S, 5, max_tries=2, nchan=1)
    solo.submit([[b"z"]])
    empty = [(np.zeros(0, np.uint8), np.zeros((0, ar.KB), np.uint8))]
    when = []
    for k in range(14):
        solo.call(empty)
        when.append((solo.sess[0].c["sent"] + solo.sess[0].c["retransmitted"], solo.sess[0].broken))
    assert when[0] == (1, 0) and when[4] == (1, 0) and when[5] == (2, 0) and when[9] == (2, 0) and when[10] == (2, 1) and when[13] == (2, 1)


def test_300_one_byte_segments_wrap_the_sequence_byte(runs):
    pair, ta, tb = runs["wrap"]
    _finished(pair, ta, tb)
    b = pair.b
    assert b.sess[0].rcv_nxt == 300 and b.ev["seq_wraps"] == 1 and b.ev["held_across_wrap"] > 0 and b.ev["successors"] > 0
    assert [x for _, x in b.sess[0].out] == [bytes([i & 0xFF]) for i in range(300)]
    assert pair.a.counters()["retransmitted"][0] > 0 and pair.k == ar.WRAP_CALLS <= 300


# ---------------------------------------------------------------- arq_device.hpp on the host

def _build(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", os.path.join(ROOT, "pirip_amd", "csrc")] + flags +
                   ["-o", exe, os.path.join(ROOT, "tests", "cprog", "arq_seq_check.cpp")], check=True)
    return exe


def _model_lines():
    out = []
    for W in range(1, 33):
        for rcv in list(range(41)) + list(range(768, 1024)):
            out.append("D %d %d %s" % (W, rcv, "".join(str(ar.data_class(seq, rcv, W)[0]) for seq in range(256))))
    for fl in range(33):
        for una in range(512, 768):
            adv = (ar.ack_advance(base, una, una + fl) for base in range(256))
            out.append("A %d %d %s" % (fl, una, "".join("-" if a < 0 else chr(48 + a) for a in adv)))
    for base, bitmap, n in ((0, 0, 6), (2, 1, 20), (255, 0xFFFFFFFF, 20), (7, 0x80000001, 116), (200, 0x00A0D000, 7)):
        out.append("K %d %d %d %s %d %d" % (base, bitmap, n, ar.ack_bytes(base, bitmap, n).hex(), base, bitmap))
    for cap, mp in ((24, 116), (24, 20), (8, 4), (10, 6), (11, 40), (248, 24796)):
        out.append("L %d %d %d" % (cap, mp, max(6, min(cap - 4, mp))))
    return out


def test_arq_device_hpp_is_the_models_arithmetic_also_under_the_host_sanitizers(tmp_path):
    want = _model_lines()
    for name, flags in (("arq_seq_check", []), ("arq_seq_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        r = subprocess.run([_build(tmp_path, name, flags)], capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", (name, r.returncode, r.stderr[-2000:])
        got = r.stdout.splitlines()
        assert len(got) == len(want) and got == want, name
    assert ar.ack_len(ar.KB, 5) == 20 and want[-6] == "L 24 116 20"


# ---------------------------------------------------------------- the binding and the library, without a device

def test_structures_have_the_headers_layout(tmp_path):
    """pirip_arq_config / pirip_arq_entry / pirip_arq_info: the ctypes twins and the numpy dtypes against what gcc makes of the header"""
    import pirip_amd
    from pirip_amd import binding
    twins = {"pirip_arq_config": binding.ArqConfig, "pirip_arq_entry": binding.ArqEntry, "pirip_arq_info": binding.ArqInfo}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pirip_hip.h"', "int main(void) {"]
    for name, T in twins.items():
        lines.append(f'    printf("S {name} %zu\\n", sizeof({name}));')
        lines += [f'    printf("F {name} {f} %zu %zu\\n", offsetof({name}, {f}), sizeof((({name} *)0)->{f}));' for f, *_ in T._fields_]
    lines += ["    return 0;", "}"]
    (tmp_path / "l.c").write_text("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "l"), str(tmp_path / "l.c")], check=True)
    size, fields = {}, {n: [] for n in twins}
    for ln in subprocess.run([str(tmp_path / "l")], check=True, capture_output=True, text=True).stdout.split("\n"):
        w = ln.split()
        if w and w[0] == "S":
            size[w[1]] = int(w[2])
        elif w:
            fields[w[1]].append((w[2], int(w[3]), int(w[4])))
    for name, T in twins.items():
        assert C.sizeof(T) == size[name]
        assert [(n, getattr(T, n).offset, getattr(T, n).size) for n, *_ in T._fields_] == fields[name]
    for dt in (np.dtype(pirip_amd.ARQ_ENTRY_DTYPE), ar.ENTRY):
        assert dt.itemsize == size["pirip_arq_entry"] == 16
        assert [(n, dt.fields[n][1], dt.fields[n][0].itemsize) for n in dt.names] == fields["pirip_arq_entry"]
    # the header's field lists are the twins' (a field added to the header alone would pass the offsets above)
    src = open(os.path.join(ROOT, "include", "pirip_hip.h")).read()
    for name, T in twins.items():
        body = re.sub(r"/\*.*?\*/", " ", src.split("struct %s {" % name)[1].split("};")[0], flags=re.S)
        names = [d.strip().split()[-1] for decl in body.split(";") if decl.strip() for d in decl.split(",")]
        assert names == [n for n, *_ in T._fields_], (name, names)
    assert pirip_amd.HipArq.SENDER_COUNTERS == ar.SENDER_COUNTERS and pirip_amd.HipArq.RECEIVER_COUNTERS == ar.RECEIVER_COUNTERS


def test_the_library_refuses_null_handles_without_a_device(built_lib):
    import pirip_amd
    from pirip_amd import binding
    BAD_ARG = -1
    out = C.c_void_p(0x1234)
    cfg = binding.ArqConfig(4, 8, 8, 8, 64)
    peers = (C.c_int * 4)(2, 2, 2, 2)
    assert built_lib.pirip_hip_arq_create(None, C.byref(cfg), peers, C.byref(out)) == BAD_ARG and out.value is None
    assert built_lib.pirip_hip_arq_create(None, C.byref(cfg), peers, None) == BAD_ARG
    for name, args in (("pirip_hip_arq_destroy", ()), ("pirip_hip_arq_get_info", (None,)), ("pirip_hip_arq_reset", (None,)),
                       ("pirip_hip_arq_submit", (None, 0, 0, None, 0, None, None, None)),
                       ("pirip_hip_arq_push_records", (None, 0, None, 0, None, 0, None, 0, None)), ("pirip_hip_arq_process", (None, 0, None)),
                       ("pirip_hip_arq_push", (None, 0, None, 0, None)), ("pirip_hip_arq_get_counters", (None,) * 19),
                       ("pirip_hip_arq_get_delivered", (0, None, None, 0, None)), ("pirip_hip_arq_get_state", (0,) + (None,) * 6)):
        assert getattr(built_lib, name)(None, *args) == BAD_ARG, name
    assert pirip_amd.HipArq._c == "pirip_hip_arq" and issubclass(pirip_amd.HipArq, binding._Handle)
    assert "HipArq" not in vars(binding)                                 # a module of its own, as HipPacket and HipDiversity are
