"""include/pirip_hip.h section S: ARQ sessions over the packet link (pirip_hip_arq_*, pirip_amd.HipArq).

Every comparison is exact: the protocol is integer arithmetic. State, counters, offered records, rings and delivered bytes come from the
host model tests/arqref.py, whose tables and sessions tests/test_arq_cpu.py shows to reach every branch and to deliver everything under
the seeded loss scripts used here. On the records path two handles run back to back, each fed the records the other offered in the call
before, minus the script; over the modem two terminals of tests/muxshapes.py's LOOP run against each other with a hole wiped into one
side's output."""
import numpy as np
import pytest

import arqref as ar
import muxshapes as ms
import pktfecref
import pktref
import sigutil
from test_packet import BAD_ARG, CANARY, CAP, FRAME, KB, PRE, UNSUPPORTED, _rng_bytes
from test_ping import LOOP_GAP, _shape_rx, _tx_side

pytestmark = pytest.mark.gpu

FEC = (4, 50)
assert (PRE, FRAME, LOOP_GAP) == (ar.PRE, ar.FRAME, ar.GAP)


# ---------------------------------------------------------------- a model node's twin on the device, records path

class _Dev:
    """HipArq over HipPacket / HipPacketFec(tx, txs) with the configuration of the model node nd; the handles it borrows live with it"""

    def __init__(self, nd, fec=None):
        import torch
        import pirip_amd
        s0, lk = nd.sess[0], nd.link
        self.nd = nd
        self.tx, self.mux, self.block, self.txs = _tx_side(2, lk.queue_syms, S=lk.S)
        assert (self.tx.preamble_syms, self.tx.frame_syms, self.tx.data_bytes) == (PRE, FRAME, KB)
        args = dict(tx=self.tx, txs=self.txs, nrx=nd.nchan, source=lk.src, filter=nd.rasm.filt, address=nd.rasm.address, max_frags=nd.max_frags,
                    pending=nd.pending, ring_entries=nd.ring_entries)
        self.pkt = pirip_amd.HipPacket(**args) if fec is None else pirip_amd.HipPacketFec(max_parity=fec[0], parity_pct=fec[1], **args)
        self.arq = pirip_amd.HipArq(self.pkt, [None if s.peer < 0 else s.peer for s in nd.sess], window=s0.W, rto=s0.rto, max_tries=s0.max_tries,
                                    queue_entries=s0.Q, out_entries=s0.E)
        assert (self.arq.nchan, self.arq.max_payload, self.arq.acklen) == (nd.nchan, nd.max_payload, nd.acklen)
        self.blk = self.block * 2
        self.out = torch.full((self.blk + 64,), CANARY, dtype=torch.uint8, device="cuda")
        self.rt = sigutil.hip_runtime()
        self.p_rec, self.stride, self.p_n = self.pkt.offered()
        self.off = torch.zeros((nd.nchan, nd.pending, 1 + KB), dtype=torch.uint8, device="cuda")
        self.cnt = torch.zeros(nd.nchan, dtype=torch.int32, device="cuda")
        self.keep = []

    def push(self, rows):
        """one call on rows[c] = (status, payload); slots behind a channel's count hold a DATA segment that would be delivered, were it read"""
        import torch
        n = len(rows)
        canary = pktref.segment(ar.data_bytes(0, b"canary"), 2, 0xFF, 99, KB, 1)[0, 1:]
        w = max([len(r[0]) for r in rows] + [1])
        st = np.full((n, w), pktref.SYNC | pktref.BITS, np.uint8)
        pl = np.tile(canary, (n, w, 1))
        nc = np.zeros(n, np.int32)
        for c, (a, b) in enumerate(rows):
            st[c, :len(a)], pl[c, :len(a)], nc[c] = a, b, len(a)
        d = [torch.from_numpy(x).cuda() for x in (st, pl, nc)]
        self.keep = [d] + self.keep[:2]
        self.arq.push_records(d[0], d[1], out=self.out.data_ptr() + 32, out_stride=self.blk, ncalls=d[2])

    def offered(self):
        """the records of the last call, per channel (synchronises)"""
        import torch
        sigutil.d2d(self.rt, self.off.data_ptr(), self.p_rec, self.nd.nchan * self.stride)
        sigutil.d2d(self.rt, self.cnt.data_ptr(), self.p_n, 4 * self.nd.nchan)
        torch.cuda.synchronize()
        off, cnt = self.off.cpu().numpy(), self.cnt.cpu().numpy()
        return [off[t, :cnt[t]].copy() for t in range(self.nd.nchan)]

    def check(self, states=True, rings=True, but_call=False):
        import torch
        nd = self.nd
        if states:
            for c, want in enumerate(nd.states()):
                assert self.arq.state(c) == want, (c, self.arq.state(c), want)
        if not rings:
            return None
        got = self.arq.counters()
        for k, v in nd.counters().items():
            assert np.array_equal(got[k], v), (k, got[k], v)
        for c, s in enumerate(nd.sess):
            ent, data = self.arq.delivered(c)
            want, wdata = s.delivered()
            assert ent.dtype == ar.ENTRY and data == wdata, c
            names = [n for n in ar.ENTRY.names if not (but_call and n == "call")]
            assert ent.shape == want.shape and all(ent[n].tobytes() == want[n].tobytes() for n in names), (c, ent, want)
        pk = self.pkt.counters()
        for k, v in list(nd.rasm.counters().items()) + list(nd.link.counters().items()):
            if k in pk:
                assert np.array_equal(pk[k], v), (k, pk[k], v)
        torch.cuda.synchronize()
        assert (self.out[:32] == CANARY).all() and (self.out[32 + self.blk:] == CANARY).all()
        return got


def _run_pair_on_device(pair, ta, tb, ncalls, fec=None, per_call=2, every=1):
    """arqref.run_pair with the two handles in step: after every call the offered records and get_state equal the model's, and the
    device's own records, minus the loss script, are the other side's next rows"""
    A, B = _Dev(pair.a, fec), _Dev(pair.b, fec)
    pos = [[0] * 4, [0] * 4]
    rows = pair.rows()
    for k in range(ncalls):
        for side, (dev, tr) in enumerate(((A, ta), (B, tb))):
            give = [tr[t][pos[side][t]:pos[side][t] + per_call] for t in range(4)]
            taken = dev.nd.submit(give)
            if any(give):
                got = dev.arq.submit(give)
                assert got.cpu().tolist() == taken, (k, side)
            pos[side] = [p + n for p, n in zip(pos[side], taken)]
        A.push(rows[0])
        B.push(rows[1])
        want = pair.call()
        off = [A.offered(), B.offered()]
        for side in (ar.AB, ar.BA):
            assert len(off[side]) == len(want[side]) and all(np.array_equal(g, w) for g, w in zip(off[side], want[side])), (k, side)
        if k % every == 0 or k == ncalls - 1:
            A.check(rings=False)
            B.check(rings=False)
        rows = (ar.rows_of_offered(off[ar.BA], pair.loss, ar.BA, k), ar.rows_of_offered(off[ar.AB], pair.loss, ar.AB, k))
    return A, B, A.check(), B.check()


# ---------------------------------------------------------------- 1. the receive rules

def test_receive_rules_equal_the_model_however_the_rows_are_cut(built_lib):
    """crafted section R rows through push_records on one handle whose channel 0 has four segments in flight: DATA in and out of order,
    duplicates held and old, outside, ACKs fresh and stale, alien, stranger, malformed; on a packet ring of two entries, an overrun"""
    chans = ar.rule_streams(ar.ack_len(KB, pktref.MAX_FRAGS))
    cuts = [pktref.cut(chans, 1, 7), pktref.between_fragments(chans), pktref.one_call(chans)]
    seen = []
    for i, calls in enumerate(cuts):
        nd = ar.rules_node()
        dev = _Dev(nd)
        segs = ar.rules_segments()
        assert dev.arq.submit(segs).cpu().tolist() == nd.submit(segs) == [ar.RULES_SUBMIT, 0, 0, 0]
        for rows in calls:
            dev.push(rows)
            nd.call(rows)
        got = dev.check()
        seen.append((got, [dev.arq.delivered(c) for c in range(4)], [dev.arq.state(c) for c in range(4)]))
        if i == 0:
            assert all(got[k][0] > 0 for k in ("sent", "acked", "delivered", "duplicate", "outside", "stale", "alien", "stranger", "malformed", "lost"))
            assert got["delivered"].tolist() == [14, 280, 3, 0] and got["acks_sent"][0] > 0 and not got["overrun"].any()
            ent, data = dev.arq.delivered(1, 2)
            assert ent["seq"].tolist() == [278, 279] and data == dev.arq.delivered(1)[1][-2:] and len(dev.arq.delivered(1, 0)[0]) == 0
            # reset forgets everything, the packet handle's counters too
            dev.arq.reset()
            assert not any(v.any() for v in dev.arq.counters().values()) and not any(v.any() for v in dev.pkt.counters().values())
            assert dev.arq.state(0) == dict.fromkeys(ar.STATE, 0) and len(dev.arq.delivered(0)[0]) == 0
    # the same rows cut into other calls: only `call` differs on the receiving side
    for got, rings, states in seen[1:]:
        for k in ar.RECEIVER_COUNTERS + ("acked",):
            assert np.array_equal(got[k], seen[0][0][k]), k
        for c in range(4):
            (ea, ba), (eb, bb) = rings[c], seen[0][1][c]
            assert ba == bb and ea["seq"].tolist() == eb["seq"].tolist() and ea["length"].tolist() == eb["length"].tolist(), c
            assert {k: v for k, v in states[c].items() if k != "ack_pending"} == {k: v for k, v in seen[0][2][c].items() if k != "ack_pending"}
    assert seen[2][1][1][0]["call"].tolist() != seen[0][1][1][0]["call"].tolist()
    # a packet ring of two entries under one call of all rows: what was overwritten unseen is counted
    nd = ar.rules_node(ring_entries=2)
    dev = _Dev(nd)
    segs = ar.rules_segments()
    dev.arq.submit(segs)
    nd.submit(segs)
    for rows in pktref.cut(chans, 3, 4):
        dev.push(rows)
        nd.call(rows)
    got = dev.check()
    assert got["overrun"][0] > 0 and got["overrun"][1] > 0 and got["overrun"][3] == 0


# ---------------------------------------------------------------- 2. two handles back to back

@pytest.mark.parametrize("fec", [None, FEC], ids=["plain", "fec"])
@pytest.mark.parametrize("seed", ar.LOSS_SEEDS)
def test_two_handles_back_to_back_under_seeded_loss(built_lib, seed, fec):
    pair, ta, tb, K = ar.loss_pair(seed, fec)
    A, B, a, b = _run_pair_on_device(pair, ta, tb, K, fec)
    for k in ("retransmitted", "duplicate", "deferred", "acks_sent"):
        assert a[k].sum() + b[k].sum() > 0, k
    assert not a["broken"].any() and not b["broken"].any() and not a["inflight"].any() and not b["waiting"].any()
    for c in range(4):
        assert B.arq.delivered(c)[1] == ta[c] and A.arq.delivered(c)[1] == tb[c], c
        assert B.arq.delivered(c)[0]["seq"].tolist() == list(range(ar.LOSS_SEGMENTS))


def test_a_full_pending_ring_defers_what_was_staged(built_lib):
    pair, ta, tb, K = ar.tight_pair()
    A, B, a, b = _run_pair_on_device(pair, ta, tb, K)
    assert a["deferred"].min() > 0 and a["retransmitted"].min() > 0 and b["duplicate"].min() > 0
    assert all(B.arq.delivered(c)[1] == ta[c] for c in range(4))


# ---------------------------------------------------------------- 3. the sequence byte wraps

def test_300_one_byte_segments_wrap_the_sequence_byte(built_lib):
    """W = 8; a call transmits a whole window of one-frame bursts and an ACK (arqref.WRAP_S symbols), so the session ends within 250 calls"""
    pair, ta, tb, K = ar.wrap_pair()
    A, B, a, b = _run_pair_on_device(pair, ta, tb, K, per_call=16, every=10)
    ent, data = B.arq.delivered(0)
    assert data == [bytes([i & 0xFF]) for i in range(300)] and ent["seq"].tolist() == list(range(300))
    assert a["acked"][0] == 300 and a["retransmitted"][0] > 0 and not a["broken"].any() and pair.b.ev["held_across_wrap"] > 0
    assert B.arq.state(0)["rcv_nxt"] == 300 and A.arq.state(0)["snd_una"] == 300


# ---------------------------------------------------------------- 4. broken

def test_a_one_way_link_breaks_the_session(built_lib):
    pair, ta, tb, K = ar.broken_pair()
    A, B, a, b = _run_pair_on_device(pair, ta, tb, K)
    assert a["broken"].tolist() == [1] * 4 and (a["sent"] + a["retransmitted"]).tolist() == [3 * ar.BROKEN_TRIES] * 4
    assert not b["delivered"].any() and a["delivered"].tolist() == [3] * 4
    # submit is refused afterwards, and a broken session still acknowledges
    assert A.arq.submit([[b"x"]] * 4).cpu().tolist() == pair.a.submit([[b"x"]] * 4) == [0] * 4
    assert A.arq.counters()["refused"].tolist() == [1] * 4 and A.check() is not None


# ---------------------------------------------------------------- 5. over the modem (tests/muxshapes.py's LOOP)

class _Node:
    """HipArq over HipPacket / HipPacketFec(rx=HipRx(chan=...), tx, txs) of the LOOP shapes, as tests/test_packet.py's _Node builds them"""

    def __init__(self, source, peer, max_frags, fec, W, rto):
        import pirip_amd
        from test_mux import _rx_handles
        lp = ms.LOOP
        self.mbf = max_frags + (pktfecref.r_of(max_frags, *fec) if fec else 0)
        self.tx, self.mux, self.block, self.txs = _tx_side(lp["M"], PRE + self.mbf * FRAME + LOOP_GAP)
        self.dem, self.ld, self.ch = _rx_handles()
        self.rx = pirip_amd.HipRx(self.dem, ldpc=self.ld, chan=self.ch, block=self.block)
        args = dict(rx=self.rx, tx=self.tx, txs=self.txs, source=source, filter=source, address=source, max_frags=max_frags, ring_entries=8)
        self.pkt = pirip_amd.HipPacketFec(max_parity=fec[0], parity_pct=fec[1], **args) if fec else pirip_amd.HipPacket(**args)
        self.arq = pirip_amd.HipArq(self.pkt, peer, window=W, rto=rto, max_tries=8, queue_entries=4, out_entries=8)
        assert self.pkt.nchan == 4 and self.pkt.nrx == 4 and self.arq.max_payload == max_frags * CAP - 6


@pytest.mark.parametrize("fec", [None, FEC], ids=["plain", "fec"])
def test_two_terminals_over_the_modem_with_a_hole_in_a_data_burst(built_lib, fec, record_property):
    """A (address 1) and B (address 2), each on the other's previous block, max_frags 3, W = 2. Every DATA packet fills its last fragment
    (tests/test_packet.py's PADDING note): segments of 24 k - 6 bytes. 544 symbols of A's output are overwritten with 128 in the middle of
    its first DATA bursts: on the plain handle those packets are lost and sent again.
    Counters of one run on the MI355X are in DESIGN.md 4.19."""
    import torch
    mf, W = 3, 2
    r = lambda k: pktfecref.r_of(k, *fec) if fec else 0
    calls = lambda frames: -(-(PRE + frames * FRAME + LOOP_GAP) // 100)
    data_calls, ack_calls = calls(mf + r(mf)), calls(1 + r(1))
    rto = data_calls + ack_calls + 8
    A, B = _Node(1, 2, mf, fec, W, rto), _Node(2, 1, mf, fec, W, rto)
    mp = A.arq.max_payload
    assert mp == 66 and rto == (33 if fec is None else 50)
    sent = [[_rng_bytes(10 * c + j, n) for j, n in enumerate((mp, 42))] for c in range(4)]
    back = [[_rng_bytes(100 + c, 18)] for c in range(4)]
    K = 2 + 3 * data_calls + rto + 2 * ack_calls + 10
    blk = A.block * 2
    spb = blk // 100                                                 # bytes of a symbol in a block of 100 symbols
    g0 = (2 + (PRE + A.mbf * FRAME) // 200) * blk + 37 * spb         # the middle of the first DATA bursts, sent from call 2 on
    g1 = g0 + FRAME * spb
    silence = torch.full((blk,), 128, dtype=torch.uint8, device="cuda")
    a_out = torch.zeros((K, blk), dtype=torch.uint8, device="cuda")
    b_out = torch.zeros((K, blk), dtype=torch.uint8, device="cuda")
    for k in range(K):
        if k == 2:                                                   # 200 symbols of silence lie in front (tests/muxshapes.py)
            ta, tb = A.arq.submit(sent), B.arq.submit(back)
        A.arq.push(b_out[k - 1] if k else silence, blk, a_out[k], blk)
        lo, hi = max(g0, k * blk) - k * blk, min(g1, (k + 1) * blk) - k * blk
        if lo < hi:
            a_out[k, lo:hi] = 128
        B.arq.push(a_out[k - 1] if k else silence, blk, b_out[k], blk)
    torch.cuda.synchronize()
    assert ta.cpu().tolist() == [2] * 4 and tb.cpu().tolist() == [1] * 4
    a, b = A.arq.counters(), B.arq.counters()
    for name, v in (("a", a), ("b", b), ("a_pkt", A.pkt.counters()), ("b_pkt", B.pkt.counters())):
        record_property(name, {k: x.tolist() for k, x in v.items()})
        print(name, {k: x.tolist() for k, x in v.items()})
    if fec:
        fa, fb = A.pkt.fec_counters(), B.pkt.fec_counters()
        record_property("b_fec", {k: x.tolist() for k, x in fb.items()})
        print("a_fec", {k: x.tolist() for k, x in fa.items()}, "b_fec", {k: x.tolist() for k, x in fb.items()})
    for c in range(4):
        ent, data = B.arq.delivered(c)
        assert data == sent[c] and ent["seq"].tolist() == [0, 1], c
        ent, data = A.arq.delivered(c)
        assert data == back[c] and ent["seq"].tolist() == [0], c
    assert not a["broken"].any() and not b["broken"].any()
    assert b["delivered"].tolist() == [2] * 4 and a["delivered"].tolist() == [1] * 4 and a["acked"].tolist() == [2] * 4 and b["acked"].tolist() == [1] * 4
    if fec is None:
        assert a["retransmitted"].sum() >= 1


# ---------------------------------------------------------------- 6. argument limits

def test_argument_limits_as_the_header_states_them(built_lib):
    import ctypes as C
    import torch
    import pirip_amd
    one = PRE + 3 * FRAME + LOOP_GAP
    tx, mux, block, txs = _tx_side(2, one, S=3)
    dem, ld, rx = _shape_rx(4)
    pkt = pirip_amd.HipPacket(tx=tx, txs=txs, nrx=4, max_frags=3, ring_entries=4)
    both = pirip_amd.HipPacket(rx=rx, tx=tx, txs=txs, max_frags=3, ring_entries=4)

    def fails(p=pkt, peers=2, **kw):
        args = dict(window=4, rto=5, max_tries=3, queue_entries=4, out_entries=1)
        args.update(kw)
        with pytest.raises(pirip_amd.PiripError, match=rf"\({BAD_ARG}\)"):
            pirip_amd.HipArq(p, peers, **args)

    fails(window=0)
    fails(window=33, queue_entries=64)
    fails(rto=0)
    fails(max_tries=0)
    fails(queue_entries=3)
    fails(out_entries=0)
    fails(peers=[2, 2, 256, 2])
    fails(peers=[2, -2, 2, 2])
    dem2, ld2, rx2 = _shape_rx(2)
    fails(p=pirip_amd.HipPacket(rx=rx2, max_frags=3, ring_entries=4), peers=[])                # no transmitter
    fails(p=pirip_amd.HipPacket(tx=tx, txs=txs, nrx=2, max_frags=3, ring_entries=4))           # nrx != nchan
    # (max_packet < 6 needs a code of fewer than 18 data bytes: the stand-in code has 32, so that limit is not reached here)
    ok = pirip_amd.HipArq(pkt, [None, 0, 255, 2], window=32, rto=1, max_tries=1, queue_entries=32, out_entries=1)
    assert (ok.window, ok.rto, ok.max_tries, ok.queue_entries, ok.out_entries, ok.max_payload, ok.acklen) == (32, 1, 1, 32, 1, 3 * CAP - 6, 20)
    L = ok.L
    cfg, out = pirip_amd.ArqConfig(4, 5, 3, 4, 1), C.c_void_p(0x55)
    peers = (C.c_int * 4)(2, 2, 2, 2)
    assert L.pirip_hip_arq_create(pkt.h, None, peers, C.byref(out)) == BAD_ARG and out.value is None
    assert L.pirip_hip_arq_create(pkt.h, C.byref(cfg), None, C.byref(out)) == BAD_ARG
    assert L.pirip_hip_arq_create(pkt.h, C.byref(cfg), peers, None) == BAD_ARG
    blk = block * 2
    o = torch.zeros(blk, dtype=torch.uint8, device="cuda")
    st = torch.zeros((4, 4), dtype=torch.uint8, device="cuda")
    pl = torch.zeros((4, 4, KB), dtype=torch.uint8, device="cuda")
    push = lambda h, n, d_out, ss=4, ps=4 * KB, payload=True: L.pirip_hip_arq_push_records(h.h, st.data_ptr(), ss, pl.data_ptr() if payload else 0, ps, 0, n,
                                                                                           d_out, blk, 0)
    assert push(ok, 4, 0) == BAD_ARG and push(ok, 4, o.data_ptr() + 1) == BAD_ARG and push(ok, -1, o.data_ptr()) == BAD_ARG
    assert push(ok, 4, o.data_ptr(), payload=False) == BAD_ARG and push(ok, 4, o.data_ptr(), ss=3) == BAD_ARG
    assert push(ok, 4, o.data_ptr(), ps=4 * KB - 1) == BAD_ARG and push(ok, 4097, o.data_ptr(), ss=4097, ps=4097 * KB) == UNSUPPORTED
    assert L.pirip_hip_arq_process(ok.h, o.data_ptr(), blk, 0) == BAD_ARG                      # the packet handle has no rx
    assert L.pirip_hip_arq_push(ok.h, o.data_ptr(), blk, o.data_ptr(), blk, 0) == BAD_ARG
    wrx = pirip_amd.HipArq(both, 2, window=2, rto=5, max_tries=3, queue_entries=2, out_entries=2)
    assert L.pirip_hip_arq_push(wrx.h, 0, blk, o.data_ptr(), blk, 0) == BAD_ARG and L.pirip_hip_arq_process(wrx.h, 0, 0, 0) == BAD_ARG
    by, ln = pl.data_ptr(), torch.zeros(16, dtype=torch.int32, device="cuda").data_ptr()
    assert L.pirip_hip_arq_submit(ok.h, 0, KB, KB, 0, 1, ln, 0, 0) == BAD_ARG and L.pirip_hip_arq_submit(ok.h, by, KB, KB, 0, 1, 0, 0, 0) == BAD_ARG
    assert L.pirip_hip_arq_submit(ok.h, by, KB, KB, 0, -1, ln, 0, 0) == BAD_ARG and L.pirip_hip_arq_submit(ok.h, by, KB, KB, 0, 0, ln, 0, 0) == 0
    got = C.c_int(-1)
    assert L.pirip_hip_arq_get_delivered(ok.h, 4, None, None, 0, C.byref(got)) == BAD_ARG and L.pirip_hip_arq_get_delivered(ok.h, -1, None, None, 0, None) == BAD_ARG
    assert L.pirip_hip_arq_get_delivered(ok.h, 0, None, None, 1, None) == BAD_ARG and L.pirip_hip_arq_get_delivered(ok.h, 0, None, None, -1, None) == BAD_ARG
    assert L.pirip_hip_arq_get_delivered(ok.h, 3, None, None, 0, C.byref(got)) == 0 and got.value == 0
    assert L.pirip_hip_arq_get_state(ok.h, 4, *([None] * 6)) == BAD_ARG and L.pirip_hip_arq_get_state(ok.h, 3, *([None] * 6)) == 0
    # submit's limits on the device: a length outside 1 .. max_payload is bad, the 33rd segment finds the ring full
    mp = ok.max_payload
    assert ok.submit([[bytes(mp), bytes(mp + 1), b"x"], [b""], [b"x"] * 33, []]).cpu().tolist() == [1, 0, 32, 0]
    c = ok.counters()
    assert c["bad"].tolist() == [1, 1, 0, 0] and c["refused"].tolist() == [0, 0, 1, 0] and c["waiting"].tolist() == [1, 0, 32, 0]
    torch.cuda.synchronize()
    assert (o == 0).all()                                            # no call ran
