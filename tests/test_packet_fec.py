"""include/pirip_hip.h section R, parity fragments (pirip_hip_pkt_create_fec, pirip_amd.HipPacketFec).

Every comparison is exact: entries, bytes, offered records and every counter come from the host model tests/pktfecref.py, which
tests/test_packet_fec_cpu.py holds to gf256_device.hpp's arithmetic and whose tables it shows to reach every corner. The loops run two
terminals against each other -- once clean, once with a frame's duration of the wideband block wiped out -- and one against a streaming
repeater that holds the longer bursts, each fed the other's previous block."""
import numpy as np
import pytest

import muxshapes as ms
import pktfecref as fr
import pktref
import sigutil
from test_packet import BAD_ARG, CAP, FRAME, KB, PRE, _push_calls, _rng_bytes, _same
from test_ping import LOOP_GAP, ROUTE, _shape_rx, _tx_side

pytestmark = pytest.mark.gpu


def _check(pkt, m, but_call_and_row=False):
    got = pkt.counters()
    got.update(pkt.fec_counters())
    for k, v in list(m.counters().items()) + list(m.fec_counters().items()):
        assert np.array_equal(got[k], v), (k, got[k], v)
    assert not got["orphan"].any()
    for c in range(m.nrx):
        ent, data = pkt.packets(c)
        want, wdata = m.packets(c)
        assert pktref.same_but_call_and_row(ent, want) if but_call_and_row else _same(ent, want), (c, ent, want)
        assert data == wdata, c
    return got


# ---------------------------------------------------------------- 1. the records path

@pytest.mark.parametrize("name", ["small", "one", "wide"])
def test_records_path_equals_the_model(built_lib, name):
    """push_records on a receive-only handle: as one call, as 12 random calls with empty ones among them, and cut between two fragments"""
    import pirip_amd
    sh = fr.SHAPES[name]
    chans = fr.streams(name)
    dem, ld, rx = _shape_rx(len(chans))
    args = dict(rx=rx, filter=fr.FILT, address=fr.ADDR, max_frags=sh[0], max_parity=sh[1], parity_pct=sh[2])
    pkt = pirip_amd.HipPacketFec(ring_entries=fr.RING, **args)
    fi = pkt.fec_info()
    assert (pkt.nrx, pkt.nchan, pkt.cap, pkt.max_packet) == (len(chans), 0, CAP, sh[0] * CAP - 4)
    assert (fi.enabled, fi.max_parity, fi.parity_pct, fi.max_burst_frames) == (1, sh[1], sh[2], sh[0] + fr.r_of(*sh))
    one = pktref.one_call(chans)
    _push_calls(pkt, one)
    ref = fr.run_rows(one, sh)
    got = _check(pkt, ref)
    assert got["recovered"][0] > 0 and got["repaired"][0] >= got["recovered"][0]
    if name == "small":
        assert all(got[k][0] > 0 for k in pktref.RX_COUNTERS + fr.FEC_COUNTERS if k != "orphan")
        ent, data = pkt.packets(0, 2)
        assert _same(ent, pkt.packets(0)[0][-2:]) and data == pkt.packets(0)[1][-2:] and len(pkt.packets(0, 0)[0]) == 0
    wide = pirip_amd.HipPacketFec(ring_entries=5000, **args)
    m = fr.run_rows(one, sh, ring_entries=5000)
    _push_calls(wide, one)
    _check(wide, m)
    cuts = pktref.cut(chans, 5, 12)
    assert any(len(st) == 0 for rows in cuts for st, _ in rows)
    for recut in (cuts, fr.between_fragments(chans)):
        wide.reset()
        assert not any(v.any() for v in wide.counters().values()) and not any(v.any() for v in wide.fec_counters().values())
        assert len(wide.packets(0)[0]) == 0
        _push_calls(wide, recut)
        _check(wide, m, but_call_and_row=True)
    if name == "small":
        # one call of 4096, 4095 and 1 rows behind them; no filter and no address
        big = fr.big_call()
        _push_calls(wide, big)
        mb = fr.run_rows(fr.between_fragments(chans) + big, sh, ring_entries=5000)
        _check(wide, mb, but_call_and_row=True)
        assert mb.c["delivered"][0] > 500 and mb.c["recovered"][0] > 100
        free = pirip_amd.HipPacketFec(rx=rx, max_frags=sh[0], ring_entries=fr.RING, max_parity=sh[1], parity_pct=sh[2])
        _push_calls(free, one)
        got = _check(free, fr.run_rows(one, sh, filt=None, address=None))
        assert not got["filtered"].any() and not got["foreign"].any()


def test_a_plain_handle_is_not_an_fec_handle(built_lib):
    import pirip_amd
    dem, ld, rx = _shape_rx(1)
    plain = pirip_amd.HipPacket(rx=rx, max_frags=5, ring_entries=4)
    info = pirip_amd.PktFecInfo()
    assert plain.L.pirip_hip_pkt_get_fec_info(plain.h, info) == 0
    assert (info.enabled, info.max_parity, info.parity_pct, info.max_burst_frames) == (0, 0, 0, 5)
    z = np.zeros(1, np.int64)
    assert plain.L.pirip_hip_pkt_get_fec_counters(plain.h, z.ctypes.data, None, None, None) == BAD_ARG
    # it receives an undamaged burst of an FEC handle as before and counts the parity frames malformed
    rec = fr.segment_fec(bytes(range(70)), 2, 7, 3, KB, *fr.SHAPES["small"])
    _push_calls(plain, [[fr.rows_of([("frames", rec[:-1], pktref.SYNC | pktref.BITS)])]])
    c = plain.counters()
    assert plain.packets(0)[1] == [bytes(range(70))] and c["malformed"].tolist() == [2] and c["delivered"].tolist() == [1]


# ---------------------------------------------------------------- 2. send and offer

def test_send_path_equals_the_model(built_lib):
    import torch
    import pirip_amd
    sh = fr.SHAPES["small"]
    mbf = sh[0] + fr.r_of(*sh)
    S, pending = 1000, 2 * (mbf + 1)
    one = PRE + mbf * FRAME + LOOP_GAP                                 # a queue of one largest burst
    tx, mux, block, txs = _tx_side(2, one, S=S)
    pkt = pirip_amd.HipPacketFec(tx=tx, txs=txs, nrx=1, source=1, max_frags=sh[0], max_parity=sh[1], parity_pct=sh[2])
    assert (pkt.nchan, pkt.pending, pkt.max_packet, pkt.max_burst_frames, mbf) == (4, pending, 116, 8, 8)
    m = fr.LinkFec(4, 1, KB, sh, pending, one, S, PRE, FRAME, LOOP_GAP)
    script = fr.send_script()
    K, blk, rl = len(script), block * 2, 1 + KB
    rt = sigutil.hip_runtime()
    p_rec, stride, p_n = pkt.offered()
    assert stride == pending * rl
    out = torch.zeros(blk, dtype=torch.uint8, device="cuda")
    off = torch.full((K, 4, pending, rl), 0xEE, dtype=torch.uint8, device="cuda")
    cnt = torch.full((K, 4), -7, dtype=torch.int32, device="cuda")
    none = [torch.zeros(64, dtype=torch.uint8, device="cuda") for _ in range(2)]
    taken, want_taken, offered = [], [], []
    for n, packets in enumerate(script):
        taken.append(pkt.send([[b for b, _ in q] for q in packets], [[d for _, d in q] for q in packets]))
        want_taken.append(m.send(packets))
        pkt.push_records(none[0], none[1], out=out, out_stride=blk, max_calls=0, status_stride=0, payload_stride=0)
        offered.append(m.call())
        sigutil.d2d(rt, off[n].data_ptr(), p_rec, 4 * stride)
        sigutil.d2d(rt, cnt[n].data_ptr(), p_n, 4 * 4)
    torch.cuda.synchronize()
    assert [t.cpu().tolist() for t in taken] == want_taken and want_taken[0] == [4, 2, 1, 0] and want_taken[6] == [1, 1, 0, 2]
    off_h, cnt_h = off.cpu().numpy(), cnt.cpu().numpy()
    for n, per in enumerate(offered):
        assert cnt_h[n].tolist() == [len(r) for r in per], n
        for t, r in enumerate(per):
            assert np.array_equal(off_h[n, t, :len(r)], r), (n, t)
    got = pkt.counters()
    for k, v in m.counters().items():
        assert np.array_equal(got[k], v), (k, got[k], v)
    assert got["refused"].tolist() == [1, 0, 0, 0] and got["bad"].tolist() == [0, 0, 2, 0] and got["sent"].tolist() == [5, 3, 1, 2]
    assert m.ev["blocked"] > 0 and m.ev["wraps"] > 0 and not got["pending"].any()
    # what was offered is the accepted packets' bursts, in order: the lengths 1, cap - 4, cap - 3, cap and max_packet among them
    sent = [p for n, packets in enumerate(script) for p in packets[0][:want_taken[n][0]]]
    assert [len(b) for b, _ in sent] == [1, CAP - 4, CAP - 3, CAP, 116]
    want = np.concatenate([fr.segment_fec(b, 1, d, i, KB, *sh) for i, (b, d) in enumerate(sent)])
    assert np.array_equal(np.concatenate([o[0] for o in offered]), want)


# ---------------------------------------------------------------- 3. the loops (tests/muxshapes.py's LOOP)

class _Node:
    """HipPacketFec(rx=HipRx(chan=...), tx, txs) of the LOOP shapes; the handles it borrows live as long as it does"""

    def __init__(self, source, max_frags, R, pct, address=None):
        import pirip_amd
        from test_mux import _rx_handles
        lp = ms.LOOP
        self.mbf = max_frags + fr.r_of(max_frags, R, pct)
        self.tx, self.mux, self.block, self.txs = _tx_side(lp["M"], PRE + self.mbf * FRAME + LOOP_GAP)
        self.dem, self.ld, self.ch = _rx_handles()
        self.rx = pirip_amd.HipRx(self.dem, ldpc=self.ld, chan=self.ch, block=self.block)
        self.pkt = pirip_amd.HipPacketFec(rx=self.rx, tx=self.tx, txs=self.txs, source=source, filter=source, address=address, max_frags=max_frags,
                                          ring_entries=8, max_parity=R, parity_pct=pct)
        assert self.pkt.rx_rows == self.rx.max_frames and self.pkt.nchan == 4 and self.pkt.nrx == 4 and self.pkt.max_burst_frames == self.mbf


LOOP_R, LOOP_PCT = 4, 50


@pytest.mark.parametrize("gap", [False, True], ids=["clean", "gap"])
def test_two_terminals_exchange_packets(built_lib, gap, record_property):
    """tests/test_packet.py's two terminals with FEC handles, R = 4 and 50 %. A's packets of 51 and 28 bytes -- the two that DESIGN.md
    4.18 records as lost with a zero-padded last fragment --, of 300 bytes (13 fragments) and of max_packet bytes arrive at B, B's
    bursts of equal length at A. gap: 544 symbols (one frame's duration) of the blocks handed from A to B are overwritten with 128 in
    the middle of the long bursts; the packets still arrive, rebuilt."""
    import torch
    mf = 13
    A, B = _Node(1, mf, LOOP_R, LOOP_PCT, address=1), _Node(2, mf, LOOP_R, LOOP_PCT, address=2)
    mp = A.pkt.max_packet
    assert mp == 308 and A.mbf == 17
    p51, p300, p28, pmax = (_rng_bytes(s, n) for s, n in ((1, 51), (3, 300), (2, 28), (4, mp)))
    sent = [p51, p300, p28, pmax]
    ks = [pktref.nfrag_of(len(b), KB) for b in sent]
    rs = [fr.r_of(k, LOOP_R, LOOP_PCT) for k in ks]
    assert ks == [3, 13, 2, 13] and rs == [2, 4, 1, 4]
    back = [_rng_bytes(10 + c, 3 * CAP - 4) for c in range(4)]
    K = 2 + -(-(PRE + A.mbf * FRAME + LOOP_GAP) // 100) + 16
    blk = A.block * 2
    spb = blk // 100                                                 # bytes of a symbol in a block of 100 symbols
    g0 = (2 + (PRE + A.mbf * FRAME) // 200) * blk + 37 * spb         # the middle of the long bursts, sent from call 2 on
    g1 = g0 + FRAME * spb
    silence = torch.full((blk,), 128, dtype=torch.uint8, device="cuda")
    a_out = torch.zeros((K, blk), dtype=torch.uint8, device="cuda")
    b_out = torch.zeros((K, blk), dtype=torch.uint8, device="cuda")
    for k in range(K):
        if k == 2:
            ta = A.pkt.send([[b] for b in sent], [[2], [2], [2], [0xFF]])
            tb = B.pkt.send([[b] for b in back], 1)
        A.pkt.push(b_out[k - 1] if k else silence, blk, a_out[k], blk)
        lo, hi = max(g0, k * blk) - k * blk, min(g1, (k + 1) * blk) - k * blk
        if gap and lo < hi:
            a_out[k, lo:hi] = 128
        B.pkt.push(a_out[k - 1] if k else silence, blk, b_out[k], blk)
    torch.cuda.synchronize()
    assert ta.cpu().tolist() == [1] * 4 and tb.cpu().tolist() == [1] * 4
    a, b = A.pkt.counters(), B.pkt.counters()
    fa, fb = A.pkt.fec_counters(), B.pkt.fec_counters()
    for name, v in (("b", b), ("fb", fb), ("a", a), ("fa", fa)):
        record_property(name, {k: x.tolist() for k, x in v.items()})
        print(name, {k: x.tolist() for k, x in v.items()})
    assert b["delivered"].tolist() == [1] * 4 and a["delivered"].tolist() == [1] * 4
    for k in ("malformed", "incomplete", "crc_fail", "lost", "foreign", "orphan"):
        assert not a[k].any() and not b[k].any(), k
    for c in range(4):
        ent, data = B.pkt.packets(c)
        assert data == [sent[c]] and ent["src"].tolist() == [1] and ent["id"].tolist() == [0] and ent["nfrag"].tolist() == [ks[c]], c
        ent, data = A.pkt.packets(c)
        assert data == [back[c]] and ent["src"].tolist() == [2] and ent["dst"].tolist() == [1], c
    assert all(fb["repaired"][c] <= rs[c] for c in range(4)) and not fa["recovered"].any()
    if gap:
        assert fb["recovered"][1] >= 1 and fb["recovered"][3] >= 1     # the long bursts lay under the gap
    else:
        assert (fb["surplus"] + fb["repaired"] <= np.array(rs)).all()


def test_packets_come_back_through_the_streaming_repeater(built_lib):
    """A terminal against a streaming repeater (source 2, filter 2, route [1, 0, 3, 2]) whose bursts hold k + r frames: every FEC burst
    comes back whole with src = 2 and is delivered; what the terminal hears of itself is filtered."""
    import torch
    import pirip_amd
    from test_mux import _rx_handles
    mf = 3
    A = _Node(1, mf, LOOP_R, LOOP_PCT)
    assert A.mbf == 5
    tx, mux, block, txs = _tx_side(ms.LOOP["M"], PRE + A.mbf * FRAME + LOOP_GAP)
    dem, ld, ch = _rx_handles()
    rx = pirip_amd.HipRx(dem, ldpc=ld, chan=ch, block=block)
    rpt = pirip_amd.HipRepeater(tx, txs, ROUTE, 2, filter=2, holdoff=1, max_burst=A.mbf, pending=A.mbf + 1, rx=rx)
    sent = [_rng_bytes(20 + c, n * CAP - 4) for c, n in enumerate((3, 2, 1, 3))]
    dst = [[0xFF], [1], [0xFF], [7]]
    ks = [3, 2, 1, 3]
    nfr = [k + fr.r_of(k, LOOP_R, LOOP_PCT) for k in ks]
    assert nfr == [5, 3, 2, 5]
    K, blk = 2 * (2 + -(-(PRE + A.mbf * FRAME + LOOP_GAP) // 100)) + 16, A.block * 2
    silence = torch.full((blk,), 128, dtype=torch.uint8, device="cuda")
    a_out = torch.zeros((K, blk), dtype=torch.uint8, device="cuda")
    r_out = torch.zeros((K, blk), dtype=torch.uint8, device="cuda")
    for k in range(K):
        if k == 2:
            taken = A.pkt.send([[b] for b in sent], dst)
        A.pkt.push(r_out[k - 1] if k else silence, blk, a_out[k], blk)
        rpt.push(a_out[k - 1] if k else silence, blk, r_out[k], blk)
    torch.cuda.synchronize()
    assert taken.cpu().tolist() == [1] * 4
    c, f, r = A.pkt.counters(), A.pkt.fec_counters(), rpt.counters()
    print({k: v.tolist() for k, v in list(c.items()) + list(f.items())}, {k: v.tolist() for k, v in r.items()})
    assert r["bursts_in"].tolist() == [1] * 4 and r["bursts_out"].tolist() == [1] * 4 and r["frames_in"].tolist() == nfr
    assert c["delivered"].tolist() == [1] * 4 and c["sent"].tolist() == [1] * 4
    for k in ("filtered", "foreign", "malformed", "orphan", "incomplete", "crc_fail", "lost"):
        assert not c[k].any(), k
    assert not f["recovered"].any() and [int(f["surplus"][ROUTE[ch]]) for ch in range(4)] == [n - k for n, k in zip(nfr, ks)]
    for ch in range(4):                                              # what went out on channel ch comes back on ROUTE[ch]
        ent, data = A.pkt.packets(ROUTE[ch])
        assert data == [sent[ch]] and ent["src"].tolist() == [2] and ent["dst"].tolist() == dst[ch] and ent["id"].tolist() == [0], ch
    # the terminal on its own output: every frame is its own and is filtered
    A.pkt.reset()
    sink = torch.zeros(blk, dtype=torch.uint8, device="cuda")
    for k in range(K // 2):
        A.pkt.push(a_out[k], blk, sink, blk)
    c = A.pkt.counters()
    assert c["filtered"].tolist() == nfr and not c["delivered"].any() and not c["incomplete"].any()
    assert (sink == 128).all() and (a_out != 128).any()


# ---------------------------------------------------------------- 4. argument limits

def test_argument_limits_as_the_header_states_them(built_lib):
    import pirip_amd
    one = PRE + 5 * FRAME + LOOP_GAP                                  # a queue of a burst of five frames
    tx, mux, block, txs = _tx_side(2, one, S=3)
    dem, ld, rx = _shape_rx(2)

    def make(**kw):
        args = dict(tx=tx, txs=txs, nrx=2, source=1, filter=1, address=1, max_frags=3, ring_entries=4, max_parity=2, parity_pct=50)
        args.update(kw)
        return pirip_amd.HipPacketFec(**args)

    def fails(**kw):
        with pytest.raises(pirip_amd.PiripError, match=rf"\({BAD_ARG}\)"):
            make(**kw)

    ok = make()                                                      # r(3) = 2: bursts of five frames, a ring of 2 * 6 records
    assert (ok.max_burst_frames, ok.pending, ok.max_packet) == (5, 12, 3 * CAP - 4)
    assert make(pending=6).pending == 6 and make(max_parity=16, parity_pct=34).max_burst_frames == 5
    fails(max_parity=0)
    fails(max_parity=17)
    fails(parity_pct=0)
    fails(parity_pct=101)
    fails(pending=5)                                                 # max_burst_frames + 1 = 6 records
    fails(max_parity=3, parity_pct=100)                              # r(3) = 3: the queue holds a burst of five
    fails(max_frags=4)                                               # r(4) = 2 likewise
    fails(txs=None)                                                  # pirip_hip_pkt_create's own rules stand
    fails(max_frags=0)
    fails(ring_entries=0)
    listener = dict(tx=None, txs=None, rx=rx)
    assert make(max_frags=84, max_parity=16, parity_pct=1, **listener).max_burst_frames == 85
    assert make(max_frags=99, max_parity=1, parity_pct=100, **listener).max_burst_frames == 100
    fails(max_frags=85, max_parity=16, parity_pct=1, **listener)    # max_frags + max_parity > 100
    fails(max_frags=100, max_parity=1, **listener)
    import ctypes as C
    cfg, out = pirip_amd.PktConfig(2, 1, 1, 1, 3, 12, 4), C.c_void_p(0x55)
    assert ok.L.pirip_hip_pkt_create_fec(rx.h, None, None, C.byref(cfg), None, C.byref(out)) == BAD_ARG and out.value is None
