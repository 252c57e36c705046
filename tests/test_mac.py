"""include/pirip_hip.h section T: half-duplex medium access over the packet link (pirip_hip_mac_*, pirip_amd.HipMac).

Every comparison is exact: the layer is integer arithmetic and one float compare. State, counters and offered records come from the host
model tests/macref.py after every call; tests/test_mac_cpu.py shows that the model does what the header says and that its scripts reach
what they claim. On the records path one handle runs the scripts; over the air two ARQ terminals of tests/muxshapes.py's LOOP share one
HipAir, each hearing the peer and itself."""
import ctypes as C

import numpy as np
import pytest

import macref as m
import pktref
import sigutil
from test_packet import BAD_ARG, CANARY, KB
from test_ping import _shape_rx, _tx_side

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- a model terminal's twin on the device, records path

def _mac_args(mac):
    r = mac.rules
    return dict(rx_of_tx=mac.rx_of_tx, sense_mask=mac.sense_mask, sense_snr=float(mac.sense_snr), slot_calls=r["slot_calls"], cw=r["cw"],
                ifs_calls=r["ifs_calls"], mute_calls=mac.mute_calls, txop_bursts=r["txop_bursts"], key=r["key"])


class _Dev:
    """HipPacket / HipPacketFec(tx, txs) with the configuration of the model terminal `term`, and a HipMac if the model has one"""

    def __init__(self, term, fec=None):
        import torch
        import pirip_amd
        lk, ra = term.link, term.rasm
        self.tx, self.mux, self.block, self.txs = _tx_side(2, lk.queue_syms, S=lk.S)
        assert (self.tx.preamble_syms, self.tx.frame_syms, self.tx.data_bytes) == (m.PRE, m.FRAME, KB)
        args = dict(tx=self.tx, txs=self.txs, nrx=ra.nrx, source=lk.src, filter=ra.filt, address=ra.address, max_frags=lk.max_frags,
                    pending=lk.pending, ring_entries=ra.E)
        self.pkt = pirip_amd.HipPacket(**args) if fec is None else pirip_amd.HipPacketFec(max_parity=fec[0], parity_pct=fec[1], **args)
        self.mac = pirip_amd.HipMac(self.pkt, **_mac_args(term.mac)) if term.mac is not None else None
        self.nchan, self.pending = lk.ntx, lk.pending
        self.blk = self.block * 2
        self.out = torch.full((self.blk + 64,), CANARY, dtype=torch.uint8, device="cuda")
        self.rt = sigutil.hip_runtime()
        self.p_rec, self.stride, self.p_n = self.pkt.offered()
        self.off = torch.zeros((self.nchan, self.pending, 1 + KB), dtype=torch.uint8, device="cuda")
        self.cnt = torch.zeros(self.nchan, dtype=torch.int32, device="cuda")
        self.keep = []

    def send(self, packets):
        return self.pkt.send([[b for b, _ in q] for q in packets], [[d for _, d in q] for q in packets]).cpu().tolist()

    def push(self, rows, stats=None):
        """one call on rows[c] = (status, payload): the slots behind a channel's count hold a packet with SYNC | BITS -- and, with stats, an
        SNRest far above any threshold -- that would be carrier and a delivery, were they read"""
        import torch
        n = len(rows)
        canary = pktref.segment(b"canary", 2, 0xFF, 99, KB, 1)[0, 1:]
        w = max([len(r[0]) for r in rows] + [1])
        st = np.full((n, w), pktref.SYNC | pktref.BITS, np.uint8)
        pl = np.tile(canary, (n, w, 1))
        nc = np.zeros(n, np.int32)
        for c, (a, b) in enumerate(rows):
            st[c, :len(a)], pl[c, :len(a)], nc[c] = a, b, len(a)
        d = [torch.from_numpy(x).cuda() for x in (st, pl, nc)]
        if self.mac is not None:
            if stats is None:
                self.mac.set_stats(None)
            else:
                ss = np.full((n, w, m.STATS_PER_FRAME), 1e9, np.float32)
                for c, s in enumerate(stats):
                    k = len(rows[c][0])
                    ss[c, :k] = np.asarray(s, np.float32).reshape(-1, m.STATS_PER_FRAME)[:k]
                d.append(torch.from_numpy(ss).cuda())
                self.mac.set_stats(d[3])
        self.keep = [d] + self.keep[:2]
        self.st_host = st
        self.pkt.push_records(d[0], d[1], out=self.out.data_ptr() + 32, out_stride=self.blk, ncalls=d[2])

    def offered(self):
        import torch
        sigutil.d2d(self.rt, self.off.data_ptr(), self.p_rec, self.nchan * self.stride)
        sigutil.d2d(self.rt, self.cnt.data_ptr(), self.p_n, 4 * self.nchan)
        torch.cuda.synchronize()
        off, cnt = self.off.cpu().numpy(), self.cnt.cpu().numpy()
        return [off[t, :cnt[t]].copy() for t in range(self.nchan)]

    def check(self, term, want_off, k=None):
        """after a call: offered records, the layer's state and counters, the packet handle's counters; the caller's rows are untouched"""
        import torch
        got = self.offered()
        assert len(got) == len(want_off) and all(np.array_equal(g, w) for g, w in zip(got, want_off)), k
        if term.mac is not None:
            for t in range(self.nchan):
                assert self.mac.state(t) == term.mac.state(t), (k, t, self.mac.state(t), term.mac.state(t))
            have = self.mac.counters()
            for name, v in term.mac.counters().items():
                assert np.array_equal(have[name], v), (k, name, have[name], v)
        pk = self.pkt.counters()
        for name, v in list(term.rasm.counters().items()) + list(term.link.counters().items()):
            if name in pk:
                assert np.array_equal(pk[name], v), (k, name, pk[name], v)
        assert np.array_equal(self.keep[0][0].cpu().numpy(), self.st_host), k
        torch.cuda.synchronize()
        assert (self.out[:32] == CANARY).all() and (self.out[32 + self.blk:] == CANARY).all()

    def packets(self, c):
        return self.pkt.packets(c)[1]


def _run(term, script, fec=None):
    dev = _Dev(term, fec)
    m.run_script(term, script, dev)
    return dev


# ---------------------------------------------------------------- 1. sense

def test_sense_at_the_wave_reductions_edges(built_lib):
    """calls of 0, 1, 63, 64, 65 and 4096 rows, a lone SYNC row at row 0, 63, 64 and the last; every channel's count is another, so the
    rows behind a count (SYNC | BITS canaries) are never carrier"""
    term = m.terminal(mac=dict(cw=1))
    script = [(([], [], [], []), rows, stats) for rows, stats, _ in m.sense_script()]
    dev = _run(term, script)
    c = dev.mac.counters()
    assert c["carrier"][0] > 10 and c["carrier"][3] > 10 and c["carrier"][1] == c["carrier"][2] == 0 and not c["own"].any()
    assert dev.mac.state(1)["idle"] == len(script)


@pytest.mark.parametrize("mask", [1, 2, 3])
def test_sense_by_snr_at_the_threshold_under_it_and_nan(built_lib, mask):
    term = m.terminal(mac=dict(cw=1, sense_mask=mask, sense_snr=m.SNR_T))
    script = [(([], [], [], []), rows, stats) for rows, stats, _ in m.snr_script()]
    dev = _run(term, script)
    # at the threshold and +inf on three row counts with bit 1; the SYNC row with bit 0
    assert dev.mac.counters()["carrier"].tolist() == [(6 if mask & 2 else 0) + (mask & 1), 0, 0, 0]
    assert dev.mac.info.sense_mask == mask and dev.mac.info.sense_snr == float(m.SNR_T)


# ---------------------------------------------------------------- 2. mute

@pytest.mark.parametrize("fec", [None, (2, 50)], ids=["plain", "fec"])
@pytest.mark.parametrize("mute_calls", [2, 0])
def test_rows_behind_an_own_burst_are_muted(built_lib, fec, mute_calls):
    """rows with BITS in every call from the own burst to mute_calls + 1 calls behind its end, and a packet open across the muted calls"""
    term = m.terminal(mac=dict(cw=1, mute_calls=mute_calls), fec=fec)
    dev = _run(term, m.mute_script(mute_calls, fec), fec)
    c = dev.mac.counters()
    assert (c["muted"].sum() > 0) == (mute_calls > 0) and c["won"].tolist() == [1, 1, 0, 1]
    for ch in range(4):
        assert dev.packets(ch) == term.rasm.packets(ch)[1], ch
    if mute_calls:
        assert len(dev.packets(3)) == (1 if fec else 0) and len(dev.packets(0)) < len(dev.packets(2))


# ---------------------------------------------------------------- 3. gate

@pytest.mark.parametrize("case", ["cw1", "cw8_ifs2_txop2", "cw8_ifs0_txop1"])
def test_gate_under_a_seeded_script_of_carrier_patterns(built_lib, case):
    """200 calls on rx_of_tx = [0, -1, 3, 2]; three bursts pending at calls 0 and 90; bursts sent while an access holds the medium. The
    ungated channel's offered bytes equal those of a second handle without the layer."""
    from test_mac_cpu import GATE_CASES
    script = [(s, r, None) for s, r in m.gate_script(3)]
    term = m.terminal(mac=dict(GATE_CASES[case], rx_of_tx=[0, -1, 3, 2], key=5))
    dev = _Dev(term)
    plain_term = m.terminal()
    plain = _Dev(plain_term)
    for k, (send, rows, stats) in enumerate(script):
        if any(send):
            assert dev.send(send) == term.link.send(send) and plain.send(send) == plain_term.link.send(send), k
        off, poff = term.call(rows, stats), plain_term.call(rows)
        dev.push(rows, stats)
        plain.push(rows)
        dev.check(term, off, k)
        if k % 10 == 0 or k == len(script) - 1:
            plain.check(plain_term, poff, k)
        assert np.array_equal(dev.offered()[1], plain.offered()[1]), k
    c = dev.mac.counters()
    assert c["won"][[0, 2, 3]].min() > 3 and c["accesses"][1] == 0 and dev.mac.state(1)["idle"] == -1


# ---------------------------------------------------------------- 4. life cycle and limits

def test_life_cycle(built_lib):
    import pirip_amd
    script = [(s, r, None) for s, r in m.gate_script(4, ncalls=40)]
    kw = dict(cw=8, ifs_calls=1, txop_bursts=1, key=11)
    term = m.terminal(mac=kw)
    dev = _Dev(term)
    with pytest.raises(pirip_amd.PiripError, match=rf"\({BAD_ARG}\)"):
        pirip_amd.HipMac(dev.pkt)                                        # a second layer on one handle
    m.run_script(term, script[:20], dev)
    assert dev.mac.counters()["deferred"].sum() > 0
    zero = dict(phase=m.IDLE, counter=0, run=0, quiet=m.RUN_MAX, idle=0)
    # pirip_hip_pkt_reset resets the layer too
    dev.pkt.reset()
    assert not any(v.any() for v in dev.mac.counters().values()) and all(dev.mac.state(t) == zero for t in range(4))
    term.link.reset(), term.rasm.reset(), term.mac.reset()
    m.run_script(term, script[:20], dev)
    # destroy: the packet handle's next calls equal an unattached handle's
    dev.mac.close()
    dev.mac = term.mac = None
    fresh = m.terminal()
    fresh.link, fresh.rasm = term.link, term.rasm
    m.run_script(fresh, script[20:], dev)
    # and a new layer may be attached afterwards; pirip_hip_arq_reset resets it through the packet handle
    dev.pkt.reset()
    mac = pirip_amd.HipMac(dev.pkt, **dict(kw, rx_of_tx=None))
    arq = pirip_amd.HipArq(dev.pkt, 2, window=2, rto=5, max_tries=3, queue_entries=2, out_entries=2)
    arq.submit([[b"x"]] * 4)
    import torch
    st = torch.zeros((4, 1), dtype=torch.uint8, device="cuda")
    pl = torch.zeros((4, 1, KB), dtype=torch.uint8, device="cuda")
    nc = torch.zeros(4, dtype=torch.int32, device="cuda")
    for _ in range(3):
        arq.push_records(st, pl, out=dev.out.data_ptr() + 32, out_stride=dev.blk, ncalls=nc)
    assert mac.counters()["accesses"].tolist() == [1] * 4
    arq.reset()
    assert not any(v.any() for v in mac.counters().values()) and all(mac.state(t) == zero for t in range(4))


def test_argument_limits_as_the_header_states_them(built_lib):
    import torch
    import pirip_amd
    one = m.BURST
    tx, mux, block, txs = _tx_side(2, one, S=3)
    pkt = pirip_amd.HipPacket(tx=tx, txs=txs, nrx=4, max_frags=3, ring_entries=4)

    def fails(p=pkt, **kw):
        with pytest.raises(pirip_amd.PiripError, match=rf"\({BAD_ARG}\)"):
            pirip_amd.HipMac(p, **kw)

    for kw in (dict(sense_mask=0), dict(sense_mask=4), dict(slot_calls=0), dict(slot_calls=(1 << 20) + 1), dict(cw=0), dict(cw=1025),
               dict(ifs_calls=-1), dict(ifs_calls=1 << 30), dict(mute_calls=-1), dict(mute_calls=(1 << 30) + 1), dict(txop_bursts=0),
               dict(txop_bursts=(1 << 30) + 1), dict(rx_of_tx=[0, 1, 2, 4]), dict(rx_of_tx=[0, 1, 2, -2]), dict(rx_of_tx=[0, 1, 1, None])):
        fails(**kw)
    dem, ld, rx = _shape_rx(4)
    fails(p=pirip_amd.HipPacket(rx=rx, max_frags=3, ring_entries=4), rx_of_tx=[])              # no transmitter
    ok = pirip_amd.HipMac(pkt, rx_of_tx=[3, None, 0, None], sense_mask=3, sense_snr=float("nan"), slot_calls=1 << 20, cw=1024, ifs_calls=(1 << 30) - 1,
                          mute_calls=1 << 30, txop_bursts=1 << 30, key=0xFFFFFFFF)
    i = ok.info
    assert (i.ntx, i.nrx, i.sense_mask, i.slot_calls, i.cw, i.ifs_calls, i.mute_calls, i.txop_bursts, i.key) == \
        (4, 4, 3, 1 << 20, 1024, (1 << 30) - 1, 1 << 30, 1 << 30, 0xFFFFFFFF) and np.isnan(i.sense_snr)
    assert ok.rx_of_tx == [3, -1, 0, -1] and ok.state(1)["idle"] == -1 and ok.state(0) == dict(phase=0, counter=0, run=0, quiet=1 << 30, idle=0)
    L = ok.L
    cfg, out = pirip_amd.MacConfig(1, 0.0, 1, 8, 0, 1, 1, 7), C.c_void_p(0x55)
    rt = (C.c_int32 * 4)(0, 1, 2, 3)
    ok.close()
    assert L.pirip_hip_mac_create(pkt.h, None, rt, C.byref(out)) == BAD_ARG and out.value is None
    assert L.pirip_hip_mac_create(pkt.h, C.byref(cfg), None, C.byref(out)) == BAD_ARG
    assert L.pirip_hip_mac_create(pkt.h, C.byref(cfg), rt, None) == BAD_ARG
    ok = pirip_amd.HipMac(pkt)
    assert L.pirip_hip_mac_get_state(ok.h, 4, *([None] * 5)) == BAD_ARG and L.pirip_hip_mac_get_state(ok.h, -1, *([None] * 5)) == BAD_ARG
    assert L.pirip_hip_mac_get_state(ok.h, 3, *([None] * 5)) == 0 and L.pirip_hip_mac_get_counters(ok.h, *([None] * 8)) == 0
    assert L.pirip_hip_mac_get_info(ok.h, None) == BAD_ARG
    stats = torch.zeros((4, 2, 10), dtype=torch.float32, device="cuda")
    ok.set_stats(stats)
    ok.set_stats(None)
    ok.close()
    # set_stats on a handle with rx: refused when bit 1 senses on the receiver's own stats rows, accepted otherwise
    both = pirip_amd.HipPacket(rx=rx, tx=tx, txs=txs, max_frags=3, ring_entries=4)
    with_snr = pirip_amd.HipMac(both, sense_mask=3, sense_snr=3.0)
    assert L.pirip_hip_mac_set_stats(with_snr.h, stats.data_ptr(), 20) == BAD_ARG and L.pirip_hip_mac_set_stats(with_snr.h, None, 0) == BAD_ARG
    with_snr.close()
    sync_only = pirip_amd.HipMac(both, sense_mask=1)
    assert L.pirip_hip_mac_set_stats(sync_only.h, stats.data_ptr(), 20) == 0
    sync_only.close()


# ---------------------------------------------------------------- 5. over the air (tests/muxshapes.py's LOOP, one HipAir for both ends)

from test_ping import LOOP_GAP, LOOP_S                                   # noqa: E402

assert (LOOP_GAP, LOOP_S) == (m.GAP, m.AIR_S)
# Each receiver hears the peer and itself at gain 1. A terminal's four channels add up to at most 95 / 255 of full scale
# (muxshapes.LOOP's steps), so both together stay under 0.75 and 25 sigma of noise fit above them: the sum cannot clip.
AIR_SIGMA, AIR_GAIN = 0.01, 1.0
AIR_SUBMIT_AT = 2                                                        # 200 symbols of silence lie in front (tests/muxshapes.py)


class _AirNode:
    """HipArq over HipPacket(rx=HipRx(chan=...), tx, txs) of the LOOP shapes with max_frags 3 and W = 2, as tests/test_arq.py's _Node builds
    it, with a HipMac when mac (its keyword arguments) is given; and its model"""

    def __init__(self, source, peer, rto, mac=None):
        import pirip_amd
        from test_mux import _rx_handles
        import muxshapes as ms
        self.queue = m.PRE + m.MAX_FRAGS * m.FRAME + LOOP_GAP
        self.tx, self.mux, self.block, self.txs = _tx_side(ms.LOOP["M"], self.queue)
        self.dem, self.ld, self.ch = _rx_handles()
        self.rx = pirip_amd.HipRx(self.dem, ldpc=self.ld, chan=self.ch, block=self.block)
        self.pkt = pirip_amd.HipPacket(rx=self.rx, tx=self.tx, txs=self.txs, source=source, filter=source, address=source, max_frags=m.MAX_FRAGS,
                                       ring_entries=8)
        self.mac = pirip_amd.HipMac(self.pkt, **mac) if mac else None
        self.arq = pirip_amd.HipArq(self.pkt, peer, window=m.AIR_W, rto=rto, max_tries=m.AIR_TRIES, queue_entries=4, out_entries=8)
        args = (4, source, peer, m.AIR_W, rto, m.AIR_TRIES, 4, 8, self.queue, LOOP_S, m.PRE, m.FRAME, LOOP_GAP)
        kw = dict(max_frags=m.MAX_FRAGS, filt=source, address=source, ring_entries=8)
        self.model = m.MacNode(*args, **kw).attach(**mac) if mac else None
        assert self.pkt.pending == (self.model.pending if mac else 2 * (m.MAX_FRAGS + 1))


class _Air:
    """two terminals on one HipAir(ntx=2, nrx=2): call k's inputs are what both put out in call k - 1. Every call's status, payload and
    stats rows and offered records are copied aside on the device and downloaded at the end."""

    def __init__(self, K, rto, macs=None):
        import torch
        import pirip_amd
        import muxshapes as ms
        self.K = K
        self.nodes = [_AirNode(1, 2, rto, macs[0] if macs else None), _AirNode(2, 1, rto, macs[1] if macs else None)]
        A = self.nodes[0]
        self.blk = A.block * 2
        paths = [(r, t, AIR_GAIN, 0, 0) for r in range(2) for t in range(2)]
        self.air = pirip_amd.HipAir(ms.LOOP["Fs"], paths, 2, 2, sigma=AIR_SIGMA, seed=7)
        self.out = torch.full((K + 1, 2, self.blk), 128, dtype=torch.uint8, device="cuda")         # out[0]: silence in front of call 0
        self.heard = torch.zeros((2, self.blk), dtype=torch.uint8, device="cuda")
        self.rows, self.pending = A.pkt.rx_rows, A.pkt.pending
        R, P = self.rows, self.pending
        z = lambda *shape, dtype=torch.uint8: torch.zeros(shape, dtype=dtype, device="cuda")
        self.log = dict(status=z(K, 2, 4, R), payload=z(K, 2, 4, R, KB), nf=z(K, 2, 4, dtype=torch.int32),
                        stats=z(K, 2, 4, R, m.STATS_PER_FRAME, dtype=torch.float32), off=z(K, 2, 4, P, 1 + KB), noff=z(K, 2, 4, dtype=torch.int32))
        self.rt = sigutil.hip_runtime()

    def call(self, k):
        lg = self.log
        self.air.push(self.out[k], self.blk, self.blk // 2, self.heard, self.blk)
        for side, nd in enumerate(self.nodes):
            nd.arq.push(self.heard[side], self.blk, self.out[k + 1, side], self.blk)
            r = nd.pkt.records()
            assert r["status_stride"] == self.rows and r["payload_stride"] == self.rows * KB
            sigutil.d2d(self.rt, lg["status"][k, side].data_ptr(), r["status"], 4 * self.rows)
            sigutil.d2d(self.rt, lg["payload"][k, side].data_ptr(), r["payload"], 4 * self.rows * KB)
            sigutil.d2d(self.rt, lg["nf"][k, side].data_ptr(), r["nframes"], 16)
            if nd.mac is not None and nd.mac.stats()[0]:
                p, stride = nd.mac.stats()
                assert stride == self.rows * m.STATS_PER_FRAME
                sigutil.d2d(self.rt, lg["stats"][k, side].data_ptr(), p, 4 * 4 * stride)
            p_rec, stride, p_n = nd.pkt.offered()
            assert stride == self.pending * (1 + KB)
            sigutil.d2d(self.rt, lg["off"][k, side].data_ptr(), p_rec, 4 * stride)
            sigutil.d2d(self.rt, lg["noff"][k, side].data_ptr(), p_n, 16)

    def run(self, ta, tb):
        import torch
        for k in range(self.K):
            if k == AIR_SUBMIT_AT:
                got = self.nodes[0].arq.submit(ta), self.nodes[1].arq.submit(tb)
            self.call(k)
        torch.cuda.synchronize()
        assert got[0].cpu().tolist() == [len(q) for q in ta] and got[1].cpu().tolist() == [len(q) for q in tb]
        return {k: v.cpu().numpy() for k, v in self.log.items()}

    def rows_of(self, log, k, side):
        nf = log["nf"][k, side]
        rows = [(log["status"][k, side, c, :nf[c]], log["payload"][k, side, c, :nf[c]]) for c in range(4)]
        return rows, [log["stats"][k, side, c, :nf[c]] for c in range(4)]


def _air_traffic():
    """two segments per channel in each direction, every DATA packet filling its last fragment (tests/test_packet.py's PADDING note)"""
    mp = m.MAX_FRAGS * pktref.cap(KB) - 6
    mk = lambda base: [[m._bytes(np.random.default_rng(base + 10 * c + j), n) for j, n in enumerate((mp, 42))] for c in range(4)]
    return mk(1000), mk(2000)


def _air_calls(log, side):
    """per channel the set of calls in which `side` was on air, from the records it offered: section K's queue, counted in symbols"""
    out = []
    for c in range(4):
        q, on = 0, set()
        for k in range(log["noff"].shape[0]):
            ctl = log["off"][k, side, c, :log["noff"][k, side, c], 0]
            q += sum(m.PRE * (x == 1) + m.FRAME * (x < 2) + LOOP_GAP * (x == 2) for x in ctl.tolist())
            if q > 0:
                on.add(k)
            q -= min(LOOP_S, q)
        out.append(on)
    return out


def _rto(slot_calls):
    """one DATA access + one ACK access + the longest backoff + a margin of 8 calls: an ACK that waits behind the peer's own DATA burst"""
    calls = lambda frames: -(-(m.PRE + frames * m.FRAME + LOOP_GAP) // LOOP_S)
    return calls(m.MAX_FRAGS) + calls(1) + slot_calls * m.AIR_CW + 8


def _measure_link(K=110):
    """One DATA burst per channel from A at call 2 and B's ACKs to it, both ends with a layer that never waits (cw = 1) and never mutes:
    what both receivers see, call by call. -> the figures DESIGN.md 4.20 records."""
    never = dict(sense_mask=3, sense_snr=1e30, slot_calls=1, cw=1, ifs_calls=0, mute_calls=0, txop_bursts=1)
    air = _Air(K, 10 * K, [dict(never, key=1), dict(never, key=2)])
    mp = m.MAX_FRAGS * pktref.cap(KB) - 6
    log = air.run([[m._bytes(np.random.default_rng(c), mp)] for c in range(4)], [[]] * 4)
    on = [_air_calls(log, 0), _air_calls(log, 1)]
    busy = set().union(*on[0], *on[1])
    fig = dict(rows_per_call=air.rows, lat_sync=[], tail_sync=[], own_tail=[], gap_sync=[], a_air=[], b_air=[])
    inside, noise = [], []
    sync_at = lambda side, c: [k for k in range(K) if (log["status"][k, side, c, :log["nf"][k, side, c]] & pktref.SYNC).any()]
    for c in range(4):
        first, last = min(on[0][c]), max(on[0][c])
        b_first = min(on[1][c]) if on[1][c] else K
        fig["a_air"].append((first, last))
        fig["b_air"].append((b_first, max(on[1][c]) if on[1][c] else K))
        heard = [k for k in sync_at(1, c) if k >= first]
        own = [k for k in sync_at(0, c) if first <= k <= b_first]
        lat = heard[0] - first
        fig["lat_sync"].append(lat)
        fig["tail_sync"].append(max(k for k in heard if k <= b_first) - last)
        fig["own_tail"].append(max(own) - last if own else None)
        fig["gap_sync"].append(max([b - a - 1 for a, b in zip(heard, heard[1:]) if b <= last + 1] + [0]))
        for k in range(first + lat + 1, last + 1):
            inside += log["stats"][k, 1, c, :log["nf"][k, 1, c], m.SNR_AT].tolist()
    for k in range(K):
        if not any(j in busy for j in range(k - 15, k + 1)):
            for side in range(2):
                for c in range(4):
                    noise += log["stats"][k, side, c, :log["nf"][k, side, c], m.SNR_AT].tolist()
    fig.update(snr_min_inside=min(inside), snr_max_noise=max(noise), n_inside=len(inside), n_noise=len(noise))
    fig["snr_lat"] = None
    if fig["snr_max_noise"] > 0 and fig["snr_min_inside"] >= 4 * fig["snr_max_noise"]:
        thr = float(np.sqrt(np.float64(fig["snr_min_inside"]) * fig["snr_max_noise"]))
        fig["sense_snr"], fig["snr_lat"] = thr, []
        for c in range(4):
            first = fig["a_air"][c][0]
            fig["snr_lat"].append(min(k for k in range(first, K) if (log["stats"][k, 1, c, :log["nf"][k, 1, c], m.SNR_AT] >= thr).any()) - first)
    a, b = (nd.arq.counters() for nd in air.nodes)
    fig["delivered"] = (a["delivered"].tolist(), b["delivered"].tolist())
    return fig, log


# Measured on this link (one run on the MI355X, _measure_link; DESIGN.md 4.20 has the figures): calls from the first call with a burst on
# air to the first call in which the peer's sense step reports carrier, per sense mode; calls behind a burst's last in which its own
# receiver still shows rows of it; the longest run of calls without a SYNC row inside a burst.
AIR_LATENCY = {1: 7, 2: 1, 3: 1}                                         # sense_mask -> calls: SYNC needs the unique word, SNRest one block
AIR_OWN_TAIL, AIR_GAP = 6, 0                                             # (rows with SYNC; SNRest falls back one call behind the burst)
# SNRest: smallest over rows inside bursts 4849.9, largest over rows of noise alone 4.963 -- more than a factor of four apart, so their
# geometric mean senses, beside SYNC
AIR_SENSE_MASK, AIR_SENSE_SNR = 3, float(np.sqrt(4849.94287109375 * 4.9632182121276855))
AIR_SLOT_CALLS = AIR_LATENCY[AIR_SENSE_MASK] + 1                         # a row may fall either side of a block boundary
AIR_MUTE_CALLS = AIR_OWN_TAIL + 2                                        # likewise, and quiet counts from 0
AIR_IFS_CALLS = AIR_GAP + 1
AIR_K = 420


def _mac_kw(key, sense_mask=None, sense_snr=None, slot_calls=None, mute_calls=None, ifs_calls=None):
    return dict(sense_mask=AIR_SENSE_MASK if sense_mask is None else sense_mask, sense_snr=AIR_SENSE_SNR if sense_snr is None else sense_snr,
                slot_calls=AIR_SLOT_CALLS if slot_calls is None else slot_calls, cw=m.AIR_CW, ifs_calls=AIR_IFS_CALLS if ifs_calls is None else ifs_calls,
                mute_calls=AIR_MUTE_CALLS if mute_calls is None else mute_calls, txop_bursts=1, key=key)


def _control_run(K=AIR_K, slot_calls=None):
    air = _Air(K, _rto(AIR_SLOT_CALLS if slot_calls is None else slot_calls))
    ta, tb = _air_traffic()
    air.run(ta, tb)
    return air, ta, tb


def _mac_run(K=AIR_K, **kw):
    macs = [_mac_kw(m.AIR_KEYS[0], **kw), _mac_kw(m.AIR_KEYS[1], **kw)]
    air = _Air(K, _rto(macs[0]["slot_calls"]), macs)
    ta, tb = _air_traffic()
    log = air.run(ta, tb)
    return air, ta, tb, log


def _replay(air, ta, tb, log):
    """the model fed the device's rows must offer the device's records in every call; -> the first (call, side, channel) that differs"""
    for k in range(air.K):
        for side, (nd, tr) in enumerate(zip(air.nodes, (ta, tb))):
            if k == AIR_SUBMIT_AT:
                assert nd.model.submit(tr) == [len(q) for q in tr]
            rows, stats = air.rows_of(log, k, side)
            off = nd.model.call(rows, stats if nd.model.mac.sense_mask & 2 else None)
            for c in range(4):
                if not np.array_equal(off[c], log["off"][k, side, c, :log["noff"][k, side, c]]):
                    return k, side, c
    return None


def test_without_the_layer_two_terminals_with_equal_timers_collide(built_lib, record_property):
    """the control run: the same nodes and schedule with no layer attached; at least one DATA packet of each direction fails to arrive"""
    air, ta, tb = _control_run()
    a, b = (nd.arq.counters() for nd in air.nodes)
    record_property("control", dict(a={k: v.tolist() for k, v in a.items()}, b={k: v.tolist() for k, v in b.items()}))
    print("control a", {k: v.tolist() for k, v in a.items()}, "b", {k: v.tolist() for k, v in b.items()})
    assert b["delivered"].sum() < sum(len(q) for q in ta) and a["delivered"].sum() < sum(len(q) for q in tb)


def test_with_the_layer_every_segment_arrives_and_the_model_predicts_every_offer(built_lib, record_property):
    """Layers attached, keys m.AIR_KEYS (tests/test_mac_cpu.py proves their draws differ), rto = _rto(slot_calls). Every segment is
    delivered once and in order in both directions, nothing is broken, every row with BITS that a terminal's own air produced is muted
    (none reaches the reassembly's own-source filter), and the model, fed every call's status and stats rows, predicts each side's offered
    records of every call byte for byte. Counters of one run on the MI355X are in DESIGN.md 4.20."""
    assert m.keys_differ(m.AIR_KEYS, m.AIR_CW)
    air, ta, tb, log = _mac_run()
    assert _replay(air, ta, tb, log) is None
    a, b = (nd.arq.counters() for nd in air.nodes)
    ma, mb = (nd.mac.counters() for nd in air.nodes)
    for name, v in (("a", a), ("b", b), ("a_mac", ma), ("b_mac", mb), ("a_pkt", air.nodes[0].pkt.counters()), ("b_pkt", air.nodes[1].pkt.counters())):
        record_property(name, {k: x.tolist() for k, x in v.items()})
        print(name, {k: x.tolist() for k, x in v.items()})
    for c in range(4):
        ent, data = air.nodes[1].arq.delivered(c)
        assert data == ta[c] and ent["seq"].tolist() == [0, 1], c
        ent, data = air.nodes[0].arq.delivered(c)
        assert data == tb[c] and ent["seq"].tolist() == [0, 1], c
    assert not a["broken"].any() and not b["broken"].any() and not a["inflight"].any() and not b["inflight"].any()
    for nd, mc in zip(air.nodes, (ma, mb)):
        assert mc["muted"].min() > 0 and not nd.pkt.counters()["filtered"].any()
        model = nd.model.mac.counters()
        for name in m.TX_COUNTERS + m.RX_COUNTERS:
            assert np.array_equal(mc[name], model[name]), name
