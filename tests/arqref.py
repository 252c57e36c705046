"""Host model of the ARQ sessions (include/pirip_hip.h section S), for tests/test_arq*.py: the statement of the rules.

Session holds one channel's sender and receiver (rules of the header: stage (a) - (d), commit, R1 - R4). Node is one terminal: the sessions
over tests/pktref.py's Link and Reassembler -- or tests/pktfecref.py's twins --, imported and not copied, stepped in the header's order
stage, send, commit, the packet handle's call, receive. Pair runs two Nodes against each other on the records path, each fed the records
the other offered in the call before, minus a loss script. The event tables are built in the manner of pktref.corner_events;
tests/test_arq_cpu.py shows that they reach every branch they claim before the device sees them."""
import numpy as np

import pktfecref
import pktref

KB = pktref.KB
DATA, ACK = 0xD0, 0xA0
ACK_MIN = 6
IN_ORDER, AHEAD, OLD, OUTSIDE = 0, 1, 2, 3

# pirip_arq_entry (16 bytes, the C layout)
ENTRY = np.dtype([("seq", "<i8"), ("call", "<i4"), ("length", "<i4")])
assert ENTRY.itemsize == 16
SENDER_COUNTERS = ("sent", "retransmitted", "acked", "acks_sent", "deferred", "refused", "bad", "broken", "waiting", "inflight")
RECEIVER_COUNTERS = ("delivered", "duplicate", "outside", "stale", "alien", "stranger", "malformed", "overrun", "lost")
STATE = ("sub_nxt", "snd_nxt", "snd_una", "rcv_nxt", "held", "ack_pending")


def ack_len(kb, max_frags):
    return max(ACK_MIN, min(pktref.cap(kb) - 4, pktref.max_packet(kb, max_frags)))


def ack_bytes(base, bitmap, n):
    """the n bytes of an ACK: type, base, the bitmap least significant byte first, the filler"""
    base &= 0xFF
    return bytes([ACK, base]) + int(bitmap).to_bytes(4, "little") + bytes((31 * base + 73 * q + 0x5A) & 0xFF for q in range(ACK_MIN, n))


def data_bytes(seq, payload):
    return bytes([DATA, seq & 0xFF]) + bytes(payload)


def data_class(seq, rcv_nxt, W):
    """rule R3's resolution of a sequence byte: (class, d)"""
    d = (seq - rcv_nxt) & 255
    if d == 0:
        return IN_ORDER, d
    if d < W:
        return AHEAD, d
    back = (rcv_nxt - seq) & 255
    return (OLD if 1 <= back <= min(W, rcv_nxt) else OUTSIDE), d


def ack_advance(base, snd_una, snd_nxt):
    """rule R4: the segments acknowledged cumulatively, or -1 for a stale ACK"""
    a = (base - snd_una) & 255
    return -1 if a > snd_nxt - snd_una else a


EVENTS = ("stage_ack", "stage_again", "stage_new", "stage_broke", "stage_broken", "stage_window_full", "stage_nothing", "commit_ack",
          "commit_again", "commit_new", "commit_untaken_ack", "commit_untaken_again", "commit_untaken_new", "submit_bad", "submit_full",
          "submit_broken", "alien_short", "alien_type", "stranger", "data_short", "in_order", "successors", "hold", "dup_held", "dup_old",
          "old_limited_by_start", "outside", "ack_short", "ack_long", "stale", "ack_cumulative", "ack_by_bit", "ack_bit_then_cumulative",
          "ack_nothing_new", "ack_bit_beyond_snd_nxt", "overrun", "out_ring_wraps", "seq_wraps", "held_across_wrap")


class Session:
    def __init__(self, peer, W, rto, max_tries, Q, E, max_payload, acklen, ev=None):
        self.peer, self.W, self.rto, self.max_tries, self.Q, self.E, self.max_payload, self.acklen = peer, W, rto, max_tries, Q, E, max_payload, acklen
        self.ev = ev if ev is not None else dict.fromkeys(EVENTS, 0)
        self.reset()

    def reset(self):
        self.sub_nxt = self.snd_nxt = self.snd_una = self.rcv_nxt = 0
        self.broken, self.ack_pending, self.held = 0, 0, 0
        self.acked, self.tries, self.due = [0] * self.W, [0] * self.W, [0] * self.W
        self.seg = {}                                                     # absolute sequence number -> bytes, until snd_una passes it
        self.reorder = {}
        self.out = []                                                     # every (entry, bytes) ever delivered
        self.c = dict.fromkeys(SENDER_COUNTERS[:8] + RECEIVER_COUNTERS[:8], 0)

    # ---- sender
    def submit(self, segs):
        k = 0
        for b in segs:
            if not 1 <= len(b) <= self.max_payload:
                self.c["bad"] += 1
                self.ev["submit_bad"] += 1
                break
            if self.broken or self.sub_nxt - self.snd_una >= self.Q:
                self.c["refused"] += 1
                self.ev["submit_broken" if self.broken else "submit_full"] += 1
                break
            self.seg[self.sub_nxt] = bytes(b)
            self.sub_nxt += 1
            k += 1
        return k

    def stage(self, n):
        """step 1 -> list of (kind, seq, bytes): kind "ack", "again" or "new" """
        items = []
        if self.ack_pending:                                              # (a)
            items.append(("ack", 0, ack_bytes(self.rcv_nxt, self.held, self.acklen)))
            self.ev["stage_ack"] += 1
        flight = range(self.snd_una, self.snd_nxt)
        if not self.broken and any(not self.acked[s % self.W] and self.due[s % self.W] <= n and self.tries[s % self.W] == self.max_tries for s in flight):
            self.broken = 1                                               # (b)
            self.c["broken"] += 1
            self.ev["stage_broke"] += 1
        if self.broken:
            self.ev["stage_broken"] += 1
            return items
        for s in flight:                                                  # (c)
            if not self.acked[s % self.W] and self.due[s % self.W] <= n:
                items.append(("again", s, data_bytes(s, self.seg[s])))
                self.ev["stage_again"] += 1
        s = self.snd_nxt                                                  # (d)
        while s - self.snd_una < self.W and s < self.sub_nxt:
            items.append(("new", s, data_bytes(s, self.seg[s])))
            self.ev["stage_new"] += 1
            s += 1
        self.ev["stage_window_full"] += s < self.sub_nxt
        self.ev["stage_nothing"] += not items
        assert len(items) <= 1 + self.W
        return items

    def commit(self, n, items, taken):
        """step 3: the taken prefix's state changes"""
        for kind, s, _ in items[:taken]:
            self.ev["commit_" + kind] += 1
            if kind == "ack":
                self.ack_pending = 0
                self.c["acks_sent"] += 1
            elif kind == "again":
                self.tries[s % self.W] += 1
                self.due[s % self.W] = n + self.rto
                self.c["retransmitted"] += 1
            else:
                assert s == self.snd_nxt
                self.tries[s % self.W], self.due[s % self.W] = 1, n + self.rto
                self.snd_nxt += 1
                self.c["sent"] += 1
        for kind, _, _ in items[taken:]:
            self.ev["commit_untaken_" + kind] += 1
        self.c["deferred"] += len(items) - taken

    # ---- receiver
    def _deliver(self, n, payload):
        e = np.zeros((), ENTRY)
        e["seq"], e["call"], e["length"] = self.rcv_nxt, n, len(payload)
        self.out.append((e, bytes(payload)))
        self.ev["out_ring_wraps"] += len(self.out) > self.E
        self.c["delivered"] += 1
        self.rcv_nxt += 1
        self.ev["seq_wraps"] += self.rcv_nxt % 256 == 0

    def skip(self, count):
        self.c["overrun"] += count
        self.ev["overrun"] += 1

    def receive(self, n, p, src):
        """step 5, one section R packet p from source src through R1 - R4"""
        L = len(p)
        if L < 2 or p[0] not in (DATA, ACK):                              # R1
            self.c["alien"] += 1
            self.ev["alien_short" if L < 2 else "alien_type"] += 1
            return
        if self.peer >= 0 and src != self.peer:                           # R2
            self.c["stranger"] += 1
            self.ev["stranger"] += 1
            return
        if p[0] == DATA:                                                  # R3
            if L < 3:
                self.c["malformed"] += 1
                self.ev["data_short"] += 1
                return
            cls, d = data_class(p[1], self.rcv_nxt, self.W)
            if cls == IN_ORDER:
                self._deliver(n, p[2:])
                self.ev["in_order"] += 1
                more, self.held = self.held & 1, self.held >> 1
                while more:
                    self.ev["successors"] += 1
                    self._deliver(n, self.reorder.pop(self.rcv_nxt))
                    more, self.held = self.held & 1, self.held >> 1
                self.ack_pending = 1
            elif cls == AHEAD:
                if self.held >> (d - 1) & 1:
                    self.c["duplicate"] += 1
                    self.ev["dup_held"] += 1
                else:
                    self.reorder[self.rcv_nxt + d] = p[2:]
                    self.held |= 1 << (d - 1)
                    self.ev["hold"] += 1
                    self.ev["held_across_wrap"] += (self.rcv_nxt & 255) + d >= 256
                self.ack_pending = 1
            elif cls == OLD:
                self.c["duplicate"] += 1
                self.ev["dup_old"] += 1
                self.ack_pending = 1
            else:
                self.c["outside"] += 1
                self.ev["outside"] += 1
                self.ev["old_limited_by_start"] += 1 <= (self.rcv_nxt - p[1]) & 255 <= self.W
            return
        if L < ACK_MIN:                                                   # R4
            self.c["malformed"] += 1
            self.ev["ack_short"] += 1
            return
        self.ev["ack_long"] += L > ACK_MIN
        base, bitmap = p[1], int.from_bytes(p[2:6], "little")
        a = ack_advance(base, self.snd_una, self.snd_nxt)
        if a < 0:
            self.c["stale"] += 1
            self.ev["stale"] += 1
            return
        new = 0
        for s in range(self.snd_una, self.snd_una + a):
            new += not self.acked[s % self.W]
            self.ev["ack_bit_then_cumulative"] += self.acked[s % self.W]
            self.ev["ack_cumulative"] += not self.acked[s % self.W]
            self.acked[s % self.W] = 0                                    # the slot is free for its next segment
            del self.seg[s]
        self.snd_una += a
        for i in range(32):
            s = self.snd_una + 1 + i
            if bitmap >> i & 1:
                if s >= self.snd_nxt:
                    self.ev["ack_bit_beyond_snd_nxt"] += 1
                elif not self.acked[s % self.W]:
                    self.acked[s % self.W] = 1
                    new += 1
                    self.ev["ack_by_bit"] += 1
        self.ev["ack_nothing_new"] += not new
        self.c["acked"] += new

    def state(self):
        return dict(sub_nxt=self.sub_nxt, snd_nxt=self.snd_nxt, snd_una=self.snd_una, rcv_nxt=self.rcv_nxt, held=self.held,
                    ack_pending=self.ack_pending)

    def delivered(self, max_entries=None):
        """what get_delivered returns: the newest min(delivered, out_entries, max) entries, oldest first, and their bytes"""
        n = min(len(self.out), self.E if max_entries is None else min(self.E, max_entries))
        kept = self.out[len(self.out) - n:]
        return np.array([e for e, _ in kept], dtype=ENTRY).reshape(n), [b for _, b in kept]


class Node:
    """One terminal: nchan sessions over a packet link. fec: None for a plain handle, or (max_parity, parity_pct)."""

    def __init__(self, nchan, src, peers, W, rto, max_tries, Q, E, queue_syms, S, pre, frame, gap, kb=KB, max_frags=pktref.MAX_FRAGS, pending=None,
                 filt=None, address=None, ring_entries=64, fec=None):
        self.nchan, self.kb, self.max_frags, self.ring_entries = nchan, kb, max_frags, ring_entries
        if fec is None:
            pending = 2 * (max_frags + 1) if pending is None else pending
            self.link = pktref.Link(nchan, src, kb, max_frags, pending, queue_syms, S, pre, frame, gap)
            self.rasm = pktref.Reassembler(nchan, kb, max_frags, filt, address, ring_entries)
        else:
            shape = (max_frags,) + tuple(fec)
            pending = 2 * (max_frags + pktfecref.r_of(*shape) + 1) if pending is None else pending
            self.link = pktfecref.LinkFec(nchan, src, kb, shape, pending, queue_syms, S, pre, frame, gap)
            self.rasm = pktfecref.ReassemblerFec(nchan, kb, max_frags, filt, address, ring_entries, *fec)
        self.pending = pending
        self.max_payload, self.acklen = pktref.max_packet(kb, max_frags) - 2, ack_len(kb, max_frags)
        self.ev = dict.fromkeys(EVENTS, 0)
        peers = [peers] * nchan if np.isscalar(peers) or peers is None else list(peers)
        self.sess = [Session(-1 if p is None else p, W, rto, max_tries, Q, E, self.max_payload, self.acklen, self.ev) for p in peers]
        self.seen = [0] * nchan
        self.n = 0

    def submit(self, segs):
        """segs[t]: list of bytes -> taken [nchan]"""
        return [s.submit(q) for s, q in zip(self.sess, segs)]

    def call(self, rows):
        """call n on rows[c] = (status, payload) -> the records offered, per channel"""
        n = self.n
        items = [s.stage(n) for s in self.sess]                           # 1
        dst = [0xFF if s.peer < 0 else s.peer for s in self.sess]
        taken = self.link.send([[(b, d) for _, _, b in it] for it, d in zip(items, dst)])         # 2
        for s, it, k in zip(self.sess, items, taken):                     # 3
            s.commit(n, it, k)
        self.rasm.call(rows)                                              # 4
        offered = self.link.call()
        for c, s in enumerate(self.sess):                                 # 5
            got = self.rasm.entries[c]
            if len(got) - self.seen[c] > self.ring_entries:
                s.skip(len(got) - self.seen[c] - self.ring_entries)
                self.seen[c] = len(got) - self.ring_entries
            for e, b in got[self.seen[c]:]:
                s.receive(n, b, int(e["src"]))
            self.seen[c] = len(got)
        self.n += 1
        return offered

    def counters(self):
        out = {k: np.array([s.c[k] for s in self.sess], np.int64) for k in SENDER_COUNTERS[:8] + RECEIVER_COUNTERS[:8]}
        out["waiting"] = np.array([s.sub_nxt - s.snd_nxt for s in self.sess], np.int64)
        out["inflight"] = np.array([s.snd_nxt - s.snd_una for s in self.sess], np.int64)
        out["lost"] = np.array([max(len(s.out) - s.E, 0) for s in self.sess], np.int64)
        return out

    def states(self):
        return [s.state() for s in self.sess]


# ---------------------------------------------------------------- two terminals on the records path

AB, BA = 0, 1


class Loss:
    """a loss script: the set `records` of (direction, call, channel, record index) to drop -- call and index as the sender offered them --,
    every record of direction one_way, and with a seed every burst with probability p"""

    def __init__(self, records=(), seed=None, p=0.0, one_way=None):
        self.records, self.seed, self.p, self.one_way = set(records), seed, p, one_way

    def lost(self, direction, call, chan, rec, burst_first):
        if direction == self.one_way or (direction, call, chan, rec) in self.records:
            return True
        return self.seed is not None and np.random.default_rng([self.seed, direction, call, chan, burst_first]).random() < self.p


def rows_of_offered(offered, loss, direction, call, kb=KB):
    """the records a terminal offered in `call`, per channel, as the other terminal's rows: a frame that arrives is SYNC | BITS with the
    record's bytes; a lost frame and the `2` record that ends a burst are rows without SYNC and BITS"""
    rows = []
    for c, rec in enumerate(offered):
        rec = np.asarray(rec, np.uint8).reshape(-1, 1 + kb)
        st, pl = np.zeros(len(rec), np.uint8), np.zeros((len(rec), kb), np.uint8)
        first = 0
        for i, r in enumerate(rec):
            if r[0] == 1:
                first = i
            if r[0] != 2 and not loss.lost(direction, call, c, i, first):
                st[i], pl[i] = pktref.SYNC | pktref.BITS, r[1:]
        rows.append((st, pl))
    return rows


class Pair:
    def __init__(self, a, b, loss=None):
        self.a, self.b, self.loss, self.k = a, b, loss or Loss(), 0
        self.off = [[np.zeros((0, 1 + a.kb), np.uint8)] * a.nchan, [np.zeros((0, 1 + b.kb), np.uint8)] * b.nchan]

    def rows(self):
        """(A's rows, B's rows) of the next call: what the other side offered in the call before"""
        return (rows_of_offered(self.off[BA], self.loss, BA, self.k - 1, self.a.kb), rows_of_offered(self.off[AB], self.loss, AB, self.k - 1, self.b.kb))

    def call(self):
        ra, rb = self.rows()
        self.off = [self.a.call(ra), self.b.call(rb)]
        self.k += 1
        return self.off


# ---------------------------------------------------------------- the shapes and scripts both test files use

SRC_A, SRC_B = 1, 2
W, MAX_TRIES, QUEUE, OUT = 4, 8, 8, 64
PRE, FRAME, GAP = 50, 544, 64                  # the stand-in code with M = 2 and tests/test_ping.py's LOOP_GAP
BURST = PRE + pktref.MAX_FRAGS * FRAME + GAP   # symbols of one largest burst: the transmit queue both test files give a terminal


def node(src, peer, S, rto, W=W, max_tries=MAX_TRIES, Q=QUEUE, E=OUT, nchan=4, ring_entries=64, fec=None, queue_syms=None, peers=None, pending=None):
    shape_r = 0 if fec is None else pktfecref.r_of(pktref.MAX_FRAGS, *fec)
    qs = PRE + (pktref.MAX_FRAGS + shape_r) * FRAME + GAP if queue_syms is None else queue_syms
    return Node(nchan, src, peer if peers is None else peers, W, rto, max_tries, Q, E, qs, S, PRE, FRAME, GAP, filt=src, address=src,
                ring_entries=ring_entries, fec=fec, pending=pending)


def _bytes(rng, n):
    return rng.integers(0, 256, n).astype(np.uint8).tobytes()


def traffic(seed, nseg, nchan=4, max_payload=114):
    """segs[t]: nseg segments of every length, the shortest and the longest among them"""
    rng = np.random.default_rng(seed)
    out = []
    for t in range(nchan):
        ln = [1, max_payload] + [int(rng.integers(1, max_payload + 1)) for _ in range(nseg - 2)]
        out.append([_bytes(rng, n) for n in ln[:nseg]])
    return out


def run_pair(pair, traffic_a, traffic_b, ncalls, per_call=2, hook=None):
    """both sides hand over per_call segments per channel and call while they have any (what is refused is handed over again), for ncalls
    calls; hook(k, offered) after every call"""
    pos = [[0] * pair.a.nchan, [0] * pair.b.nchan]
    for k in range(ncalls):
        for side, (nd, tr) in enumerate(((pair.a, traffic_a), (pair.b, traffic_b))):
            give = [tr[t][pos[side][t]:pos[side][t] + per_call] for t in range(nd.nchan)]
            for t, n in enumerate(nd.submit(give)):
                pos[side][t] += n
        off = pair.call()
        if hook:
            hook(k, off)
    return pos


# ---------------------------------------------------------------- event tables of the receive rules (one handle, crafted rows)

PEER, OWN = 2, 1                               # the tables' session: the peer is 2, own frames have src 1 and the address is 1
RULES_SUBMIT = 4                               # segments handed over before call 0: they are all in flight when the ACKs arrive


def _pkt(ev, payload, src=PEER, dst=OWN):
    ev.append(("pkt", bytes(payload), src, dst, len(ev) & 0xFF))


def corner_events(rng, acklen):
    """channel 0 of the tables, W = 4: every branch of R1 - R4 at least once"""
    ev = []
    D = lambda seq, n=9, **kw: _pkt(ev, data_bytes(seq, _bytes(rng, n)), **kw)
    A = lambda base, bitmap, n=acklen, **kw: _pkt(ev, ack_bytes(base, bitmap, n), **kw)
    D(255)                                                                # before anything was received there is no old segment: outside
    D(0, 1), D(1, 114)                                                    # in order, the shortest and the longest
    D(3), D(3), D(6), D(7)                                                # held; held already; d = 4 = W and d = 5: outside
    D(2)                                                                  # in order, and the held successor behind it
    D(1), D(0), D(3)                                                      # old duplicates, back = 3, 4 and 1
    _pkt(ev, b"\xD0"), _pkt(ev, b"\x55" + _bytes(rng, 20)), _pkt(ev, b"\x00\x01\x02")                # alien: short, other types
    D(4, src=3), A(0, 0, src=3)                                           # stranger
    _pkt(ev, bytes([DATA, 4])), _pkt(ev, ack_bytes(1, 0, 6)[:5])          # malformed: DATA without a byte, ACK of five bytes
    A(2, 0b1), A(2, 0b1), A(9, 0)                                         # 0, 1 cumulatively and 3 by bit; nothing new; stale
    A(4, 0b111, 6)                                                        # 2 cumulatively, 3 once more (counted once), bits beyond snd_nxt
    A(4, 0, 20)                                                           # everything is acknowledged: a == 0 == snd_nxt - snd_una
    A(5, 0)                                                               # stale: nothing is in flight
    for s in range(4, 10):
        D(s, 30)                                                          # the output ring of four wraps
    D(12), D(11), D(13), D(10)                                            # three held, delivered behind 10
    return ev


def random_events(rng, nseg, W=W, dup=0.2, swap=0.5):
    """segments 0 .. nseg - 1 from the peer, shuffled inside the window, some sent twice, some far outside"""
    order = list(range(nseg))
    for i in range(0, nseg - W, W):
        if rng.random() < swap:
            part = order[i:i + W]
            rng.shuffle(part)
            order[i:i + W] = part
    ev = []
    for s in order:
        _pkt(ev, data_bytes(s, _bytes(rng, int(rng.integers(1, 115)))))
        if rng.random() < dup:
            _pkt(ev, data_bytes(s + int(rng.integers(-6, 7)), _bytes(rng, 5)))
    return ev


def rule_streams(acklen, seed=31):
    """the four channels of the tables, row after row: the corners; random reordering across the sequence byte's wrap; plain datagrams
    and segments of two sources on a session with peer -1; nothing"""
    rng = np.random.default_rng(seed)
    free = []
    for s in range(3):
        _pkt(free, data_bytes(s, _bytes(rng, 40)), src=5 + s)
        _pkt(free, b"\x01" + _bytes(rng, 29), src=9)
    empty = (np.zeros(0, np.uint8), np.zeros((0, KB), np.uint8))
    return [pktref.rows_of(corner_events(rng, acklen)), pktref.rows_of(random_events(rng, 280)), pktref.rows_of(free), empty]


RULES_RING = 512                               # packets of the packet handle's ring under the tables: one call of all rows fits


def rules_node(ring_entries=RULES_RING, E=4, fec=None):
    """the terminal the tables are pushed through: W = 4, an output ring of four, peers 2, 2, whoever, 2; no retransmission in time"""
    return node(OWN, None, 1000, 1000, E=E, ring_entries=ring_entries, fec=fec, peers=[PEER, PEER, None, PEER])


def rules_segments():
    """what channel 0 hands over before call 0: one fragment each, so that the pending ring takes all four at once"""
    rng = np.random.default_rng(32)
    return [[_bytes(rng, 18) for _ in range(RULES_SUBMIT)], [], [], []]


def run_rules(calls, **kw):
    nd = rules_node(**kw)
    segs = rules_segments()
    assert nd.submit(segs) == [RULES_SUBMIT, 0, 0, 0]
    for rows in calls:
        nd.call(rows)
    return nd, segs


# ---------------------------------------------------------------- the sessions both test files run (records path)

LINK_S, LINK_RTO = BURST, 12                   # symbols a call transmits: one largest burst of a plain handle (a queue holds no less); calls until a segment is sent again
LOSS_SEEDS = (5, 7)
LOSS_P = 0.3
LOSS_SEGMENTS, LOSS_CALLS = 7, 150


def loss_pair(seed, fec=None):
    """two terminals, about 30 % of the bursts of both directions dropped -> (pair, A's traffic, B's traffic, calls)"""
    a, b = node(SRC_A, SRC_B, LINK_S, LINK_RTO, fec=fec), node(SRC_B, SRC_A, LINK_S, LINK_RTO, fec=fec)
    return Pair(a, b, Loss(seed=seed, p=LOSS_P)), traffic(100 + seed, LOSS_SEGMENTS), traffic(200 + seed, LOSS_SEGMENTS), LOSS_CALLS


BROKEN_TRIES, BROKEN_CALLS = 3, 60


def broken_pair():
    """nothing A sends arrives: A's sessions break after max_tries transmissions of their first segment; B's segments arrive and are never
    acknowledged, because A's ACKs are lost too, so B's break as well"""
    a, b = (node(s, p, LINK_S, LINK_RTO, max_tries=BROKEN_TRIES) for s, p in ((SRC_A, SRC_B), (SRC_B, SRC_A)))
    return Pair(a, b, Loss(one_way=AB)), traffic(300, 3), traffic(301, 3), BROKEN_CALLS


WRAP_SEGMENTS, WRAP_W, WRAP_RTO, WRAP_CALLS, WRAP_SEED, WRAP_P = 300, 8, 5, 250, 3, 0.06
WRAP_QUEUE = (WRAP_W + 1) * (PRE + FRAME + GAP)                          # a window of one-frame bursts and an ACK: what a call transmits
WRAP_S = WRAP_QUEUE
WRAP_PENDING = 2 * (WRAP_W + 1)


def wrap_pair():
    """300 one-byte segments on channel 0 of four from A to B with W = 8, some bursts lost: the sequence byte passes 255 with segments held out of
    order. A call transmits a whole window, so that the session stays within a few hundred calls."""
    a, b = (node(s, p, WRAP_S, WRAP_RTO, W=WRAP_W, Q=2 * WRAP_W, queue_syms=WRAP_QUEUE, pending=WRAP_PENDING, E=512)
            for s, p in ((SRC_A, SRC_B), (SRC_B, SRC_A)))
    return Pair(a, b, Loss(seed=WRAP_SEED, p=WRAP_P)), [[bytes([i & 0xFF]) for i in range(WRAP_SEGMENTS)], [], [], []], [[]] * 4, WRAP_CALLS


TIGHT_S, TIGHT_RTO, TIGHT_CALLS = 1000, 4, 40


def tight_pair():
    """no loss, but a call transmits a third of a largest burst and a segment is sent again after four calls: the pending ring is full
    when retransmissions and new segments are staged, and what arrives twice is counted"""
    a, b = node(SRC_A, SRC_B, TIGHT_S, TIGHT_RTO, max_tries=20), node(SRC_B, SRC_A, TIGHT_S, TIGHT_RTO, max_tries=20)
    rng = np.random.default_rng(41)
    big = [[_bytes(rng, 114) for _ in range(5)] for _ in range(4)]
    return Pair(a, b), big, traffic(42, 3), TIGHT_CALLS
