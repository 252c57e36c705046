"""Host model of the packet link (include/pirip_hip.h section R), for tests/test_packet*.py.

The wire format and segment(); per receive channel the reassembly rules a - h of the header, the ring of delivered packets and the
counters (Reassembler); per transmit channel the pending ring of whole bursts that send() fills and the offer step that empties it into
section K's queue, kept as a symbol count exactly as tests/rptref.py keeps it (Link). The CRC-32 is zlib's. The row tables are built here
from little scripts of events; tests/test_packet_cpu.py shows that they reach every corner they claim before the device sees them."""
import zlib

import numpy as np

import rptref
import txref

SYNC, BITS = txref.RX_SYNC, txref.RX_BITS
KB = rptref.KB
HEADER = 6
EVERYONE = 0xFF
MAX_FRAMES = txref.REPEAT_MAX_FRAMES

# pirip_pkt_entry (24 bytes, the C layout)
ENTRY = np.dtype([("seq", "<i8"), ("call", "<i4"), ("row", "<i4"), ("length", "<i4"), ("src", "u1"), ("dst", "u1"), ("id", "u1"), ("nfrag", "u1")])
assert ENTRY.itemsize == 24
RX_COUNTERS = ("delivered", "filtered", "foreign", "malformed", "orphan", "incomplete", "crc_fail", "lost")
TX_COUNTERS = ("sent", "refused", "bad", "pending")


def cap(kb):
    return kb - HEADER - 2


def max_packet(kb, max_frags):
    return max_frags * cap(kb) - 4


def nfrag_of(L, kb):
    return -(-(L + 4) // cap(kb))


def segment(packet, src, dst, id, kb, max_frags):
    """the burst of one packet: uint8 [nfrag + 1, 1 + kb] -- control 1, 0, ..., 0 in front of the frames, then the `2` record of zeros.
    ValueError for a length outside 1 .. max_packet."""
    packet = bytes(packet)
    L, c = len(packet), cap(kb)
    if not 1 <= L <= max_packet(kb, max_frags):
        raise ValueError("length %d outside 1 .. %d" % (L, max_packet(kb, max_frags)))
    body = packet + zlib.crc32(packet).to_bytes(4, "little")
    n = nfrag_of(L, kb)
    rec = np.zeros((n + 1, 1 + kb), np.uint8)
    for f in range(n):
        part = body[f * c:(f + 1) * c]
        rec[f, 0] = 1 if f == 0 else 0
        rec[f, 1:1 + HEADER] = [src, dst, id & 0xFF, f, n, len(part)]
        rec[f, 1 + HEADER:1 + HEADER + len(part)] = np.frombuffer(part, np.uint8)
    rec[n, 0] = 2
    return rec


# ---------------------------------------------------------------- reassembly

class Reassembler:
    def __init__(self, nrx, kb, max_frags, filt, address, ring_entries):
        self.nrx, self.kb, self.max_frags, self.filt, self.address, self.E = nrx, kb, max_frags, filt, address, ring_entries
        self.reset()

    def reset(self):
        self.n = 0
        self.open = [None] * self.nrx                                        # dict src, id, nfrag, next, body
        self.entries = [[] for _ in range(self.nrx)]                          # every (entry, bytes) ever delivered
        self.c = {k: np.zeros(self.nrx, np.int64) for k in RX_COUNTERS}
        self.ev = dict(cut_inside_packet=0, sync_only_inside=0, foreign_inside=0, bits_without_sync=0, short_body=0, wraps=0,
                       max_rows=0, ids=set(), bad_headers=set(), interrupted_by_first=0, duplicate=0, other_src=0, no_open=0)

    def _close(self, c):
        if self.open[c] is not None:
            self.open[c] = None
            self.c["incomplete"][c] += 1

    def call(self, rows):
        """call n: rows[c] = (status [nf], payload [nf, kb])"""
        C = cap(self.kb)
        for c, (st, pl) in enumerate(rows):
            nf = len(st)
            self.ev["max_rows"] = max(self.ev["max_rows"], nf)
            self.ev["cut_inside_packet"] += self.open[c] is not None
            for f in range(nf):
                v = int(st[f])
                src, dst, pid, idx, nfrag, ln = (int(x) for x in pl[f][:HEADER])
                if not v & SYNC:                                              # a
                    self._close(c)
                if v & BITS and self.filt is not None and src == self.filt:   # b
                    v &= ~BITS
                    self.c["filtered"][c] += 1
                if not v & BITS:                                              # c
                    self.ev["sync_only_inside"] += self.open[c] is not None
                    continue
                self.ev["bits_without_sync"] += not v & SYNC
                bad = [not 1 <= nfrag <= self.max_frags, idx >= nfrag, not 1 <= ln <= C, idx < nfrag - 1 and ln != C]
                if any(bad):                                                  # d
                    self.ev["bad_headers"].add(bad.index(True))
                    self._close(c)
                    self.c["malformed"][c] += 1
                    continue
                if self.address is not None and dst not in (self.address, EVERYONE):           # e
                    self.ev["foreign_inside"] += self.open[c] is not None
                    self.c["foreign"][c] += 1
                    continue
                o = self.open[c]
                if idx == 0:                                                  # f
                    self.ev["interrupted_by_first"] += o is not None
                    self._close(c)
                    o = self.open[c] = dict(src=src, id=pid, nfrag=nfrag, next=0, body=b"")
                elif not (o is not None and (o["src"], o["id"], o["nfrag"], o["next"]) == (src, pid, nfrag, idx)):              # g
                    if o is None:
                        self.ev["no_open"] += 1
                    elif (o["src"], o["id"], o["nfrag"]) != (src, pid, nfrag):
                        self.ev["other_src"] += o["src"] != src
                    elif idx == o["next"] - 1:
                        self.ev["duplicate"] += 1
                    self._close(c)
                    self.c["orphan"][c] += 1
                    continue
                o["body"] += bytes(pl[f][HEADER:HEADER + ln])
                o["next"] += 1
                self.ev["ids"].add(pid)
                if o["next"] < o["nfrag"]:
                    continue
                self.open[c] = None                                           # h
                body = o["body"]
                if len(body) < 5 or zlib.crc32(body[:-4]) != int.from_bytes(body[-4:], "little"):
                    self.ev["short_body"] += len(body) < 5
                    self.c["crc_fail"][c] += 1
                    continue
                e = np.zeros((), ENTRY)
                e["seq"], e["call"], e["row"], e["length"] = len(self.entries[c]), self.n, f, len(body) - 4
                e["src"], e["dst"], e["id"], e["nfrag"] = src, dst, pid, nfrag
                self.entries[c].append((e, body[:-4]))
                self.c["delivered"][c] += 1
            self.c["lost"][c] = max(len(self.entries[c]) - self.E, 0)
            self.ev["wraps"] += len(self.entries[c]) > self.E
        self.n += 1

    def packets(self, c, max_entries=None):
        """what get_packets returns: the newest min(delivered, ring_entries, max) entries, oldest first, and their bytes"""
        n = min(len(self.entries[c]), self.E if max_entries is None else min(self.E, max_entries))
        kept = self.entries[c][len(self.entries[c]) - n:]
        return np.array([e for e, _ in kept], dtype=ENTRY).reshape(n), [b for _, b in kept]

    def counters(self):
        return dict(self.c)


def same_but_call_and_row(a, b):
    """two entry arrays equal in every field except call and row"""
    names = [n for n in ENTRY.names if n not in ("call", "row")]
    return a.shape == b.shape and all(a[n].tobytes() == b[n].tobytes() for n in names)


# ---------------------------------------------------------------- row tables

FILT, ADDR, MAX_FRAGS, RING = 1, 7, 5, 4      # the tables' link: own frames have src 1, the address is 7, packets of up to 116 bytes


def rows_of(events, kb=KB):
    """a channel's rows from a script of events:
         ("pkt", bytes, src, dst, id[, max_frags])   the packet's frames, each SYNC | BITS
         ("frames", records, status)                  frames of segment()'s records (without the end record) with this status
         ("row", status, header bytes)                one row, its payload zeros behind the header
         ("gap",)                                     one row without SYNC and BITS"""
    st, pl = [], []
    for ev in events:
        if ev[0] == "pkt":
            rec = segment(ev[1], ev[2], ev[3], ev[4], kb, ev[5] if len(ev) > 5 else MAX_FRAGS)
            for r in rec[:-1]:
                st.append(SYNC | BITS)
                pl.append(r[1:].copy())
        elif ev[0] == "frames":
            for r in ev[1]:
                st.append(ev[2])
                pl.append(np.asarray(r[1:], np.uint8).copy())
        elif ev[0] == "row":
            p = np.zeros(kb, np.uint8)
            p[:len(ev[2])] = ev[2]
            st.append(ev[1])
            pl.append(p)
        else:
            st.append(0)
            pl.append(np.zeros(kb, np.uint8))
    return np.array(st, np.uint8), np.array(pl, np.uint8).reshape(len(st), kb)


def _bytes(rng, n):
    return rng.integers(0, 256, n).astype(np.uint8).tobytes()


def corner_events(rng, kb=KB):
    """channel 0 of the tables: every rule of the header at least once"""
    C, B = cap(kb), SYNC | BITS
    mp = max_packet(kb, MAX_FRAGS)
    ev = [("pkt", _bytes(rng, L), 2, ADDR, i) for i, L in enumerate((1, C - 4, C - 3, C))]            # 1, 1, 2, 2 fragments
    ev += [("pkt", _bytes(rng, mp), 2, EVERYONE, 254), ("pkt", _bytes(rng, 30), 2, ADDR, 255), ("pkt", _bytes(rng, 30), 2, ADDR, 0), ("gap",)]
    ev += [("pkt", _bytes(rng, 40), FILT, ADDR, 9)]                            # the terminal's own: filtered
    ev += [("pkt", _bytes(rng, 40), 2, 9, 10)]                                 # for somebody else: foreign
    three = segment(_bytes(rng, 60), 3, ADDR, 20, kb, MAX_FRAGS)               # 64 bytes of body: three fragments
    assert three.shape[0] == 4
    # bad headers: nfrag 0, nfrag above max_frags, idx >= nfrag, len 0, len above cap, a short fragment that is not the last; the last
    # of them in the middle of a packet
    for hdr in ([2, ADDR, 11, 0, 0, C], [2, ADDR, 11, 0, MAX_FRAGS + 1, C], [2, ADDR, 11, 2, 2, C], [2, ADDR, 11, 0, 1, 0], [2, ADDR, 11, 0, 1, C + 1]):
        ev.append(("row", B, hdr))
    ev += [("frames", three[:1], B), ("row", B, [3, ADDR, 20, 1, 3, C - 1])]
    # a new first fragment interrupts; a duplicate fragment; a fragment of another sender in mid-packet; a fragment with nothing open
    ev += [("frames", three[:2], B), ("pkt", _bytes(rng, 50), 2, ADDR, 21)]
    ev += [("frames", three[:2], B), ("frames", three[1:2], B), ("frames", three[2:3], B)]
    other = three[1:2].copy()
    other[0, 1] = 4
    ev += [("frames", three[:1], B), ("frames", other, B)]
    # a flipped body byte; a body of fewer than five bytes
    flipped = segment(_bytes(rng, 45), 2, ADDR, 22, kb, MAX_FRAGS)
    flipped[1, 1 + HEADER + 3] ^= 0x10
    ev += [("frames", flipped[:-1], B), ("row", B, [2, ADDR, 23, 0, 1, 4, 1, 2, 3, 4])]
    # a row without SYNC closes; a row with SYNC alone and a foreign row in the middle change nothing
    ev += [("frames", three[:2], B), ("gap",), ("frames", three[2:3], B)]
    ev += [("frames", three[:1], B), ("row", SYNC, []), ("row", B, [2, 9, 30, 0, 1, 5]), ("frames", three[1:3], B)]
    # BITS without SYNC: closes what is open, then the row is looked at like any other
    ev += [("frames", three[:1], B), ("frames", segment(_bytes(rng, 7), 5, ADDR, 31, kb, MAX_FRAGS)[:1], BITS)]
    return ev


def random_events(rng, npackets, kb=KB, damage=0.15):
    """packets of every length from senders 2 .. 4 with ids that count up, some of them damaged: a fragment missing, doubled or flipped"""
    ev, mp = [], max_packet(kb, MAX_FRAGS)
    for i in range(npackets):
        rec = segment(_bytes(rng, int(rng.integers(1, mp + 1))), int(rng.integers(2, 5)), ADDR if rng.random() < 0.7 else EVERYONE, i, kb, MAX_FRAGS)[:-1]
        if rng.random() < damage:
            k = int(rng.integers(0, rec.shape[0]))
            how = int(rng.integers(0, 3))
            if how == 0:
                rec = np.delete(rec, k, axis=0)
            elif how == 1:
                rec = np.insert(rec, k, rec[k], axis=0)
            else:
                rec[k, 1 + HEADER] ^= 0x01
        ev.append(("frames", rec, SYNC | BITS))
        if rng.random() < 0.3:
            ev.append(("gap",))
    return ev


def streams(seed=11):
    """the three channels of the tables, row after row"""
    rng = np.random.default_rng(seed)
    return [rows_of(corner_events(rng)), rows_of(random_events(rng, 40)), rows_of(random_events(rng, 6, damage=0.0))]


def cut(chans, seed, ncalls):
    """per-channel rows cut into ncalls consecutive calls (some of them empty): list over calls of [(status, payload)] per channel"""
    rng = np.random.default_rng(seed)
    cuts = [np.concatenate([[0], np.sort(rng.integers(0, len(st) + 1, ncalls - 1)), [len(st)]]) for st, _ in chans]
    return [[(st[cuts[c][p]:cuts[c][p + 1]], pl[cuts[c][p]:cuts[c][p + 1]]) for c, (st, pl) in enumerate(chans)] for p in range(ncalls)]


def one_call(chans):
    return [[(st, pl) for st, pl in chans]]


def between_fragments(chans):
    """two calls, cut behind the first fragment of channel 0's first packet of several fragments"""
    st, pl = chans[0]
    k = next(f for f in range(len(st)) if pl[f, 4] > 1 and pl[f, 3] == 0) + 1
    return [[(s[:k], p[:k]) for s, p in chans], [(s[k:], p[k:]) for s, p in chans]]


def big_call(seed=12, rows=4096):
    """one call of 4096, 4095 and 1 rows: packets back to back"""
    rng = np.random.default_rng(seed)
    out = []
    for n in (rows, rows - 1, 1):
        st, pl = rows_of(random_events(rng, n // 2 + 1))
        out.append((st[:n], pl[:n]))
    return [out]


def run_rows(calls, ring_entries=RING, filt=FILT, address=ADDR, max_frags=MAX_FRAGS, kb=KB):
    m = Reassembler(len(calls[0]), kb, max_frags, filt, address, ring_entries)
    for rows in calls:
        m.call(rows)
    return m


# ---------------------------------------------------------------- send and offer

class Link:
    """the transmit side: send() into the pending rings, call() = the offer step and the S symbols section K's process dequeues"""

    def __init__(self, ntx, src, kb, max_frags, pending, queue_syms, S, pre, frame, gap):
        self.ntx, self.src, self.kb, self.max_frags, self.pending = ntx, src, kb, max_frags, pending
        self.queue_syms, self.S, self.pre, self.frame = queue_syms, S, pre, frame
        self.gap = [gap] * ntx if np.isscalar(gap) else list(gap)
        self.reset()

    def reset(self):
        self.n = 0
        self.ring = [[] for _ in range(self.ntx)]
        self.head, self.tail, self.queued = [0] * self.ntx, [0] * self.ntx, [0] * self.ntx
        self.c = {k: np.zeros(self.ntx, np.int64) for k in ("sent", "refused", "bad")}
        self.ev = dict(wraps=0, blocked=0, max_bursts_per_offer=0)

    def send(self, packets):
        """packets[t]: list of (bytes, dst) -> taken [ntx]"""
        taken = []
        for t, q in enumerate(packets):
            k = 0
            for b, dst in q:
                if not 1 <= len(b) <= max_packet(self.kb, self.max_frags):
                    self.c["bad"][t] += 1
                    break
                rec = segment(b, self.src, dst, int(self.c["sent"][t]) % 256, self.kb, self.max_frags)
                if rec.shape[0] > self.pending - (self.tail[t] - self.head[t]):
                    self.c["refused"][t] += 1
                    break
                self.ev["wraps"] += self.tail[t] % self.pending + rec.shape[0] > self.pending
                self.ring[t].append(rec)
                self.tail[t] += rec.shape[0]
                self.c["sent"][t] += 1
                k += 1
            taken.append(k)
        return taken

    def call(self):
        """call n -> offered [ntx] record arrays"""
        offered = []
        for t in range(self.ntx):
            take = []
            while self.ring[t]:
                b = self.ring[t][0]
                cost = rptref.burst_cost(b.shape[0] - 1, self.pre, self.frame, self.gap[t])
                if cost > self.queue_syms - self.queued[t]:
                    self.ev["blocked"] += 1
                    break
                self.ring[t].pop(0)
                self.queued[t] += cost
                self.head[t] += b.shape[0]
                take.append(b)
            self.ev["max_bursts_per_offer"] = max(self.ev["max_bursts_per_offer"], len(take))
            offered.append(np.concatenate(take) if take else np.zeros((0, 1 + self.kb), np.uint8))
            self.queued[t] -= min(self.S, self.queued[t])
        self.n += 1
        return offered

    def counters(self):
        out = dict(self.c)
        out["pending"] = np.array([t - h for h, t in zip(self.head, self.tail)], np.int64)
        return out


def send_script(kb=KB, max_frags=MAX_FRAGS, seed=13):
    """what the send tests hand over on four channels, call by call: list over calls of packets[t] = [(bytes, dst)]. With a pending ring
    of 2 * (max_frags + 1) records and a queue of one largest burst, channel 0 finds its ring full (a prefix is taken), channel 1 hands
    over a bad length in front of a good packet, channel 2 a burst that waits for the queue, channel 3 nothing at first."""
    rng = np.random.default_rng(seed)
    mp = max_packet(kb, max_frags)
    P = lambda L, dst=ADDR: (_bytes(rng, L), dst)
    calls = [[[P(mp), P(mp), P(mp)], [P(10), P(mp + 1), P(20)], [P(mp), P(cap(kb))], []],
             [[], [P(20), (b"", ADDR)], [P(1)], [P(300 if mp >= 300 else mp // 2, EVERYONE)]]]
    calls += [[[], [], [], []] for _ in range(3)]
    calls += [[[P(5)], [], [P(cap(kb))], [P(1), P(2), P(3)]]]                  # channel 2's burst lies across the ring's wrap
    return calls
