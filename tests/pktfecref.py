"""Host model of the packet link's parity fragments (include/pirip_hip.h section R), for tests/test_packet_fec*.py.

GF(2^8) with the polynomial 0x11D, its multiply defined bit by bit; the Cauchy matrix; r_of; pad; segment_fec(); per receive channel
the rules A - G of the header (ReassemblerFec, with an `ev` dict of the corners reached). What parity fragments do not change -- the
sizes, the entry ring, the event scripts' form, the cuts into calls -- is tests/pktref.py's. Nothing here is taken from the library: the
product is the schoolbook one, the inverse a search, the solve plain Gauss-Jordan with pivoting over Python integers."""
import zlib

import numpy as np

import pktref
from pktref import BITS, ENTRY, EVERYONE, HEADER, KB, SYNC, cap, max_packet, nfrag_of  # noqa: F401

POLY = 0x11D
FEC_COUNTERS = ("recovered", "repaired", "duplicate", "surplus")


def gf_mul(a, b):
    """a(x) b(x) mod x^8 + x^4 + x^3 + x^2 + 1, bit by bit"""
    p = 0
    for k in range(8):
        if (b >> k) & 1:
            p ^= a << k
    for k in range(14, 7, -1):
        if (p >> k) & 1:
            p ^= POLY << (k - 8)
    return p


MUL = np.array([[gf_mul(a, b) for b in range(256)] for a in range(256)], np.uint8)          # the model's own table, for speed
INV = np.zeros(256, np.uint8)
for _a in range(1, 256):
    INV[_a] = next(b for b in range(1, 256) if MUL[_a, b] == 1)


def gf_inv(a):
    return int(INV[a])


def cauchy(R, max_frags):
    """C[j][i] = inverse(j XOR (R + i)), uint8 [R, max_frags]"""
    return np.array([[gf_inv(j ^ (R + i)) for i in range(max_frags)] for j in range(R)], np.uint8)


def r_of(k, R, pct):
    return max(1, min(R, -(-k * pct // 100)))


def pad(id, q):
    x = (((id << 16) | q) * 2654435761) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 2246822519) & 0xFFFFFFFF
    x ^= x >> 13
    return x >> 24


def parity_of(bodies, R, r, max_frags):
    """bodies uint8 [k, cap] -> the r parity bodies uint8 [r, cap]"""
    k = bodies.shape[0]
    Cm = cauchy(R, max_frags)
    out = np.zeros((r, bodies.shape[1]), np.uint8)
    for j in range(r):
        for i in range(k):
            out[j] ^= MUL[Cm[j, i], bodies[i]]
    return out


def segment_fec(packet, src, dst, id, kb, max_frags, R, pct):
    """the burst of one packet of an FEC handle: uint8 [k + r + 1, 1 + kb] -- control 1, 0, ..., 0 in front of the k data and r parity
    frames, then the `2` record of zeros. ValueError for a length outside 1 .. max_packet."""
    packet = bytes(packet)
    L, c = len(packet), cap(kb)
    if not 1 <= L <= max_packet(kb, max_frags):
        raise ValueError("length %d outside 1 .. %d" % (L, max_packet(kb, max_frags)))
    k = nfrag_of(L, kb)
    r = r_of(k, R, pct)
    body = packet + zlib.crc32(packet).to_bytes(4, "little")
    body += bytes(pad(id & 0xFF, q) for q in range(L + 4, k * c))
    bodies = np.frombuffer(body, np.uint8).reshape(k, c)
    lastlen = L + 4 - (k - 1) * c
    rec = np.zeros((k + r + 1, 1 + kb), np.uint8)
    for f in range(k + r):
        rec[f, 0] = 1 if f == 0 else 0
        rec[f, 1:1 + HEADER] = [src, dst, id & 0xFF, f, k, c if f < k - 1 else lastlen]
    rec[:k, 1 + HEADER:1 + HEADER + c] = bodies
    rec[k:k + r, 1 + HEADER:1 + HEADER + c] = parity_of(bodies, R, r, max_frags)
    rec[k + r, 0] = 2
    return rec


def solve(A, S):
    """A uint8 [m, m] regular, S uint8 [m, n] -> X with A X = S, by Gauss-Jordan with a pivot search"""
    m = A.shape[0]
    A, S = A.copy(), S.copy()
    for c in range(m):
        p = next(a for a in range(c, m) if A[a, c])
        A[[c, p]], S[[c, p]] = A[[p, c]], S[[p, c]]
        inv = gf_inv(int(A[c, c]))
        A[c], S[c] = MUL[inv, A[c]], MUL[inv, S[c]]
        for a in range(m):
            if a != c and A[a, c]:
                fa = int(A[a, c])
                A[a] ^= MUL[fa, A[c]]
                S[a] ^= MUL[fa, S[c]]
    assert np.array_equal(A, np.eye(m, dtype=np.uint8))
    return S


def decode(frags, k, R, max_frags):
    """frags: dict idx -> uint8 [cap] of exactly k fragments of a packet of k data fragments -> the k data bodies uint8 [k, cap]"""
    assert len(frags) == k
    c = len(next(iter(frags.values())))
    Cm = cauchy(R, max_frags)
    D = np.zeros((k, c), np.uint8)
    have = [i for i in range(k) if i in frags]
    miss = [i for i in range(k) if i not in frags]
    rows = sorted(i - k for i in frags if i >= k)
    assert len(rows) == len(miss)
    for i in have:
        D[i] = frags[i]
    if miss:
        S = np.zeros((len(rows), c), np.uint8)
        for a, p in enumerate(rows):
            S[a] = frags[k + p]
            for i in have:
                S[a] ^= MUL[Cm[p, i], D[i]]
        D[miss] = solve(Cm[np.ix_(rows, miss)], S)
    return D


# ---------------------------------------------------------------- reassembly

class ReassemblerFec:
    def __init__(self, nrx, kb, max_frags, filt, address, ring_entries, R, pct):
        self.nrx, self.kb, self.max_frags, self.filt, self.address, self.E, self.R, self.pct = nrx, kb, max_frags, filt, address, ring_entries, R, pct
        self.reset()

    def reset(self):
        self.n = 0
        self.st = [dict(phase=0, key=None, frags={}, lastlen=0) for _ in range(self.nrx)]       # phase 0 none, 1 collecting, 2 closed
        self.entries = [[] for _ in range(self.nrx)]
        self.c = {k: np.zeros(self.nrx, np.int64) for k in pktref.RX_COUNTERS + FEC_COUNTERS}
        self.ev = dict(cut_inside_packet=0, no_sync_inside=0, bits_without_sync=0, sync_only_inside=0, foreign_inside=0, bad_headers=set(),
                       lastlen_conflict=0, lost_last=0, lost_first=0, parity_first=0, surplus_after_delivery=0, surplus_after_crc_fail=0,
                       crc_fail_decoded=0, crc_fail_plain=0, other_src=0, ids=set(), max_m=0, wraps=0, max_rows=0, short_body=0,
                       plain_burst=0)

    def call(self, rows):
        """call n: rows[c] = (status [nf], payload [nf, kb])"""
        C = cap(self.kb)
        for c, (st, pl) in enumerate(rows):
            s = self.st[c]
            nf = len(st)
            self.ev["max_rows"] = max(self.ev["max_rows"], nf)
            self.ev["cut_inside_packet"] += s["phase"] == 1
            for f in range(nf):
                v = int(st[f])
                src, dst, pid, idx, nfrag, ln = (int(x) for x in pl[f][:HEADER])
                if not v & SYNC:                                              # A
                    self.ev["no_sync_inside"] += s["phase"] == 1
                    self.ev["bits_without_sync"] += bool(v & BITS)
                    continue
                if v & BITS and self.filt is not None and src == self.filt:   # B
                    v &= ~BITS
                    self.c["filtered"][c] += 1
                if not v & BITS:                                              # C
                    self.ev["sync_only_inside"] += s["phase"] == 1
                    continue
                key = (src, pid, nfrag)
                same = s["phase"] != 0 and s["key"] == key
                r = r_of(nfrag, self.R, self.pct) if 1 <= nfrag <= self.max_frags else 0
                states = idx >= nfrag - 1
                bad = [not 1 <= nfrag <= self.max_frags, idx >= nfrag + r, not 1 <= ln <= C, idx < nfrag - 1 and ln != C,
                       same and s["phase"] == 1 and states and s["lastlen"] != 0 and ln != s["lastlen"]]
                if any(bad):                                                  # D
                    self.ev["bad_headers"].add(bad.index(True))
                    self.ev["lastlen_conflict"] += bad.index(True) == 4
                    self.c["malformed"][c] += 1
                    continue
                if self.address is not None and dst not in (self.address, EVERYONE):           # E
                    self.ev["foreign_inside"] += s["phase"] == 1
                    self.c["foreign"][c] += 1
                    continue
                if same and s["phase"] == 2:                                  # F
                    self.ev["surplus_after_delivery" if s["delivered"] else "surplus_after_crc_fail"] += 1
                    self.c["surplus"][c] += 1
                    continue
                if same and idx in s["frags"]:
                    self.c["duplicate"][c] += 1
                    continue
                if not same:
                    if s["phase"] == 1:
                        self.ev["other_src"] += s["key"][0] != src
                        self.c["incomplete"][c] += 1
                    s.update(phase=1, key=key, frags={}, lastlen=0)
                    self.ev["parity_first"] += idx >= nfrag
                s["frags"][idx] = np.array(pl[f][HEADER:HEADER + C], np.uint8)
                if states:
                    s["lastlen"] = ln
                self.ev["ids"].add(pid)
                if len(s["frags"]) < nfrag:
                    continue
                s["phase"], s["delivered"] = 2, False                        # G
                m = sum(1 for i in range(nfrag) if i not in s["frags"])
                self.ev["max_m"] = max(self.ev["max_m"], m)
                self.ev["lost_last"] += nfrag - 1 not in s["frags"]
                self.ev["lost_first"] += 0 not in s["frags"]
                self.ev["plain_burst"] += m == 0 and idx == nfrag - 1
                body = decode(s["frags"], nfrag, self.R, self.max_frags).tobytes()
                L = (nfrag - 1) * C + s["lastlen"] - 4
                if L < 1 or zlib.crc32(body[:L]) != int.from_bytes(body[L:L + 4], "little"):
                    self.ev["short_body"] += L < 1
                    self.ev["crc_fail_decoded" if m else "crc_fail_plain"] += 1
                    self.c["crc_fail"][c] += 1
                    continue
                s["delivered"] = True
                e = np.zeros((), ENTRY)
                e["seq"], e["call"], e["row"], e["length"] = len(self.entries[c]), self.n, f, L
                e["src"], e["dst"], e["id"], e["nfrag"] = src, dst, pid, nfrag
                self.entries[c].append((e, body[:L]))
                self.c["delivered"][c] += 1
                if m:
                    self.c["recovered"][c] += 1
                    self.c["repaired"][c] += m
            self.c["lost"][c] = max(len(self.entries[c]) - self.E, 0)
            self.ev["wraps"] += len(self.entries[c]) > self.E
        self.n += 1

    packets = pktref.Reassembler.packets

    def counters(self):
        """get_counters' [nrx] part"""
        return {k: self.c[k] for k in pktref.RX_COUNTERS}

    def fec_counters(self):
        return {k: self.c[k] for k in FEC_COUNTERS}


# ---------------------------------------------------------------- row tables

FILT, ADDR, RING = pktref.FILT, pktref.ADDR, pktref.RING
SHAPES = {"small": (5, 3, 50), "one": (1, 1, 100), "wide": (84, 16, 100)}         # max_frags, R, parity_pct


def _bytes(rng, n):
    return rng.integers(0, 256, n).astype(np.uint8).tobytes()


def burst(rng, L, src, dst, id, shape, kb=KB):
    """the frames of a packet of L random bytes (without the end record)"""
    mf, R, pct = shape
    return segment_fec(_bytes(rng, L), src, dst, id, kb, mf, R, pct)[:-1]


def rows_of(events, kb=KB):
    """pktref.rows_of's events ("frames", "row", "gap"), and ("lose", records, indices): the records but those at the indices, each
    SYNC | BITS"""
    ev2 = []
    for ev in events:
        if ev[0] == "lose":
            keep = [i for i in range(len(ev[1])) if i not in set(ev[2])]
            ev2.append(("frames", ev[1][keep], SYNC | BITS))
        else:
            ev2.append(ev)
    return pktref.rows_of(ev2, kb)


def corner_events(rng, kb=KB):
    """channel 0 of the small shape's tables: every rule of the header at least once (shape (5, 3, 50): r = 1, 1, 2, 2, 3)"""
    sh, C, B = SHAPES["small"], cap(kb), SYNC | BITS
    mp = max_packet(kb, sh[0])
    ev = []
    for i, L in enumerate((1, C - 4, C - 3, C, mp)):                           # whole bursts: the parity behind the packet is surplus
        ev.append(("frames", burst(rng, L, 2, ADDR, i, sh), B))
    p3 = burst(rng, 60, 3, ADDR, 20, sh)                                      # k = 3, r = 2; 64 body bytes: lastlen 16
    assert p3.shape[0] == 5 and p3[2, 6] == 16 and p3[3, 6] == 16
    ev += [("lose", p3, [2])]                                                # the last data fragment lost: lastlen from the parity
    p3b = burst(rng, 60, 3, ADDR, 21, sh)
    ev += [("lose", p3b, [0])]                                               # fragment 0 lost
    p3c = burst(rng, 61, 3, EVERYONE, 22, sh)
    ev += [("frames", p3c[[4, 3, 1]], B), ("frames", p3c[[0, 2]], B)]         # parity first; then two fragments of surplus
    p3d = burst(rng, 62, 3, ADDR, 23, sh)
    ev += [("frames", p3d[[0, 0, 1]], B), ("lose", p3d, [0, 1])]              # a duplicate; 2 completes the packet, 3 and 4 are surplus
    # ids 254, 255, 0 with a loss each; an own packet (filtered); a packet for somebody else (foreign), one of its frames in mid-packet
    for i in (254, 255, 0):
        ev += [("lose", burst(rng, 30, 2, ADDR, i, sh), [i & 1])]
    ev += [("frames", burst(rng, 40, FILT, ADDR, 9, sh), B), ("frames", burst(rng, 40, 2, 9, 10, sh), B)]
    # a flipped body byte without a decode (then the parity is surplus after a crc_fail) and with one
    fl = burst(rng, 45, 2, ADDR, 30, sh).copy()
    fl[1, 1 + HEADER + 3] ^= 0x10
    ev += [("frames", fl, B)]
    fl2 = burst(rng, 45, 2, ADDR, 31, sh).copy()
    fl2[2, 1 + HEADER + 5] ^= 0x01                                            # k = 3; a padding byte of the last data fragment: the parity covers it
    ev += [("lose", fl2, [0])]
    # bad headers: nfrag 0, nfrag above max_frags, idx >= nfrag + r, len 0, len above cap, a short data fragment that is not the last,
    # a parity fragment of len 0 -- the last two in the middle of a packet, which they leave alone
    for hdr in ([2, ADDR, 40, 0, 0, C], [2, ADDR, 40, 0, sh[0] + 1, C], [2, ADDR, 40, 3, 2, C], [2, ADDR, 40, 0, 1, 0], [2, ADDR, 40, 0, 1, C + 1]):
        ev.append(("row", B, hdr))
    p3e = burst(rng, 60, 3, ADDR, 41, sh)
    ev += [("frames", p3e[:1], B), ("row", B, [3, ADDR, 41, 1, 3, C - 1]), ("row", B, [3, ADDR, 41, 4, 3, 0])]
    # ... a conflicting lastlen: parity 3 states 16, a forged fragment 2 states 15 (malformed), then fragments 1 and 4 complete the packet
    ev += [("frames", p3e[3:4], B), ("row", B, [3, ADDR, 41, 2, 3, 15]), ("frames", p3e[[1, 4]], B)]
    # a row without SYNC in mid-packet changes nothing, with BITS or without; SYNC alone and a foreign row neither
    p3f = burst(rng, 58, 4, ADDR, 42, sh)
    ev += [("frames", p3f[:1], B), ("gap",), ("frames", p3f[1:2], BITS), ("row", SYNC, []), ("row", B, [2, 9, 30, 0, 1, 5]), ("frames", p3f[2:4], B)]
    # two senders interleaved throw each other out; a packet left open is closed by the next one
    pa, pb = burst(rng, 50, 5, ADDR, 50, sh), burst(rng, 50, 6, ADDR, 50, sh)
    ev += [("frames", pa[:2], B), ("frames", pb[:2], B), ("frames", pa[2:], B), ("frames", pb[2:], B)]
    # a plain sender's burst, whole; and one body of fewer than five bytes
    ev += [("frames", pktref.segment(_bytes(rng, 70), 7, ADDR, 60, kb, sh[0])[:-1], B), ("row", B, [2, ADDR, 61, 0, 1, 4, 1, 2, 3, 4])]
    return ev


def random_events(rng, npackets, shape, kb=KB, losses=None, damage=0.3):
    """packets of every length from senders 2 .. 4 with ids that count up; of each burst `losses` fragments (default: up to r + 1 of them,
    r + 1 seldom) are lost, and some bursts have a fragment doubled or flipped"""
    ev, mp = [], max_packet(kb, shape[0])
    for i in range(npackets):
        rec = burst(rng, int(rng.integers(1, mp + 1)), int(rng.integers(2, 5)), ADDR if rng.random() < 0.7 else EVERYONE, i, shape, kb)
        k = int(rec[0, 5])
        r = rec.shape[0] - k
        n = losses if losses is not None else int(rng.integers(0, r + 1)) if rng.random() < 0.9 else r + 1
        lose = rng.choice(rec.shape[0], n, replace=False).tolist()
        rec = rec[[i for i in range(rec.shape[0]) if i not in lose]]
        if len(rec) and rng.random() < damage:
            j = int(rng.integers(0, rec.shape[0]))
            if rng.random() < 0.5:
                rec = np.insert(rec, j, rec[j], axis=0)
            else:
                rec = rec.copy()
                rec[j, 1 + HEADER] ^= 0x01
        ev.append(("frames", rec, SYNC | BITS))
        if rng.random() < 0.3:
            ev.append(("gap",))
    return ev


def streams(name, seed=21):
    """the channels of a shape's tables, row after row"""
    rng = np.random.default_rng(seed)
    sh = SHAPES[name]
    if name == "small":
        return [rows_of(corner_events(rng)), rows_of(random_events(rng, 40, sh)), rows_of(random_events(rng, 6, sh, losses=0, damage=0.0))]
    if name == "one":                                                         # 1-byte packets whose only data fragment is lost
        ev = [("lose", burst(rng, 1, 2, ADDR, i, sh), [0] if i % 3 else []) for i in range(12)]
        return [rows_of(ev), rows_of(random_events(rng, 10, sh))]
    # wide: full-length packets with all 16 erasures, data and parity mixed; and random ones
    ev = []
    for i in range(3):
        rec = burst(rng, max_packet(KB, sh[0]) - i, 2, ADDR, i, sh)
        assert rec.shape[0] == 100
        ev.append(("lose", rec, rng.choice(100, 16, replace=False).tolist() if i else [0, 83] + list(range(20, 30)) + [84, 90, 98, 99]))
    return [rows_of(ev), rows_of(random_events(rng, 4, sh))]


def big_call(seed=22, rows=4096):
    """one call of 4096, 4095 and 1 rows of the small shape: bursts back to back"""
    rng = np.random.default_rng(seed)
    out = []
    for n in (rows, rows - 1, 1):
        st, pl = rows_of(random_events(rng, n // 3 + 1, SHAPES["small"]))
        assert len(st) >= n
        out.append((st[:n], pl[:n]))
    return [out]


def between_fragments(chans):
    """two calls, cut between two fragments of channel 0's first packet that is still open there"""
    st, pl = chans[0]
    same = [f for f in range(1, len(st)) if tuple(pl[f, [0, 2, 4]]) == tuple(pl[f - 1, [0, 2, 4]])]
    k = next((f for f in same if pl[f, 4] > 1 and pl[f - 1, 3] == 0), same[0])          # (a packet of one fragment is never open: its burst)
    return [[(s[:k], p[:k]) for s, p in chans], [(s[k:], p[k:]) for s, p in chans]]


def run_rows(calls, shape, ring_entries=RING, filt=FILT, address=ADDR, kb=KB):
    mf, R, pct = shape
    m = ReassemblerFec(len(calls[0]), kb, mf, filt, address, ring_entries, R, pct)
    for rows in calls:
        m.call(rows)
    return m


# ---------------------------------------------------------------- send and offer

class LinkFec(pktref.Link):
    """pktref.Link with bursts of k + r frames: one burst is placed whole, k + r + 1 records of room, else refused"""

    def __init__(self, ntx, src, kb, shape, pending, queue_syms, S, pre, frame, gap):
        self.R, self.pct = shape[1], shape[2]
        super().__init__(ntx, src, kb, shape[0], pending, queue_syms, S, pre, frame, gap)

    def send(self, packets):
        taken = []
        for t, q in enumerate(packets):
            k = 0
            for b, dst in q:
                if not 1 <= len(b) <= max_packet(self.kb, self.max_frags):
                    self.c["bad"][t] += 1
                    break
                rec = segment_fec(b, self.src, dst, int(self.c["sent"][t]) % 256, self.kb, self.max_frags, self.R, self.pct)
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


def send_script(kb=KB, shape=SHAPES["small"], seed=23):
    """four channels, call by call, on a pending ring of 2 * (max_frags + r + 1) = 18 records and a queue of one largest burst: channel 0
    hands over the lengths 1, cap - 4, cap - 3, cap (14 records) and a full-length packet that no longer fits (refused), later one that
    lies across the ring's wrap; channel 1 two full-length packets that fill the ring to its last record; channel 2 a bad length in front
    of a good packet; channel 3 nothing at first"""
    rng = np.random.default_rng(seed)
    mp, C = max_packet(kb, shape[0]), cap(kb)
    P = lambda L, dst=ADDR: (_bytes(rng, L), dst)
    calls = [[[P(1), P(C - 4), P(C - 3), P(C), P(mp)], [P(mp), P(mp)], [P(10), P(mp + 1), P(20)], []]]
    calls += [[[], [], [], []] for _ in range(5)]
    calls += [[[P(mp)], [P(1)], [(b"", ADDR)], [P(mp, EVERYONE), P(2)]]]
    calls += [[[], [], [], []] for _ in range(3)]
    return calls
