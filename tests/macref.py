"""Host model of the medium-access layer (include/pirip_hip.h section T), for tests/test_mac*.py: the statement of the rules.

draw() and gate_step() are the header's arithmetic; Mac holds the per-channel state over a tests/pktref.py Link (or tests/pktfecref.py's
twin), imported and not copied: sense() is steps 0 and 1 and gives the rows as the reassembly reads them, offer() is step 2 around the
link's offer. Terminal is one packet handle with the layer, MacNode one tests/arqref.py Node with it. Medium puts two MacNodes on one
modelled half-duplex channel. tests/test_mac_cpu.py shows what the scripts reach before the device sees them."""
import numpy as np

import arqref
import pktref
import rptref

SYNC, BITS = pktref.SYNC, pktref.BITS
KB = pktref.KB
IDLE, CONTEND, HOLD = 0, 1, 2
RUN_MAX = 1 << 30
STATS_PER_FRAME, SNR_AT = 10, 5
TX_COUNTERS = ("accesses", "won", "backoff", "deferred", "bursts")
RX_COUNTERS = ("carrier", "own", "muted")
STATE = ("phase", "counter", "run", "quiet", "idle")
M32 = 0xFFFFFFFF


def draw(key, t, a, cw):
    x = (key ^ (t * 0x9E3779B9) ^ ((a & M32) * 0x85EBCA6B)) & M32
    x ^= x >> 16
    x = x * 0x7FEB352D & M32
    x ^= x >> 15
    x = x * 0x846CA68B & M32
    x ^= x >> 16
    return x * cw >> 32


def gate_step(g, rules, t, due, queued, idle):
    """rules 1 - 4 on the dict g (phase, counter, run, accesses, won, backoff, deferred) -> limit; rules: dict slot_calls, cw, ifs_calls,
    txop_bursts, key"""
    if g["phase"] == HOLD and not queued:
        g["phase"] = IDLE
    if g["phase"] == IDLE and due:
        g["phase"] = CONTEND
        g["counter"] = rules["slot_calls"] * draw(rules["key"], t, g["accesses"], rules["cw"])
        g["accesses"] += 1
    if g["phase"] == CONTEND:
        if idle > rules["ifs_calls"] and g["counter"] == 0:
            g["phase"], g["run"] = HOLD, 0
            g["won"] += 1
        elif idle > rules["ifs_calls"]:
            g["counter"] -= 1
            g["backoff"] += 1
        else:
            g["deferred"] += 1
    return max(rules["txop_bursts"] - g["run"], 0) if g["phase"] == HOLD else 0


def run_next(run, restart):
    return 0 if restart else min(run + 1, RUN_MAX)


def new_gate():
    return dict(phase=IDLE, counter=0, run=0, accesses=0, won=0, backoff=0, deferred=0)


class Mac:
    def __init__(self, link, nrx, rx_of_tx=None, sense_mask=1, sense_snr=0.0, slot_calls=1, cw=8, ifs_calls=0, mute_calls=1, txop_bursts=1, key=1):
        self.link, self.nrx = link, nrx
        self.rx_of_tx = list(range(link.ntx)) if rx_of_tx is None else [-1 if c is None else c for c in rx_of_tx]
        self.tx_of_rx = [-1] * nrx
        for t, c in enumerate(self.rx_of_tx):
            if c >= 0:
                assert self.tx_of_rx[c] < 0
                self.tx_of_rx[c] = t
        self.sense_mask, self.sense_snr, self.mute_calls = sense_mask, np.float32(sense_snr), mute_calls
        self.rules = dict(slot_calls=slot_calls, cw=cw, ifs_calls=ifs_calls, txop_bursts=txop_bursts, key=key & M32)
        self.reset()

    def reset(self):
        ntx = self.link.ntx
        self.g = [new_gate() for _ in range(ntx)]
        self.bursts = [0] * ntx
        self.quiet, self.air = [RUN_MAX] * ntx, [0] * ntx
        self.idle = [0] * self.nrx
        self.c = {k: np.zeros(self.nrx, np.int64) for k in RX_COUNTERS}
        self.ev = dict(mute_kept_sync=0, muted_open_packet=0, carrier_sync=0, carrier_snr=0, nan_rows=0, hold_exhausted=0, due_while_hold=0,
                       contend_to_hold_same_call=0, limited=0)
        self.last_own, self.last_carrier = [0] * self.nrx, [0] * self.nrx

    def sense(self, rows, stats=None):
        """steps 0 and 1 of a call on rows[c] = (status, payload), stats[c] = float32 [nf, 10] or None -> the rows the reassembly reads"""
        self.quiet = [run_next(q, a) for q, a in zip(self.quiet, self.air)]
        out = []
        for c, (st, pl) in enumerate(rows):
            st = np.asarray(st, np.uint8)
            t = self.tx_of_rx[c]
            own = t >= 0 and self.quiet[t] < self.mute_calls
            carrier = False
            if own:
                self.c["muted"][c] += int(np.count_nonzero(st & BITS))
                self.ev["mute_kept_sync"] += int(np.count_nonzero((st & BITS != 0) & (st & SYNC != 0)))
                st = st & np.uint8(~BITS & 0xFF)
            else:
                if self.sense_mask & 1 and np.any(st & SYNC):
                    carrier = True
                    self.ev["carrier_sync"] += 1
                if self.sense_mask & 2 and stats is not None and stats[c] is not None and len(st):
                    snr = np.asarray(stats[c], np.float32).reshape(-1, STATS_PER_FRAME)[:len(st), SNR_AT]
                    self.ev["nan_rows"] += int(np.count_nonzero(np.isnan(snr)))
                    with np.errstate(invalid="ignore"):
                        if np.any(snr >= self.sense_snr):
                            carrier = True
                            self.ev["carrier_snr"] += 1
            self.c["own"][c] += own
            self.c["carrier"][c] += carrier
            self.idle[c] = run_next(self.idle[c], own or carrier)
            self.last_own[c], self.last_carrier[c] = int(own), int(carrier)
            out.append((st, pl))
        return out

    def offer(self):
        """step 2 and the link's offer under its limits -> offered [ntx] record arrays (pktref.Link.call's loop, with the limit)"""
        lk = self.link
        offered = []
        for t in range(lk.ntx):
            c = self.rx_of_tx[t]
            limit = None
            if c >= 0:
                g = self.g[t]
                was = g["phase"]
                self.ev["due_while_hold"] += was == HOLD and bool(lk.ring[t]) and lk.queued[t] > 0
                limit = gate_step(g, self.rules, t, bool(lk.ring[t]), lk.queued[t] > 0, self.idle[c])
                self.ev["contend_to_hold_same_call"] += was == IDLE and g["phase"] == HOLD
                self.ev["hold_exhausted"] += g["phase"] == HOLD and limit == 0
            take = []
            while lk.ring[t] and (limit is None or len(take) < limit):
                b = lk.ring[t][0]
                cost = rptref.burst_cost(b.shape[0] - 1, lk.pre, lk.frame, lk.gap[t])
                if cost > lk.queue_syms - lk.queued[t]:
                    lk.ev["blocked"] += 1
                    break
                lk.ring[t].pop(0)
                lk.queued[t] += cost
                lk.head[t] += b.shape[0]
                take.append(b)
            if limit is not None:
                self.ev["limited"] += limit > 0 and bool(lk.ring[t]) and len(take) == limit
                self.g[t]["run"] += len(take)
                self.bursts[t] += len(take)
            lk.ev["max_bursts_per_offer"] = max(lk.ev["max_bursts_per_offer"], len(take))
            offered.append(np.concatenate(take) if take else np.zeros((0, 1 + lk.kb), np.uint8))
            self.air[t] = int(lk.queued[t] > 0)                              # what the process of this call dequeues
            lk.queued[t] -= min(lk.S, lk.queued[t])
        lk.n += 1
        return offered

    def state(self, t):
        c = self.rx_of_tx[t]
        g = self.g[t]
        return dict(phase=g["phase"], counter=g["counter"], run=g["run"], quiet=self.quiet[t], idle=self.idle[c] if c >= 0 else -1)

    def counters(self):
        out = {k: np.array([g[k] for g in self.g], np.int64) for k in TX_COUNTERS[:4]}
        out["bursts"] = np.array(self.bursts, np.int64)
        out.update(self.c)
        return out


class Terminal:
    """one packet handle (transmit side and reassembly) with or without the layer"""

    def __init__(self, link, rasm, mac=None):
        self.link, self.rasm, self.mac = link, rasm, mac

    def call(self, rows, stats=None):
        if self.mac is None:
            self.rasm.call(rows)
            return self.link.call()
        open_before = [o is not None for o in getattr(self.rasm, "open", [])]
        seen = self.mac.sense(rows, stats)
        self.mac.ev["muted_open_packet"] += sum(o and own for o, own in zip(open_before, self.mac.last_own))
        self.rasm.call(seen)
        return self.mac.offer()


class MacNode(arqref.Node):
    """arqref.Node whose packet handle has the layer attached: Node.call with steps 0 - 2 in the places the header gives them"""

    def attach(self, **kw):
        self.mac = Mac(self.link, self.nchan, **kw)
        return self

    def call(self, rows, stats=None):
        n = self.n
        items = [s.stage(n) for s in self.sess]
        dst = [0xFF if s.peer < 0 else s.peer for s in self.sess]
        taken = self.link.send([[(b, d) for _, _, b in it] for it, d in zip(items, dst)])
        for s, it, k in zip(self.sess, items, taken):
            s.commit(n, it, k)
        self.rasm.call(self.mac.sense(rows, stats))
        offered = self.mac.offer()
        for c, s in enumerate(self.sess):
            got = self.rasm.entries[c]
            if len(got) - self.seen[c] > self.ring_entries:
                s.skip(len(got) - self.seen[c] - self.ring_entries)
                self.seen[c] = len(got) - self.ring_entries
            for e, b in got[self.seen[c]:]:
                s.receive(n, b, int(e["src"]))
            self.seen[c] = len(got)
        self.n += 1
        return offered


# ---------------------------------------------------------------- tables for tests/cprog/mac_gate_check.cpp

DRAW_KEYS = (0, 1, 0xDEADBEEF, 0xFFFFFFFF)
DRAW_CWS = (1, 2, 3, 8, 1024)
DRAW_AS = tuple(range(64)) + (M32,)


def draw_lines():
    return ["D %d %d %d %d %d" % (key, t, a, cw, draw(key, t, a, cw)) for key in DRAW_KEYS for cw in DRAW_CWS for t in range(8) for a in DRAW_AS]


GATE_RULES = dict(slot_calls=3, cw=8, key=0x1234ABCD)


def gate_lines():
    """every combination of phase, counter 0 .. 3, run 0 .. 2, due, queued, idle 0 .. 3, ifs_calls 0 .. 2, txop_bursts 1 .. 2, on channel 5
    at access 7:  G <the inputs> | phase counter run accesses won backoff deferred limit"""
    out = []
    for ifs in range(3):
        for txop in (1, 2):
            rules = dict(GATE_RULES, ifs_calls=ifs, txop_bursts=txop)
            for phase in (IDLE, CONTEND, HOLD):
                for counter in range(4):
                    for run in range(3):
                        for due in (0, 1):
                            for queued in (0, 1):
                                for idle in range(4):
                                    g = dict(new_gate(), phase=phase, counter=counter, run=run, accesses=7)
                                    limit = gate_step(g, rules, 5, due, queued, idle)
                                    out.append("G %d %d %d %d %d %d %d %d | %d %d %d %d %d %d %d %d" % (
                                        ifs, txop, phase, counter, run, due, queued, idle, g["phase"], g["counter"], g["run"], g["accesses"], g["won"],
                                        g["backoff"], g["deferred"], limit))
    return out


def table_text():
    head = "R %d %d %d" % (GATE_RULES["slot_calls"], GATE_RULES["cw"], GATE_RULES["key"])
    return "\n".join([head] + draw_lines() + gate_lines()) + "\n"


# ---------------------------------------------------------------- the shapes and scripts both test files use (records path)

PRE, FRAME, GAP = arqref.PRE, arqref.FRAME, arqref.GAP
MAX_FRAGS = 3
BURST = PRE + MAX_FRAGS * FRAME + GAP           # symbols of one largest burst
REC_S = 700                                    # symbols a records-path call transmits: a one-frame burst (658) is one call on air, a largest burst three
FILT, ADDR = 1, 7


def terminal(mac=None, fec=None, queue_bursts=2, pending=None, S=REC_S, ring_entries=16, filt=FILT, address=ADDR):
    """a four-channel packet terminal of the stand-in code; mac: Mac's keyword arguments, or None for none"""
    import pktfecref
    if fec is None:
        pending = 4 * (MAX_FRAGS + 1) if pending is None else pending
        link = pktref.Link(4, FILT, KB, MAX_FRAGS, pending, queue_bursts * BURST, S, PRE, FRAME, GAP)
        rasm = pktref.Reassembler(4, KB, MAX_FRAGS, filt, address, ring_entries)
    else:
        shape = (MAX_FRAGS,) + tuple(fec)
        r = pktfecref.r_of(*shape)
        pending = 4 * (MAX_FRAGS + r + 1) if pending is None else pending
        link = pktfecref.LinkFec(4, FILT, KB, shape, pending, queue_bursts * (BURST + r * FRAME), S, PRE, FRAME, GAP)
        rasm = pktfecref.ReassemblerFec(4, KB, MAX_FRAGS, filt, address, ring_entries, *fec)
    return Terminal(link, rasm, None if mac is None else Mac(link, 4, **mac))


def _bytes(rng, n):
    return rng.integers(0, 256, n).astype(np.uint8).tobytes()


def empty_rows(n=4):
    return [(np.zeros(0, np.uint8), np.zeros((0, KB), np.uint8)) for _ in range(n)]


def lone_rows(nf, at, status, n=4, chan=0):
    """a call of nf rows on channels 0 and 3, nf // 2 on channel 1 and nf - 1 on channel 2 (so that a staging of the call has rows behind
    two channels' counts), with `status` at row `at` of channel `chan` alone"""
    counts = [nf, nf // 2, max(nf - 1, 0), nf][:n]
    rows = [(np.zeros(k, np.uint8), np.zeros((k, KB), np.uint8)) for k in counts]
    if at is not None:
        rows[chan][0][at] = status
    return rows


SENSE_SIZES = (0, 1, 63, 64, 65, 4096)


def sense_script():
    """list of (rows, stats or None, note): the wave reduction's edges under sense_mask 1; every channel sees another row set"""
    out = []
    for nf in SENSE_SIZES:
        out.append((lone_rows(nf, None, 0), None, "nothing in %d rows" % nf))
        for at in sorted({0, 63, 64, nf - 1}):
            if 0 <= at < nf:
                for chan in (0, 3):
                    out.append((lone_rows(nf, at, SYNC, chan=chan), None, "SYNC at %d of %d" % (at, nf)))
    out.append((lone_rows(65, 64, BITS), None, "BITS without SYNC is no carrier"))
    return out


def stats_rows(nf, at=None, snr=0.0, base=-5.0, n=4, chan=0):
    st = [np.full((nf, STATS_PER_FRAME), base, np.float32) for _ in range(n)]
    if at is not None:
        st[chan][at, SNR_AT] = snr
    return st


SNR_T = np.float32(6.25)


def snr_script():
    """list of (rows, stats, note) for sense_snr = SNR_T: a lone row at the threshold, just under it, NaN; stats absent"""
    under = np.nextafter(SNR_T, np.float32(-np.inf), dtype=np.float32)
    out = []
    for nf, at in ((1, 0), (65, 64), (130, 63)):
        for v, note in ((SNR_T, "at"), (under, "under"), (np.float32("nan"), "nan"), (np.float32("inf"), "inf")):
            out.append((lone_rows(nf, None, 0), stats_rows(nf, at, v), "%s the threshold, row %d of %d" % (note, at, nf)))
    out.append((lone_rows(3, 1, SYNC), stats_rows(3), "SYNC under weak stats"))
    out.append((lone_rows(3, None, 0), None, "no stats"))
    return out


def packet_rows(payloads, src=2, dst=ADDR, first_id=0, n=4, fec=None, max_frags=MAX_FRAGS):
    """rows[c]: the frames of one packet per channel (payloads[c] bytes or None), each SYNC | BITS"""
    import pktfecref
    rows = []
    for c in range(n):
        if payloads[c] is None:
            rows.append((np.zeros(0, np.uint8), np.zeros((0, KB), np.uint8)))
            continue
        if fec is None:
            rec = pktref.segment(payloads[c], src, dst, first_id + c, KB, max_frags)[:-1]
        else:
            rec = pktfecref.segment_fec(payloads[c], src, dst, first_id + c, KB, max_frags, *fec)[:-1]
        rows.append((np.full(len(rec), SYNC | BITS, np.uint8), rec[:, 1:].copy()))
    return rows


def split_rows(rows, k):
    """rows cut behind row k of every channel: (first part, second part)"""
    return [(s[:k], p[:k]) for s, p in rows], [(s[k:], p[k:]) for s, p in rows]


def gate_script(seed, ncalls=200, p_carrier=0.35, p_send=0.12):
    """per call: (packets[t] to send, rows with or without a lone SYNC row per channel): seeded carrier patterns in runs, and sends that
    pile up to three bursts"""
    rng = np.random.default_rng(seed)
    busy = [0] * 4
    out = []
    for k in range(ncalls):
        rows = []
        for c in range(4):
            if busy[c] == 0 and rng.random() < p_carrier / 3:
                busy[c] = int(rng.integers(1, 6))
            nf = int(rng.integers(0, 4))
            st = np.zeros(nf, np.uint8)
            if busy[c] and nf:
                st[int(rng.integers(0, nf))] = SYNC
            busy[c] = max(busy[c] - 1, 0)
            rows.append((st, np.zeros((nf, KB), np.uint8)))
        send = []
        for t in range(4):
            q = []
            if k in (0, 90):                                             # three bursts pending at once
                q = [(_bytes(rng, 10 + t), ADDR), (_bytes(rng, 30), ADDR), (_bytes(rng, 5), ADDR)]
            elif rng.random() < p_send:
                q = [(_bytes(rng, int(rng.integers(1, pktref.max_packet(KB, MAX_FRAGS) + 1))), ADDR)]
            send.append(q)
        out.append((send, rows))
    return out


# ---------------------------------------------------------------- two terminals on one modelled half-duplex medium

class Medium:
    """Two MacNodes (or arqref.Nodes when gate is False) a and b with all channels on one modelled medium per channel. A terminal is on air
    on channel t in call k iff its section K queue is not empty when call k processes. A burst offered in call k behind q symbols of queue
    lies in the calls k + q // S .. k + (q + cost - 1) // S; it reaches the peer iff the peer is on air on that channel in none of them, and
    then its frames are the peer's rows, SYNC | BITS, `lag` calls after its last call. A call on air shows at the peer -- and at the sender
    itself, on the receive channel it listens on -- as one row with SYNC alone `lag` calls later, and the own burst's frames come back to the
    sender as the peer's do: that is what the mute is for."""

    def __init__(self, a, b, lag, gate=True):
        self.nodes, self.lag, self.gate, self.k = (a, b), lag, gate, 0
        n = a.nchan
        self.air = [dict(), dict()]                                       # side -> {(call, chan): 1}
        self.flight = [[], []]                                            # side -> [(chan, first call, last call, records)]
        self.collided, self.arrived = [0, 0], [0, 0]
        self.n = n

    def rows_for(self, side):
        """the rows of call k: what ended `lag` calls ago, and one SYNC row for a call on air `lag` calls ago"""
        k, lag, n = self.k, self.lag, self.n
        st = [[] for _ in range(n)]
        pl = [[] for _ in range(n)]
        for src in (side, 1 - side):                                      # the own echo first, then the peer's bursts
            for c, first, last, rec in self.flight[src]:
                if last + lag != k:
                    continue
                hit = src != side and any((j, c) in self.air[side] for j in range(first, last + 1))
                if src != side:
                    self.collided[src] += hit
                    self.arrived[src] += not hit
                if hit:
                    continue
                for r in rec:
                    if r[0] != 2:
                        st[c].append(SYNC | BITS)
                        pl[c].append(r[1:])
            for c in range(n):
                if (k - lag, c) in self.air[src] and not st[c]:
                    st[c].append(SYNC)
                    pl[c].append(np.zeros(KB, np.uint8))
        return [(np.array(st[c], np.uint8), np.array(pl[c], np.uint8).reshape(len(st[c]), KB)) for c in range(n)]

    def call(self):
        """one call of both terminals -> (offered per side, rows per side)"""
        rows = [self.rows_for(0), self.rows_for(1)]
        off = []
        for side, nd in enumerate(self.nodes):
            lk = nd.link
            q0 = list(lk.queued)
            o = nd.call(rows[side])
            off.append(o)
            for c, rec in enumerate(o):
                rec = np.asarray(rec, np.uint8).reshape(-1, 1 + KB)
                q, start = q0[c], 0
                for i, r in enumerate(rec):
                    if r[0] == 2:
                        burst = rec[start:i + 1]
                        cost = rptref.burst_cost(len(burst) - 1, lk.pre, lk.frame, lk.gap[c])
                        self.flight[side].append((c, self.k + q // lk.S, self.k + (q + cost - 1) // lk.S, burst))
                        q, start = q + cost, i + 1
                if q > 0:
                    self.air[side][(self.k, c)] = 1
        self.k += 1
        return off, rows


AIR_KEYS = (0x0000A11C, 0x0000B0B5)              # the two ends' keys; tests/test_mac_cpu.py proves their draws differ
AIR_CW = 8


def keys_differ(keys=AIR_KEYS, cw=AIR_CW, accesses=8, nchan=4):
    return all(draw(keys[0], t, a, cw) != draw(keys[1], t, a, cw) for t in range(nchan) for a in range(accesses))


def find_keys(cw=AIR_CW, start=1):
    """the first pair (k, k + 1) from `start` on whose draws differ: how AIR_KEYS may be chosen again"""
    k = start
    while not keys_differ((k, k + 1), cw):
        k += 1
    return k, k + 1


# ---------------------------------------------------------------- scripts of whole calls: (packets to send per channel, rows, stats)

def mute_script(mute_calls, fec=None):
    """Own bursts and rows with BITS in every call behind them; call 0 brings no rows on channels 0 - 2, so that the bursts go out at
    once (cw = 1). Channel 0: a one-frame own burst in call 0 (one call on air), from call 1 on a packet arrives in every call; channel 1: a
    largest own burst (three calls on air), likewise; channel 2: no own burst, likewise -- never muted; channel 3: the first fragment of a
    three-fragment packet in call 0, a one-frame own burst in call 1, the second fragment in call 2 (muted when mute_calls > 0) and the
    third in call mute_calls + 3: a packet open across the muted calls."""
    rng = np.random.default_rng(77)
    big = pktref.max_packet(KB, MAX_FRAGS)
    three = packet_rows([None, None, None, _bytes(rng, big)], fec=fec)[3]
    out = []
    for k in range(mute_calls + 7):
        send = [[], [], [], []]
        if k == 0:
            send[0], send[1] = [(_bytes(rng, 9), ADDR)], [(_bytes(rng, big), ADDR)]
        if k == 1:
            send[3] = [(_bytes(rng, 9), ADDR)]
        rows = packet_rows([_bytes(rng, 20), _bytes(rng, 20), _bytes(rng, 20), None] if k else [None] * 4, first_id=4 * k, fec=fec)
        at = {0: 0, 2: 1, mute_calls + 3: 2}.get(k)
        if at is not None:                                               # (an FEC handle's parity fragments come with the last)
            end = at + 1 if at < 2 else None
            rows[3] = (three[0][at:end], three[1][at:end])
        out.append((send, rows, None))
    return out


def run_script(term, script, dev=None):
    """the model terminal through a script; with dev (tests/test_mac.py's twin on the device) every call is compared -> offered per call"""
    offs = []
    for k, (send, rows, stats) in enumerate(script):
        if any(send):
            taken = term.link.send(send)
            if dev is not None:
                assert dev.send(send) == taken, k
        off = term.call(rows, stats) if term.mac is not None else term.call(rows)
        if dev is not None:
            dev.push(rows, stats)
            dev.check(term, off, k)
        offs.append(off)
    return offs


# ---------------------------------------------------------------- two ARQ terminals on one medium (tests/test_mac.py's air run in the model)

AIR_S, AIR_W, AIR_TRIES = 100, 2, 8             # symbols per call of the LOOP shapes; window; transmissions before a session breaks
AIR_SEGMENTS = 3


def air_calls(frames):
    return -(-(PRE + frames * FRAME + GAP) // AIR_S)


def air_rto(slot_calls, cw=AIR_CW, margin=8):
    """one DATA access + one ACK access + the longest backoff + a margin"""
    return air_calls(MAX_FRAGS) + air_calls(1) + slot_calls * cw + margin


def air_pair(gate, lag, slot_calls=None, rto=None, keys=AIR_KEYS, sense_mask=1, sense_snr=0.0):
    """-> Medium of two terminals A (1) and B (2) with equal timers; gate False: plain arqref.Nodes"""
    slot_calls = lag + 1 if slot_calls is None else slot_calls
    rto = air_rto(slot_calls) if rto is None else rto
    nodes = []
    for (src, peer), key in zip(((1, 2), (2, 1)), keys):
        args = (4, src, peer, AIR_W, rto, AIR_TRIES, 4, 8, BURST, AIR_S, PRE, FRAME, GAP)
        kw = dict(max_frags=MAX_FRAGS, filt=src, address=src, ring_entries=8)
        if gate:
            nodes.append(MacNode(*args, **kw).attach(sense_mask=sense_mask, sense_snr=sense_snr, slot_calls=slot_calls, cw=AIR_CW, ifs_calls=lag,
                                                     mute_calls=lag + 1, txop_bursts=1, key=key))
        else:
            nodes.append(arqref.Node(*args, **kw))
    return Medium(nodes[0], nodes[1], lag, gate)


def air_traffic(max_payload):
    """both directions: AIR_SEGMENTS segments per channel, the first fills its last fragment"""
    mk = lambda base: [[arqref._bytes(np.random.default_rng(base + 10 * c + j), n) for j, n in enumerate((max_payload, 42, 18)[:AIR_SEGMENTS])]
                       for c in range(4)]
    return mk(1000), mk(2000)


def run_air(med, ta, tb, ncalls, submit_at=2):
    for k in range(ncalls):
        if k == submit_at:
            assert med.nodes[0].submit(ta) == [len(q) for q in ta] and med.nodes[1].submit(tb) == [len(q) for q in tb]
        med.call()
    return med
