"""Host model of the streaming repeater's intake and offer (include/pirip_hip.h section M), for tests/test_repeater_stream*.py:
per receive channel rtl_fsk's --filter and frame_repeater.c's state machine (txref.repeater_replay, run on the records since the open burst
began), per transmit channel a pending ring of whole bursts with ready tags and section K's queue as a symbol count. It returns the
records offered per call and channel and the counters, and notes which corners a schedule reaches.

A schedule is a dict: calls (per call, per receive channel (status uint8 [n], payload uint8 [n, kb])), route, source, filter (None or a
byte), holdoff, max_burst, pending, queue_syms, S, ntx. schedules() builds the ones both test files run; tests/test_repeater_stream_cpu.py
shows what they reach before the device sees them."""
import numpy as np

import txref

SYNC, BITS = txref.RX_SYNC, txref.RX_BITS
KB = 32                                       # the stand-in code's data bytes
GAP_SYMS = 7


def burst_cost(frames, pre, frame, gap):
    """symbols of the records 1, 0 * (frames - 1), 2: the framer's layout rule"""
    return pre + frames * frame + gap


def _closed_prefix(status):
    """(records up to and including the last one that ends a burst, whether a burst is open behind it)"""
    receiving, end = False, 0
    for i, st in enumerate(status):
        if not receiving:
            receiving = st == (SYNC | BITS)
        elif not (st & SYNC):
            receiving, end = False, i + 1
    return end, receiving


def _bursts(records):
    """Tx records -> list of bursts (each uint8 [frames + 1, 1 + kb], ending in its `2`)"""
    ends = [i + 1 for i in range(records.shape[0]) if records[i, 0] == 2]
    return [records[a:b] for a, b in zip([0] + ends[:-1], ends)]


class Model:
    def __init__(self, nrx, route, source, filt, holdoff, max_burst, pending, queue_syms, S, pre, frame, gap, ntx=None, kb=KB):
        self.nrx, self.route, self.source, self.filt = nrx, list(route), source, filt
        self.holdoff, self.max_burst, self.pending, self.queue_syms, self.S = holdoff, max_burst, pending, queue_syms, S
        self.ntx = ntx if ntx is not None else max([r for r in route if r >= 0] + [0]) + 1
        self.pre, self.frame, self.kb = pre, frame, kb
        self.gap = [gap] * self.ntx if np.isscalar(gap) else list(gap)
        self.reset()

    def reset(self):
        self.n = 0
        self.open_st = [np.zeros(0, np.uint8) for _ in range(self.nrx)]       # records since the open burst began (filtered status)
        self.open_pl = [np.zeros((0, self.kb), np.uint8) for _ in range(self.nrx)]
        self.open_since = [None] * self.nrx
        self.ring = [[] for _ in range(self.ntx)]                             # (records, ready, call it ended in)
        self.head, self.tail = [0] * self.ntx, [0] * self.ntx
        self.queued = [0] * self.ntx
        names_rx, names_tx = ("bursts_in", "frames_in", "filtered", "unrouted"), ("bursts_out", "dropped")
        self.c = {k: np.zeros(self.nrx, np.int64) for k in names_rx}
        self.c.update({k: np.zeros(self.ntx, np.int64) for k in names_tx})
        # corners reached
        self.ev = dict(filtered_first=0, filtered_middle=0, max_open_calls=0, waits=set(), blocked=[], drop_while_waiting=0, cut=0,
                       wraps=0, max_bursts_per_offer=0)
        self._blocked_since = [None] * self.ntx

    def counters(self):
        out = dict(self.c)
        out["pending"] = np.array([t - h for h, t in zip(self.head, self.tail)], np.int64)
        return out

    def _intake(self, c, status, payload):
        st = np.array(status, dtype=np.uint8).copy()
        pl = np.asarray(payload, dtype=np.uint8).reshape(-1, self.kb)
        was_open = self.open_st[c].size > 0
        receiving = was_open
        for i in range(st.size):                                             # rtl_fsk.cpp:334
            hit = bool(st[i] & BITS) and self.filt is not None and pl[i, 0] == self.filt
            if hit:
                self.c["filtered"][c] += 1
                if not receiving and st[i] == (SYNC | BITS):
                    self.ev["filtered_first"] += 1
                if receiving:
                    self.ev["filtered_middle"] += 1
                st[i] &= ~BITS & 0xFF
            if not receiving:
                receiving = st[i] == (SYNC | BITS)
            elif not (st[i] & SYNC):
                receiving = False
        if self.open_st[c].size == 0 and st.size:
            # records in front of a burst's start change nothing: the replay begins where it would begin
            starts = np.flatnonzero(st == (SYNC | BITS))
            if starts.size == 0:
                return []
            st, pl = st[starts[0]:], pl[starts[0]:]
        allst, allpl = np.concatenate([self.open_st[c], st]), np.concatenate([self.open_pl[c], pl])
        end, still = _closed_prefix(allst)
        out = _bursts(txref.repeater_replay(allst[:end], allpl[:end], self.source))
        if out:                                                              # the first of them may have been open for several calls
            self.ev["max_open_calls"] = max(self.ev["max_open_calls"], self.n - (self.open_since[c] if was_open else self.n) + 1)
        rest_st, rest_pl = allst[end:], allpl[end:]
        if still:
            first = np.flatnonzero(rest_st == (SYNC | BITS))[0]
            if not (was_open and end == 0):
                self.open_since[c] = self.n
            self.open_st[c], self.open_pl[c] = rest_st[first:], rest_pl[first:]
        else:
            self.open_st[c], self.open_pl[c] = rest_st[:0], rest_pl[:0]
            self.open_since[c] = None
        kept = []
        for b in out:                                                        # frames beyond max_burst are dropped where the original asserts
            if b.shape[0] - 1 > self.max_burst:
                self.ev["cut"] += 1
                b = np.concatenate([b[:self.max_burst], b[-1:]])
            kept.append(b)
        return kept

    def call(self, records):
        """one call: records[c] = (status, payload) -> offered [ntx] record arrays"""
        for c, (status, payload) in enumerate(records):
            for b in self._intake(c, status, payload):
                self.c["bursts_in"][c] += 1
                self.c["frames_in"][c] += b.shape[0] - 1
                t = self.route[c]
                if t < 0:
                    self.c["unrouted"][c] += 1
                    continue
                if b.shape[0] > self.pending - (self.tail[t] - self.head[t]):
                    self.c["dropped"][t] += 1
                    if self.ring[t]:
                        self.ev["drop_while_waiting"] += 1
                    continue
                if self.tail[t] % self.pending + b.shape[0] > self.pending:
                    self.ev["wraps"] += 1
                self.ring[t].append((b, self.n + self.holdoff, self.n))
                self.tail[t] += b.shape[0]
        offered = []
        for t in range(self.ntx):
            take = []
            while self.ring[t]:
                b, ready, ended = self.ring[t][0]
                if ready > self.n:
                    break
                cost = burst_cost(b.shape[0] - 1, self.pre, self.frame, self.gap[t])
                if cost > self.queue_syms - self.queued[t]:
                    if self._blocked_since[t] is None:
                        self._blocked_since[t] = self.n
                    break
                if self._blocked_since[t] is not None:
                    self.ev["blocked"].append(self.n - self._blocked_since[t])
                    self._blocked_since[t] = None
                else:
                    self.ev["waits"].add(self.n - ended)
                self.ring[t].pop(0)
                self.queued[t] += cost
                self.head[t] += b.shape[0]
                self.c["bursts_out"][t] += 1
                take.append(b)
            self.ev["max_bursts_per_offer"] = max(self.ev["max_bursts_per_offer"], len(take))
            offered.append(np.concatenate(take) if take else np.zeros((0, 1 + self.kb), np.uint8))
            self.queued[t] -= min(self.S, self.queued[t])
        self.n += 1
        return offered


def run(sched, pre, frame, gap=GAP_SYMS):
    """a schedule on a fresh model -> (offered[n][t], model)"""
    m = Model(len(sched["route"]), sched["route"], sched["source"], sched["filter"], sched["holdoff"], sched["max_burst"], sched["pending"],
              sched["queue_syms"], sched["S"], pre, frame, gap, ntx=sched["ntx"])
    return [m.call(recs) for recs in sched["calls"]], m


# ---------------------------------------------------------------- schedules

def cut_calls(rng, streams, ncalls):
    """per-channel (status, payload) streams cut into ncalls consecutive pieces each, some empty, some of one record"""
    cuts = []
    for st, _ in streams:
        n = len(st)
        if rng.random() < 0.3:
            cut = np.sort(rng.integers(0, min(n, 3) + 1, ncalls - 1))
        else:
            cut = np.sort(rng.integers(0, n + 1, ncalls - 1))
        cuts.append(np.concatenate([[0], cut, [n]]))
    return [[(st[cuts[c][p]:cuts[c][p + 1]], pl[cuts[c][p]:cuts[c][p + 1]]) for c, (st, pl) in enumerate(streams)] for p in range(ncalls)]


def fixture_streams():
    """the kb = 32 cases of tests/golden/repeater_cases.npz with at most 60 calls and bursts of at most 12 frames"""
    out = []
    for c in txref.repeater_cases():
        if c["kb"] != KB or c["status"].size > 60:
            continue
        longest = max([b.shape[0] - 1 for b in _bursts(c["out"])] + [0])
        if longest <= 12:
            out.append(c)
    return out


def _frames(rng, status, first=None):
    """(status, payload) of a hand-written status list; first: byte 0 per record (None: a byte that is no filter byte)"""
    st = np.array(status, dtype=np.uint8)
    pl = rng.integers(0, 256, (st.size, KB)).astype(np.uint8)
    pl[:, 0] = 0x11
    if first is not None:
        for i, b in first.items():
            pl[i, 0] = b
    return st, pl


def corner_streams(rng, filt):
    """four receive channels, record after record; `filt`: the byte 0 that is filtered"""
    B, S2, E = BITS | SYNC, SYNC, 0
    # 0: a filtered first frame (no burst starts), a filtered middle frame, then a burst of 7 frames: cut at max_burst, and long
    s0 = [B, S2, E] + [0, 0] + [B, B, B, E] + [B] * 7 + [E]
    f0 = {0: filt, 6: filt}
    # 1: two bursts of one frame that end close together, a pause, then three bursts of 2 frames back to back (the third finds the ring full)
    s1 = [B, E, B, E] + [0] * 6 + [B, B, E, B, B, E, B, B, E] + [0] * 4 + [B, B, E]
    # 2: unrouted
    s2 = [B, B, E, 0, B, E]
    # 3: bursts of 2 frames, steadily: the ring wraps
    s3 = [B, B, E] * 6
    return [_frames(rng, s0, f0), _frames(rng, s1), _frames(rng, s2), _frames(rng, s3)]


def one_per_call(streams, extra=6):
    """record i of every channel in call i, and `extra` calls of nothing behind"""
    n = max(len(st) for st, _ in streams) + extra
    return [[(st[i:i + 1], pl[i:i + 1]) for st, pl in streams] for i in range(n)]


def schedules(pre, frame, gap=GAP_SYMS):
    """the schedules both test files run, for a modem whose preamble / frame are pre / frame symbols: list of dicts"""
    out = []
    cases = fixture_streams()
    streams = [(c["status"], c["payload"]) for c in cases]
    K = len(cases)
    ample = burst_cost(12, pre, frame, gap) * 3
    rng = np.random.default_rng(77)
    base = dict(route=list(range(K)), ntx=K, source=0x5C, filter=None, holdoff=0, max_burst=12, pending=64, queue_syms=ample, S=3)
    out.append(dict(base, name="fixture_one_call", calls=[streams] + [[(st[:0], pl[:0]) for st, pl in streams]] * 2))
    out.append(dict(base, name="fixture_pieces", calls=cut_calls(rng, streams, 9)))
    perm = list(rng.permutation(K))
    out.append(dict(base, name="fixture_permuted", route=[int(p) for p in perm], holdoff=2, calls=cut_calls(rng, streams, 7)))
    # the corners: four receive channels onto three transmit channels, one record per call
    filt = 0x5C
    cs = corner_streams(np.random.default_rng(78), filt)
    one, two = burst_cost(1, pre, frame, gap), burst_cost(2, pre, frame, gap)
    corner = dict(route=[2, 0, -1, 1], ntx=3, source=filt, filter=filt, max_burst=3, pending=5, S=3, calls=one_per_call(cs))
    # Transmit channel 0 gets its first burst (one frame) in call 1 + h and sends S = 3 symbols per call from then on, so in call 12 + h,
    # when the third burst (two frames) is due, 2 one - 33 symbols are queued. With this queue the free space is then 2 S short of that
    # burst: it waits at the head of the line in calls 12 + h and 13 + h and goes in in call 14 + h.
    q = 2 * one + two - 33 - 2 * 3
    assert q >= burst_cost(3, pre, frame, gap)
    for h in (0, 1, 3):
        out.append(dict(corner, name="corners_holdoff%d" % h, holdoff=h, queue_syms=q))
    return out
