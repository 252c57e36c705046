"""Host model of the ping terminal's log and schedule (include/pirip_hip.h section N), for tests/test_ping*.py.

Log: per receive channel rtl_fsk -L's sample clock (rtl_fsk.cpp:260: every row consumed what the row in front of it announced),
rtl_fsk's --filter, one entry per row that still has BITS, a ring of log_entries entries and the counters. Schedule: per transmit channel
the due rule, the burst's cost by the framer's layout rule (rptref.burst_cost) against section K's queue kept as a symbol count, exactly
as tests/rptref.py keeps it. The burst's records are built here from the test payload; tests/test_ping_cpu.py pins them to
fsk_ldpc_framer --testframes. Both models note which corners their inputs reach."""
import numpy as np

import rptref
import txref

SYNC, BITS = txref.RX_SYNC, txref.RX_BITS
KB = rptref.KB
INFO, STATS = 10, 10                          # PIRIP_LDPC_INFO_PER_CALL, PIRIP_STATS_PER_FRAME
CHUNK = 64                                    # rows the log kernel takes at a time

# pirip_ping_entry (40 bytes, the C layout)
ENTRY = np.dtype([("t_samples", "<i8"), ("call", "<i4"), ("row", "<i4"), ("S", "<f4"), ("N", "<f4"), ("SNRest", "<f4"), ("ecdd", "<i4"),
                  ("eraw", "<i4"), ("source", "u1"), ("seq", "u1"), ("status", "u1"), ("iters", "u1")])
assert ENTRY.itemsize == 40
RX_COUNTERS = ("frames", "filtered", "decoded", "crc_fail", "bit_errors", "lost")
TX_COUNTERS = ("bursts_sent", "frames_sent", "skipped")


def burst_records(payload, frames, source, seq):
    """the records of one burst of test frames: uint8 [frames + 1, 1 + kb] -- control 1, 0, ..., 0 with the test payload, the source byte in
    byte 0 and, with seq, (f + 1) & 0xff in byte 1; then the `2` record of zeros"""
    payload = np.asarray(payload, dtype=np.uint8)
    rec = np.zeros((frames + 1, 1 + payload.size), np.uint8)
    for f in range(frames):
        rec[f, 0] = 1 if f == 0 else 0
        rec[f, 1:] = payload
        rec[f, 1] = source
        if seq:
            rec[f, 2] = (f + 1) & 0xFF
    rec[frames, 0] = 2
    return rec


# ---------------------------------------------------------------- the schedule

class Schedule:
    def __init__(self, ntx, frames, period, first_call, max_bursts, queue_syms, S, pre, frame, gap, burst):
        self.ntx, self.frames, self.period, self.max_bursts = ntx, frames, period, max_bursts
        self.first = [0] * ntx if first_call is None else list(first_call)
        self.queue_syms, self.S, self.pre, self.frame = queue_syms, S, pre, frame
        self.gap = [gap] * ntx if np.isscalar(gap) else list(gap)
        self.burst = burst
        self.reset()

    def reset(self):
        self.n = 0
        self.queued = [0] * self.ntx
        self.c = {k: np.zeros(self.ntx, np.int64) for k in TX_COUNTERS}

    def call(self):
        """call n -> offered [ntx] record arrays (the burst, or no record)"""
        offered = []
        for t in range(self.ntx):
            since = self.n - self.first[t]
            due = since >= 0 and since % self.period == 0 and (self.max_bursts == 0 or self.c["bursts_sent"][t] < self.max_bursts)
            cost = rptref.burst_cost(self.frames, self.pre, self.frame, self.gap[t])
            if due and cost <= self.queue_syms - self.queued[t]:
                self.queued[t] += cost
                self.c["bursts_sent"][t] += 1
                self.c["frames_sent"][t] += self.frames
                offered.append(self.burst)
            else:
                self.c["skipped"][t] += due
                offered.append(self.burst[:0])
            self.queued[t] -= min(self.S, self.queued[t])
        self.n += 1
        return offered


def schedules(pre, frame, gap, frames=3, S=100):
    """the three schedules both test files run on four transmit channels: dicts of Schedule's arguments and the calls to run"""
    cost = rptref.burst_cost(frames, pre, frame, gap)
    calls_per_burst = -(-cost // S)
    base = dict(ntx=4, frames=frames, S=S, pre=pre, frame=frame, gap=gap)
    return [
        dict(base, name="staggered", period=calls_per_burst + 3, first_call=[0, 1, 2, calls_per_burst // 2], max_bursts=0, queue_syms=2 * cost,
             calls=2 * calls_per_burst + 8),
        dict(base, name="cutoff", period=calls_per_burst + 1, first_call=[0, 0, 3, 3], max_bursts=2, queue_syms=2 * cost, calls=3 * calls_per_burst + 10),
        # a queue of exactly one burst and a period shorter than a burst takes to send: due bursts find the queue busy
        dict(base, name="tight", period=max(calls_per_burst // 3, 1), first_call=None, max_bursts=0, queue_syms=cost, calls=2 * calls_per_burst + 5),
    ]


def run_schedule(s, burst):
    m = Schedule(s["ntx"], s["frames"], s["period"], s["first_call"], s["max_bursts"], s["queue_syms"], s["S"], s["pre"], s["frame"], s["gap"], burst)
    return [m.call() for _ in range(s["calls"])], m


# ---------------------------------------------------------------- the log

class Log:
    def __init__(self, nrx, nin0, filt, log_entries, want):
        self.nrx, self.nin0, self.filt, self.E = nrx, nin0, filt, log_entries
        self.want = np.asarray(want, dtype=np.uint8)
        self.reset()

    def reset(self):
        self.n = 0
        self.samples, self.next_nin = [0] * self.nrx, [self.nin0] * self.nrx
        self.entries = [[] for _ in range(self.nrx)]                          # every entry ever appended
        self.c = {k: np.zeros(self.nrx, np.int64) for k in RX_COUNTERS}
        self.ev = dict(filtered=0, crc_fail=0, empty_calls=0, nins_in_one_call=set(), wraps=0, call_larger_than_ring=0, max_rows=0)

    def call(self, rows):
        """call n: rows[c] = (status [nf], payload [nf, kb], info [nf, 10], stats float32 [nf, 10])"""
        kb = self.want.size
        for c, (st, pl, info, stats) in enumerate(rows):
            nf = len(st)
            self.ev["max_rows"] = max(self.ev["max_rows"], nf)
            self.ev["empty_calls"] += nf == 0
            stats = np.asarray(stats, dtype=np.float32).reshape(nf, STATS)
            if nf:
                self.ev["nins_in_one_call"].add(frozenset(int(x) for x in stats[:, 6]))
            at = self.c["frames"][c] % self.E
            logged = 0
            for f in range(nf):
                self.samples[c] += self.next_nin[c]                           # rtl_fsk.cpp:260
                self.next_nin[c] = int(stats[f, 6])
                v = int(st[f])
                decoded = info[f][6] >= 0
                self.c["decoded"][c] += decoded
                if decoded and not v & BITS:
                    self.c["crc_fail"][c] += 1
                    self.ev["crc_fail"] += 1
                if v & BITS and self.filt is not None and pl[f][0] == self.filt:                  # rtl_fsk.cpp:271
                    self.c["filtered"][c] += 1
                    self.ev["filtered"] += 1
                    continue
                if not v & BITS:
                    continue
                e = np.zeros((), ENTRY)
                e["t_samples"], e["call"], e["row"] = self.samples[c], self.n, f
                e["S"], e["N"], e["SNRest"] = stats[f, 8], stats[f, 9], stats[f, 5]
                e["ecdd"] = int(np.unpackbits(np.asarray(pl[f][2:kb - 2], np.uint8) ^ self.want[2:kb - 2]).sum())
                e["eraw"] = info[f][8]
                e["source"], e["seq"], e["status"], e["iters"] = pl[f][0], pl[f][1], v, min(max(int(info[f][4]), 0), 255)
                self.entries[c].append(e)
                self.c["frames"][c] += 1
                self.c["bit_errors"][c] += int(e["ecdd"])
                logged += 1
            self.ev["wraps"] += at + logged > self.E
            self.ev["call_larger_than_ring"] += logged > self.E
            self.c["lost"][c] = max(len(self.entries[c]) - self.E, 0)
        self.n += 1

    def log(self, c, max_entries=None):
        """what get_log returns: the newest min(written, log_entries, max) entries, oldest first"""
        n = min(len(self.entries[c]), self.E if max_entries is None else min(self.E, max_entries))
        return np.array(self.entries[c][len(self.entries[c]) - n:], dtype=ENTRY).reshape(n)

    def counters(self):
        return dict(self.c)


N0, STEP = 2000, 4                            # the demodulator's N and its timing step of the tables: nin is N - STEP, N or N + STEP
FILT = 1
# floats that show a copy from an arithmetic result: a denormal, the largest and the smallest normal numbers, negative zero
SPECIAL = np.array([1e-42, 3.4028235e38, 1.1754944e-38, -0.0, 1.0, 2.5e-7], dtype=np.float32)


def _rows(rng, nf, want, every_row_logged=False):
    """nf rows of one channel: statuses of every kind, sources 1 (filtered), 2 and 3, payloads a few bit errors off the test payload"""
    kb = want.size
    if every_row_logged:
        st = np.full(nf, SYNC | BITS, np.uint8)
    else:
        st = rng.choice(np.array([0, 1, SYNC, SYNC | BITS, SYNC | BITS, BITS, SYNC | 8, SYNC | BITS | 8], np.uint8), nf)
    pl = np.tile(want, (nf, 1))
    pl[:, 0] = rng.choice([2, 3] if every_row_logged else [FILT, 2, 3], nf)
    pl[:, 1] = rng.integers(0, 256, nf)
    for f in range(nf):
        for _ in range(int(rng.integers(0, 4))):
            pl[f, rng.integers(0, kb)] ^= 1 << int(rng.integers(0, 8))         # bytes 0, 1 and the CRC's included: those do not count
    info = rng.integers(0, 50, (nf, INFO)).astype(np.int32)
    info[:, 4] = rng.choice([0, 1, 15, 255, 256, 1000], nf)
    info[:, 6] = np.where(rng.random(nf) < 0.7, rng.integers(0, 500, nf), -1)   # decoded or not, whatever the status says
    stats = rng.normal(size=(nf, STATS)).astype(np.float32)
    stats[:, 6] = N0 + STEP * rng.integers(-1, 2, nf)
    stats[:, 8] = np.abs(stats[:, 8]) * 1e-3
    stats[:, 9] = np.abs(stats[:, 9]) * 1e-6
    k = rng.random(nf) < 0.3
    stats[k, 8] = rng.choice(SPECIAL, int(k.sum()))
    k = rng.random(nf) < 0.3
    stats[k, 9] = rng.choice(SPECIAL, int(k.sum()))
    return st, pl, info, stats


LOG_ENTRIES = 8
# rows per call and channel (three receive channels): 65 and 130 rows cross the kernel's chunk of 64 once and twice, the call of 20
# logs more rows than the ring holds
ROWS = [[5, 0, 3], [65, 1, 0], [0, 0, 0], [130, 2, 7], [20, 3, 1], [1, 0, 64]]


def log_calls(want, rows=ROWS, seed=5):
    """the hand-made calls of the log tests: list over calls of [(status, payload, info, stats)] * 3"""
    rng = np.random.default_rng(seed)
    want = np.asarray(want, dtype=np.uint8)
    calls = [[_rows(rng, nf, want, every_row_logged=(n == 4 and c == 0)) for c, nf in enumerate(per)] for n, per in enumerate(rows)]
    # call 0, channel 2: nin of N - STEP, N and N + STEP in one call; channel 0: a filtered frame and a decoded frame with a bad CRC
    calls[0][2][3][:, 6] = [N0 - STEP, N0, N0 + STEP]
    st, pl, info, _ = calls[0][0]
    st[1], pl[1, 0], info[1, 6] = SYNC | BITS, FILT, 40
    st[2], info[2, 6] = SYNC, 40
    return calls


def recut(calls, seed):
    """the same rows per channel, cut into other calls (some of them empty)"""
    rng = np.random.default_rng(seed)
    nrx, ncalls = len(calls[0]), len(calls) + 2
    cat = [[np.concatenate([call[c][k] for call in calls]) for k in range(4)] for c in range(nrx)]
    cuts = [np.concatenate([[0], np.sort(rng.integers(0, len(cat[c][0]) + 1, ncalls - 1)), [len(cat[c][0])]]) for c in range(nrx)]
    return [[tuple(x[cuts[c][p]:cuts[c][p + 1]] for x in cat[c]) for c in range(nrx)] for p in range(ncalls)]


def run_log(calls, want, log_entries=LOG_ENTRIES, filt=FILT, nin0=N0):
    m = Log(len(calls[0]), nin0, filt, log_entries, want)
    for rows in calls:
        m.call(rows)
    return m


def same_but_call_and_row(a, b):
    """two logs equal in every field except call and row"""
    names = [n for n in ENTRY.names if n not in ("call", "row")]
    return a.shape == b.shape and all(a[n].tobytes() == b[n].tobytes() for n in names)
