"""Host model of the streaming transmitter's queues (include/pirip_hip.h section K), for tests/test_txs*.py: per channel
a ring of `cap` symbols with all-or-nothing append, pop of up to S symbols per call padded with carrier off, and the underrun / refused
counters. It returns each channel's symbol timeline -- what section I's modulator and section J's multiplexer are run on, in one piece,
to get the bytes the device must give -- and notes which of the queue's paths a schedule reaches.

A schedule is a list of steps, ("S", [(r0, r1) | None per channel]) -- offer records [r0, r1) of the channel's plan -- or ("P",). It is
made by running the model itself under a fixed policy (make_schedule), so that it is known before the device sees it."""
import numpy as np

OFF = 0xFF
PRE, FRAME, GAP = 0, 1, 2


def record_lens(ctl, pre_syms, frame_syms, gap):
    """symbols each record makes: 1 preamble + frame, 0 frame, 2 the gap, anything else nothing"""
    return [pre_syms + frame_syms if c == 1 else frame_syms if c == 0 else gap if c == 2 else 0 for c in ctl]


def record_tags(ctl, pre_syms, frame_syms, gap):
    """per record (kind int8 [len], pos int32 [len]): what each of its symbols is, and where in its frame (or preamble, or gap) it lies"""
    out = []
    for c in ctl:
        if c == 1:
            out.append((np.r_[np.full(pre_syms, PRE), np.full(frame_syms, FRAME)].astype(np.int8), np.r_[np.arange(pre_syms), np.arange(frame_syms)]))
        elif c == 0:
            out.append((np.full(frame_syms, FRAME, np.int8), np.arange(frame_syms)))
        elif c == 2:
            out.append((np.full(gap, GAP, np.int8), np.arange(gap)))
        else:
            out.append((np.zeros(0, np.int8), np.zeros(0, np.int64)))
    return out


class Model:
    """nchan queues. send(offers): offers[c] = None or (symbols uint8, kind, pos) -> taken [nchan] bool; process() -> sent [nchan]."""

    def __init__(self, nchan, S, cap):
        self.nchan, self.S, self.cap = nchan, S, cap
        self.reset()

    def reset(self):
        K = self.nchan
        self.ring = np.full((K, self.cap), OFF, np.uint8)
        self.kind = np.full((K, self.cap), -1, np.int8)
        self.pos = np.zeros((K, self.cap), np.int64)
        self.head, self.tail = [0] * K, [0] * K
        self.sent, self.underrun, self.refused = np.zeros(K, np.int64), np.zeros(K, np.int64), np.zeros(K, np.int64)
        self.timeline = [[] for _ in range(K)]
        self.calls = 0
        # which paths were reached
        self.wraps = 0                          # appends or pops that cross the end of the ring
        self.mid_frame_starts = 0               # calls whose first dequeued symbol lies inside a frame, not at its start
        self.last_kind = [-1] * K               # kind of the channel's last dequeued symbol
        self.open_gap_underrun = [False] * K    # the channel ran dry behind a gap symbol and has sent nothing since
        self.gap_underruns = 0                  # ... and then sent more: an underrun enclosed in a burst's gap

    def queued(self):
        return np.array([t - h for h, t in zip(self.head, self.tail)], np.int64)

    def send(self, offers):
        taken = np.zeros(self.nchan, bool)
        for c, off in enumerate(offers):
            if off is None:
                continue
            sy, kind, pos = off
            n = len(sy)
            if n > self.cap - (self.tail[c] - self.head[c]):
                self.refused[c] += 1
                continue
            at = (self.tail[c] + np.arange(n)) % self.cap
            if n and at[0] + n > self.cap:
                self.wraps += 1
            self.ring[c, at], self.kind[c, at], self.pos[c, at] = sy, kind, pos
            self.tail[c] += n
            taken[c] = True
        return taken

    def process(self):
        sent = np.zeros(self.nchan, np.int64)
        for c in range(self.nchan):
            n = min(self.S, self.tail[c] - self.head[c])
            at = (self.head[c] + np.arange(n)) % self.cap
            if n and at[0] + n > self.cap:
                self.wraps += 1
            row = np.full(self.S, OFF, np.uint8)
            row[:n] = self.ring[c, at]
            self.timeline[c].append(row)
            if n:
                if self.kind[c, at[0]] == FRAME and self.pos[c, at[0]] > 0:
                    self.mid_frame_starts += 1
                if self.open_gap_underrun[c]:
                    self.gap_underruns += 1
                    self.open_gap_underrun[c] = False
                self.last_kind[c] = int(self.kind[c, at[-1]])
            if n < self.S and self.last_kind[c] == GAP:
                self.open_gap_underrun[c] = True
            self.head[c] += n
            self.sent[c] += n
            self.underrun[c] += self.S - n
            sent[c] = n
        self.calls += 1
        return sent

    def timelines(self):
        """uint8 [nchan, calls * S]"""
        return np.stack([np.concatenate(t) if t else np.zeros(0, np.uint8) for t in self.timeline])


def offer(ctl, lens, syms, tags, r0, r1):
    """records [r0, r1) of one channel as a Model offer; syms: the channel's symbols record after record (None: zeros, for a model run
    that only counts)"""
    a, b = int(np.sum(lens[:r0])), int(np.sum(lens[:r1]))
    kind = np.concatenate([tags[r][0] for r in range(r0, r1)]) if r1 > r0 else np.zeros(0, np.int8)
    pos = np.concatenate([tags[r][1] for r in range(r0, r1)]) if r1 > r0 else np.zeros(0, np.int64)
    return (np.zeros(b - a, np.uint8) if syms is None else syms[a:b]), kind, pos


def burst_ends(ctl):
    """index behind each burst of a plan: the records up to and including a 2 (and the plan's end)"""
    ends = [i + 1 for i, c in enumerate(ctl) if c == 2]
    if not ends or ends[-1] != len(ctl):
        ends.append(len(ctl))
    return ends


def make_schedule(plans, lens, tags, S, cap, tail_calls=2):
    """The policy, run on the model: before every process call each channel is offered its next burst, again and again while it is
    refused -- except that after every second burst the channel waits until its queue has run dry and one more call has passed, so that
    an underrun falls behind that burst's gap. Channel c starts c calls late. Ends tail_calls calls after everything was sent."""
    K = len(plans)
    m = Model(K, S, cap)
    ends = [burst_ends(p) for p in plans]
    nxt, bi = [0] * K, [0] * K
    wait = [None] * K                          # None, ("dry", underruns when the burst went in) or ("until", call)
    steps = []
    while True:
        offers, marks = [None] * K, [None] * K
        for c in range(K):
            if bi[c] >= len(ends[c]) or m.calls < c:
                continue
            if wait[c] is not None:
                if wait[c][0] == "dry" or m.calls < wait[c][1]:
                    continue
                wait[c] = None
            offers[c] = offer(plans[c], lens[c], None, tags[c], nxt[c], ends[c][bi[c]])
            marks[c] = (nxt[c], ends[c][bi[c]])
        if any(o is not None for o in offers):
            taken = m.send(offers)
            steps.append(("S", marks))
            for c in range(K):
                if taken[c]:
                    nxt[c] = ends[c][bi[c]]
                    bi[c] += 1
                    if bi[c] % 2 == 0:
                        wait[c] = ("dry", int(m.underrun[c]))
        m.process()
        steps.append(("P",))
        for c in range(K):
            if wait[c] is not None and wait[c][0] == "dry" and m.underrun[c] > wait[c][1]:
                wait[c] = ("until", m.calls + 1)
        if all(bi[c] >= len(ends[c]) for c in range(K)) and not m.queued().any():
            break
        assert m.calls < 100000, "the schedule does not end: a burst larger than the queue?"
    steps += [("P",)] * tail_calls
    return steps


def cli_schedule(plans, lens, tags, S, cap):
    """fsk_ldpc_tx_channels --block's policy, run on the model: before every block each channel is offered its next burst again and again
    until one is refused or its input is exhausted; the end is when every input is exhausted and every queue is empty"""
    K = len(plans)
    m = Model(K, S, cap)
    ends = [burst_ends(p) if p else [] for p in plans]
    nxt, bi = [0] * K, [0] * K
    steps = []
    while True:
        refused = [False] * K
        while True:
            marks = [None if refused[c] or bi[c] >= len(ends[c]) else (nxt[c], ends[c][bi[c]]) for c in range(K)]
            if all(mk is None for mk in marks):
                break
            taken = m.send([None if mk is None else offer(plans[c], lens[c], None, tags[c], mk[0], mk[1]) for c, mk in enumerate(marks)])
            steps.append(("S", marks))
            for c, mk in enumerate(marks):
                if mk is None:
                    continue
                if taken[c]:
                    nxt[c] = mk[1]
                    bi[c] += 1
                else:
                    refused[c] = True
        if all(bi[c] >= len(ends[c]) for c in range(K)) and not m.queued().any():
            return steps
        m.process()
        steps.append(("P",))


def replay(steps, plans, lens, tags, syms, S, cap, on_send=None, on_process=None):
    """runs the steps on a fresh model; on_send(marks, taken) / on_process(sent) see every step's result -> the model"""
    m = Model(len(plans), S, cap)
    for st in steps:
        if st[0] == "S":
            offers = [None if mk is None else offer(plans[c], lens[c], None if syms is None else syms[c], tags[c], mk[0], mk[1])
                      for c, mk in enumerate(st[1])]
            taken = m.send(offers)
            if on_send:
                on_send(st[1], taken)
        else:
            sent = m.process()
            if on_process:
                on_process(sent)
    return m


# ---------------------------------------------------------------- the shapes tests/test_txs.py runs, and their record plans
FIR, LINEAR = 0, 1
CODE_N, CODE_K = 136, 104                     # the smallest accumulator code of tests/test_tx_shapes.py: a frame is 168 bits
PLANS = [[1, 2, 1, 2, 1, 2], [1, 0, 2, 1, 2, 0, 2], [1, 2, 1, 2, 7, 1, 2]]     # a frame without preamble; a control byte that sends nothing
GAP_SYMS = 7

# name -> dict: wideband Fs, D, kind, transition_bw, Rs, M, f1 per channel, shift, offsets, outputs, noutputs, S, pad (the output rows
# start `pad` samples off their 16-byte alignment), and what the shape is for: Q and H as the handle must report them
SHAPES = {
    "h0_lin_d1": dict(Fs=40000, D=1, kind=LINEAR, tbw=0.05, Rs=1000, M=2, f1=[1000, -7000], shift=2000, offsets=[0, 5001], outputs=None,
                      noutputs=1, S=3, pad=0, Q=1, H=0),
    "h1_d6_outs": dict(Fs=240000, D=6, kind=FIR, tbw=0.05, Rs=1000, M=2, f1=[1000, -7000, 3001, 1000, -15000], shift=2000,
                       offsets=[-90000, -30000, 30001, 90000, 7], outputs=[0, 2, 0, 2, 2], noutputs=3, S=1, pad=1, Q=14, H=1),
    "h2_ts8": dict(Fs=240000, D=6, kind=FIR, tbw=0.05, Rs=5000, M=4, f1=[1000, -17000, 2001], shift=5000, offsets=[-60000, 1, 60000],
                   outputs=None, noutputs=1, S=3, pad=0, Q=14, H=2),
    "h2_long": dict(Fs=240000, D=6, kind=FIR, tbw=0.0125, Rs=1000, M=2, f1=[1000, 5000], shift=2000, offsets=[-119999, 60001], outputs=None,
                    noutputs=1, S=1, pad=0, Q=54, H=2),
    "h10_d1": dict(Fs=40000, D=1, kind=FIR, tbw=0.05, Rs=5000, M=4, f1=[1000, -16000], shift=5000, offsets=[0, -5000], outputs=None,
                   noutputs=1, S=3, pad=3, Q=79, H=10),
    # a block of 2400 samples: two tiles of 2048 outputs
    "tile_d30": dict(Fs=1200000, D=30, kind=FIR, tbw=0.05, Rs=1000, M=2, f1=[1000, -3000], shift=2000, offsets=[-500003, 1], outputs=None,
                     noutputs=1, S=2, pad=0, Q=3, H=1),
    # 9 channels on one output: two staging groups
    "k9_d6": dict(Fs=240000, D=6, kind=FIR, tbw=0.05, Rs=1000, M=4, f1=[1000 + 17 * c for c in range(9)], shift=2000,
                  offsets=[-100000 + 25000 * c for c in range(9)], outputs=None, noutputs=1, S=7, pad=0, Q=14, H=1),
}


def shape_plans(name):
    """(plans, lens, tags, cap) of a shape: channel c runs PLANS[c % 3]; the queue holds the largest burst and S + 3 symbols more, so that
    the burst behind it is refused until the first has drained and then goes in across the end of the ring"""
    sh = SHAPES[name]
    bps = 1 if sh["M"] == 2 else 2
    pre, frame = 50 * (sh["M"] // 2), (32 + CODE_N) // bps
    K = len(sh["f1"])
    plans = [PLANS[c % 3] for c in range(K)]
    lens = [record_lens(p, pre, frame, GAP_SYMS) for p in plans]
    tags = [record_tags(p, pre, frame, GAP_SYMS) for p in plans]
    burst = max(sum(l[a:b]) for p, l in zip(plans, lens) for a, b in zip([0] + burst_ends(p)[:-1], burst_ends(p)))
    return plans, lens, tags, burst + sh["S"] + 3
