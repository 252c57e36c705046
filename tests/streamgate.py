"""The stream gate: does every step of a call run on the caller's stream, and does the host return without waiting?

A *family* (tests/streamshapes.py FAMILIES) is a handle or a stack of handles with a short fixed sequence of calls. build(name, seed)
makes a Case of fresh handles: its input buffers (each with the real input in a staging tensor and a decoy of the same format in place),
its output tensors, the calls as functions of a stream, and what the handles expose of their device state.

reference() runs the calls on the null stream with a synchronise after each: the run the family's own test holds to its model.
gated() runs them on a non-blocking side stream behind a spin kernel (the gate): the real inputs are copied into place behind the gate,
so a step that leaves the stream runs during the gate, on the decoy or ahead of the step that feeds it, and the bytes differ; a call
that waits for the stream returns after the gate has drained, and side.query() says so. Nothing here restates a model."""
import time

import numpy as np

import sigutil
import streamshapes as ss

CANARY = 0xA5
NON_BLOCKING = 1                                           # hipStreamNonBlocking


class Case:
    """ins: [(dst, real, decoy)] device tensors of one shape; outs: name -> device tensor; calls: [(entry point, fn(stream))];
    reset: fn(stream) or None; sane: fn(reference result) or None; rings: name -> (device pointer, bytes) of state the handles expose; counters: () -> name -> numpy array
    (synchronises); keep: what must stay alive"""

    def __init__(self):
        self.ins, self.outs, self.calls, self.reset, self.rings, self.counters, self.keep, self.sane = [], {}, [], None, {}, None, [], None

    def add_in(self, real, decoy):
        """real, decoy: numpy arrays of one shape and type -> the device tensor the calls read (holds the decoy)"""
        import torch
        assert real.shape == decoy.shape and real.dtype == decoy.dtype and not np.array_equal(real, decoy), "a decoy must differ"
        r, d = torch.from_numpy(np.ascontiguousarray(real)).cuda(), torch.from_numpy(np.ascontiguousarray(decoy)).cuda()
        dst = d.clone()
        self.ins.append((dst, r, d))
        return dst

    def add_in_dev(self, dst, real, decoy):
        """the same for tensors that are on the device already (dst may be a view of a handle's own landing zone)"""
        import torch
        assert real.shape == decoy.shape == dst.shape and not torch.equal(real, decoy), "a decoy must differ"
        dst.copy_(decoy)
        self.ins.append((dst, real, decoy))
        return dst

    def add_out(self, name, shape, dtype):
        import torch
        t = torch.empty(shape, dtype=dtype, device="cuda")
        t.view(torch.uint8).fill_(CANARY)
        self.outs[name] = t
        return t

    def close(self):
        for h in self.keep:
            if hasattr(h, "close"):
                h.close()


_rt = None


def runtime():
    global _rt
    if _rt is None:
        import ctypes as C
        _rt = sigutil.hip_runtime()
        _rt.hipStreamGetFlags.argtypes = [C.c_void_p, C.POINTER(C.c_uint)]
    return _rt


def copy_on(stream, dst, src, n):
    """n bytes device to device, enqueued on `stream` (an int)"""
    assert runtime().hipMemcpyAsync(dst, src, n, 3, stream or None) == 0


def view_bytes(ptr, n):
    """a uint8 tensor over n bytes of device memory that a handle owns (the handle must outlive it)"""
    import torch

    class _Mem:
        __cuda_array_interface__ = {"shape": (n,), "typestr": "|u1", "data": (ptr, False), "version": 2}
    return torch.as_tensor(_Mem(), device="cuda")


def assert_non_blocking(side):
    """a blocking side stream would wait for the null stream and the null stream for it: the gate could not tell a misrouted step"""
    import ctypes as C
    flags = C.c_uint(0xFFFF)
    assert runtime().hipStreamGetFlags(side.cuda_stream, C.byref(flags)) == 0
    assert flags.value & NON_BLOCKING, f"torch.cuda.Stream() is a blocking stream here (flags {flags.value:#x}): the gated tests cannot conclude"


_cycles_per_ms = None


def cycles_per_ms():
    """torch.cuda._sleep counts device clocks: one short sleep between two events, once per session"""
    global _cycles_per_ms
    if _cycles_per_ms is None:
        import torch
        torch.cuda._sleep(1000)                            # (the kernel's first launch loads it)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        n = 20_000_000
        a.record()
        torch.cuda._sleep(n)
        b.record()
        torch.cuda.synchronize()
        _cycles_per_ms = n / max(a.elapsed_time(b), 1e-3)
    return _cycles_per_ms


PROBE_MS, PROBE_TRIES = 20, 12
_pool, _held = [], []


def runs_beside_the_null_stream(side):
    """Streams share a few hardware queues, which the runtime hands out as streams are made, and a queue runs its work in order: a side
    stream on the null stream's queue would hold a step misrouted to the null stream back behind the gate, in its proper place, and the
    gate would see nothing. So: a short spin on `side`, one small kernel on the null stream behind it -- does that kernel finish while
    the spin still runs?"""
    import torch
    assert torch.cuda.default_stream().cuda_stream == 0 and torch.cuda.current_stream().cuda_stream == 0, "the probe is for the null stream"
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    done = torch.cuda.Event()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        torch.cuda._sleep(int(PROBE_MS * cycles_per_ms()))
    word.add_(1)
    done.record()
    t0 = time.perf_counter()
    while not done.query() and (time.perf_counter() - t0) * 1e3 < PROBE_MS / 2:
        pass
    beside = done.query() and not side.query()
    side.synchronize()
    torch.cuda.synchronize()
    return beside


def side_stream(k=0):
    """the k-th of this session's side streams: non-blocking, and shown -- again at every use -- to run beside the null stream"""
    import torch
    tried = 0
    while True:
        while len(_pool) <= k:
            assert tried < PROBE_TRIES, (f"none of {tried} new streams runs beside the null stream (they share its hardware queue): "
                                         "the gated tests cannot conclude")
            s = torch.cuda.Stream()
            tried += 1
            assert_non_blocking(s)
            if runs_beside_the_null_stream(s):
                _pool.append(s)
            else:
                _held.append(s)                            # (kept: a stream that is let go gives its place to the next one made)
        if runs_beside_the_null_stream(_pool[k]):
            return _pool[k]
        _held.append(_pool.pop(k))


def _fill(case):
    import torch
    for dst, _, decoy in case.ins:
        dst.copy_(decoy)
    for t in case.outs.values():
        t.view(torch.uint8).fill_(CANARY)


def _snap_alloc(case):
    import torch
    snap = {"out:" + k: torch.empty_like(t) for k, t in case.outs.items()}
    snap.update({"ring:" + k: torch.empty(n, dtype=torch.uint8, device="cuda") for k, (_, n) in case.rings.items()})
    return snap


def _snap_on(case, snap, stream):
    """copies of every output and exposed ring, enqueued on `stream`"""
    for k, t in case.outs.items():
        copy_on(stream, snap["out:" + k].data_ptr(), t.data_ptr(), t.numel() * t.element_size())
    for k, (p, n) in case.rings.items():
        copy_on(stream, snap["ring:" + k].data_ptr(), p() if callable(p) else p, n)    # (a callable: host state that names the last call's rows)


def _host(snap):
    return {k: t.cpu().numpy().reshape(-1).view(np.uint8).copy() for k, t in snap.items()}


def reference(case):
    """the calls on the null stream, each followed by a synchronise -> name -> bytes (outputs, rings, then counters)"""
    import torch
    _fill(case)
    for dst, real, _ in case.ins:
        dst.copy_(real)
    torch.cuda.synchronize()
    for _, fn in case.calls:
        fn(0)
        torch.cuda.synchronize()
    snap = _snap_alloc(case)
    _snap_on(case, snap, 0)
    torch.cuda.synchronize()
    res = _host(snap)
    if case.counters:
        res.update({"counter:" + k: np.ascontiguousarray(v).reshape(-1).view(np.uint8).copy() for k, v in case.counters().items()})
    return res


class Gate:
    """one gated side stream over one case"""

    def __init__(self, case, gate_ms, k=0):
        self.case, self.gate_ms = case, gate_ms
        self.side = side_stream(k)
        self.snaps = [_snap_alloc(case), _snap_alloc(case)]
        self.enqueue_ms = 0.0
        _fill(case)

    def open(self):
        """the gate, then the real inputs into place behind it (after a synchronise: decoys and canaries are in place)"""
        import torch
        cycles = int(self.gate_ms * cycles_per_ms())
        self.t0 = time.perf_counter()
        with torch.cuda.stream(self.side):
            torch.cuda._sleep(cycles)
        self._place()

    def _place(self):
        import torch
        with torch.cuda.stream(self.side):
            for dst, real, _ in self.case.ins:
                dst.copy_(real, non_blocking=True)

    def check(self, what):
        self.enqueue_ms = (time.perf_counter() - self.t0) * 1e3
        assert not self.side.query(), (f"{what}: the side stream had drained when the call returned, {self.enqueue_ms:.2f} ms after the gate of "
                                       f"{self.gate_ms:.0f} ms was enqueued -- the call waited for its stream (or the host took longer than the gate)")
        # a call that waits for its stream and then enqueues more leaves the stream busy: it shows in the time alone. The gate is at least
        # four times what the host needs for the whole sequence, so a return in the gate's second half is a wait, not a slow host.
        assert self.enqueue_ms < self.gate_ms / 2, (f"{what}: returned {self.enqueue_ms:.2f} ms after the gate of {self.gate_ms:.0f} ms was enqueued, "
                                                    f"the whole sequence takes the host about {ss.FAMILIES[self.case.name]['enqueue_ms']} ms -- the call waited "
                                                    "for its stream")

    def call(self, i):
        name, fn = self.case.calls[i]
        fn(self.side.cuda_stream)
        self.check(f"call {i} ({name})")

    def finish_pass(self, k):
        _snap_on(self.case, self.snaps[k], self.side.cuda_stream)

    def again(self):
        """reset where the family has one, canaries, decoys and the real inputs once more -- all on the side stream"""
        import torch
        if self.case.reset:
            self.case.reset(self.side.cuda_stream)
            self.check("reset")
        with torch.cuda.stream(self.side):
            for t in self.case.outs.values():
                t.view(torch.uint8).fill_(CANARY)
            for dst, _, decoy in self.case.ins:
                dst.copy_(decoy, non_blocking=True)
        self._place()

    def results(self):
        """after the synchronise: per pass name -> bytes, the counters with the last pass"""
        res = [_host(s) for s in self.snaps]
        if self.case.counters:
            res[-1].update({"counter:" + k: np.ascontiguousarray(v).reshape(-1).view(np.uint8).copy()
                            for k, v in self.case.counters().items()})
        return res


def gated(case, gate_ms, passes=2):
    """-> ([pass 0's bytes, pass 1's bytes], enqueue time in ms of everything behind the gate)"""
    import torch
    g = Gate(case, gate_ms)
    torch.cuda.synchronize()
    g.open()
    for k in range(passes):
        if k:
            g.again()
        for i in range(len(case.calls)):
            g.call(i)
        g.finish_pass(k)
    g.check("the last snapshot")
    g.side.synchronize()
    torch.cuda.synchronize()
    g.snaps = g.snaps[:passes]
    return g.results(), g.enqueue_ms


def gated_pair(case_a, case_b, gate_ms):
    """two cases of one family on two gated side streams at once, call by call -> ([a's bytes], [b's bytes], enqueue ms)"""
    import torch
    ga, gb = Gate(case_a, gate_ms, 0), Gate(case_b, gate_ms, 1)
    assert ga.side.cuda_stream != gb.side.cuda_stream
    torch.cuda.synchronize()
    ga.open()
    gb.open()
    gb.t0 = ga.t0
    for i in range(len(case_a.calls)):
        ga.call(i)
        gb.call(i)
    ga.finish_pass(0)
    gb.finish_pass(0)
    ga.check("the last snapshot")
    gb.check("the last snapshot")
    ga.side.synchronize()
    gb.side.synchronize()
    torch.cuda.synchronize()
    ga.snaps, gb.snaps = ga.snaps[:1], gb.snaps[:1]
    return ga.results()[0], gb.results()[0], gb.enqueue_ms


def same(got, want, what):
    """bytes for bytes, every name"""
    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    for k in sorted(want):
        if not np.array_equal(got[k], want[k]):
            bad = np.flatnonzero(got[k] != want[k]) if got[k].shape == want[k].shape else []
            raise AssertionError(f"{what}: {k} differs from the reference run in {len(bad)} of {want[k].size} bytes"
                                 f"{', the first at ' + str(int(bad[0])) if len(bad) else ''}")


_references = {}


def reference_of(name, seed, oracle=None):
    """the reference run of (family, seed), once per session: (bytes, the decoy's bytes where the family keeps them)"""
    key = (name, seed)
    if key not in _references:
        case = build(name, seed, oracle)
        res = reference(case)
        assert not case.outs or any(k.startswith("out:") and (v != CANARY).any() for k, v in res.items()), "the reference run wrote nothing"
        if case.sane:
            case.sane(res)                                 # the sequence reaches what the family is for
        _references[key] = res
        case.close()
    return _references[key]


def run_family(name, oracle=None, record_property=None):
    """the gated test of a family: both passes equal the reference run"""
    fam = ss.FAMILIES[name]
    want = reference_of(name, 0, oracle)
    case = build(name, 0, oracle)
    got, ms = gated(case, fam["gate_ms"])
    if record_property:
        record_property("enqueue_ms", round(ms, 3))
        record_property("gate_ms", fam["gate_ms"])
    print(f"{name}: {2 * len(case.calls)} calls enqueued in {ms:.2f} ms behind a gate of {fam['gate_ms']} ms")
    same({k: v for k, v in got[0].items()}, {k: v for k, v in want.items() if not k.startswith("counter:")}, name + ", first pass")
    same(got[1], want, name + ", second pass (behind reset)")
    case.close()
    return ms


def run_pair(name, oracle=None, record_property=None):
    """the pairs test of a family: seeds 0 and 1 on two side streams at once, each equal to its own reference run"""
    fam = ss.FAMILIES[name]
    wa, wb = reference_of(name, 0, oracle), reference_of(name, 1, oracle)
    assert any(not np.array_equal(wa[k], wb[k]) for k in wa), "the two seeds should give different results"
    ca, cb = build(name, 0, oracle), build(name, 1, oracle)
    a, b, ms = gated_pair(ca, cb, fam["gate_ms"])
    if record_property:
        record_property("enqueue_ms", round(ms, 3))
        record_property("gate_ms", fam["gate_ms"])
    print(f"{name}: 2 x {len(ca.calls)} calls enqueued in {ms:.2f} ms behind gates of {fam['gate_ms']} ms")
    same(a, wa, name + ", seed 0 beside seed 1")
    same(b, wb, name + ", seed 1 beside seed 0")
    ca.close()
    cb.close()
    return ms


# ---- the families ---------------------------------------------------------------------------------------------------------------------------
BUILDERS = {}


def family(name):
    def deco(fn):
        BUILDERS[name] = fn
        return fn
    return deco


def build(name, seed, oracle=None):
    case = BUILDERS[name](seed, oracle)
    case.name = name
    assert [c for c, _ in case.calls] == ss.FAMILIES[name]["sequence"], (name, [c for c, _ in case.calls])
    return case


@family("tbits")
def _tbits(seed, oracle):
    """push (rows of one bit per byte), push (packed rows), and push_records on a second counter: nothing comes out but the counters"""
    import pirip_amd
    import tbitsshapes as ts
    c = Case()
    d = ss.tbits_inputs(seed)
    tb = pirip_amd.HipTestBits(nstreams=d["rows"][0].shape[0])
    rec = pirip_amd.HipTestBits(nstreams=d["status"][0].shape[0])
    rec.set_payload(ts.REC_DB)
    c.keep += [tb, rec]
    t = {k: c.add_in(*v) for k, v in d.items()}
    rb = ts.SYN["row_bits"]
    c.calls = [
        ("pirip_hip_tbits_push", lambda st: tb.push(t["rows"], nframes=t["nframes"], row_bits=rb, stream=st)),
        ("pirip_hip_tbits_push", lambda st: tb.push(t["packed"], nframes=t["nframes_packed"], row_bits=rb, packed=True, stream=st)),
        ("pirip_hip_tbits_push_records", lambda st: rec.push_records(t["status"], t["payload"], t["info"], ncalls=t["ncalls"], stream=st)),
    ]

    def reset(st):
        tb.reset(stream=st)
        rec.reset(stream=st)
    c.reset = reset
    c.rings["counters"] = (tb.counters_device(), tb.nstreams * 32)
    c.counters = lambda: dict(list(tb.counters().items()) + [("rec_" + k, v) for k, v in rec.record_counters().items()])
    return c


@family("spec")
def _spec(seed, oracle):
    """push x 3 in uneven calls, rows and bands out: the host remembers where in the tail the next call begins"""
    import torch
    import specshapes as sh
    from test_spectrum import _handle
    c = Case()
    nfft, hop, fmt, avg = ss.SPEC["case"]
    h = _handle(nfft, hop, fmt, avg)
    c.keep.append(h)
    iq = c.add_in(*ss.spec_inputs(seed)["iq"])
    n, R, nb = iq.shape[1], ss.SPEC["rows"], len(sh.bands(nfft))
    rows = c.add_out("rows", (sh.NSTREAMS, R, nfft), torch.float32)
    bands = c.add_out("bands", (nb, R, 12), torch.uint8)
    spare_r = c.add_out("no_rows", (sh.NSTREAMS, 1, nfft), torch.float32)          # what a call that completes nothing is handed
    spare_b = c.add_out("no_bands", (nb, 1, 12), torch.uint8)
    done, at = [0], [0]

    def push(k):
        def fn(st):
            m = h.nrows(k)
            assert done[0] + m < R, "room for a row more than the input completes"
            r, b = (rows, bands) if m else (spare_r, spare_b)
            h.push_raw(_p(iq) + at[0] * 2, n * 2, k, _p(r) + (done[0] * nfft * 4 if m else 0), nfft, R * nfft if m else nfft,
                       _p(b) + (done[0] * 12 if m else 0), R if m else 1, stream=st)
            done[0] += m
            at[0] += k
        return ("pirip_hip_spec_push", fn)

    c.calls = [push(k) for k in ss.spec_cuts(n)]

    def reset(st):
        h.reset(stream=st)
        done[0] = at[0] = 0
    c.reset = reset
    return c


@family("air")
def _air(seed, oracle):
    """per handle (static paths, drifting paths, fading paths): push 4500, set_sigma, push 1800 -- the second push reads every delay's first
    samples from the rings, behind the carry step; noise on throughout"""
    import torch
    import pirip_amd
    import airshapes as sh
    c = Case()
    a = ss.AIR
    Fs = a["Fs"]
    _, paths = sh.inputs(Fs, "u8", seed=seed)
    kw = dict(sigma=sh.SIGMA, seed=sh.SEED + seed)
    drifting = [p + (0,) for p in paths] + a["drifting"]
    handles = {
        "static": (pirip_amd.HipAir(Fs, paths, sh.NTX, sh.NRX, **kw), 0),
        "drifting": (pirip_amd.HipAir(Fs, drifting, sh.NTX, sh.NRX, max_slip=a["max_slip"], **kw), a["age"]),
        "fading": (pirip_amd.HipAir(Fs, [p + (0,) for p in paths] + a["extra"], sh.NTX, sh.NRX, max_slip=a["max_slip"], fades=a["fades"](len(paths)), **kw), 0),
    }
    iq = c.add_in(*ss.air_inputs(seed)["iq"])
    n = iq.shape[1]
    first, second = sh.CALLS
    assert first + second == n
    for name, (air, age) in handles.items():
        c.keep.append(air)
        out = c.add_out(name, (sh.NRX, n, 2), torch.uint8)
        c.calls += [
            ("pirip_hip_air_push", lambda st, air=air, out=out: air.push(_p(iq), n * 2, first, _p(out), n * 2, stream=st)),
            ("pirip_hip_air_set_sigma", lambda st, air=air: air.set_sigma(a["sigma2"], stream=st)),
            ("pirip_hip_air_push", lambda st, air=air, out=out: air.push(_p(iq) + first * 2, n * 2, second, _p(out) + first * 2, n * 2, stream=st)),
        ]

    def reset(st):
        for air, age in handles.values():
            air.reset(a["n0"], stream=st, age=age)             # age: pirip_hip_air_reset_drift, else pirip_hip_air_reset
            air.set_sigma(sh.SIGMA, stream=st)
    c.reset = reset
    reset(0)
    torch.cuda.synchronize()
    return c


class _Node:
    """a packet terminal of muxshapes' LOOP with calls of S symbols: HipPacket or HipPacketFec over HipRx(chan=...), HipTx and HipTxStream"""

    def __init__(self, source, mf, fec=None, S=None, with_rx=True, **kw):
        import pirip_amd
        import muxshapes as ms
        import pktfecref as fr
        from test_mux import _rx_handles
        from test_packet import FRAME, PRE
        from test_ping import LOOP_GAP, _tx_side
        frames = mf + (fr.r_of(mf, *fec) if fec else 0)
        self.tx, self.mux, self.block, self.txs = _tx_side(ms.LOOP["M"], PRE + frames * FRAME + LOOP_GAP, S=S or ss.LINK["S"])
        self.rx = None
        if with_rx:
            self.dem, self.ld, self.ch = _rx_handles()
            self.rx = pirip_amd.HipRx(self.dem, ldpc=self.ld, chan=self.ch, block=self.block)
        args = dict(rx=self.rx, tx=self.tx, txs=self.txs, source=source, filter=source, address=source, max_frags=mf, ring_entries=8, **kw)
        self.pkt = pirip_amd.HipPacket(**args) if fec is None else pirip_amd.HipPacketFec(max_parity=fec[0], parity_pct=fec[1], **args)
        self.blk = self.block * 2

    def handles(self):
        return [self.pkt] + ([self.rx, self.dem, self.ld, self.ch] if self.rx else []) + [self.txs, self.tx, self.mux]


def far_end_iq(seed, fec):
    """in front of the gate: the far terminal sends one packet per channel, addressed to the near one, behind a block of silence ->
    uint8 tensor [blocks, block * 2] of its wideband output; with fec a frame's worth in the middle of the second data frame is wiped out"""
    import torch
    from test_packet import FRAME, PRE
    _, x = ss.link_inputs(seed, bool(fec))
    B = _Node(ss.LINK["far"], x["mf"], fec, with_rx=False, nrx=1)
    K = ss.LINK["blocks"]
    out = torch.zeros((K, B.blk), dtype=torch.uint8, device="cuda")
    none = torch.zeros(64, dtype=torch.uint8, device="cuda")
    for k in range(K):
        if k == 1:
            B.pkt.send([[b] for b in x["far"]], ss.LINK["own"])
        B.pkt.push_records(none, none, out=out[k], out_stride=B.blk, max_calls=0, status_stride=0, payload_stride=0)
    torch.cuda.synchronize()
    assert (out[0] == 128).all() and (out[1] != 128).any()
    if fec:
        per_sym = B.blk // ss.LINK["S"]
        a = (PRE + FRAME + FRAME // 4) * per_sym
        out[1, a:a + (FRAME // 2) * per_sym] = 128
    for h in B.handles():
        h.close()
    return out


def _link_rings(c, pkt, with_records, tag=""):
    p_rec, stride, p_n = pkt.offered()
    c.rings["offered" + tag], c.rings["noffered" + tag] = (p_rec, pkt.nchan * stride), (p_n, pkt.nchan * 4)
    if with_records:                                       # the receiver's rows of the last process / push
        R = pkt.rx_rows
        c.rings["rx_status"] = (lambda: pkt.records()["status"], pkt.nrx * R)
        c.rings["rx_payload"] = (lambda: pkt.records()["payload"], pkt.nrx * R * pkt.data_bytes)
        c.rings["rx_nframes"] = (lambda: pkt.records()["nframes"], pkt.nrx * 4)


def _packets(pkt):
    out = {}
    for ch in range(pkt.nrx):
        ent, data = pkt.packets(ch)
        out["entries%d" % ch], out["bytes%d" % ch] = ent.view(np.uint8), np.frombuffer(b"".join(data), np.uint8)
    return out


def _link(seed, fec):
    """send (device tensors), push_records (the caller's rows), push x 4 (the far end's wideband blocks through the receiver)"""
    import torch
    c = Case()
    d, x = ss.link_inputs(seed, bool(fec))
    A = _Node(ss.LINK["own"], x["mf"], fec)
    c.keep += A.handles()
    pkt, K = A.pkt, ss.LINK["blocks"]
    far = far_end_iq(seed, fec)
    wide = c.add_in_dev(torch.empty_like(far), far, torch.full_like(far, 128))
    t = {k: c.add_in(*v) for k, v in d.items()}
    npk = torch.from_numpy(x["npk"]).cuda()
    dst = torch.full((4, 2), ss.LINK["far"], dtype=torch.uint8, device="cuda")
    taken = c.add_out("taken", (4,), torch.int32)
    out = c.add_out("iq", (K + 1, A.blk), torch.uint8)
    c.keep += [npk, dst]
    c.calls = [("pirip_hip_pkt_send", lambda st: pkt.send(t["raw"], dst, lengths=t["lengths"], npk=npk, taken=taken, stream=st)),
               ("pirip_hip_pkt_push_records", lambda st: pkt.push_records(t["status"], t["payload"], out=out[0], out_stride=A.blk, ncalls=t["ncalls"], stream=st))]
    zone_ptr, _ = A.rx.input()
    view_bytes(zone_ptr, A.blk).fill_(128)

    def process(st):
        copy_on(st, zone_ptr, _p(wide[0]), A.blk)
        pkt.process(out=out[1], out_stride=A.blk, stream=st)
    c.calls.append(("pirip_hip_pkt_process", process))
    c.calls += [("pirip_hip_pkt_push", lambda st, k=k: pkt.push(wide[k], A.blk, out=out[k + 1], out_stride=A.blk, stream=st)) for k in range(1, K)]
    c.reset = lambda st: pkt.reset(stream=st)
    _link_rings(c, pkt, True)
    c.rings["input"] = (zone_ptr, A.blk)

    def counters():
        got = dict(pkt.counters())
        if fec:
            got.update(pkt.fec_counters())
        got.update(_packets(pkt))
        return got
    c.counters = counters

    def sane(res):
        n = res["counter:delivered"].view(np.int64)
        assert (n >= 1).all(), ("the caller's rows should deliver a packet per channel", n)
        if not fec:
            assert n.sum() > 4, ("the far end's blocks should deliver packets too", n)
        if fec:
            assert res["counter:recovered"].view(np.int64).sum() > 0, "a lost fragment should have been rebuilt"
    c.sane = sane
    return c


@family("pkt")
def _pkt(seed, oracle):
    return _link(seed, None)


@family("fec")
def _fec(seed, oracle):
    import pktfecref as fr
    return _link(seed, fr.SHAPES[ss.FEC_SHAPE][1:])


@family("arq_air")
def _arq_air(seed, oracle):
    """HipArq over a packet terminal with a receiver: submit, process (the block copied into the landing zone on the same stream), push x 3
    on the far end's wideband blocks -- plain datagrams, which the sessions count and leave alone, while the own segments go out"""
    import torch
    import pirip_amd
    c = Case()
    d, x = ss.link_inputs(seed)
    A = _Node(ss.LINK["own"], x["mf"])
    arq = pirip_amd.HipArq(A.pkt, ss.LINK["far"], window=4, rto=2, max_tries=8, out_entries=8)
    c.keep += [arq] + A.handles()
    K = ss.LINK["blocks"]
    far = far_end_iq(seed, None)
    wide = c.add_in_dev(torch.empty_like(far), far, torch.full_like(far, 128))
    seg, lengths = c.add_in(*d["raw"]), c.add_in(*d["lengths"])
    nseg = torch.from_numpy(x["npk"]).cuda()
    taken = c.add_out("taken", (4,), torch.int32)
    out = c.add_out("iq", (K, A.blk), torch.uint8)
    c.keep.append(nseg)
    zone_ptr, _ = A.rx.input()
    view_bytes(zone_ptr, A.blk).fill_(128)

    def process(st):
        copy_on(st, zone_ptr, _p(wide[0]), A.blk)
        arq.process(out[0], A.blk, stream=st)
    c.calls = [("pirip_hip_arq_submit", lambda st: arq.submit(seg, lengths=lengths, nseg=nseg, taken=taken, stream=st)), ("pirip_hip_arq_process", process)]
    c.calls += [("pirip_hip_arq_push", lambda st, k=k: arq.push(wide[k], A.blk, out[k], A.blk, stream=st)) for k in range(1, K)]
    c.reset = lambda st: arq.reset(stream=st)
    _link_rings(c, A.pkt, True)

    def counters():
        got = dict(arq.counters())
        got.update({"pkt_" + k: v for k, v in A.pkt.counters().items()})
        return got
    c.counters = counters

    def sane(res):
        assert res["counter:sent"].view(np.int64).sum() > 0 and res["counter:retransmitted"].view(np.int64).sum() > 0
        assert res["counter:pkt_delivered"].view(np.int64).sum() > 0, "the far end's datagrams should reach the packet layer"
    c.sane = sane
    return c


@family("ldpc")
def _ldpc(seed, oracle):
    """section A and E's batch entry points on the diversity family's four receivers: demod_batch (magnitudes out), ldpc_rx_batch on
    them, clear_estimators, demod_batch again, the LLR stage and the decoder on their own, and the chain as two groups"""
    import ctypes as C
    import torch
    import pirip_amd
    from test_diversity import _demod, _Rows
    c = Case()
    S = ss.div_shape(oracle, seed)
    R = ss.DIV["G"] * ss.DIV["B"]
    iq = c.add_in(*ss.div_inputs(seed, oracle)["iq"])
    nsamp = iq.shape[1]
    dem = _demod(pirip_amd, S, R)
    ld = pirip_amd.HipLdpc(S["path"], S["M"], Nsym=S["Nsym"], nstreams=R)
    halves = [(_demod(pirip_amd, S, R // 2), pirip_amd.HipLdpc(S["path"], S["M"], Nsym=S["Nsym"], nstreams=R // 2)) for _ in range(2)]
    c.keep += [ld, dem] + [h for pair in halves for h in pair]
    maxf, per, spf = dem.max_frames_for(nsamp), S["per"], pirip_amd.STATS_PER_FRAME
    a, b, g = _Rows(torch, pirip_amd, R, maxf, S["kb"], per), _Rows(torch, pirip_amd, R, maxf, S["kb"], per), _Rows(torch, pirip_amd, R, maxf, S["kb"])
    for tag, rows in (("a_", a), ("b_", b), ("g_", g)):
        for k in ("status", "payload", "info", "stats", "nframes", "consumed", "filt"):
            if getattr(rows, k) is not None and not (tag == "b_" and k in ("status", "payload", "info")):
                c.outs[tag + k] = getattr(rows, k)
    ncw = maxf * S["Nbits"] // S["n"]
    llr = c.add_out("llr", (maxf, S["Nbits"]), torch.float32)
    bits = c.add_out("bits", (ncw, S["n"]), torch.uint8)
    itp = c.add_out("iter_pcc", (ncw, 2), torch.int32)

    def demod(rows):
        return lambda st: dem.demod_batch(_p(iq), nsamp * 2, nsamp, 0, 0, _p(rows.filt), maxf * per, _p(rows.stats), maxf * spf, _p(rows.nframes),
                                          _p(rows.consumed), maxf, stream=st)

    def raw(name, *args):
        rc = getattr(ld.L, name)(*args)
        assert rc == 0, (name, rc)

    def groups(st):
        h = R // 2
        pirip_amd.HipLdpc.chain_batch_groups([(halves[i][1], halves[i][0], _p(iq[i * h]), _p(g.status[i * h]), _p(g.payload[i * h]), _p(g.info[i * h]),
                                               _p(g.nframes[i * h:]), _p(g.consumed[i * h:]), _p(g.stats[i * h])) for i in range(2)],
                                             nsamp * 2, nsamp, maxf, stats_stride=maxf * spf, stream=st)
    c.calls = [
        ("pirip_hip_demod_batch", demod(a)),
        ("pirip_hip_ldpc_rx_batch", lambda st: ld.rx_batch(_p(a.filt), maxf * per, _p(a.nframes), maxf, _p(a.status), _p(a.payload), _p(a.info), stream=st)),
        ("pirip_hip_clear_estimators", lambda st: raw("pirip_hip_clear_estimators", dem.h, C.c_void_p(st))),
        ("pirip_hip_demod_batch", demod(b)),
        ("pirip_hip_ldpc_llr", lambda st: raw("pirip_hip_ldpc_llr", ld.h, _p(b.filt), maxf, _p(llr), C.c_void_p(st))),
        ("pirip_hip_ldpc_decode_llr", lambda st: raw("pirip_hip_ldpc_decode_llr", ld.h, _p(llr), ncw, _p(bits), _p(itp), C.c_void_p(st))),
        ("pirip_hip_fsk_ldpc_rx_batch_groups", groups),
    ]

    def reset(st):
        for d_, l_ in [(dem, ld)] + halves:
            d_.reset(stream=st)
            l_.reset(stream=st)
    c.reset = reset

    def sane(res):
        assert (res["out:a_status"] & pirip_amd.RX_BITS).any() and (res["out:g_status"] & pirip_amd.RX_BITS).any(), "some frames should decode"
    c.sane = sane
    # section E: the receiver's work rows grow with the largest call it has seen, and such a call waits for its stream -- once, here
    for _, fn in c.calls:
        fn(0)
    reset(0)
    torch.cuda.synchronize()
    return c


@family("arq")
def _arq(seed, oracle):
    """submit, then push_records x 4 on arqref's rule tables: the segments go out, go out again after two calls without an ACK, and are
    acknowledged; DATA of the peer is delivered and acknowledged"""
    import torch
    from test_arq import _Dev
    c = Case()
    dev = _Dev(ss.arq_node())
    arq, pkt = dev.arq, dev.pkt
    c.keep += [arq, pkt, dev.txs, dev.tx, dev.mux, dev]
    t = {k: c.add_in(*v) for k, v in ss.arq_inputs(seed).items()}
    K = ss.ARQ["calls"]
    taken = c.add_out("taken", (4,), torch.int32)
    out = c.add_out("iq", (K, dev.blk), torch.uint8)
    c.calls = [("pirip_hip_arq_submit", lambda st: arq.submit(t["segments"], lengths=t["lengths"], nseg=t["nseg"], taken=taken, stream=st))]
    c.calls += [("pirip_hip_arq_push_records", lambda st, k=k: arq.push_records(t["status"][k], t["payload"][k], out=out[k], out_stride=dev.blk,
                                                                                ncalls=t["ncalls"][k], stream=st)) for k in range(K)]
    c.reset = lambda st: arq.reset(stream=st)
    _link_rings(c, pkt, False)

    def counters():
        got = dict(arq.counters())
        got.update({"pkt_" + k: v for k, v in pkt.counters().items()})
        for ch in range(4):
            ent, data = arq.delivered(ch)
            got["entries%d" % ch], got["bytes%d" % ch] = ent.view(np.uint8), np.frombuffer(b"".join(data), np.uint8)
            got["state%d" % ch] = np.array(list(arq.state(ch).values()), np.int64)
        return got
    c.counters = counters

    def sane(res):
        for k in ("sent", "retransmitted", "acked", "acks_sent", "delivered"):
            assert res["counter:" + k].view(np.int64)[0] > 0, k
    c.sane = sane
    return c


@family("mac")
def _mac(seed, oracle):
    """per sense mode (a row with RX_SYNC; a row whose SNRest reaches the threshold) one packet terminal with the layer attached: send,
    then push_records x 3 -- carrier in the first call defers the burst, the backoff lets it out in the idle calls behind"""
    import torch
    import macref as m
    from test_mac import _Dev
    c = Case()
    t = {k: c.add_in(*v) for k, v in ss.mac_inputs(seed).items()}
    K = ss.MAC["calls"]
    dst = torch.full((4, 1), m.ADDR, dtype=torch.uint8, device="cuda")
    c.keep.append(dst)
    devs = []
    for mask in ss.MAC["masks"]:
        dev = _Dev(m.terminal(mac=dict(cw=ss.MAC["cw"], sense_mask=mask, sense_snr=m.SNR_T, key=7 + seed)))
        devs.append(dev)
        c.keep += [dev.mac, dev.pkt, dev.txs, dev.tx, dev.mux, dev]
        taken = c.add_out("taken%d" % mask, (4,), torch.int32)
        out = c.add_out("iq%d" % mask, (K, dev.blk), torch.uint8)
        c.calls.append(("pirip_hip_pkt_send", lambda st, dev=dev, taken=taken: dev.pkt.send(t["raw"], dst, lengths=t["lengths"], taken=taken, stream=st)))

        def call(st, k, dev=dev, out=out):
            dev.mac.set_stats(t["stats"][k])
            dev.pkt.push_records(t["status"][k], t["payload"][k], out=out[k], out_stride=dev.blk, ncalls=t["ncalls"][k], stream=st)
        c.calls += [("pirip_hip_pkt_push_records", lambda st, k=k, call=call: call(st, k)) for k in range(K)]
        _link_rings(c, dev.pkt, False, str(mask))

    def reset(st):
        for dev in devs:
            dev.mac.reset(stream=st)
            dev.pkt.reset(stream=st)
    c.reset = reset

    def counters():
        got = {}
        for mask, dev in zip(ss.MAC["masks"], devs):
            got.update({"mac%d_%s" % (mask, k): v for k, v in dev.mac.counters().items()})
            got.update({"pkt%d_%s" % (mask, k): v for k, v in dev.pkt.counters().items()})
            got.update({"%s_%d" % (k, mask): v for k, v in _packets(dev.pkt).items()})
            got["state%d" % mask] = np.array([list(dev.mac.state(ch).values()) for ch in range(4)], np.int64)
        return got
    c.counters = counters

    def sane(res):
        for mask in ss.MAC["masks"]:
            assert res["counter:mac%d_carrier" % mask].view(np.int64).sum() > 0, ("the first call should be carrier under sense mode", mask)
            assert res["counter:mac%d_bursts" % mask].view(np.int64).sum() > 0, mask
    c.sane = sane
    return c


def _loop_blocks(seed, block_bytes, K):
    """rx_loop's wideband IQ cut into K blocks of a terminal, silence (byte 128) behind it -> uint8 tensor [K, block bytes]"""
    import torch
    wide, _ = loop_wide(seed)
    out = torch.full((K * block_bytes,), 128, dtype=torch.uint8, device="cuda")
    n = min(wide.numel(), out.numel())
    out[:n] = wide.view(-1)[:n]
    return out.view(K, block_bytes)


def _terminal(seed, kind):
    """push_records (the caller's rows), process (the block copied into the receiver's landing zone on the same stream), push x 4"""
    import torch
    import pirip_amd
    import muxshapes as ms
    from test_mux import _rx_handles
    from test_ping import LOOP_GAP, ROUTE, _tx_side
    c = Case()
    lp, K = ms.LOOP, ss.TERM["blocks"]
    tx, mux, block, txs = _tx_side(lp["M"], 50 + lp["nframes"] * 544 + LOOP_GAP, S=ss.TERM["S"])
    dem, ld, ch = _rx_handles()
    rx = pirip_amd.HipRx(dem, ldpc=ld, chan=ch, block=block)
    blk = block * 2
    d = dict(ss.rpt_inputs(seed) if kind == "rpt" else ss.ping_inputs(seed))
    d.pop("records")
    t = {k: c.add_in(*v) for k, v in d.items()}
    real = _loop_blocks(seed, blk, K)
    wide = c.add_in_dev(torch.empty_like(real), real, torch.full_like(real, 128))
    out = c.add_out("iq", (K + 1, blk), torch.uint8)
    if kind == "rpt":
        h = pirip_amd.HipRepeater(tx, txs, ROUTE, 2, filter=2, holdoff=1, max_burst=lp["nframes"], pending=lp["nframes"] + 1, rx=rx)
        first = ("pirip_hip_rpt_push_records", lambda st: h.push_records(t["status"], t["payload"], out[0], blk, ncalls=t["ncalls"], stream=st))
        rows = ("status", "payload", "info")
    else:
        h = pirip_amd.HipPing(rx=rx, tx=tx, txs=txs, source=1, filter=1, frames=lp["nframes"], seq=True, period=2, first_call=[0, 1, 2, 3], max_bursts=2,
                              log_entries=16)
        first = ("pirip_hip_ping_push_records", lambda st: h.push_records(t["status"], t["payload"], t["info"], t["stats"], out=out[0], out_stride=blk,
                                                                          ncalls=t["ncalls"], stream=st))
        rows = ("status", "payload", "info", "stats")
    c.keep += [h, rx, dem, ld, ch, txs, tx, mux]
    zone_ptr, _ = rx.input()
    view_bytes(zone_ptr, blk).fill_(128)
    name = "pirip_hip_%s_" % kind

    def process(st):
        copy_on(st, zone_ptr, _p(wide[0]), blk)
        h.process(out[1], blk, stream=st)
    c.calls = [first, (name + "process", process)]
    c.calls += [(name + "push", lambda st, k=k: h.push(wide[k], blk, out[k + 1], blk, stream=st)) for k in range(1, K)]
    c.reset = lambda st: h.reset(stream=st)
    R = h.rx_rows                                          # the receiver's rows of the last process / push
    size = dict(status=R, payload=R * h.data_bytes, info=R * 10 * 4, stats=R * 10 * 4)
    for k in rows:
        c.rings["rx_" + k] = (lambda k=k: h.records()[k], h.nrx * size[k])
    c.rings["rx_nframes"] = (lambda: h.records()["nframes"], h.nrx * 4)
    p_rec, stride, p_n = h.offered()
    c.rings["offered"], c.rings["noffered"] = (p_rec, h.nchan * stride), (p_n, h.nchan * 4)
    c.rings["input"] = (zone_ptr, blk)

    def counters():
        got = dict(h.counters())
        got.update({"txs_" + k: v for k, v in txs.counters().items()})
        if kind == "ping":
            got.update({"log%d" % ch_: h.log(ch_).view(np.uint8) for ch_ in range(h.nrx)})
        return got
    c.counters = counters

    def sane(res):
        n = lambda k: res["counter:" + k].view(np.int64)
        if kind == "rpt":
            assert n("bursts_in").sum() > 4 and n("bursts_out").sum() >= 4, "the rows' bursts and the blocks' bursts should both be repeated"
        else:
            assert n("frames").sum() > 12 and n("bursts_sent").sum() >= 4, ("the rows' and the blocks' frames should be logged, the bursts sent",
                                                                            n("frames"), n("bursts_sent"))
    c.sane = sane
    torch.cuda.synchronize()
    return c


@family("rpt")
def _rpt(seed, oracle):
    return _terminal(seed, "rpt")


@family("ping")
def _ping(seed, oracle):
    return _terminal(seed, "ping")


@family("div")
def _div(seed, oracle):
    """the FSK_LDPC chain over two groups of two branches, collect behind it, push_candidates with four crafted candidates, flush"""
    import torch
    import pirip_amd
    from test_diversity import SKEW, _demod, _Rows
    c = Case()
    d = ss.DIV
    S = ss.div_shape(oracle, seed)
    x = ss.div_inputs(seed, oracle)
    R = d["G"] * d["B"]
    iq, llr = c.add_in(*x["iq"]), c.add_in(*x["llr"])
    nsamp = iq.shape[1]
    dem = _demod(pirip_amd, S, R)
    maxf = dem.max_frames_for(nsamp)
    ld = pirip_amd.HipLdpc(S["path"], S["M"], Nsym=S["Nsym"], nstreams=R)
    dv = pirip_amd.HipDiversity(ld, d["B"], S["Ts"], dem.N, SKEW, maxf, log_entries=64)
    c.keep += [dv, ld, dem]
    rows = _Rows(torch, pirip_amd, R, maxf, S["kb"])
    for k in ("status", "payload", "info", "stats", "nframes", "consumed"):
        c.outs[k] = getattr(rows, k)
    far = 10 ** 7
    tag = torch.tensor([far, far + SKEW // 2, far + 5, far + 5000], dtype=torch.int64, device="cuda")
    gb = torch.tensor([0, 1, 2, 3], dtype=torch.int32, device="cuda")
    solo = torch.zeros(4, dtype=torch.uint8, device="cuda")
    clock = torch.full((R,), 10 ** 9, dtype=torch.int64, device="cuda")
    c.keep += [tag, gb, solo, clock]
    c.calls = [
        ("pirip_hip_fsk_ldpc_rx_batch", lambda st: ld.chain_batch(dem, _p(iq), nsamp * 2, nsamp, _p(rows.status), _p(rows.payload), _p(rows.info),
                                                                  _p(rows.nframes), _p(rows.consumed), maxf, _p(rows.stats),
                                                                  maxf * pirip_amd.STATS_PER_FRAME, stream=st)),
        ("pirip_hip_div_collect", lambda st: dv.collect(rows.status, rows.info, rows.stats, nframes=rows.nframes, stream=st)),
        ("pirip_hip_div_push_candidates", lambda st: dv.push_candidates(llr, tag, gb, solo, clock, stream=st)),
        ("pirip_hip_div_flush", lambda st: dv.flush(stream=st)),
    ]

    def reset(st):
        dv.reset(stream=st)
        ld.reset(stream=st)
        dem.reset(stream=st)
    c.reset = reset
    last = dv.last()
    c.rings["last_count"] = (last["count"], 4 * d["G"])

    def counters():
        got = dict(dv.counters())
        for g in range(d["G"]):
            e, pl = dv.log(g)
            got["entries%d" % g], got["payloads%d" % g] = e.view(np.uint8), pl
        return got
    c.counters = counters

    def sane(res):
        assert (res["counter:clusters"].view(np.int64) >= 3).all(), "every group should combine the chain's frames and the candidates"
        assert res["counter:bits"].view(np.int64).sum() > 0
    c.sane = sane
    # section E: the receiver's work rows grow with the largest call it has seen, and such a call waits for its stream -- once, here
    c.calls[0][1](0)
    reset(0)
    torch.cuda.synchronize()
    return c


_tmp = None


def tmp_dir():
    global _tmp
    if _tmp is None:
        import tempfile
        _tmp = tempfile.mkdtemp(prefix="streamgate")
    return _tmp


def _p(t):
    return t.data_ptr()


@family("rx_plain")
def _rx_plain(seed, oracle):
    """HipRx.push x 3 on the plain u8 CFG1 shape: the wave kernel's exact-first-frame prologue and frame cache, the carry between blocks"""
    import torch
    import pirip_amd
    from test_stream_rx import _demod
    c = Case()
    real, decoy = ss.rx_plain_inputs(seed, oracle)["iq"]
    nch, K = ss.RX_PLAIN["nch"], ss.RX_PLAIN["blocks"]
    dem = _demod(sigutil.CFG1, nch, "u8")
    assert dem.kernel() == "wave"
    block = 3 * dem.N + 17
    rx = pirip_amd.HipRx(dem, block=block)
    c.keep += [rx, dem]
    R = rx.max_frames
    iq = c.add_in(real, decoy)
    bits = c.add_out("bits", (K, nch, R, dem.Nbits), torch.uint8)
    filt = c.add_out("rx_filt", (K, nch, R, dem.M * dem.Nsym), torch.float32)
    stats = c.add_out("stats", (K, nch, R, 10), torch.float32)
    nfr = c.add_out("nframes", (K, nch), torch.int32)
    stride = K * block * 2
    for k in range(K):
        c.calls.append(("pirip_hip_rx_push", lambda st, k=k: rx.push(
            _p(iq) + k * block * 2, stride, _p(bits[k]), R * dem.Nbits, _p(filt[k]), R * dem.M * dem.Nsym, d_stats=_p(stats[k]), stats_stride=R * 10,
            d_nframes=_p(nfr[k]), stream=st)))
    c.reset = lambda st: rx.reset(stream=st)
    c.counters = lambda: dict(zip(("consumed", "backlog"), rx.counters()))
    return c


def loop_wide(seed):
    """muxshapes' loopback on the device, in front of the gate: the records of loop_records(seed) through HipTx and HipMux -> (wideband
    u8 IQ tensor [n_wide, 2], modem samples per channel)"""
    import torch
    import pirip_amd
    import muxshapes as ms
    from test_mux import _tx_rows
    lp = ms.LOOP
    mx = pirip_amd.HipMux(lp["Fs"], lp["D"], lp["offsets"], gains=ms.LOOP_GAINS)
    rows, nmod = _tx_rows(ss.rx_loop_inputs(seed)["records"][0], mx.Q)
    wide = torch.zeros((nmod * lp["D"], 2), dtype=torch.uint8, device="cuda")
    mx.batch(rows.data_ptr(), (mx.Q - 1 + nmod) * 8, mx.Q - 1 + nmod, wide.data_ptr(), nmod * lp["D"] * 2, m0=-(mx.Q - 1))
    torch.cuda.synchronize()
    mx.close()
    return wide, nmod


@family("rx_loop")
def _rx_loop(seed, oracle):
    """HipRx with a channelizer in front and the FSK_LDPC chain behind, records and statistics rows out, on muxshapes' loopback in five
    blocks that cut frames: push, push, process (the block copied into the landing zone on the same stream), push, process"""
    import torch
    import pirip_amd
    import muxshapes as ms
    from test_mux import _rx_handles
    c = Case()
    D, K = ms.LOOP["D"], ss.RX_LOOP["blocks"]
    wide, nmod = loop_wide(seed)
    other, nmod2 = loop_wide(seed + 100)
    assert nmod == nmod2
    Bm = nmod // K
    Bm -= 37 if Bm % 2000 == 0 else 0                      # a demodulator frame is 2000 modem samples: the blocks cut frames
    block = Bm * D
    dem, ld, ch = _rx_handles()
    rx = pirip_amd.HipRx(dem, ldpc=ld, chan=ch, block=block)
    c.keep += [rx, dem, ld, ch]
    R, nb = rx.max_frames, ld.data_bytes
    iq = c.add_in_dev(torch.empty_like(wide), wide, other)
    zone_ptr, _ = rx.input()
    zone = view_bytes(zone_ptr, block * 2)
    zone.copy_(other.view(-1)[:block * 2])
    c.rings["input"] = (zone_ptr, block * 2)
    st_ = c.add_out("status", (K, 4, R), torch.uint8)
    pl = c.add_out("payload", (K, 4, R, nb), torch.uint8)
    info = c.add_out("info", (K, 4, R, 10), torch.int32)
    stats = c.add_out("stats", (K, 4, R, 10), torch.float32)
    nfr = c.add_out("nframes", (K, 4), torch.int32)

    def outs(k):
        return dict(d_status=_p(st_[k]), d_payload=_p(pl[k]), d_info=_p(info[k]), d_stats=_p(stats[k]), stats_stride=R * 10, d_nframes=_p(nfr[k]))

    def push(k):
        return ("pirip_hip_rx_push", lambda st: rx.push(_p(iq) + k * block * 2, block * 2, stream=st, **outs(k)))

    def process(k):
        def fn(st):
            copy_on(st, zone_ptr, _p(iq) + k * block * 2, block * 2)
            rx.process(stream=st, **outs(k))
        return ("pirip_hip_rx_process", fn)

    c.calls = [push(0), push(1), process(2), push(3), process(4)]
    c.reset = lambda st: rx.reset(stream=st)
    c.counters = lambda: dict(zip(("consumed", "backlog"), rx.counters()))
    torch.cuda.synchronize()
    return c


@family("chan")
def _chan(seed, oracle):
    import torch
    import pirip_amd
    import muxshapes as ms
    c = Case()
    ch = pirip_amd.HipChan(ss.CHAN["Fs"], ss.CHAN["D"], ms.LOOP["offsets"])
    c.keep.append(ch)
    iq = c.add_in(*ss.chan_inputs(seed)["iq"])
    n_in = ss.CHAN["n_in"]
    no = ch.nout(n_in)
    out = c.add_out("channels", (ss.CHAN["calls"], ch.nchan, no, 2), torch.float32)
    for k in range(ss.CHAN["calls"]):
        c.calls.append(("pirip_hip_chan_batch", lambda st, k=k: ch.batch(_p(iq[k]), n_in * 2, n_in, _p(out[k]), no * 8, t0=ss.CHAN["t0"][k], stream=st)))
    return c


@family("decim")
def _decim(seed, oracle):
    import torch
    import pirip_amd
    c = Case()
    dec = pirip_amd.HipDecim(ss.DECIM["D"], out_s16=True)
    c.keep.append(dec)
    iq = c.add_in(*ss.decim_inputs(seed)["iq"])
    n_in, ns = ss.DECIM["n_in"], ss.DECIM["nstreams"]
    no = dec.nout(n_in)
    out = c.add_out("decimated", (ss.DECIM["calls"], ns, no, 2), torch.int16)
    for k in range(ss.DECIM["calls"]):
        c.calls.append(("pirip_hip_decim_batch", lambda st, k=k: dec.batch(_p(iq[k]), n_in * 2, n_in, _p(out[k]), no * 4, ns, stream=st)))
    return c


@family("mux")
def _mux(seed, oracle):
    import torch
    import pirip_amd
    import muxshapes as ms
    c = Case()
    Fs, D, tbw, offsets, outputs, noutputs, branch, _ = ms.SHAPES[ss.MUX["shape"]]
    real, decoy = ss.mux_inputs(seed)["z"]
    n_in = real.shape[2]
    _, g = ms.inputs(ss.MUX["shape"], n_in)
    mx = pirip_amd.HipMux(Fs, D, offsets, outputs=outputs, gains=g, transition_bw=tbw, noutputs=noutputs)
    c.keep.append(mx)
    z = c.add_in(real.view(np.float32), decoy.view(np.float32))
    no = mx.nout(n_in)
    out = c.add_out("wide", (ss.MUX["calls"], noutputs, no, 2), torch.uint8)
    for k in range(ss.MUX["calls"]):
        c.calls.append(("pirip_hip_mux_batch", lambda st, k=k: mx.batch(_p(z[k]), n_in * 8, n_in, _p(out[k]), no * 2, m0=ss.MUX["m0"][k], stream=st)))
    return c


def _tx_handle():
    import pirip_amd
    t = ss.TX
    return pirip_amd.HipTx(sigutil.STANDIN_CODE, t["Fs"], t["Rs"], t["M"], nstreams=len(t["f1"]), f1=t["f1"], shift=t["shift"], lead=t["lead"],
                           gap=t["gap"])


@family("tx")
def _tx(seed, oracle):
    """repeat_records -> frame -> modulate (noise on, counts from the device) and records_to_iq: every buffer between the stages is
    written by the stage before it"""
    import torch
    import pirip_amd
    c = Case()
    t = ss.TX
    tx = _tx_handle()
    c.keep.append(tx)
    d = ss.tx_inputs(seed)
    B, w, kb, nsym = len(t["f1"]), t["ncalls"], tx.data_bytes, t["nsym"]
    status, payload, rec, nrec = (c.add_in(*d[k]) for k in ("status", "payload", "records", "nrec"))
    cap = tx.repeat_max_records(w)
    ms_ = tx.max_syms(cap)
    rep = c.add_out("repeated", (B, cap, 1 + kb), torch.uint8)
    nrep = c.add_out("nrepeated", (B,), torch.int32)
    syms = c.add_out("syms", (B, ms_), torch.uint8)
    nsy = c.add_out("nsym", (B,), torch.int32)
    iq = c.add_out("iq", (B, nsym * tx.Ts, 2), torch.uint8)
    iq2 = c.add_out("iq2", (B, nsym * tx.Ts, 2), torch.float32)
    nsy2 = c.add_out("nsym2", (B,), torch.int32)
    c.calls = [
        ("pirip_hip_tx_repeat_records", lambda st: tx.repeat_records(_p(status), w, _p(payload), w * kb, w, t["source"], _p(rep), cap * (1 + kb), cap,
                                                                     d_nrec=_p(nrep), stream=st)),
        ("pirip_hip_tx_frame", lambda st: tx.frame(_p(rep), cap * (1 + kb), cap, _p(syms), ms_, ms_, d_nrec=_p(nrep), d_nsym=_p(nsy), stream=st)),
        ("pirip_hip_tx_modulate", lambda st: tx.modulate(_p(syms), ms_, nsym, _p(iq), nsym * tx.Ts * 2, d_nsym=_p(nsy), amp=t["amp"], sigma=t["sigma"],
                                                         seed=5 + seed, stream=st)),
        ("pirip_hip_tx_records_to_iq", lambda st: tx.records_to_iq(_p(rec), rec[0].numel(), rec.shape[1], nsym, _p(iq2), nsym * tx.Ts * 8,
                                                                   out_format=pirip_amd.IN_CF32, d_nrec=_p(nrec), d_nsym=_p(nsy2), sigma=t["sigma"],
                                                                   seed=9 + seed, stream=st)),
    ]
    c.reset = lambda st: tx.reset(stream=st)
    # section I: the handle's work rows grow "when a call is larger than any before it" -- once, here, on the decoy and in front of the gate
    for _, fn in c.calls:
        fn(0)
    tx.reset()
    torch.cuda.synchronize()
    return c


_txs_code = None


def txs_code():
    global _txs_code
    if _txs_code is None:
        import txsref
        from test_tx_shapes import write_code
        _txs_code = write_code(tmp_dir(), txsref.CODE_N, txsref.CODE_K)
    return _txs_code


@family("txs")
def _txs(seed, oracle):
    """send, process x 2, send (across the end of the ring), process x 2 (a pop across the end of the ring)"""
    import torch
    import pirip_amd
    import txsref
    from test_txs import _handles
    c = Case()
    sh = dict(txsref.SHAPES[ss.TXS["shape"]], S=ss.TXS["S"])
    tx, _, mux = _handles(sh, "u8", txs_code())
    lens = txsref.record_lens(ss.TXS["plan"], 50 * (sh["M"] // 2), 32 + txsref.CODE_N, txsref.GAP_SYMS)
    cap = sum(lens) + sh["S"] + 3
    assert sum(lens) > 2 * sh["S"] and 2 * sum(lens) > cap, "the second burst must go in across the end of the ring"
    txs = pirip_amd.HipTxStream(tx, mux, sh["S"] * sh["D"] * tx.Ts, cap)
    c.keep += [txs, tx, mux]
    d = ss.txs_inputs(seed)
    rec, nrec = c.add_in(*d["records"]), c.add_in(*d["nrec"])
    K, max_rec = txs.nchan, rec.shape[2]
    taken = c.add_out("taken", (2, K), torch.int32)
    sent = c.add_out("sent", (4, K), torch.int32)
    out = c.add_out("wide", (txs.noutputs, 4 * txs.block, 2), torch.uint8)

    def send(i):
        return ("pirip_hip_txs_send", lambda st: txs.send(_p(rec[i]), rec[i, 0].numel(), max_rec, d_nrec=_p(nrec[i]), d_taken=_p(taken[i]), stream=st))

    def process(k):
        return ("pirip_hip_txs_process", lambda st: txs.process(_p(out) + k * txs.block * 2, 4 * txs.block * 2, d_sent=_p(sent[k]), stream=st))

    c.calls = [send(0), process(0), process(1), send(1), process(2), process(3)]
    c.reset = lambda st: txs.reset(stream=st)
    c.counters = txs.counters
    # section K: a send "with a larger max_rec than any before it grows the handle's work rows" -- once, here, in front of the gate
    c.calls[0][1](0)
    txs.reset()
    torch.cuda.synchronize()
    return c
