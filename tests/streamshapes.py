"""The stream contract of include/pirip_hip.h as data: which gated test calls each entry point that takes a hip_stream, the families
those tests run (tests/streamgate.py), and every place in pirip_amd/csrc that names a literal stream or blocks the host. Pure Python, no
GPU: tests/test_stream_order_cpu.py holds the tables to the header and the sources, and proves on the host models alone that each
family's decoy input gives another result than its real input -- the condition under which a gated comparison can fail at all.

ENTRY_POINTS has one entry per function of the header with a `void *hip_stream` parameter:
    ("test", "tests/test_stream_order.py::<test>")   the gated test whose sequence calls it
    ("exempt", reason)                                 the header itself says the call synchronises (quoted), or no gated call applies
FAMILIES: per family the sequence of entry points, what the decoy is, the host enqueue time of the gated sequence (both passes) as
measured on an MI355X, and the gate it led to (>= 4 x that time).
LITERAL_STREAM / BLOCKING: (file under pirip_amd/csrc, substring of the line, occurrences, reason)."""
import functools

import numpy as np

T = "tests/test_stream_order.py::"


# ---- the families' inputs: (real, decoy) per input buffer, as numpy arrays, from a seed -----------------------------------------------------
RX_PLAIN = dict(nch=8, blocks=3)                           # test_stream_process_does_not_synchronise's shape: CFG1, u8, the wave kernel


@functools.lru_cache(maxsize=None)
def rx_plain_inputs(seed, oracle):
    """three blocks of 3 N + 17 samples of eight CFG1 channels, each on its own clock; the decoy is another seed's recording"""
    import sigutil
    from test_stream_rx import _channels
    N = sigutil.CFG1["Fs"] // sigutil.CFG1["Rs"] * 50
    n = RX_PLAIN["blocks"] * (3 * N + 17)
    return {"iq": (_channels(oracle, sigutil.CFG1, RX_PLAIN["nch"], n, "u8", seed=3 + seed),
                   _channels(oracle, sigutil.CFG1, RX_PLAIN["nch"], n, "u8", seed=53 + seed))}


def _bytes(seed, shape):
    return np.random.default_rng(seed).integers(0, 256, shape).astype(np.uint8)


CHAN = dict(Fs=240000, D=6, n_in=6 * 1200 + 84, calls=3, t0=(0, 2 ** 31 + 5, -7))     # the loopback's channelizer (muxshapes.LOOP)
DECIM = dict(D=45, nstreams=3, n_in=45 * 300 + 91, calls=3)                          # D = 45: the convert-once (shared) kernel


@functools.lru_cache(maxsize=None)
def chan_inputs(seed):
    """u8 IQ noise [calls, n_in, 2]; the decoy is silence (byte 128)"""
    x = _bytes(700 + seed, (CHAN["calls"], CHAN["n_in"], 2))
    return {"iq": (x, np.full_like(x, 128))}


@functools.lru_cache(maxsize=None)
def decim_inputs(seed):
    x = _bytes(800 + seed, (DECIM["calls"], DECIM["nstreams"], DECIM["n_in"], 2))
    return {"iq": (x, np.full_like(x, 128))}


MUX = dict(shape="d6_k8", calls=3, m0=(-5, 2 ** 31 + 3, 10 ** 6))


@functools.lru_cache(maxsize=None)
def mux_inputs(seed):
    """complex float noise [calls, K, n_in] of muxshapes' d6_k8 (and its gains); the decoy is zeros"""
    import muxref
    import muxshapes as ms
    Fs, D, tbw, offsets, outputs, noutputs, branch, m0 = ms.SHAPES[MUX["shape"]]
    n_in = branch + muxref.q_of(ms.taps_len(muxref.FIR, D, tbw), D) - 1
    rng = np.random.default_rng(900 + seed)
    z = (rng.normal(size=(MUX["calls"], len(offsets), n_in)) + 1j * rng.normal(size=(MUX["calls"], len(offsets), n_in))).astype(np.complex64)
    return {"z": (z, np.zeros_like(z))}


TX = dict(Fs=240000, Rs=10000, M=2, f1=[10037, 10411, 20011, -29959], shift=10000, lead=[0, 3, 10, 65], gap=[40, 0, 7, 129], ncalls=8,
          source=0x31, nsym=2600, sigma=0.6, amp=20.0)
RX_SYNC, RX_BITS = 2, 4


@functools.lru_cache(maxsize=None)
def tx_inputs(seed):
    """what HipTx reads: a receiver's status / payload rows for repeat_records (per stream one burst of 1 .. 3 frames that ends inside the
    call) and Tx records for records_to_iq; the decoys are an all-zero status column (no burst: no record comes out) and record counts of
    zero"""
    import txref
    rng = np.random.default_rng(1000 + seed)
    B, w, kb = len(TX["f1"]), TX["ncalls"], 32
    status = np.zeros((B, w), np.uint8)
    for s in range(B):
        nfr = 1 + (s + seed) % 3
        status[s, 1 + s % 2: 1 + s % 2 + nfr] = RX_SYNC | RX_BITS
        status[s, 1 + s % 2 + nfr] = RX_BITS if s % 2 else 0          # the burst ends with a last frame, or at a row without one
    payload = rng.integers(0, 256, (B, w, kb)).astype(np.uint8)
    plans = [[1, 0, 2], [1, 2, 1, 2], [1, 0, 0, 2], [7, 1, 2]]
    rec = np.full((B, 4, 1 + kb), 3, np.uint8)
    for s, p in enumerate(plans):
        rec[s, :len(p)] = txref.records(rng, p, kb)
    nrec = np.array([len(p) for p in plans], np.int32)
    return {"status": (status, np.zeros_like(status)), "payload": (payload, np.roll(payload, 1, axis=2)), "records": (rec, np.roll(rec, 1, axis=2)),
            "nrec": (nrec, np.zeros_like(nrec))}


TXS = dict(shape="h0_lin_d1", S=100, plan=[1, 2])          # txsref's smallest shape with a block of 100 symbols: two bursts wrap the ring


@functools.lru_cache(maxsize=None)
def txs_inputs(seed):
    """per send one burst (preamble + frame, end of burst) for each channel; the decoy offers nothing (record counts of zero)"""
    import txref
    import txsref
    rng = np.random.default_rng(1100 + seed)
    K = len(txsref.SHAPES[TXS["shape"]]["f1"])
    rec = np.stack([np.stack([txref.records(rng, TXS["plan"], txsref.CODE_K // 8) for _ in range(K)]) for _ in range(2)])
    nrec = np.full((2, K), len(TXS["plan"]), np.int32)
    return {"records": (rec, np.roll(rec, 1, axis=3)), "nrec": (nrec, np.zeros_like(nrec))}


TBITS = dict(split=4)                                      # tbitsshapes' synthetic rows: the first four as bytes, the last five packed


@functools.lru_cache(maxsize=None)
def tbits_inputs(seed):
    """tbitsshapes' synthetic rows (seed > 0: with bits flipped) and row counts, and its crafted records; the decoys are rows of zero
    bits, row counts of zero, and records that nothing counts of (status 0, info -1)"""
    import pirip_amd
    import tbitsref
    import tbitsshapes as ts
    rows = ts.syn_rows().copy()
    if seed:
        rows ^= (np.random.default_rng(1200 + seed).random(rows.shape) < 0.02).astype(np.uint8)
    k = TBITS["split"]
    nf = np.array(ts.SYN["nframes"], np.int32)
    a, b = rows[:, :k], tbitsref.pack_rows(rows[:, k:], pad=1)
    nfa, nfb = nf.clip(0, k), (nf - k).clip(0, rows.shape[1] - k)
    status, payload, info, ncalls = ts.crafted_records(pirip_amd.testframe_payload(8 * ts.REC_DB))
    if seed:
        payload = payload ^ (np.random.default_rng(1300 + seed).random(payload.shape) < 0.05).astype(np.uint8)
    return {"rows": (a, np.zeros_like(a)), "packed": (b, np.zeros_like(b)), "nframes": (nfa, np.zeros_like(nfa)), "nframes_packed": (nfb, np.zeros_like(nfb)),
            "status": (status, np.zeros_like(status)), "payload": (payload, np.zeros_like(payload)), "info": (info, np.full_like(info, -1)),
            "ncalls": (ncalls, np.zeros_like(ncalls))}


SPEC = dict(case=(1024, 512, "u8", 3), rows=3)             # nfft 1024, half overlap, three segments per row, u8


def spec_cuts(n):
    """three uneven calls; the second leaves the tail at an odd position inside a half segment"""
    a = 2 * n // 5 + 1
    return [a, 333, n - a - 333]


@functools.lru_cache(maxsize=None)
def spec_inputs(seed):
    """specshapes' three streams (seed > 0: rotated in time); the decoy is silence (byte 128)"""
    import specshapes as sh
    x = np.roll(sh.inputs(*SPEC["case"]), 977 * seed, axis=1)
    return {"iq": (x, np.full_like(x, 128))}


AIR = dict(Fs=240000, drifting=[(0, 0, 0.1, 40, 77, 300000), (0, 1, -0.1, 9, 0, -1000000)], max_slip=20, age=2000, n0=240000 - 5,
           extra=[(0, 0, 0.02, 40, 77, 300000), (0, 1, -0.02, 9, 0, 0)], fades=lambda m: [(m, 20.0, 0.0, 1), (m + 1, 7.0, 4.0, 2), (1, 20.0, 1.0, 3)],
           sigma2=[0.0, 0.2, 0.05, 0.1])                    # tests/test_air_fade.py's static, drifting and fading handles on airshapes' layout


@functools.lru_cache(maxsize=None)
def air_inputs(seed):
    """airshapes' three transmitters, 6300 u8 samples; the decoy is silence (byte 128)"""
    import airshapes as sh
    x, _ = sh.inputs(AIR["Fs"], "u8", seed=seed)
    return {"iq": (x, np.full_like(x, 128))}


LINK = dict(S=1000, max_frags=3, blocks=4, own=1, far=2, w=4)        # the packet terminals: muxshapes' LOOP, calls of 1000 symbols
FEC_SHAPE = "small"                                        # pktfecref.SHAPES: (max_frags, max_parity, parity_pct)


@functools.lru_cache(maxsize=None)
def link_inputs(seed, fec=False):
    """what a packet terminal reads in [send, push_records, push x 4]: the packets handed to send (two rows per channel, lengths, counts),
    the caller's record rows (per channel one packet of the far end -- with parity fragments and its first data fragment lost when fec),
    and the far end's packets, whose wideband IQ the far terminal makes on the device in front of the gate. The decoys: lengths of zero
    (every packet is refused as bad), an all-zero status column, and silence (byte 128) for the IQ."""
    import pktfecref as fr
    import pktref
    rng = np.random.default_rng((1500 if fec else 1400) + seed)
    mf = fr.SHAPES[FEC_SHAPE][0] if fec else LINK["max_frags"]
    mp, kb, w = pktref.max_packet(pktref.KB, mf), pktref.KB, (mf + 4 if fec else LINK["w"])
    raw = rng.integers(0, 256, (4, 2, mp)).astype(np.uint8)
    lengths = np.array([[1, mp], [pktref.cap(kb), 0], [mp, 30], [17, 0]], np.int32)
    npk = np.array([2, 1, 2, 1], np.int32)
    status, payload, ncalls = np.zeros((4, w), np.uint8), np.zeros((4, w, kb), np.uint8), np.zeros(4, np.int32)
    for c in range(4):
        body = rng.integers(0, 256, 2 * pktref.cap(kb) - 4 if fec else 20 + c).astype(np.uint8).tobytes()
        if fec:
            rec = fr.segment_fec(body, LINK["far"], LINK["own"], c, kb, *fr.SHAPES[FEC_SHAPE])[1:-1]   # the first data fragment is lost
        else:
            rec = pktref.segment(body, LINK["far"], LINK["own"], c, kb, mf)[:-1]
        n = len(rec)
        status[c, :n], payload[c, :n], ncalls[c] = pktref.SYNC | pktref.BITS, rec[:, 1:], n
    # the far end's packets fill their last fragment and make bursts of three frames: three data fragments, or with fec two and one parity
    far = [rng.integers(0, 256, (2 if fec else mf) * pktref.cap(kb) - 4).astype(np.uint8).tobytes() for _ in range(4)]
    return {"raw": (raw, np.roll(raw, 1, axis=2)), "lengths": (lengths, np.zeros_like(lengths)), "status": (status, np.zeros_like(status)),
            "payload": (payload, np.roll(payload, 1, axis=2)), "ncalls": (ncalls, np.zeros_like(ncalls))}, dict(npk=npk, far=far, mf=mf)


def pkt_inputs(seed):
    return link_inputs(seed)[0]


def fec_inputs(seed):
    return link_inputs(seed, True)[0]


ARQ = dict(S=1000, rto=2, calls=4)                          # arqref's rules terminal with a retransmission after two calls


def arq_rows(seed):
    """arqref's rule tables (DATA in and out of order, ACKs fresh and stale, ...) cut into four calls at 30, 55 and 80 % of each channel"""
    import arqref as ar
    import pktref
    chans = ar.rule_streams(ar.ack_len(pktref.KB, pktref.MAX_FRAGS), seed=31 + seed)
    cuts = [[0] + [len(st) * p // 100 for p in (30, 55, 80)] + [len(st)] for st, _ in chans]
    return [[(st[cuts[c][k]:cuts[c][k + 1]], pl[cuts[c][k]:cuts[c][k + 1]]) for c, (st, pl) in enumerate(chans)] for k in range(ARQ["calls"])]


def arq_node():
    import arqref as ar
    return ar.node(ar.OWN, None, ARQ["S"], ARQ["rto"], E=4, ring_entries=ar.RULES_RING, peers=[ar.PEER, ar.PEER, None, ar.PEER])


def stage_rows(calls, kb, extra=()):
    """calls[k][c] = (status, payload) -> status uint8 [K, n, w], payload uint8 [K, n, w, kb], counts int32 [K, n]; rows behind a count
    are zeros"""
    K, n = len(calls), len(calls[0])
    w = max([len(r[0]) for rows in calls for r in rows] + [1])
    st, pl, nc = np.zeros((K, n, w), np.uint8), np.zeros((K, n, w, kb), np.uint8), np.zeros((K, n), np.int32)
    for k, rows in enumerate(calls):
        for c, (a, b) in enumerate(rows):
            st[k, c, :len(a)], pl[k, c, :len(a)], nc[k, c] = a, b, len(a)
    return st, pl, nc


@functools.lru_cache(maxsize=None)
def arq_inputs(seed):
    """four segments for channel 0 (and two for channel 1), then the rule tables' rows in four calls; the decoys: segment counts of zero
    and an all-zero status column"""
    import pktref
    rng = np.random.default_rng(1600 + seed)
    seg = rng.integers(0, 256, (4, 4, 18)).astype(np.uint8)
    lengths = np.full((4, 4), 18, np.int32)
    nseg = np.array([4, 2, 0, 0], np.int32)
    st, pl, nc = stage_rows(arq_rows(seed), pktref.KB)
    return {"segments": (seg, np.roll(seg, 1, axis=2)), "lengths": (lengths, np.zeros_like(lengths)), "nseg": (nseg, np.zeros_like(nseg)),
            "status": (st, np.zeros_like(st)), "payload": (pl, np.roll(pl, 1, axis=3)), "ncalls": (nc, np.zeros_like(nc))}


MAC = dict(masks=(1, 2), cw=2, calls=3)                     # macref's records-path terminal under both sense modes


def mac_calls(seed):
    """per call (rows, stats): carrier on channels 0 and 3 in the first call -- a lone SYNC row, which sense bit 0 reads, and an SNRest at
    the threshold in another row, which bit 1 reads -- beside one packet of the far end per channel; then two idle calls"""
    import macref as m
    rng = np.random.default_rng(1700 + seed)
    rows = m.packet_rows([rng.integers(0, 256, 30 + c).astype(np.uint8).tobytes() for c in range(4)])
    stats = [np.full((len(st) + 2, m.STATS_PER_FRAME), -5.0, np.float32) for st, _ in rows]
    first = []
    for c, (st, pl) in enumerate(rows):
        st2, pl2 = np.concatenate([st, np.zeros(2, np.uint8)]), np.concatenate([pl, np.zeros((2, pl.shape[1]), np.uint8)])
        if c in (0, 3):
            st2[-2] = m.SYNC
            stats[c][-1, m.SNR_AT] = m.SNR_T
        first.append((st2, pl2))
    idle = m.lone_rows(2, None, 0)
    return [(first, stats), (idle, m.stats_rows(2)), (idle, m.stats_rows(2))]


@functools.lru_cache(maxsize=None)
def mac_inputs(seed):
    """one packet per channel for send, then three calls of rows and statistics rows; the decoys: lengths of zero, an all-zero status
    column, statistics far under the threshold"""
    import macref as m
    import pktref
    rng = np.random.default_rng(1800 + seed)
    raw = rng.integers(0, 256, (4, 1, 40)).astype(np.uint8)
    lengths = np.array([[10], [40], [1], [25]], np.int32)
    calls = mac_calls(seed)
    st, pl, nc = stage_rows([r for r, _ in calls], pktref.KB)
    ss = np.full(st.shape + (m.STATS_PER_FRAME,), -5.0, np.float32)
    for k, (_, stats) in enumerate(calls):
        for c, s in enumerate(stats):
            ss[k, c, :len(s)] = s
    return {"raw": (raw, np.roll(raw, 1, axis=2)), "lengths": (lengths, np.zeros_like(lengths)), "status": (st, np.zeros_like(st)),
            "payload": (pl, np.roll(pl, 1, axis=3)), "ncalls": (nc, np.zeros_like(nc)), "stats": (ss, np.full_like(ss, -50.0))}


TERM = dict(S=1000, blocks=5, rows=6)                      # repeater and ping terminal on muxshapes' LOOP, calls of 1000 symbols


@functools.lru_cache(maxsize=None)
def rpt_inputs(seed):
    """the caller's rows for push_records: per channel one burst of one to three frames that ends inside the call (no byte 0 is the
    repeater's own source); the decoy is an all-zero status column. The wideband blocks are rx_loop's, made on the device."""
    import rptref
    rng = np.random.default_rng(1900 + seed)
    w = TERM["rows"]
    status, payload = np.zeros((4, w), np.uint8), rng.integers(0, 256, (4, w, rptref.KB)).astype(np.uint8)
    payload[:, :, 0] = 7
    for c in range(4):
        status[c, 1:2 + (c + seed) % 3] = RX_SYNC | RX_BITS
    ncalls = np.array([w, w - 1, w, w - 2], np.int32)
    return {"status": (status, np.zeros_like(status)), "payload": (payload, np.roll(payload, 1, axis=2)), "ncalls": (ncalls, np.zeros_like(ncalls)),
            "records": rx_loop_inputs(seed)["records"]}


@functools.lru_cache(maxsize=None)
def ping_inputs(seed):
    """the caller's rows for push_records: pingref's rows of every kind of status, with info and statistics rows; the decoys are an
    all-zero status column and row counts of zero"""
    import pingref
    import pirip_amd
    rng = np.random.default_rng(2000 + seed)
    want = pirip_amd.testframe_payload(8 * pingref.KB)
    w = TERM["rows"]
    rows = [pingref._rows(rng, w, want) for _ in range(4)]
    status, payload, info, stats = (np.stack([np.asarray(r[i]) for r in rows]) for i in range(4))
    ncalls = np.array([w, w - 1, w, w - 2], np.int32)
    return {"status": (status, np.zeros_like(status)), "payload": (payload, np.roll(payload, 1, axis=2)), "info": (info, np.full_like(info, -1)),
            "stats": (stats, np.zeros_like(stats)), "ncalls": (ncalls, np.zeros_like(ncalls)), "records": rx_loop_inputs(seed)["records"]}


DIV = dict(M=2, Nsym=50, n=512, k=256, G=2, B=2, frames=2, ebno=5.0)            # divshapes.DEVICE_SHAPES[0]


@functools.lru_cache(maxsize=None)
def div_shape(oracle, seed):
    from test_diversity import _shape
    d = DIV
    return _shape(oracle, None, d["M"], d["Nsym"], d["n"], d["k"], d["frames"], 2100 + seed)


@functools.lru_cache(maxsize=None)
def div_inputs(seed, oracle):
    """u8 IQ of two groups of two branches (test_diversity's _inputs) for the chain call in front of collect, and four crafted candidates
    for push_candidates; the decoys: carrier-less bytes 127 and soft bits of the other sign"""
    from test_diversity import _inputs
    d = DIV
    u8 = _inputs(oracle, div_shape(oracle, seed), d["G"], d["B"], d["ebno"], seed=3 + seed)
    rng = np.random.default_rng(2200 + seed)
    llr = (rng.normal(0, 6, (4, d["n"]))).astype(np.float16)
    return {"iq": (u8, np.full_like(u8, 127)), "llr": (llr.view(np.int16), (-llr).view(np.int16))}


RX_LOOP = dict(blocks=5)                                  # muxshapes.LOOP: four FSK_LDPC channels on one 240 kS/s stream


@functools.lru_cache(maxsize=None)
def rx_loop_inputs(seed):
    """the loopback's Tx records; the decoy is another seed's: the wideband IQ of either is made on the device in front of the gate"""
    import muxshapes as ms
    return {"records": (ms.loop_records(21 + seed), ms.loop_records(121 + seed))}


# ---- the families -----------------------------------------------------------------------------------------------------------------------------
# sequence: the entry points the gated run calls, in order (a second pass repeats them behind `reset`); enqueue_ms: the longest host time
# from the gate's enqueue to the return of the last call of the gated sequence seen on an MI355X; gate_ms >= 4 x enqueue_ms.
def _fam(sequence, reset, decoy, inputs, handles):
    return dict(sequence=sequence, reset=reset, decoy=decoy, inputs=inputs, handles=handles)


# family: (enqueue_ms, gate_ms) -- the larger of the gated and the pairs test's enqueue times on an MI355X (perf_counter from the gate's
# enqueue to the return of the last call: both passes, their copies and snapshots included), rounded up, and the gate it led to. The
# host needs a millisecond at most; the gates are 100 ms so that a loaded host still returns in the gate's first half.
MEASURED = {
    "rx_plain": (0.35, 100), "rx_loop": (0.7, 100), "chan": (0.2, 100), "decim": (0.2, 100), "mux": (0.25, 100), "tx": (0.4, 100), "txs": (0.4, 100),
    "tbits": (0.35, 100), "spec": (0.25, 100), "air": (0.5, 100), "div": (0.5, 100), "arq": (0.6, 100), "mac": (0.9, 100), "rpt": (1.05, 100),
    "ping": (1.15, 100), "pkt": (1.05, 100), "fec": (1.0, 100), "arq_air": (0.9, 100), "ldpc": (0.8, 100),
}


SEQ_PKT = ["pirip_hip_pkt_send", "pirip_hip_pkt_push_records", "pirip_hip_pkt_process"] + ["pirip_hip_pkt_push"] * 3
FAMILIES = {
    "rx_plain": _fam(["pirip_hip_rx_push"] * 3, ["pirip_hip_rx_reset"], "another seed's recording", rx_plain_inputs, "HipRx over HipDemod (u8, wave kernel)"),
    "rx_loop": _fam(["pirip_hip_rx_push", "pirip_hip_rx_push", "pirip_hip_rx_process", "pirip_hip_rx_push", "pirip_hip_rx_process"], ["pirip_hip_rx_reset"],
                    "the wideband IQ of another seed's records", rx_loop_inputs, "HipRx over HipChan, HipDemod (cf32) and HipLdpc"),
    "chan": _fam(["pirip_hip_chan_batch"] * 3, [], "silence (byte 128)", chan_inputs, "HipChan"),
    "decim": _fam(["pirip_hip_decim_batch"] * 3, [], "silence (byte 128)", decim_inputs, "HipDecim (D = 45)"),
    "mux": _fam(["pirip_hip_mux_batch"] * 3, [], "zero samples", mux_inputs, "HipMux (d6_k8)"),
    "tx": _fam(["pirip_hip_tx_repeat_records", "pirip_hip_tx_frame", "pirip_hip_tx_modulate", "pirip_hip_tx_records_to_iq"], ["pirip_hip_tx_reset"],
               "an all-zero status column, record counts of zero", tx_inputs, "HipTx"),
    "txs": _fam(["pirip_hip_txs_send", "pirip_hip_txs_process", "pirip_hip_txs_process", "pirip_hip_txs_send", "pirip_hip_txs_process",
                 "pirip_hip_txs_process"], ["pirip_hip_txs_reset"], "record counts of zero: nothing is offered", txs_inputs,
                "HipTxStream over HipTx and HipMux"),
    "tbits": _fam(["pirip_hip_tbits_push", "pirip_hip_tbits_push", "pirip_hip_tbits_push_records"], ["pirip_hip_tbits_reset"],
                  "rows of zero bits, row counts of zero, records of status 0 and info -1", tbits_inputs, "HipTestBits (two handles)"),
    "spec": _fam(["pirip_hip_spec_push"] * 3, ["pirip_hip_spec_reset"], "silence (byte 128)", spec_inputs, "HipSpectrum"),
    "air": _fam(["pirip_hip_air_push", "pirip_hip_air_set_sigma", "pirip_hip_air_push"] * 3, ["pirip_hip_air_reset", "pirip_hip_air_reset_drift"],
                "silence (byte 128)", air_inputs, "HipAir: static, drifting and fading paths"),
    "pkt": _fam(SEQ_PKT, ["pirip_hip_pkt_reset"],
                "lengths of zero, an all-zero status column, silence (byte 128)", pkt_inputs,
                "HipPacket over HipRx (HipChan, HipDemod, HipLdpc), HipTx and HipTxStream"),
    "fec": _fam(SEQ_PKT, ["pirip_hip_pkt_reset"],
                "lengths of zero, an all-zero status column, silence (byte 128)", fec_inputs,
                "HipPacketFec over HipRx, HipTx and HipTxStream, fragments lost"),
    "arq": _fam(["pirip_hip_arq_submit"] + ["pirip_hip_arq_push_records"] * 4, ["pirip_hip_arq_reset"],
                "segment counts of zero, an all-zero status column", arq_inputs, "HipArq over HipPacket, HipTx and HipTxStream"),
    "mac": _fam((["pirip_hip_pkt_send"] + ["pirip_hip_pkt_push_records"] * 3) * 2, ["pirip_hip_mac_reset", "pirip_hip_pkt_reset"],
                "lengths of zero, an all-zero status column, statistics under the threshold", mac_inputs,
                "HipMac on HipPacket, sense modes 1 and 2"),
    "rpt": _fam(["pirip_hip_rpt_push_records", "pirip_hip_rpt_process"] + ["pirip_hip_rpt_push"] * 4, ["pirip_hip_rpt_reset"],
                "an all-zero status column, silence (byte 128)", rpt_inputs, "HipRepeater over HipRx, HipTx and HipTxStream"),
    "ping": _fam(["pirip_hip_ping_push_records", "pirip_hip_ping_process"] + ["pirip_hip_ping_push"] * 4, ["pirip_hip_ping_reset"],
                 "an all-zero status column, row counts of zero, silence (byte 128)", ping_inputs,
                 "HipPing over HipRx, HipTx and HipTxStream"),
    "div": _fam(["pirip_hip_fsk_ldpc_rx_batch", "pirip_hip_div_collect", "pirip_hip_div_push_candidates", "pirip_hip_div_flush"],
                ["pirip_hip_div_reset", "pirip_hip_ldpc_reset", "pirip_hip_reset"], "carrier-less bytes (127), soft bits of the other sign",                div_inputs, "HipDiversity over HipLdpc and HipDemod"),
    "arq_air": _fam(["pirip_hip_arq_submit", "pirip_hip_arq_process"] + ["pirip_hip_arq_push"] * 3, ["pirip_hip_arq_reset"],
                    "lengths of zero, silence (byte 128)", pkt_inputs, "HipArq over HipPacket with HipRx, HipTx and HipTxStream"),
    "ldpc": _fam(["pirip_hip_demod_batch", "pirip_hip_ldpc_rx_batch", "pirip_hip_clear_estimators", "pirip_hip_demod_batch", "pirip_hip_ldpc_llr",
                  "pirip_hip_ldpc_decode_llr", "pirip_hip_fsk_ldpc_rx_batch_groups"], ["pirip_hip_reset", "pirip_hip_ldpc_reset"],
                 "carrier-less bytes (127)", div_inputs, "HipDemod and HipLdpc, the batch entry points of sections A and E"),
}
for _name, _f in FAMILIES.items():
    _f["enqueue_ms"], _f["gate_ms"] = MEASURED[_name]


# ---- literal streams and blocking calls in pirip_amd/csrc --------------------------------------------------------------------------------------
# LITERAL_STREAM: (file, how the line begins behind its indentation -- the longest entry that fits names the line --, occurrences, reason) for every hipLaunchKernelGGL,
# hipMemsetAsync, hipMemcpyAsync, hipMemcpy2DAsync or hipMemcpyToSymbolAsync whose stream argument is a literal 0, nullptr or NULL.
_D = "section D's host-buffer entry points (csdr's convert_u8_f, convert_f_s16, fir_decimate_cc): no stream parameter, synchronous"
_ST = "a self-test entry point without a stream parameter: the default stream, and the call reads the result back (the caller synchronises atan2)"
LITERAL_STREAM = [
    ("decim_kernels.hip", "hipLaunchKernelGGL(cvt_u8_f_kernel, dim3(blocks), dim3(kThreads), 0,", 1, _D),
    ("decim_kernels.hip", "hipLaunchKernelGGL(cvt_f_s16_kernel, dim3(blocks), dim3(kThreads), 0", 1, _D),
    ("decim_kernels.hip", "hipLaunchKernelGGL(decim_f32_kernel, dim3((unsigned)((n_out + kThrea", 1, _D),
    ("fsk_demod_general.hip", "hipLaunchKernelGGL(atan2_selftest_kernel, dim3((n + 255) / 256), dim", 1, _ST),
    ("fsk_demod_wave.hip", "hipLaunchKernelGGL(sqrt_selftest_kernel, dim3(4096), dim3(256), 0, 0", 2, _ST),
    ("fsk_demod_wave.hip", "hipLaunchKernelGGL(div_selftest_kernel<3>, dim3(4096), dim3(256), 0,", 2, _ST),
    ("fsk_demod_wave.hip", "hipLaunchKernelGGL(div_selftest_kernel<50>, dim3(4096), dim3(256), 0", 3, _ST),
]

# BLOCKING: the same for every hipMemcpy(, hipMemset(, hipMemcpyToSymbol(, hipDeviceSynchronize and hipStreamSynchronize; a line that
# several functions share word for word is one entry with all their reasons.
WHY = dict(
    create="create: the handle is complete when the call returns (the header: create synchronises the device)",
    destroy="destroy: waits for the handle's work on its device, then frees",
    getter='a getter or checking aid that copies to the host (the header: "synchronises the device")',
    host="a host-buffer convenience call: uploads, runs, downloads",
    setter="a setter with host arrays or one that moves the handle to another kernel: waits for calls in flight (the header: synchronises)",
    capture='pirip_hip_demod_capture and its host-buffer form: "The call synchronises `hip_stream` (it decides on the host what to re-run)"',
    synth='pirip_hip_synth_cu8: "Synchronous on hip_stream" (its host tables go out of scope)',
    selftest="a self-test on the default stream that reads its result back",
    timing="behind #ifdef PIRIP_WAVE_TIMING, which no build of the library defines",
    grow="grow_dev: work rows that grow wait for the calls that may still use the old ones (sections E, I and K say so)",
    reserve="pirip_hip_rx_create sizes the FSK_LDPC receiver's work rows ahead of the calls: create synchronises the device",
    shim="the codec2 shim's freedv_rawdatacomprx: a synchronous host-buffer call",
    sectiond="section D's host-buffer entry points: synchronous by contract",
)
BLOCKING = [
    ("arq_kernels.hip", "PIRIP_HIPCHK(hipDeviceSynchronize());", 1, "create"),
    ("capture.hip", "#define CAP_H2D(dst, src, bytes, st) do { PIRIP_HIPCHK(hipMemcpyAsync(ds", 1, "capture"),
    ("capture.hip", "PIRIP_HIPCHK(hipStreamSynchronize(st));", 8, "capture"),
    ("capture.hip", "if (in_bytes) PIRIP_HIPCHK(hipMemcpy(w->d_in, in, in_bytes, hipMemcpyHos", 1, "capture"),
    ("capture.hip", "if (nf) PIRIP_HIPCHK(hipMemcpy(bits, w->d_bits, (size_t)nf * fb, hipMemc", 1, "capture"),
    ("capture.hip", "if (rx_filt && nf) PIRIP_HIPCHK(hipMemcpy(rx_filt, w->d_filt, sizeof(flo", 1, "capture"),
    ("capture.hip", "if (stats && nf) PIRIP_HIPCHK(hipMemcpy(stats, w->d_ostats, sizeof(float", 1, "capture"),
    ("capture.hip", "PIRIP_HIPCHK(hipMemcpy(&sc, h->d_scal, sizeof(sc), hipMemcpyDeviceToHost", 1, "capture"),
    ("codec2_shim.hip", "if (hipMemcpy(f->d_in, demod_in, bytes, hipMemcpyHostToDevice) != hipSuc", 1, "shim"),
    ("codec2_shim.hip", 'if (hipDeviceSynchronize() != hipSuccess) die("hipDeviceSynchronize", PI', 1, "shim"),
    ("codec2_shim.hip", "bool ok = hipMemcpy(&nf, f->d_nfr, sizeof(nf), hipMemcpyDeviceToHost) ==", 2, "shim"),
    ("codec2_shim.hip", "hipMemcpy(pl.data(), f->d_payload, pl.size(), hipMemcpyDeviceToHost) == ", 1, "shim"),
    ("codec2_shim.hip", "hipMemcpy(in, f->d_info, sizeof(in), hipMemcpyDeviceToHost) == hipSucces", 1, "shim"),
    ("codec2_shim.hip", "hipMemcpy(stats, f->d_stats, sizeof(stats), hipMemcpyDeviceToHost) == hi", 1, "shim"),
    ("decim_kernels.hip", "hipMemcpy(d_in, in, sizeof(TI) * (size_t)n, hipMemcpyHostToDevice) == hi", 1, "sectiond"),
    ("decim_kernels.hip", "hipMemcpy(out, d_out, sizeof(TO) * (size_t)n, hipMemcpyDeviceToHost) == ", 1, "sectiond"),
    ("decim_kernels.hip", "hipMemcpy(p, lut.data(), sizeof(float) * 256, hipMemcpyHostToDevice) != ", 1, "sectiond"),
    ("decim_kernels.hip", "hipMemcpy(d_in, input, sizeof(float2) * (size_t)input_size, hipMemcpyHos", 1, "sectiond"),
    ("decim_kernels.hip", "hipMemcpy(d_taps, taps, sizeof(float) * (size_t)taps_length, hipMemcpyHo", 1, "sectiond"),
    ("decim_kernels.hip", "hipMemcpy(output, d_out, sizeof(float2) * (size_t)n_out, hipMemcpyDevice", 1, "sectiond"),
    ("div_kernels.hip", "PIRIP_HIPCHK(hipDeviceSynchronize());", 2, "create getter"),
    ("div_kernels.hip", "PIRIP_HIPCHK(hipMemcpy(host_llr, d->d_comb + ((size_t)group * d->P + slo", 1, "getter"),
    ("fsk_demod_wave.hip", "e = hipMemset(d, 0, sizeof(*d));", 1, "selftest"),
    ("fsk_demod_wave.hip", "e = hipMemcpy(mismatches, d, sizeof(*d), hipMemcpyDeviceToHost);", 1, "selftest"),
    ("fsk_demod_wave.hip", "e = hipMemset(d, 0, 2 * sizeof(*d));", 1, "selftest"),
    ("fsk_demod_wave.hip", "e = hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost);", 1, "selftest"),
    ("fsk_demod_wave.hip", "(void)hipStreamSynchronize(stream);", 1, "timing"),
    ("fsk_demod_wave.hip", "if (hipMemcpyToSymbol(HIP_SYMBOL(pirip::g_wave_timeline), &p, sizeof(p))", 1, "timing"),
    ("fsk_demod_wave.hip", "if (hipMemcpyToSymbol(HIP_SYMBOL(pirip::g_wave_timeline_rows), &n, sizeo", 1, "timing"),
    ("hip_host.hpp", "if (bytes) PIRIP_HIPCHK(hipMemset(*p, byte, bytes));", 1, "create"),
    ("hip_host.hpp", "if (bytes) PIRIP_HIPCHK(hipMemcpy(*p, src, bytes, hipMemcpyHostToDevice)", 1, "create"),
    ("hip_host.hpp", "if (sync == GrowSync::stream) PIRIP_HIPCHK(hipStreamSynchronize(st));", 1, "grow"),
    ("hip_host.hpp", "if (sync == GrowSync::device) PIRIP_HIPCHK(hipDeviceSynchronize());", 1, "grow"),
    ("hip_host.hpp", "(void)hipDeviceSynchronize();", 1, "destroy"),
    ("hip_host.hpp", "PIRIP_HIPCHK(hipDeviceSynchronize());", 1, "getter"),
    ("hip_host.hpp", "PIRIP_HIPCHK(hipMemcpy(out.data(), d_src, sizeof(T) * out.size(), hipMem", 1, "getter"),
    ("ldpc_rx.hip", "(void)hipDeviceSynchronize();", 1, "destroy"),
    ("ldpc_rx.hip", "PIRIP_HIPCHK(hipMemcpy(host_llr, h->d_llr_hist + (size_t)s * n, sizeof(u", 1, "getter"),
    ("ldpc_rx.hip", "PIRIP_HIPCHK(hipDeviceSynchronize());                  // (calls in flig", 1, "reserve"),
    ("ldpc_rx.hip", "PIRIP_HIPCHK(hipMemcpy(h->d_h_filt, rx_filt, sizeof(float) * per * ncall", 1, "host"),
    ("ldpc_rx.hip", "PIRIP_HIPCHK(hipDeviceSynchronize());", 1, "host"),
    ("ldpc_rx.hip", "PIRIP_HIPCHK(hipMemcpy(status, h->d_h_status, (size_t)ncalls, hipMemcpyD", 1, "host"),
    ("ldpc_rx.hip", "PIRIP_HIPCHK(hipMemcpy(payload, h->d_h_payload, nb * ncalls, hipMemcpyDe", 1, "host"),
    ("ldpc_rx.hip", "PIRIP_HIPCHK(hipMemcpy(info, h->d_h_info, sizeof(int32_t) * kInfoPerCall", 1, "host"),
    ("mac_kernels.hip", "PIRIP_HIPCHK(hipDeviceSynchronize());", 1, "create"),
    ("mac_kernels.hip", "(void)hipDeviceSynchronize();                                // the pack", 1, "destroy"),
    ("ping_kernels.hip", "PIRIP_HIPCHK(hipDeviceSynchronize());", 1, "create"),
    ("pirip_capi.hip", "PIRIP_HIPCHK(hipStreamSynchronize(nullptr));", 1, "create setter"),
    ("pirip_capi.hip", "(void)hipDeviceSynchronize();", 1, "destroy"),
    ("pirip_capi.hip", "if (in_bytes) PIRIP_HIPCHK(hipMemcpy(h->d_stage_in, in, in_bytes, hipMem", 1, "host"),
    ("pirip_capi.hip", "PIRIP_HIPCHK(hipDeviceSynchronize());", 7, "host getter setter"),
    ("pirip_capi.hip", "PIRIP_HIPCHK(hipMemcpy(&nf, h->d_stage_nframes, sizeof(nf), hipMemcpyDev", 1, "host"),
    ("pirip_capi.hip", "PIRIP_HIPCHK(hipMemcpy(&cons, h->d_stage_consumed, sizeof(cons), hipMemc", 1, "host"),
    ("pirip_capi.hip", "if (bits && nf) PIRIP_HIPCHK(hipMemcpy(bits, h->d_stage_bits, (size_t)nf", 1, "host"),
    ("pirip_capi.hip", "if (rx_filt && nf) PIRIP_HIPCHK(hipMemcpy(rx_filt, h->d_stage_filt, size", 1, "host"),
    ("pirip_capi.hip", "if (stats && nf) PIRIP_HIPCHK(hipMemcpy(stats, h->d_stage_stats, sizeof(", 1, "host"),
    ("pirip_capi.hip", "PIRIP_HIPCHK(hipMemcpy(&sc, h->d_scal, sizeof(sc), hipMemcpyDeviceToHost", 1, "host"),
    ("pirip_capi.hip", "PIRIP_HIPCHK(hipMemcpy(Sf_host, h->d_Sf + (size_t)s * h->plan.d.Ndft, si", 1, "getter"),
    ("pirip_capi.hip", "PIRIP_HIPCHK(hipMemset(h->d_eye, 0, bytes));", 1, "setter"),
    ("pirip_capi.hip", "PIRIP_HIPCHK(hipMemcpy(rx_eye, h->d_eye + (size_t)s * kEyeTraces * kEyeP", 1, "getter"),
    ("pirip_capi.hip", "PIRIP_HIPCHK(hipMemcpy(sc.data(), h->d_scal, sizeof(StreamScalars) * sc.", 1, "setter"),
    ("pirip_capi.hip", "PIRIP_HIPCHK(hipMemcpy(h->d_scal, sc.data(), sizeof(StreamScalars) * sc.", 1, "setter"),
    ("pirip_capi.hip", "PIRIP_HIPCHK(hipMemcpy(&sc, h->d_scal + s, sizeof(sc), hipMemcpyDeviceTo", 2, "getter"),
    ("pkt_kernels.hip", "PIRIP_HIPCHK(hipMemcpy(p->d_cauchy, cm.data(), cm.size(), hipMemcpyHostT", 1, "create"),
    ("pkt_kernels.hip", "PIRIP_HIPCHK(hipDeviceSynchronize());", 1, "create"),
    ("rpt_kernels.hip", "PIRIP_HIPCHK(hipDeviceSynchronize());", 1, "create"),
    ("stream_rx.hip", "PIRIP_HIPCHK(hipDeviceSynchronize());", 2, "create getter"),
    ("stream_rx.hip", "if (consumed_total) PIRIP_HIPCHK(hipMemcpy(consumed_total, rx->d_total, ", 1, "getter"),
    ("stream_rx.hip", "if (backlog) PIRIP_HIPCHK(hipMemcpy(backlog, rx->d_carry, sizeof(int32_t", 1, "getter"),
    ("stream_rx.hip", "PIRIP_HIPCHK(hipMemcpy(&flag, rx->d_flag, sizeof(flag), hipMemcpyDeviceT", 1, "getter"),
    ("synth_kernels.hip", "ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(st) == hipS", 1, "synth"),
    ("testbits_kernels.hip", "PIRIP_HIPCHK(hipDeviceSynchronize());", 1, "create"),
    ("testbits_kernels.hip", "PIRIP_HIPCHK(hipDeviceSynchronize());                      // (a push_re", 1, "setter"),
    ("tx_kernels.hip", "PIRIP_HIPCHK(hipDeviceSynchronize());", 2, "create setter"),
    ("tx_kernels.hip", "PIRIP_HIPCHK(hipDeviceSynchronize());                    // calls in fli", 1, "setter"),
    ("tx_kernels.hip", "PIRIP_HIPCHK(hipMemcpy(h->d_fm, fm.data(), sizeof(uint32_t) * fm.size(),", 1, "setter"),
    ("tx_kernels.hip", "PIRIP_HIPCHK(hipMemcpy(h->d_tm, tm.data(), sizeof(uint32_t) * tm.size(),", 1, "setter"),
    ("tx_kernels.hip", "PIRIP_HIPCHK(hipMemcpy(h->d_lead, lead.data(), sizeof(int32_t) * lead.si", 1, "setter"),
    ("tx_kernels.hip", "PIRIP_HIPCHK(hipMemcpy(h->d_gap, gap.data(), sizeof(int32_t) * gap.size(", 1, "setter"),
    ("txs_kernels.hip", "PIRIP_HIPCHK(hipDeviceSynchronize());", 1, "create"),
]


# ---- every entry point of the header that takes a hip_stream --------------------------------------------------------------------------------
def _t(family):
    return ("test", T + "test_%s_gated" % family)


ENTRY_POINTS = {
    # section A
    "pirip_hip_reset": _t("div"),
    "pirip_hip_clear_estimators": _t("ldpc"),
    "pirip_hip_demod_batch": _t("ldpc"),
    "pirip_hip_demod_capture": ("exempt", 'the header: "The call synchronises `hip_stream` (it decides on the host what to re-run)."'),
    # section B
    "pirip_hip_decim_batch": _t("decim"),
    "pirip_hip_synth_cu8": ("exempt", 'the header: "Noise-free output is bit-identical to fsk_mod_c. Synchronous on hip_stream."'),
    # section E
    "pirip_hip_ldpc_reset": _t("div"),
    "pirip_hip_ldpc_rx_batch": _t("ldpc"),
    "pirip_hip_fsk_ldpc_rx_batch": _t("div"),
    "pirip_hip_fsk_ldpc_rx_batch_groups": _t("ldpc"),
    "pirip_hip_ldpc_llr": _t("ldpc"),
    "pirip_hip_ldpc_decode_llr": _t("ldpc"),
    # section G
    "pirip_hip_rx_process": _t("rx_loop"),
    "pirip_hip_rx_push": _t("rx_plain"),
    "pirip_hip_rx_reset": _t("rx_plain"),
    # section H
    "pirip_hip_chan_batch": _t("chan"),
    # section I
    "pirip_hip_tx_reset": _t("tx"),
    "pirip_hip_tx_frame": _t("tx"),
    "pirip_hip_tx_modulate": _t("tx"),
    "pirip_hip_tx_records_to_iq": _t("tx"),
    "pirip_hip_tx_repeat_records": _t("tx"),
    # section J
    "pirip_hip_mux_batch": _t("mux"),
    # section K (pirip_hip_txs_send in the case the header excepts -- "a call with a larger max_rec than any before it grows the handle's
    # work rows, as in section I" -- is made once in front of the gate; the gated sends are the ones that do not grow)
    "pirip_hip_txs_send": _t("txs"),
    "pirip_hip_txs_process": _t("txs"),
    "pirip_hip_txs_reset": _t("txs"),
    # section L
    "pirip_hip_tbits_push": _t("tbits"),
    "pirip_hip_tbits_reset": _t("tbits"),
    "pirip_hip_tbits_push_records": _t("tbits"),
    # section M
    "pirip_hip_rpt_push_records": _t("rpt"),
    "pirip_hip_rpt_process": _t("rpt"),
    "pirip_hip_rpt_push": _t("rpt"),
    "pirip_hip_rpt_reset": _t("rpt"),
    # section N
    "pirip_hip_ping_push_records": _t("ping"),
    "pirip_hip_ping_process": _t("ping"),
    "pirip_hip_ping_push": _t("ping"),
    "pirip_hip_ping_reset": _t("ping"),
    # section O
    "pirip_hip_air_set_sigma": _t("air"),
    "pirip_hip_air_push": _t("air"),
    "pirip_hip_air_reset": _t("air"),
    "pirip_hip_air_reset_drift": _t("air"),
    # section P
    "pirip_hip_spec_push": _t("spec"),
    "pirip_hip_spec_reset": _t("spec"),
    # section Q
    "pirip_hip_div_reset": _t("div"),
    "pirip_hip_div_collect": _t("div"),
    "pirip_hip_div_push_candidates": _t("div"),
    "pirip_hip_div_flush": _t("div"),
    # section R
    "pirip_hip_pkt_send": _t("pkt"),
    "pirip_hip_pkt_push_records": _t("pkt"),
    "pirip_hip_pkt_process": _t("pkt"),
    "pirip_hip_pkt_push": _t("pkt"),
    "pirip_hip_pkt_reset": _t("pkt"),
    # section S
    "pirip_hip_arq_submit": _t("arq"),
    "pirip_hip_arq_push_records": _t("arq"),
    "pirip_hip_arq_process": _t("arq_air"),
    "pirip_hip_arq_push": _t("arq_air"),
    "pirip_hip_arq_reset": _t("arq"),
    # section T
    "pirip_hip_mac_reset": _t("mac"),
    # include/pirip_hip_rccl.h
    "pirip_hip_gather_bits": ("exempt", "one call per rank under the caller's ncclComm_t: a single process on one device cannot make it, and the "
                                        "sends and receives it enqueues run inside RCCL on the stream it is handed "
                                        "(tests/test_gather_fake_nccl.py holds its layout against a stand-in library on the CPU)"),
}
