"""Inputs of tests/test_testbits.py (GPU) and tests/test_testbits_cpu.py, which shows on the reference alone (tests/tbitsref.py) that they
reach the cases they are meant for. Every reference result is computed once and shared."""
import functools

import numpy as np

import tbitsref

# 1. synthetic rows: 5 streams of at most 9 rows of 50 bits, the default frame
SYN = dict(F=100, row_bits=50, max_frames=9, nframes=[0, 1, 2, 7, 9], thresh=0.1)
SYN_OFFSETS = [0, 13, 9, 8, 71]                 # stream 2 (two rows): the frame from its 10th bit on, valid only thanks to the zero prefix
SYN_ERRORS = [[0, 9, 10, 12, 3, 0], [1, 11, 9, 0, 2, 5], [0, 10, 9, 12, 1, 0], [9, 11, 3, 0, 7, 2], [0, 9, 10, 12, 9, 4]]
SYN_SPLITS = [1, 3, 0, 5]                       # the same rows as calls of 1, 3, 0 and 5 rows


@functools.lru_cache(maxsize=None)
def default_frame(F=100):
    from oracle import binding as ob
    return ob.get_test_bits(F, F)


@functools.lru_cache(maxsize=None)
def syn_rows():
    """uint8 [5, 9, 50]"""
    rng = np.random.default_rng(12)
    n = SYN["max_frames"] * SYN["row_bits"]
    rows = [tbitsref.framed_bits(default_frame(), SYN_ERRORS[s], SYN_OFFSETS[s], rng)[:n] for s in range(5)]
    return np.stack(rows).reshape(5, SYN["max_frames"], SYN["row_bits"])


@functools.lru_cache(maxsize=None)
def syn_want(nframes):
    return tbitsref.count_streams(syn_rows(), list(nframes), default_frame(), SYN["thresh"])


# errs exactly at the limit: (F, valid_thresh, errors in the one frame sent, valid?)
LIMIT_CASES = [(100, 0.1, 9, True), (100, 0.1, 10, False), (100, 0.07, 6, True), (100, 0.07, 7, False), (100, 0.07, 8, False),
               (300, 0.09, 27, True), (300, 0.09, 28, False)]


@functools.lru_cache(maxsize=None)
def limit_bits(F, e):
    """an inverted default frame (no window near the frame), then the frame with e errors: 2 F bits, one window to decide"""
    f = default_frame(F)
    b = f.copy()
    b[np.random.default_rng(100 * F + e).choice(F, size=e, replace=False)] ^= 1
    return np.concatenate([1 - f, b])


# 2. frame sizes around the word boundaries of the packed window, each with every row length
SWEEP_F = [1, 8, 31, 32, 33, 64, 65, 100, 257, 4096]
SWEEP_ROW_BITS = [1, 50, 64, 100]
SWEEP_UNIT = 1600                               # lcm of the row lengths: one bit stream per F serves them all


def sweep_thresh(F):
    return 0.5 if F <= 8 else 0.1


@functools.lru_cache(maxsize=None)
def sweep_frame(F):
    if F == 8:
        return np.ones(8, dtype=np.uint8)       # a constant frame: neighbouring windows are valid together
    return np.random.default_rng(1000 + F).integers(0, 2, F).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def sweep_bits(F):
    """uint8 [3, total]: frames with 0, the largest valid, the smallest invalid and 0 errors in turn, each stream at its own offset
    behind its own random lead"""
    thr = float(tbitsref.limit(F, sweep_thresh(F)))
    vmax = int(np.ceil(thr)) - 1                # errs < thr
    total = SWEEP_UNIT * -(-(4 * F + 40) // SWEEP_UNIT)
    rng = np.random.default_rng(2000 + F)
    out = []
    for s in range(3):
        errs = [[0, vmax, min(vmax + 1, F), 0][i % 4] for i in range(total // F + 2)]
        lead = rng.integers(0, 2, 5 * s).astype(np.uint8)
        out.append(tbitsref.framed_bits(sweep_frame(F), errs, (F * s) // 3, rng, lead)[:total])
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def sweep_want(F):
    b = sweep_bits(F)
    res = [tbitsref.count(b[s], sweep_frame(F), sweep_thresh(F)) for s in range(b.shape[0])]
    return {k: np.array([r[k] for r in res], dtype=np.int64) for k in tbitsref.NAMES}


# 3. grid edges
@functools.lru_cache(maxsize=None)
def many_streams():
    """uint8 [300, 3, 50]: more streams than a wave has lanes and than a workgroup would hold"""
    rng = np.random.default_rng(31)
    rows = [tbitsref.framed_bits(default_frame(), [s % 13, (s // 13) % 13, 0], s % 60, rng)[:150] for s in range(300)]
    return np.stack(rows).reshape(300, 3, 50)


@functools.lru_cache(maxsize=None)
def long_stream(nrows=3000):
    """uint8 [1, nrows, 50]: many tiles of one stream"""
    rng = np.random.default_rng(32)
    n = nrows * 50
    errs = [i % 13 for i in range(n // 100 + 2)]
    return tbitsref.framed_bits(default_frame(), errs, 37, rng)[:n].reshape(1, nrows, 50)


@functools.lru_cache(maxsize=None)
def want_of(name):
    rows = {"many": many_streams, "long": long_stream, "calls200": lambda: long_stream()[:, :600].reshape(3, 200, 50)}[name]()
    return tbitsref.count_streams(rows, [rows.shape[1]] * rows.shape[0], default_frame(), 0.1)


# 6. records: crafted status / payload / info rows
REC_DB = 32


def crafted_records(want):
    """(status [3, 6], payload [3, 6, 32], info [3, 6, 10], ncalls): decoded and not, CRC good and not, errors in bytes 0, 1 (not
    compared), 2, data_bytes - 3 (compared) and data_bytes - 2 (the CRC: not compared)"""
    n, R, db = 3, 6, REC_DB
    rng = np.random.default_rng(61)
    status = rng.choice([0, 2, 6, 14, 3], size=(n, R)).astype(np.uint8)
    payload = np.tile(np.asarray(want, dtype=np.uint8), (n, R, 1))
    info = np.full((n, R, tbitsref.INFO_PER_CALL), -1, dtype=np.int32)
    info[:, :, 6] = rng.choice([-1, 0, 17, 543], size=(n, R))
    info[0, 0, 6], info[0, 1, 6], info[1, 0, 6] = 5, -1, 0
    for s in range(n):
        for r, (byte, mask) in enumerate([(0, 0xff), (1, 0x81), (2, 0x07), (db - 3, 0xf0), (db - 2, 0xff), (7, 0x00)]):
            payload[s, (r + s) % R, byte] ^= mask
    payload[2, 3, 10:14] ^= 0x55
    return status, payload, info, np.array([6, 4, 9], dtype=np.int32)
