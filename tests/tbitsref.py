"""Reference of the test-frame counter (include/pirip_hip.h section L) in numpy, for tests/test_testbits*.py.

Uncoded: fsk_put_test_bits' sliding comparison for any frame and frame size. With b the bits of a stream in order and b[i] = 0 for i < 0,
position j has errs = Hamming distance of b[j - F + 1 .. j] to the frame and is valid iff float32(errs) < float32(thresh) * float32(F) --
PutBits::push's own expression in its own precision; a valid position adds 1 to packets, F to bits and errs to errors.
Coded: rtl_fsk --testframes' ecdd over records, tallied."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "pirip_amd", "bin")
RX_BITS = 4
INFO_PER_CALL = 10
NAMES = ("packets", "bits", "errors", "pushed")
REC_NAMES = ("frames", "bits", "errors", "frames_in_error", "crc_ok")


def limit(F, thresh):
    """the float the error count is compared with"""
    return np.float32(thresh) * np.float32(F)


def window_errs(bits, frame, hist=None):
    """errs of every position of `bits` (int64 [len(bits)]); hist: the F - 1 bits in front (None: zeros)"""
    frame = np.asarray(frame, dtype=np.uint8)
    F = frame.size
    pre = np.zeros(F - 1, dtype=np.uint8) if hist is None else np.asarray(hist, dtype=np.uint8)
    assert pre.size == F - 1
    b = np.concatenate([pre, np.asarray(bits, dtype=np.uint8) & 1])
    n = b.size - (F - 1)
    out = np.zeros(n, dtype=np.int64)
    step = max(1, (1 << 24) // F)
    for j in range(0, n, step):
        w = np.lib.stride_tricks.sliding_window_view(b[j:j + min(step, n - j) + F - 1], F)
        out[j:j + w.shape[0]] = (w != frame[None, :]).sum(axis=1)
    return out


class Counter:
    """one stream's counter, fed call by call"""

    def __init__(self, frame, thresh=0.1):
        self.frame = np.asarray(frame, dtype=np.uint8).copy()
        self.F = self.frame.size
        self.thr = limit(self.F, thresh)
        self.reset()

    def reset(self):
        self.hist = np.zeros(self.F - 1, dtype=np.uint8)
        self.packets = self.bits = self.errors = self.pushed = 0

    def push(self, bits):
        bits = np.asarray(bits, dtype=np.uint8).reshape(-1) & 1
        e = window_errs(bits, self.frame, self.hist)
        valid = e.astype(np.float32) < self.thr
        self.packets += int(valid.sum())
        self.bits += int(valid.sum()) * self.F
        self.errors += int(e[valid].sum())
        self.pushed += bits.size
        self.hist = np.concatenate([self.hist, bits])[-(self.F - 1):] if self.F > 1 else self.hist
        return e

    def counters(self):
        return {k: getattr(self, k) for k in NAMES}


def count(bits, frame, thresh=0.1):
    c = Counter(frame, thresh)
    c.push(bits)
    return c.counters()


def count_streams(rows, nframes, frame, thresh=0.1):
    """rows uint8 [n, max_frames, row_bits] (one bit per byte), nframes [n] (clamped to [0, max_frames]) -> dict of int64 [n]"""
    n, maxf = rows.shape[0], rows.shape[1]
    nf = np.clip(np.asarray(nframes, dtype=np.int64), 0, maxf)
    res = [count(rows[s, :nf[s]].reshape(-1), frame, thresh) for s in range(n)]
    return {k: np.array([r[k] for r in res], dtype=np.int64) for k in NAMES}


def put_test_bits_tool(bits, F=100, thresh=0.1, packet_pass=0, ber_pass=0.0):
    """the CPU tool (pirip::PutBits) on the bits: (its summary line, (packets, bits, errors), exit code)"""
    cmd = [os.path.join(BIN, "fsk_put_test_bits"), "-q", "-f", str(F), "-t", repr(float(thresh)), "-p", str(packet_pass), "-b", repr(float(ber_pass)), "-"]
    p = subprocess.run(cmd, input=np.asarray(bits, dtype=np.uint8).tobytes(), capture_output=True)
    line = [ln for ln in p.stderr.decode().split("\n") if ln.startswith("[")][-1]
    t = line.replace(",", " ").split()
    return line, (int(t[0].strip("[]")), int(t[t.index("tested") + 1]), int(t[t.index("errors") + 1])), p.returncode


def assert_matches_cpu(oracle, bits, F=100, thresh=0.1):
    """for the default frame the reference equals oracle.put_test_bits and the fsk_put_test_bits tool (PutBits); returns the counters"""
    frame = oracle.get_test_bits(F, F)
    got = count(bits, frame, thresh)
    o = oracle.put_test_bits(bits, framesize=F, valid_thresh=thresh)
    assert (got["packets"], got["bits"], got["errors"]) == (o["packets"], o["bits"], o["errors"]), (got, o)
    _, tool, _ = put_test_bits_tool(bits, F, thresh)
    assert (got["packets"], got["bits"], got["errors"]) == tool, (got, tool)
    return got


def pack_rows(rows, pad=0):
    """[..., row_bits] one bit per byte -> [..., ceil(row_bits / 8)] MSB first, the pad bits of the last byte set to `pad`"""
    rb = rows.shape[-1]
    padded = np.concatenate([rows & 1, np.full(rows.shape[:-1] + ((-rb) % 8,), pad, dtype=np.uint8)], axis=-1)
    return np.packbits(padded, axis=-1)


def record_tally(status, payload, info, ncalls, want):
    """status [n, R], payload [n, R, data_bytes], info [n, R, 10], ncalls [n] (clamped) -> dict of int64 [n]: rtl_fsk.cpp's rule -- a record
    counts when info[6] >= 0, its errors the popcount of payload ^ want over bytes 2 .. data_bytes - 3"""
    n, R, db = payload.shape
    nc = np.clip(np.asarray(ncalls, dtype=np.int64), 0, R)
    out = {k: np.zeros(n, dtype=np.int64) for k in REC_NAMES}
    want = np.asarray(want, dtype=np.uint8)
    for s in range(n):
        for r in range(nc[s]):
            out["crc_ok"][s] += bool(status[s, r] & RX_BITS)
            if info[s, r, 6] < 0:
                continue
            e = int(np.unpackbits(payload[s, r, 2:db - 2] ^ want[2:db - 2]).sum())
            out["frames"][s] += 1
            out["bits"][s] += 8 * max(db - 4, 0)
            out["errors"][s] += e
            out["frames_in_error"][s] += e > 0
    return out


def framed_bits(frame, errors, offset=0, rng=None, lead=None):
    """test frames one after the other, frame i with errors[i] bits flipped (at positions drawn from rng), the first `offset` bits
    dropped; lead: bits put in front"""
    rng = rng or np.random.default_rng(0)
    F = len(frame)
    out = []
    for e in errors:
        f = np.array(frame, dtype=np.uint8)
        f[rng.choice(F, size=min(e, F), replace=False)] ^= 1
        out.append(f)
    b = np.concatenate(out)[offset:]
    return b if lead is None else np.concatenate([np.asarray(lead, dtype=np.uint8), b])
