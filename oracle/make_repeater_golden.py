#!/usr/bin/env python3
"""oracle/make_repeater_golden.py -- drives oracle/_ref/frame_repeater (the reference's own program, oracle/build_ref_repeater.sh) over
generated receiver record streams and writes tests/golden/repeater_cases.npz: per case the bytes the program read on stdin (records of
one status byte + kb payload bytes) and the bytes it wrote on stdout (Tx records of one burst-control byte + kb bytes). Only data the
program reads and writes is stored. The file is deterministic: fixed seeds, fixed archive timestamps.

Cases: kb in {13, 32, 37}, three source bytes, 41 hand-written status sequences per kb that name each branch of the state machine
(NAMED below) and 110 / 50 / 50 random ones. Status bytes come from {0, 2, 4, 6, 8, 0xA, 0xC, 0xE, 1}; the random draw picks a burst length of
1 .. 100 frames first and then fills it, so that long bursts occur; no burst exceeds 100 frames (the program asserts there)."""
import io
import os
import subprocess
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "oracle", "_ref", "frame_repeater")
OUT = os.path.join(ROOT, "tests", "golden", "repeater_cases.npz")
KBS = (13, 32, 37)
SOURCES = (0x00, 0x07, 0xFF)
N_RANDOM = {13: 110, 32: 50, 37: 50}
SYNC, BITS, ERR = 2, 4, 8
VALUES = (0, 2, 4, 6, 8, 0xA, 0xC, 0xE, 1)

NAMED = [
    ("empty input", []),
    ("idle only", [0, 0, 1, 0]),
    ("clean burst of three", [0, 2, 6, 6, 6, 2, 0, 0]),
    ("clean burst, two of them", [2, 6, 6, 2, 0, 0, 2, 6, 2, 0]),
    ("one frame, SYNC drops at once", [6, 0]),
    ("first record carries BIT_ERRORS: no start", [0xE, 0]),
    ("first record carries BIT_ERRORS, the burst starts at the next clean one", [0xE, 6, 6, 2, 0]),
    ("only frames with BIT_ERRORS: nothing is ever sent", [2, 0xE, 0xE, 0xE, 2, 0]),
    ("SYNC without BITS does not start", [2, 2, 2, 0]),
    ("BITS without SYNC does not start", [4, 4, 0]),
    ("BITS|ERR without SYNC does not start", [0xC, 0]),
    ("trial sync does not start", [1, 1, 0]),
    ("status 7 is not SYNC|BITS: no start", [7, 0]),
    ("BITS without SYNC inside a burst: append and flush in one record", [6, 4]),
    ("BITS|ERR without SYNC inside a burst: append and flush", [6, 6, 0xC, 0]),
    ("a frame with BIT_ERRORS inside a burst is taken", [6, 0xE, 6, 2, 0]),
    ("SYNC|ERR without BITS inside a burst: stays open, takes nothing", [6, 0xA, 0xA, 6, 0]),
    ("status 8 ends a burst", [6, 6, 8]),
    ("status 1 ends a burst", [6, 1]),
    ("SYNC held without BITS between frames", [6, 2, 2, 6, 2, 2, 2, 6, 2, 0]),
    ("back to back: flush then start in the next record", [6, 0, 6, 0, 6, 0]),
    ("back to back through append-and-flush", [6, 4, 6, 4, 6, 4]),
    ("the record that ends a burst cannot start one: 6 4 4 6", [6, 4, 4, 6, 0]),
    ("burst open at the end of input: nothing written", [6, 6, 6]),
    ("a burst, then one left open", [6, 6, 0, 6, 6, 2]),
    ("a single 6 left open", [6]),
    ("each value alone while idle", [0, 2, 4, 8, 0xA, 0xC, 0xE, 1]),
    ("each value after a start", [6, 0, 6, 2, 0, 6, 4, 6, 8, 6, 0xA, 0, 6, 0xC, 6, 0xE, 0, 6, 1]),
    ("burst of exactly 100 frames, ended by 0", [6] * 100 + [0]),
    ("burst of exactly 100 frames, the last by append-and-flush", [6] * 99 + [4]),
    ("burst of 99 frames", [2] + [6] * 99 + [2, 0]),
    ("100 frames with gaps of SYNC alone and BIT_ERRORS frames", ([6] + [2, 0xE, 6, 0xA] * 33)[:-1] + [2, 0]),
    ("3 frames, then 64 idle, then 3", [6, 6, 6, 0] + [0] * 64 + [6, 6, 6, 0]),
    ("63, 64 and 65 records before the start", [0] * 63 + [6, 0] + [2] * 64 + [6, 0] + [0] * 65 + [6, 0]),
    ("many one-frame bursts", [6, 0] * 12),
    ("many two-frame bursts by append-and-flush", [6, 4] * 12),
    ("alternating 6 and E while idle and receiving", [0xE, 6, 0xE, 6, 0xE, 0, 0xE, 6, 0]),
    ("0xC then 6: the first does nothing, the second starts", [0xC, 6, 0xC]),
    ("start, then only SYNC until the end of input", [6] + [2] * 30),
    ("ends with a flush in the last record", [0, 0, 6, 6, 6, 0]),
    ("long idle", [0] * 70),
]


def random_status(rng):
    """a record stream whose bursts have 1 .. 100 frames: the length is drawn first (skewed to short ones, or exactly 100), then filled"""
    st = []
    if rng.random() < 0.15:                                   # values drawn independently: short bursts, every transition
        return [int(v) for v in rng.choice(VALUES, int(rng.integers(1, 120)))]
    for _ in range(int(rng.integers(1, 3))):
        st += [int(v) for v in rng.choice([0, 0, 2, 2, 4, 8, 0xA, 0xC, 0xE, 1], int(rng.integers(0, 12)))]
        L = 100 if rng.random() < 0.04 else int(np.floor(np.exp(rng.uniform(0.0, 1.0) ** 2 * np.log(101.0))))
        L = min(max(L, 1), 100)
        st.append(SYNC | BITS)
        n = 1
        flush_with_bits = rng.random() < 0.3 and L > 1
        while n < L - (1 if flush_with_bits else 0):
            v = int(rng.choice([6, 6, 6, 6, 0xE, 2, 0xA]))
            st.append(v)
            n += 1 if v & BITS else 0
        st += [int(v) for v in rng.choice([2, 0xA], int(rng.integers(0, 3)))]
        if rng.random() < 0.1:
            return st                                         # left open at the end of input
        st.append(int(rng.choice([4, 0xC])) if flush_with_bits else int(rng.choice([0, 0, 8, 1])))
    return st


def check_bursts(st):
    n, rec = 0, False
    for v in st:
        if not rec:
            rec, n = (v == 6), 1
        else:
            n += 1 if v & BITS else 0
            assert n <= 100, "a burst above 100 frames: the program asserts"
            rec = bool(v & SYNC)


def cases():
    out = []
    for kb in KBS:
        rng = np.random.default_rng(20201100 + kb)
        seqs = [(name, st) for name, st in NAMED] + [("random %d" % i, random_status(rng)) for i in range(N_RANDOM[kb])]
        for i, (name, st) in enumerate(seqs):
            check_bursts(st)
            rec = rng.integers(0, 256, (len(st), 1 + kb)).astype(np.uint8)
            rec[:, 0] = st
            out.append((kb, SOURCES[i % len(SOURCES)], name, rec))
    return out


def run(kb, source, rec):
    p = subprocess.run([EXE, str(8 * kb), "0x%02x" % source], input=rec.tobytes(), capture_output=True)
    assert p.returncode == 0, (p.returncode, p.stderr[-300:])
    return np.frombuffer(p.stdout, dtype=np.uint8)


def save_npz(path, arrays):
    """np.savez with fixed member timestamps: the same arrays give the same file"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), version=(1, 0), allow_pickle=False)
            zi = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.external_attr = 0o644 << 16
            z.writestr(zi, buf.getvalue())


def main():
    if not os.path.exists(EXE):
        sys.exit("oracle/_ref/frame_repeater missing: run oracle/build_ref_repeater.sh first")
    cs = cases()
    outs = [run(kb, src, rec) for kb, src, _, rec in cs]
    longest = max((int(np.diff(np.flatnonzero(np.concatenate([[1], o.reshape(-1, 1 + kb)[:, 0] == 2]))).max(initial=0)) - 1)
                  for (kb, _, _, _), o in zip(cs, outs) if o.size)
    assert longest == 100, longest                            # a burst of exactly 100 frames is among them and none is longer
    ins = [rec.reshape(-1) for _, _, _, rec in cs]
    save_npz(OUT, {
        "kb": np.array([c[0] for c in cs], dtype=np.int32), "source": np.array([c[1] for c in cs], dtype=np.int32),
        "name": np.array([c[2].encode() for c in cs]),
        "stdin": np.concatenate(ins), "stdin_end": np.cumsum([a.size for a in ins]).astype(np.int64),
        "stdout": np.concatenate(outs), "stdout_end": np.cumsum([a.size for a in outs]).astype(np.int64)})
    print(f"{len(cs)} cases, {sum(a.size for a in ins)} bytes in, {sum(a.size for a in outs)} bytes out, longest burst {longest} -> {OUT} "
          f"({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
