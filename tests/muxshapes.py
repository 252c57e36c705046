"""Shape tables and inputs shared by tests/test_mux_cpu.py (no GPU: the tables reach the paths they claim, the float64 chain alone
passes the loopback) and tests/test_mux.py (the device)."""
import os
import subprocess

import numpy as np

import chanref
import muxref
import txref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "pirip_amd", "bin")
CODE = os.path.join(ROOT, "pirip_amd", "data", "standin_256_512_4.code")

FS24 = 1 << 24


def edge(Fs):
    return Fs // 2 - 1 if Fs % 2 == 0 else (Fs - 1) // 2


# name -> (Fs, D, transition_bw, offsets, outputs, noutputs, branch outputs (n_in - Q + 1), m0)
SHAPES = {
    # D = 1: the filter alone; 9 channels on one output, three groups of 3 (LDS) with the FIR
    "d1_k9": (2400000, 1, 0.05, [0, 1, -1199999, 1199999, -1, 345678, -700003, 5, 250000], None, 1, 2301, 0),
    "d2_k3": (FS24, 2, 0.05, [0, edge(FS24), -edge(FS24)], None, 1, 1151, 12345),
    "d6_k8": (240000, 6, 0.05, [-90000, -30000, 30001, 90000, 0, 1, -1, 119999], None, 1, 701, -5),
    "d6_long": (240000, 6, 0.0125, [-119999, 0, 60001], None, 1, 501, 7),
    # two outputs with unequal channel counts, outputs 1 and 3 empty
    "d30_outs": (2400000, 30, 0.05, [-700003, 1, 0, 1199999, -1], [0, 2, 0, 2, 2], 4, 77, 2 ** 31 + 3),
    "d30_k9": (2400000, 30, 0.05, [-875000, -625000, -375000, -125000, 125000, 375000, 625000, 875000, 3], None, 1, 75, 0),
    "d45_k1": (FS24 - 1, 45, 0.05, [-edge(FS24 - 1)], None, 1, 51, -1000),
    "d125_k3": (2400000, 125, 0.05, [1199999, 0, -1], None, 1, 19, 99),
}
KINDS = [(s, k) for s in SHAPES for k in (muxref.FIR, muxref.LINEAR) if not (s == "d6_long" and k == muxref.LINEAR)]


def taps_len(kind, D, tbw):
    return chanref.filter_len(tbw) if kind == muxref.FIR else 2 * D - 1


def channels_of(outputs, K, noutputs):
    out = [0] * K if outputs is None else outputs
    return [[c for c in range(K) if out[c] == i] for i in range(noutputs)]


def inputs(name, n_in):
    """(z complex64 [K, n_in], gains float32 [K]): unit-variance noise, gains of both signs between 0.02 and 0.12 in magnitude"""
    K = len(SHAPES[name][3])
    rng = np.random.default_rng(sorted(SHAPES).index(name) + 40)
    z = (rng.normal(size=(K, n_in)) + 1j * rng.normal(size=(K, n_in))).astype(np.complex64)
    g = (rng.uniform(0.02, 0.12, K) * np.where(np.arange(K) % 2, -1.0, 1.0)).astype(np.float32)
    return z, g


# ---- the loopback: four FSK_LDPC channels on one 240 kS/s stream, the deployed shape of tests/test_channelizer.py ------------------------
# Chosen so that the float64 chain alone passes (tests/test_mux_cpu.py): amplitudes of 20 .. 30 u8 steps as that test uses (a modem sample
# has modulus 2, the FIR has unity gain: gain = steps / 255), 200 symbols and more of silence in front (tests/test_tx.py: with 40 the
# receiver misses the first frame at some timing offsets), 700 behind (a frame is delivered once a further frame's worth has arrived).
LOOP = dict(Fs=240000, D=6, offsets=[-90000, -30000, 30001, 90000], mFs=40000, Rs=1000, M=2, P=10, f1=1000, shift=2000, est_min=500,
            est_max=15000, steps=[20.0, 30.0, 20.0, 25.0], lead=[200, 207, 214, 221], tail=700, nframes=3)
LOOP_GAINS = (np.array(LOOP["steps"]) / 255.0).astype(np.float32)


def loop_records(seed=21):
    """uint8 [4, 4, 1 + kb]: per channel one burst of three frames with random payloads and the end-of-burst record"""
    rng = np.random.default_rng(seed)
    return np.stack([txref.records(rng, [1] + [0] * (LOOP["nframes"] - 1) + [2], 32) for _ in LOOP["offsets"]])


def loop_syms(rec):
    """the symbol rows HipTx makes of the records, from the framer tool: uint8 [4, nsym]"""
    rows = []
    for c in range(rec.shape[0]):
        p = subprocess.run([os.path.join(BIN, "fsk_ldpc_framer"), "--code", CODE, "-m", "2", "--packed", "--gap", "0", "-", "-"],
                           input=rec[c].tobytes(), capture_output=True)
        assert p.returncode == 0, p.stderr
        bits = np.frombuffer(p.stdout, dtype=np.uint8)
        rows.append(np.concatenate([np.full(LOOP["lead"][c], txref.OFF, np.uint8), txref.bits_to_syms(bits, 2)]))
    nsym = max(len(r) for r in rows) + LOOP["tail"]
    return np.stack([np.concatenate([r, np.full(nsym - len(r), txref.OFF, np.uint8)]) for r in rows])
