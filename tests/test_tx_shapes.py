"""The device transmitter (include/pirip_hip.h section I) away from the one point tests/test_tx.py visits: the framer on four code
shapes (m = 32, 96, 304, 256 parity rows: less than one wave, a partial last group of 64, more than four groups) checked against
fsk_ldpc_framer AND, independently of this project's encoder, against H, the CRC16 and the UW of the code file; and the modulator at
the limits its exactness argument names (Fs = 2^24, Ts from 1 to 1024, tones at 0, +-1, +-(Fs/2 - 1) and next to multiples of Rs, rows
aligned to the sample only, more than 65535 streams), against tests/txref.py's float64 formula with the bound derived there."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sigutil
import txref
from test_ldpc import _write_random_code

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "pirip_amd", "bin")
OFF = txref.OFF
UNSUPPORTED = -6
CODE_SHAPES = [(136, 104), (200, 104), (600, 296), (512, 256)]      # m = 32, 96, 304, 256; kb = 13, 13, 37, 32; 32 + n even for all


def write_code(tmp_path, n, k):
    path = os.path.join(str(tmp_path), "acc_%d_%d.code" % (n, k))
    _write_random_code(path, n, k, 3, seed=n)
    return path


def parse_code(path):
    """(n, k, uw bits [32], H uint8 [m, n]) from the code-file text, in numpy and nothing else"""
    lines = [ln.split() for ln in open(path).read().split("\n") if ln.strip() and not ln.startswith("#")]
    kv = {t[0]: t[1:] for t in lines if not t[0].isdigit()}
    n, k, m = int(kv["n"][0]), int(kv["k"][0]), int(kv["rows"][0])
    at = next(i for i, t in enumerate(lines) if t[0] == "rows")
    H = np.zeros((m, n), dtype=np.uint8)
    for r in range(m):
        H[r, [int(c) for c in lines[at + 1 + r]]] = 1
    assert m == n - k
    return n, k, np.array([int(b) for b in kv["uw"]], dtype=np.uint8), H


def check_frames(bits, plan, recs, lead_bits, gap_bits, pre_bits, n, k, uw, H, crc16):
    """walks one stream's framer output by its record plan: every frame is UW | c with H c = 0, the record's bytes, and their CRC16"""
    at, frames = lead_bits, 0
    assert not bits[:lead_bits].any()
    for ctl, rec in zip(plan, recs):
        if ctl == 2:
            assert not bits[at:at + gap_bits].any()
            at += gap_bits
        elif ctl in (0, 1):
            at += pre_bits if ctl == 1 else 0
            fr = bits[at:at + 32 + n]
            assert np.array_equal(fr[:32], uw)
            c = fr[32:].astype(np.int64)
            assert not ((H.astype(np.int64) @ c) % 2).any(), "H c != 0"
            by = np.packbits(fr[32:32 + k])
            assert np.array_equal(by[:-2], rec[1:k // 8 - 1])
            assert (int(by[-2]) << 8 | int(by[-1])) == crc16(by[:-2])
            at += 32 + n
            frames += 1
    assert at == bits.size
    return frames


def framer_case(oracle, code, M, n, k, rng, B=6):
    """mixed-control record plans through pirip_hip_tx_frame: the device bits equal fsk_ldpc_framer --packed, every frame satisfies H,
    carries the CRC16 and the file's UW, the symbols are the bits' -> number of frames checked"""
    import torch
    import pirip_amd
    bps = 1 if M == 2 else 2
    lead = [int(v) for v in rng.integers(0, 140, B)]
    gap = [int(v) for v in rng.integers(0, 140, B)]
    tx = pirip_amd.HipTx(code, 240000, 10000, M, nstreams=B, f1=10000, shift=10000, lead=lead, gap=gap)
    kb = tx.data_bytes
    assert kb == k // 8 and tx.bits_per_frame == 32 + n
    plans = [txref.burst_plan(rng, 1 + s % 3, 1 + (s * 5) % 7) for s in range(B)]
    plans[1] = [0, 1, 2, 2, 0, 7, 1, 0, 2]                           # a frame before any preamble, two ends in a row, an unknown control byte
    plans[2] = txref.burst_plan(rng, 25, 3)                          # more than 64 records
    recs = [txref.records(rng, p, kb) for p in plans]
    max_rec = max(len(p) for p in plans)
    host = np.ones((B, max_rec + 2, 1 + kb), dtype=np.uint8)
    for s in range(B):
        host[s, :len(plans[s])] = recs[s]
    nrec = np.array([len(p) for p in plans], dtype=np.int32)
    cap = tx.max_syms(max_rec)
    d_rec, d_nrec = torch.from_numpy(host).cuda(), torch.from_numpy(nrec).cuda()
    syms = torch.full((B, cap + 5), 0xAA, dtype=torch.uint8, device="cuda")
    bits = torch.full((B, (cap + 5) * bps), 0xAA, dtype=torch.uint8, device="cuda")
    nsym = torch.zeros(B, dtype=torch.int32, device="cuda")
    tx.frame(d_rec.data_ptr(), host[0].size, max_rec, syms.data_ptr(), cap + 5, cap, d_nrec=d_nrec.data_ptr(), d_nsym=nsym.data_ptr(),
             d_bits=bits.data_ptr(), bits_stride=(cap + 5) * bps)
    torch.cuda.synchronize()
    syms, bits, nsym = syms.cpu().numpy(), bits.cpu().numpy(), nsym.cpu().numpy()
    pn, pk, uw, H = parse_code(code)
    assert (pn, pk) == (n, k)
    crc16 = oracle.OracleLdpc(oracle.parse_code_file(code), M).crc16
    frames = 0
    for s in range(B):
        want = np.concatenate([np.zeros(lead[s] * bps, dtype=np.uint8), sigutil.run_framer(["-m", str(M), "--packed", "--gap", str(gap[s] * bps), "-", "-"], recs[s].tobytes(), code)])
        assert nsym[s] * bps == want.size, (s, nsym[s], want.size)
        assert np.array_equal(bits[s, :want.size], want), (s, np.flatnonzero(bits[s, :want.size] != want)[:8])
        assert (bits[s, want.size:] == 0xAA).all() and (syms[s, nsym[s]:] == 0xAA).all()
        frames += check_frames(bits[s, :want.size], plans[s], recs[s], lead[s] * bps, gap[s] * bps, tx.preamble_syms * bps, n, k, uw, H, crc16)
        off = txref.carrier_mask(plans[s], lead[s], gap[s], tx.preamble_syms, tx.frame_syms)
        assert np.array_equal(syms[s, :nsym[s]], np.where(off, OFF, txref.bits_to_syms(want, M))), s
    return frames


@pytest.mark.gpu
@pytest.mark.parametrize("M", [2, 4])
@pytest.mark.parametrize("n,k", CODE_SHAPES)
def test_framer_on_other_code_shapes_against_the_tool_and_against_h(oracle, built_lib, tmp_path, n, k, M):
    assert (32 + n) % 2 == 0
    frames = framer_case(oracle, write_code(tmp_path, n, k), M, n, k, np.random.default_rng(1000 * M + n))
    assert frames > 30


def test_an_odd_frame_is_refused_for_four_fsk_at_create_and_by_the_cli(built_lib, tmp_path):
    """32 + n odd: half a symbol per frame with M = 4. The refusal comes before the device is looked for, so it is the same everywhere."""
    code = write_code(tmp_path, 137, 104)
    h = C.c_void_p()
    assert built_lib.pirip_hip_tx_create(code.encode(), 240000, 10000, 4, 1, -1, C.byref(h)) == UNSUPPORTED and not h.value
    p = subprocess.run([os.path.join(BIN, "fsk_ldpc_tx"), "--code", code, "-m", "4", "--testframes", "1", "240000", "10000", "10000", "10000", "/dev/zero", "-"],
                       capture_output=True)
    assert p.returncode == 2 and p.stdout == b"" and b"pirip_hip_tx_create" in p.stderr, (p.returncode, p.stderr)
    rc = built_lib.pirip_hip_tx_create(code.encode(), 240000, 10000, 2, 1, -1, C.byref(h))      # M = 2 is served (or there is no device)
    assert rc in (0, -3)
    if rc == 0:
        built_lib.pirip_hip_tx_destroy(h)


# ---------------------------------------------------------------- modulator at its stated limits

FS24 = 1 << 24
# (Fs, Rs, M, shift, first tones, symbols per stream, u8 amp). Tones: 0, +-1, +-(Fs/2 - 1), and j Rs +- 1, for which Ts f is just
# above / below a multiple of Fs; with shift = Rs +- small every symbol's tone stays next to such a multiple.
LIMIT_SHAPES = [
    (FS24, 1 << 14, 2, (1 << 14) + 3, [0, 1, -1, FS24 // 2 - 1, -(FS24 // 2 - 1), 5 * (1 << 14) + 1, 7 * (1 << 14) - 1, 1234567], 260, 32.0),
    (FS24, 1 << 21, 4, (1 << 21) - 1, [0, 1, -1, FS24 // 2 - 1, -(FS24 // 2 - 1), (1 << 21) + 1, 3 * (1 << 21) - 1, 7654321], 3000, 32.0),
    (90000, 10000, 2, 10001, [0, 1, -1, 44999, -44999, 20001, 29999, 12347], 3000, 32.0),
    (30000, 10000, 4, 9999, [0, 1, -1, 14999, -14999, 10001, 19999, 7001], 5000, 32.0),
    (FS24, FS24, 2, FS24 - 2, [0, 1, -1, FS24 // 2 - 1, -(FS24 // 2 - 1), 3, 9999991, 16777213], 20000, 32.0),
    (9600, 9600, 4, 2401, [0, 1, -1, 4799, -4799, 7, 1201, 2399], 20000, 32.0),
]
LIMIT_IDS = ["Fs%d-Ts%d-M%d" % (s[0], s[0] // s[1], s[2]) for s in LIMIT_SHAPES]


def limit_symbols(shape):
    Fs, Rs, M, shift, f1s, nsym, amp = shape
    rng = np.random.default_rng(Fs // Rs + M)
    host = rng.integers(0, M, (len(f1s), nsym)).astype(np.uint8)
    host[1, 40:75] = OFF
    host[2, :9] = OFF
    return host


def test_float64_formula_meets_few_rounding_ties_on_the_limit_tones():
    """tests below allow one u8 level of difference only within BOUND * amp of a tie and cap the share of such samples at 1e-3: a
    condition on the inputs. The float64 formula alone stays below a quarter of that cap on every (shape, first tone) used here."""
    for shape in LIMIT_SHAPES:
        Fs, Rs, M, shift, f1s, nsym, amp = shape
        host = limit_symbols(shape)
        for s, f1 in enumerate(f1s):
            _, v = txref.quantise(txref.mod_f64(host[s], f1, shift, Fs, Fs // Rs), amp)
            share = float(np.mean(txref.near_tie(v, amp)))
            assert share < 1e-3 / 4, (Fs, Rs, M, f1, share)


def modulate_rows(tx, d_syms, nsym, fmt, blocks=None, byte_offset=0, pad=0, **kw):
    """-> numpy [B, nsym * Ts, 2]; rows start byte_offset into the buffer and are pad bytes apart beyond their length; the buffer around
    them must keep its fill"""
    import torch
    import pirip_amd
    B, Ts = d_syms.shape[0], tx.Ts
    bs = 2 if fmt == pirip_amd.IN_CU8_FSKDEMOD else 8
    row = nsym * Ts * bs
    buf = torch.full((byte_offset + B * (row + pad) + 64,), 0xCD, dtype=torch.uint8, device="cuda")
    base = buf.data_ptr() + byte_offset
    at = 0
    for n in (blocks or [nsym]):
        tx.modulate(d_syms.data_ptr() + at, d_syms.shape[1], n, base + at * Ts * bs, row + pad, out_format=fmt, **kw)
        at += n
    assert at == nsym
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert (h[:byte_offset] == 0xCD).all() and (h[byte_offset + B * (row + pad):] == 0xCD).all()
    body = h[byte_offset:byte_offset + B * (row + pad)].reshape(B, row + pad)
    assert (body[:, row:] == 0xCD).all()
    o = np.ascontiguousarray(body[:, :row])
    return o.reshape(B, -1, 2) if bs == 2 else o.view(np.float32).reshape(B, -1, 2)


def check_against_formula(cf, u8, sy, f1, shift, Fs, Ts, amp, tag):
    """one stream: cf32 within BOUND of the float64 formula, u8 equal to its quantiser except within BOUND * amp of a tie
    -> (largest cf32 error, samples near a tie, samples)"""
    y = txref.mod_f64(sy, f1, shift, Fs, Ts)
    err = max(float(np.max(np.abs(cf[:, 0] - y.real))), float(np.max(np.abs(cf[:, 1] - y.imag))))
    assert err <= txref.BOUND, (tag, err)
    off = np.repeat(sy == OFF, Ts)
    assert not cf[off].any() and (u8[off] == 127).all(), tag
    q, v = txref.quantise(y, amp)
    diff = np.abs(u8.astype(np.int64) - q)
    tie = txref.near_tie(v, amp)
    assert diff.max() <= 1 and not diff[~tie].any(), (tag, int(diff.max()), int(np.count_nonzero(diff[~tie])))
    return err, int(np.count_nonzero(tie)), tie.size


@pytest.mark.gpu
@pytest.mark.parametrize("shape", LIMIT_SHAPES, ids=LIMIT_IDS)
def test_modulator_at_its_stated_limits(built_lib, shape, tmp_path):
    import torch
    import pirip_amd
    Fs, Rs, M, shift, f1s, nsym, amp = shape
    Ts, B = Fs // Rs, len(f1s)
    host = limit_symbols(shape)
    tx = pirip_amd.HipTx(write_code(tmp_path, 136, 104), Fs, Rs, M, nstreams=B, f1=f1s, shift=shift)
    d = torch.from_numpy(host).cuda()
    cf = modulate_rows(tx, d, nsym, pirip_amd.IN_CF32)
    tx.reset()
    u8 = modulate_rows(tx, d, nsym, pirip_amd.IN_CU8_FSKDEMOD, amp=amp)
    tx.reset()
    blocks = [1, 2, 5, 63, 64, 65, nsym - 200]
    cf_parts = modulate_rows(tx, d, nsym, pirip_amd.IN_CF32, blocks=blocks)
    tx.reset()
    u8_parts = modulate_rows(tx, d, nsym, pirip_amd.IN_CU8_FSKDEMOD, blocks=blocks, amp=amp)
    assert np.array_equal(cf.view(np.uint32), cf_parts.view(np.uint32)) and np.array_equal(u8, u8_parts)
    worst = ties = total = 0
    for s in range(B):
        err, t, n = check_against_formula(cf[s], u8[s], host[s], f1s[s], shift, Fs, Ts, amp, (Fs, Rs, f1s[s]))
        worst = max(worst, err); ties += t; total += n
    print(f"Fs {Fs} Ts {Ts} M {M}: cf32 largest component error {worst:.3e} (bound {txref.BOUND:.3e}); {ties} of {total} samples within the bound of a tie")
    assert ties <= 1e-3 * total


@pytest.mark.gpu
@pytest.mark.parametrize("Ts", [24, 9])
def test_rows_aligned_to_the_sample_only(built_lib, tmp_path, Ts):
    """u8 rows that start 2 bytes and cf32 rows that start 8 bytes off a 16-byte boundary, with strides that keep every row there (and
    move it): the per-sample store path, bytes equal to the aligned call's, nothing written around the rows"""
    import torch
    import pirip_amd
    Fs, Rs, M, f1s, shift = Ts * 10000, 10000, 2, [10037, 20011, 7001, -30000 + 41, 12345], 10000
    nsym = 333
    rng = np.random.default_rng(Ts)
    host = rng.integers(0, M, (len(f1s), nsym)).astype(np.uint8)
    host[3, 100:140] = OFF
    d = torch.from_numpy(host).cuda()
    tx = pirip_amd.HipTx(write_code(tmp_path, 136, 104), Fs, Rs, M, nstreams=len(f1s), f1=f1s, shift=shift)
    for fmt, unit in ((pirip_amd.IN_CU8_FSKDEMOD, 2), (pirip_amd.IN_CF32, 8)):
        tx.reset()
        ref = modulate_rows(tx, d, nsym, fmt, amp=32.0, sigma=0.3, seed=9)
        for off, pad in ((unit, 0), (unit, unit), (0, unit), (16 - unit, 16), (0, 3 * unit)):
            tx.reset()
            got = modulate_rows(tx, d, nsym, fmt, byte_offset=off, pad=pad, amp=32.0, sigma=0.3, seed=9, blocks=[7, 1, nsym - 8])
            assert np.array_equal(got.view(np.uint8), ref.view(np.uint8)), (fmt, off, pad)
    tx.reset()
    cf = modulate_rows(tx, d, nsym, pirip_amd.IN_CF32, byte_offset=8, pad=8)
    tx.reset()
    u8 = modulate_rows(tx, d, nsym, pirip_amd.IN_CU8_FSKDEMOD, byte_offset=2, pad=2, amp=32.0)
    for s in range(len(f1s)):
        check_against_formula(cf[s], u8[s], host[s], f1s[s], shift, Fs, Ts, 32.0, (Ts, s))


@pytest.mark.gpu
def test_sixty_six_thousand_streams_each_row_against_the_formula(built_lib, tmp_path):
    """more streams than one grid dimension holds: the stream index is blockIdx.y + 65535 blockIdx.z. Every stream has its own tone and
    symbols, so a row written for another stream, or not written, fails."""
    import torch
    import pirip_amd
    Fs, Rs, M, shift, B, nsym = 240000, 10000, 4, 10000, 66000, 4
    Ts = Fs // Rs
    rng = np.random.default_rng(66)
    host = rng.integers(0, M, (B, nsym)).astype(np.uint8)
    f1 = (1000 + 7 * np.arange(B)) % 50000 + 13
    tx = pirip_amd.HipTx(write_code(tmp_path, 136, 104), Fs, Rs, M, nstreams=B, f1=f1, shift=shift)
    d = torch.from_numpy(host).cuda()
    cf = modulate_rows(tx, d, nsym, pirip_amd.IN_CF32)
    f = (f1[:, None] + host.astype(np.int64) * shift) % Fs
    A = np.concatenate([np.zeros((B, 1), dtype=np.int64), np.cumsum((f * Ts) % Fs, axis=1)], axis=1) % Fs
    p = (A[:, :-1, None] + np.arange(1, Ts + 1)[None, None, :] * f[:, :, None]) % Fs
    y = 2.0 * np.exp(2j * np.pi * p.reshape(B, -1).astype(np.float64) / Fs)
    assert np.array_equal(y[5], txref.mod_f64(host[5], int(f1[5]), shift, Fs, Ts))       # the vectorised formula is txref's
    err = np.maximum(np.abs(cf[:, :, 0] - y.real), np.abs(cf[:, :, 1] - y.imag)).max(axis=1)
    print(f"{B} streams: cf32 largest component error {err.max():.3e} (bound {txref.BOUND:.3e})")
    assert (err <= txref.BOUND).all(), np.flatnonzero(err > txref.BOUND)[:8]
