"""include/pirip_hip.h section L (test-frame counter) without a GPU: the library, the header and the binding are there; the numpy reference
the GPU tests hold the kernel to (tests/tbitsref.py) equals the CPU counter; and the inputs of tests/test_testbits.py reach, on the
reference alone, the cases they are meant for -- so that the GPU tests cannot pass on inputs that count nothing."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import tbitsref
import tbitsshapes as ts

TBITS_SYMBOLS = ("pirip_hip_tbits_create", "pirip_hip_tbits_destroy", "pirip_hip_tbits_push", "pirip_hip_tbits_get_counters",
                 "pirip_hip_tbits_counters_device", "pirip_hip_tbits_reset", "pirip_hip_tbits_testframe_payload", "pirip_hip_tbits_set_payload",
                 "pirip_hip_tbits_push_records", "pirip_hip_tbits_get_record_counters")
NO_DEVICE, UNSUPPORTED, BAD_ARG = -3, -6, -1


def test_library_header_and_binding(built_lib):
    import pirip_amd
    out = subprocess.run(["nm", "-D", "--defined-only", pirip_amd.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    hdr = open(os.path.join(tbitsref.ROOT, "include", "pirip_hip.h")).read()
    assert "section L" in hdr
    for n in TBITS_SYMBOLS:
        assert n in exported and hasattr(built_lib, n) and n + "(" in hdr, n
    sig = inspect.signature(pirip_amd.HipTestBits)
    for k, v in (("framesize", 100), ("valid_thresh", 0.1), ("frame", None), ("device", -1)):
        assert sig.parameters[k].default == v, k
    push = inspect.signature(pirip_amd.HipTestBits.push).parameters
    assert list(push)[:2] == ["self", "bits"] and push["nframes"].default is None and push["packed"].default is False and push["stream"].default is None
    for m in ("push", "push_records", "counters", "record_counters", "reset", "set_payload", "close"):
        assert callable(getattr(pirip_amd.HipTestBits, m)), m


def test_create_argument_checks_and_no_device(built_lib):
    import pirip_amd
    h = C.c_void_p()
    frame = np.zeros(4097, dtype=np.uint8)
    create = built_lib.pirip_hip_tbits_create
    assert create(0, 0.1, None, 1, -1, C.byref(h)) == BAD_ARG
    assert create(100, 0.1, None, 0, -1, C.byref(h)) == BAD_ARG
    assert create(100, 0.1, None, 1, -1, None) == BAD_ARG
    frame[3] = 2
    assert create(8, 0.1, frame.ctypes.data, 1, -1, C.byref(h)) == BAD_ARG            # a frame byte that is no bit
    frame[3] = 1
    assert create(4097, 0.1, frame.ctypes.data, 1, -1, C.byref(h)) == UNSUPPORTED
    if pirip_amd.device_count() == 0:
        assert create(100, 0.1, None, 4, -1, C.byref(h)) == NO_DEVICE and not h.value
        with pytest.raises(pirip_amd.PiripError, match=r"\(-3\)"):
            pirip_amd.HipTestBits(nstreams=4)


def test_testframe_payload_is_what_the_framer_packs(built_lib):
    """pirip_amd.testframe_payload(k) against fsk_ldpc_framer --testframes: the frame's data bits behind the 32-bit unique word, packed MSB
    first; bytes 0 and 1 carry source / sequence and the last two the CRC, which is why the tally leaves them out"""
    import pirip_amd
    p = subprocess.run([os.path.join(tbitsref.BIN, "fsk_ldpc_framer"), "--code", pirip_amd.STANDIN_CODE, "--testframes", "1", "/dev/zero", "-"],
                       capture_output=True, check=True)
    bits = np.frombuffer(p.stdout, dtype=np.uint8)
    k = 256
    assert len(bits) > 32 + 512                                                         # preamble, then one frame of 32 + n bits
    i = len(bits) - (32 + 512)
    data = np.packbits(bits[i + 32:i + 32 + k])
    want = pirip_amd.testframe_payload(k)
    assert want.shape == (k // 8,) and want.dtype == np.uint8
    assert np.array_equal(data[:k // 8 - 2], want[:k // 8 - 2])                         # (without --source / --seq bytes 0, 1 are the payload's own)
    assert 0 < int(np.unpackbits(want).sum()) < k
    assert built_lib.pirip_hip_tbits_testframe_payload(12, want.ctypes.data) == BAD_ARG


def test_reference_equals_the_cpu_counter(oracle, built_lib):
    rng = np.random.default_rng(5)
    bits = oracle.get_test_bits(1000)
    bits[rng.choice(1000, size=40, replace=False)] ^= 1
    for b in (bits, bits[9:], bits[37:537], rng.integers(0, 2, 700).astype(np.uint8)):
        for thr in (0.1, 0.07, 0.3):
            tbitsref.assert_matches_cpu(oracle, b, 100, thr)
    tbitsref.assert_matches_cpu(oracle, oracle.get_test_bits(300, 24), 24, 0.2)


def test_zero_prefix_makes_a_packet(oracle, built_lib):
    """the default frame from its 10th bit on: the window that ends with the frame's last bit starts with 9 of the counter's zeros,
    at most 9 errors, below the limit 10"""
    f = ts.default_frame()
    got = tbitsref.assert_matches_cpu(oracle, f[9:])
    assert got["packets"] == 1 and got["errors"] == int(f[:9].sum()) <= 9
    want = ts.syn_want(tuple(ts.SYN["nframes"]))
    assert want["packets"][2] >= 1 and ts.SYN["nframes"][2] * ts.SYN["row_bits"] == 100 - 9 + 9   # stream 2 of the GPU test: 100 bits, offset 9
    assert np.array_equal(ts.syn_rows()[2].reshape(-1)[:91], f[9:])


def test_the_limit_is_the_float_expression(oracle, built_lib):
    """errs exactly at the limit. The limit is PutBits' float product, not an integer worked out by hand: 0.1f * 100 is 10.0f (9 valid, 10
    not); 0.09f * 300 is 27.000002f, so 27 errors ARE valid where 0.09 * 300 = 27 says they are not. 0.07f * 100: the issue that asked for
    this counter expected the product above 7 (it is, in double: 7.00000003) and 7 errors valid -- in float, which is what PutBits, the
    oracle and fsk_put_test_bits compute, it rounds to exactly 7.0f and 7 errors are NOT valid; the CPU counter decides, and all agree."""
    for F, thr, e, valid in ts.LIMIT_CASES:
        got = tbitsref.assert_matches_cpu(oracle, ts.limit_bits(F, e), F, thr)
        assert got["packets"] == (1 if valid else 0) and got["errors"] == (e if valid else 0), (F, thr, e)
    assert float(tbitsref.limit(100, 0.1)) == 10.0 and float(tbitsref.limit(100, 0.07)) == 7.0 < float(np.float32(0.07)) * 100
    assert float(tbitsref.limit(300, 0.09)) > 27.0


def test_overlapping_windows_all_count():
    frame, thr = ts.sweep_frame(8), ts.sweep_thresh(8)
    assert (frame == 1).all()
    got = tbitsref.count(np.ones(20, dtype=np.uint8), frame, thr)
    # position j < 7 still has 7 - j zeros of the prefix in its window: fewer than 0.5 * 8 = 4 errors from position 4 on, 16 positions
    assert got["packets"] == 16 and got["bits"] == 16 * 8 and got["errors"] == 3 + 2 + 1
    assert ts.sweep_want(8)["packets"].min() > ts.sweep_bits(8).shape[1] // 8 // 2


def test_call_boundaries():
    f = ts.default_frame()
    rng = np.random.default_rng(7)
    bits = tbitsref.framed_bits(f, [0, 3, 9, 10, 0, 2], 23, rng)
    whole = tbitsref.count(bits, f)
    assert whole["packets"] >= 4
    for cuts in ([50], [0, 50, 50, 577], [1, 2, 3, 99, 100, 101, 350], list(range(50, 577, 50))):
        c = tbitsref.Counter(f)
        for a, b in zip([0] + cuts, cuts + [bits.size]):
            c.push(bits[a:b])                    # (calls of 0 bits, and calls shorter than F - 1 = 99 bits among them)
        assert c.counters() == whole, cuts
    # one call of one 50-bit row: fewer bits than the history holds
    c = tbitsref.Counter(f)
    c.push(bits[:50])
    assert c.hist.size == 99 and np.array_equal(c.hist[-50:], bits[:50]) and not c.hist[:49].any()


def test_packed_rows_ignore_their_pad_bits():
    rows = ts.syn_rows()
    p0, p1 = tbitsref.pack_rows(rows, 0), tbitsref.pack_rows(rows, 1)
    assert p0.shape == (5, 9, 7) and not np.array_equal(p0, p1)
    assert np.array_equal(np.unpackbits(p1, axis=-1)[..., :50], rows) and (np.unpackbits(p1, axis=-1)[..., 50:] == 1).all()


def test_synthetic_rows_reach_both_sides_of_the_limit():
    full = ts.syn_want((9,) * 5)
    sent = sum(len([e for e in errs[:4]]) for errs in ts.SYN_ERRORS)
    assert 0 < full["packets"].sum() < sent                    # some frames count, some do not
    assert {9, 10, 12} <= {e for errs in ts.SYN_ERRORS for e in errs}
    want = ts.syn_want(tuple(ts.SYN["nframes"]))
    assert want["pushed"].tolist() == [0, 50, 100, 350, 450] and want["packets"][0] == 0 and want["packets"][4] >= 2
    assert all(np.array_equal(ts.syn_want((-3, 1, 2, 7, 12))[k], want[k]) for k in want)       # the reference clamps as the device must
    assert sum(ts.SYN_SPLITS) == ts.SYN["max_frames"] and 0 in ts.SYN_SPLITS


@pytest.mark.parametrize("F", ts.SWEEP_F)
def test_sweep_inputs_count_valid_and_invalid_frames(F):
    want, b = ts.sweep_want(F), ts.sweep_bits(F)
    assert b.shape[1] % ts.SWEEP_UNIT == 0 and all(b.shape[1] % rb == 0 for rb in ts.SWEEP_ROW_BITS)
    frames = b.shape[1] // F
    assert (want["packets"] >= 1).all() and (want["pushed"] == b.shape[1]).all()
    if F > 8:
        assert (want["packets"] < frames).all() and (want["errors"] > 0).all()      # the frames one error over the limit do not count


def test_grid_inputs_and_record_inputs():
    assert (ts.want_of("many")["packets"] > 0).sum() > 50 and (ts.want_of("many")["packets"] == 0).sum() > 20
    assert ts.want_of("long")["packets"][0] > 1000 and ts.want_of("long")["pushed"][0] == 150000 > 2048 * 70
    assert (ts.want_of("calls200")["packets"] > 50).all()
    want = np.arange(ts.REC_DB, dtype=np.uint8)
    st, pl, info, nc = ts.crafted_records(want)
    t = tbitsref.record_tally(st, pl, info, nc, want)
    assert (t["frames"] > 0).all() and (t["frames"] < np.clip(nc, 0, 6)).any() and t["errors"].sum() > 0
    assert (t["frames_in_error"] < t["frames"]).any() and t["crc_ok"].sum() > 0
    # errors in bytes 0, 1 and data_bytes - 2 are not compared: only the flips in bytes 2, data_bytes - 3 and 10 .. 13 can count
    assert t["errors"].sum() <= 3 * (3 + 4) + 16
