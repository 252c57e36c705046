"""include/pirip_hip.h section R, parity fragments, without a GPU: the host model tests/pktfecref.py that tests/test_packet_fec.py holds
the device to. The arithmetic of pirip_amd/csrc/gf256_device.hpp is the model's, byte for byte; every loss pattern the code promises to
survive decodes in the model and one loss more never delivers; FEC and plain handles hear each other as the header says; the records
are frames the framer accepts; the tables reach every corner they claim; the two structures have the header's layout."""
import ctypes as C
import itertools
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

import pktfecref as fr
import pktref
import sigutil

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KB, CAP = pktref.KB, pktref.cap(pktref.KB)
PRE, FRAME, GAP = 50, 544, 7
B = pktref.SYNC | pktref.BITS


# ---------------------------------------------------------------- the arithmetic

def test_the_models_field_is_a_field():
    assert fr.gf_mul(2, 0x80) == 0x1D and fr.gf_mul(0x53, 1) == 0x53 and fr.gf_mul(0, 77) == 0
    assert all(fr.MUL[a, fr.INV[a]] == 1 for a in range(1, 256)) and fr.INV[0] == 0
    assert np.array_equal(fr.MUL, fr.MUL.T) and sorted(fr.MUL[3, 1:].tolist()) == list(range(1, 256))
    x, seen = 1, set()
    for _ in range(255):                                                      # x generates the multiplicative group: 0x11D is primitive
        seen.add(x)
        x = fr.gf_mul(x, 2)
    assert len(seen) == 255 and x == 1
    assert [fr.r_of(k, 16, 20) for k in (1, 5, 6, 80, 81, 100)] == [1, 1, 2, 16, 16, 16] and fr.r_of(4, 3, 75) == 3 and fr.r_of(5, 16, 40) == 2


@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_gf256_device_hpp_is_the_models_arithmetic(tmp_path, flags):
    exe = str(tmp_path / "pkt_gf_check")
    subprocess.run(["g++", "-std=c++17"] + flags + ["-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", os.path.join(ROOT, "pirip_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tests", "cprog", "pkt_gf_check.cpp")], check=True)
    out = np.frombuffer(subprocess.run([exe], capture_output=True, check=True).stdout, np.uint8)
    assert out.size == 65536 * 5 + 256 + 16 * 84 + 300 + 256 * 64
    mul, out = out[:65536].reshape(256, 256), out[65536:]
    assert np.array_equal(mul, fr.MUL)
    packed, out = out[:65536 * 4].reshape(256, 256, 4), out[65536 * 4:]
    a = np.arange(256)
    words = np.stack([a, (a + 85) & 255, (a + 170) & 255, 255 - a], axis=1)                     # [a, e]
    assert np.array_equal(packed, fr.MUL[words[:, None, :], a[None, :, None]])
    inv, out = out[:256], out[256:]
    assert np.array_equal(inv, fr.INV)
    cm, out = out[:16 * 84].reshape(16, 84), out[16 * 84:]
    assert np.array_equal(cm, fr.cauchy(16, 84)) and cm.all()
    rs, out = out[:300].reshape(100, 3), out[300:]
    assert rs.tolist() == [[fr.r_of(k, 16, 20), fr.r_of(k, 3, 50), fr.r_of(k, 1, 100)] for k in range(1, 101)]
    assert out.reshape(256, 64).tolist() == [[fr.pad(i, 37 * n) for n in range(64)] for i in range(256)]


# ---------------------------------------------------------------- loss patterns

def _one_packet(rec, lose, shape, order=None):
    """the model over a burst's frames but those at `lose`, in `order`"""
    keep = [i for i in range(rec.shape[0] - 1) if i not in lose]
    if order is not None:
        keep = [keep[i] for i in order(len(keep))]
    return fr.run_rows([[fr.rows_of([("frames", rec[keep], B)])]], shape, filt=None, address=None)


@pytest.mark.parametrize("R,k,r,pct", [(3, 1, 1, 50), (3, 4, 3, 75), (16, 5, 2, 40)])
def test_every_pattern_of_up_to_r_losses_decodes_and_one_more_never_delivers(R, k, r, pct):
    shape = (k, R, pct)
    packet = np.random.default_rng(k).integers(0, 256, pktref.max_packet(KB, k)).astype(np.uint8).tobytes()
    rec = fr.segment_fec(packet, 2, 7, 5, KB, k, R, pct)
    assert rec.shape[0] == k + r + 1
    n = 0
    for nl in range(r + 2):
        for lose in itertools.combinations(range(k + r), nl):
            m = _one_packet(rec, lose, shape)
            lost_data = sum(1 for i in lose if i < k)
            if nl <= r:
                assert m.packets(0)[1] == [packet], lose
                assert (m.c["recovered"][0], m.c["repaired"][0]) == (int(lost_data > 0), lost_data), lose
                assert m.c["surplus"][0] == r - nl
            else:
                assert m.c["delivered"][0] == 0 and not m.c["crc_fail"].any() and m.st[0]["phase"] == (nl < k + r), lose
            n += 1
    assert n == sum(len(list(itertools.combinations(range(k + r), nl))) for nl in range(r + 2))


def test_200_random_patterns_of_16_losses_of_100_fragments_decode():
    shape = fr.SHAPES["wide"]
    rng = np.random.default_rng(84)
    packet = rng.integers(0, 256, pktref.max_packet(KB, 84)).astype(np.uint8).tobytes()
    rec = fr.segment_fec(packet, 2, 7, 200, KB, *shape)
    assert rec.shape[0] == 101 and fr.r_of(84, 16, 100) == 16
    ms = set()
    for _ in range(200):
        lose = rng.choice(100, 16, replace=False).tolist()
        m = _one_packet(rec, lose, shape, order=rng.permutation)
        assert m.packets(0)[1] == [packet], lose
        ms.add(int(m.c["repaired"][0]))
    m = _one_packet(rec, list(range(84, 100)), shape)                         # every parity fragment lost: nothing to decode
    assert m.packets(0)[1] == [packet] and m.c["repaired"][0] == 0
    m = _one_packet(rec, list(range(16)), shape)                              # sixteen data fragments lost: the largest system
    assert m.packets(0)[1] == [packet] and m.c["repaired"][0] == 16 and m.ev["max_m"] == 16
    assert len(ms) > 3 and _one_packet(rec, list(range(17)), shape).c["delivered"][0] == 0


# ---------------------------------------------------------------- interoperation and the wire format

def test_fec_and_plain_handles_hear_each_other():
    sh = fr.SHAPES["small"]
    packet = bytes(range(70))
    rec = fr.segment_fec(packet, 2, 7, 3, KB, *sh)
    k, r = 4, 2
    assert rec.shape[0] == k + r + 1
    plain = pktref.run_rows([[pktref.rows_of([("frames", rec[:-1], B)])]], filt=None, address=None)
    assert plain.packets(0)[1] == [packet] and plain.c["malformed"][0] == r and plain.c["delivered"][0] == 1
    assert not plain.c["orphan"].any() and not plain.c["incomplete"].any() and not plain.c["crc_fail"].any()
    lossy = pktref.run_rows([[pktref.rows_of([("frames", rec[[0, 1, 3, 4, 5]], B)])]], filt=None, address=None)
    assert lossy.c["delivered"][0] == 0 and lossy.c["orphan"][0] == 1                            # what the parity is for
    old = pktref.segment(packet, 2, 7, 3, KB, sh[0])
    m = fr.run_rows([[fr.rows_of([("frames", old[:-1], B)])]], sh, filt=None, address=None)
    assert m.packets(0)[1] == [packet] and not m.c["recovered"].any() and not m.c["surplus"].any() and not m.c["malformed"].any()
    # the data fragments differ from a plain sender's in the padding alone
    assert np.array_equal(rec[:k, :7], old[:k, :7]) and np.array_equal(rec[:k - 1], old[:k - 1])
    ll = rec[k - 1, 6]
    assert np.array_equal(rec[k - 1, :7 + ll], old[k - 1, :7 + ll]) and not old[k - 1, 7 + ll:].any()


@pytest.mark.parametrize("L", [1, CAP - 4, CAP - 3, CAP, 116])
def test_a_packets_records_are_frames_the_framer_accepts(built_lib, L):
    mf, R, pct = fr.SHAPES["small"]
    rng = np.random.default_rng(L)
    packet = rng.integers(0, 256, L).astype(np.uint8).tobytes()
    pid = 300 + L
    rec = fr.segment_fec(packet, 0x21, 0x42, pid, KB, mf, R, pct)
    k = {1: 1, CAP - 4: 1, CAP - 3: 2, CAP: 2, 116: 5}[L]
    r = {1: 1, 2: 1, 5: 3}[k]
    n = k + r
    last = L + 4 - (k - 1) * CAP
    assert rec.shape == (n + 1, 1 + KB) and rec[:, 0].tolist() == [1] + [0] * (n - 1) + [2] and not rec[n, 1:].any()
    assert rec[:n, 1].tolist() == [0x21] * n and rec[:n, 2].tolist() == [0x42] * n and rec[:n, 3].tolist() == [pid & 0xFF] * n
    assert rec[:n, 4].tolist() == list(range(n)) and rec[:n, 5].tolist() == [k] * n
    assert rec[:n, 6].tolist() == [CAP] * (k - 1) + [last] * (1 + r) and not rec[:n, KB - 1:].any()          # the parity's len is the last data fragment's
    body = rec[:k, 7:7 + CAP].tobytes()
    assert body[:L + 4] == packet + zlib.crc32(packet).to_bytes(4, "little")
    assert list(body[L + 4:]) == [fr.pad(pid & 0xFF, q) for q in range(L + 4, k * CAP)]
    if k * CAP - L - 4 >= 8:
        assert len(set(body[L + 4:])) > 2                                    # whitened: no run of equal bytes
    for j in range(r):
        want = np.zeros(CAP, np.uint8)
        for i in range(k):
            want ^= np.array([fr.gf_mul(fr.gf_inv(j ^ (R + i)), int(x)) for x in rec[i, 7:7 + CAP]], np.uint8)
        assert np.array_equal(rec[k + j, 7:7 + CAP], want), j
    bits = sigutil.run_framer(["-m", "2", "--packed", "--gap", str(GAP), "-", "-"], rec.tobytes())
    assert bits.size == PRE + n * FRAME + GAP
    for f in range(n):
        data = np.packbits(bits[PRE + f * FRAME + 32:PRE + f * FRAME + 32 + 8 * KB])
        assert np.array_equal(data[:KB - 2], rec[f, 1:KB - 1]), f


def test_a_length_outside_the_range_is_refused():
    for L in (0, 117):
        with pytest.raises(ValueError):
            fr.segment_fec(bytes(L), 1, 2, 3, KB, *fr.SHAPES["small"])
    assert fr.segment_fec(bytes(116), 1, 2, 3, KB, *fr.SHAPES["small"]).shape[0] == 5 + 3 + 1


# ---------------------------------------------------------------- reassembly

def _same_packets(a, b, but_call_and_row=False):
    (ea, ba), (eb, bb) = a, b
    same = pktref.same_but_call_and_row(ea, eb) if but_call_and_row else ea.tobytes() == eb.tobytes()
    return same and ba == bb


def test_the_tables_raise_every_counter_and_reach_every_corner():
    sh = fr.SHAPES["small"]
    chans = fr.streams("small")
    m = fr.run_rows(pktref.cut(chans, 1, 7), sh)
    ev = m.ev
    for k in pktref.RX_COUNTERS + fr.FEC_COUNTERS:
        assert (m.c[k][0] > 0) == (k != "orphan"), (k, m.c[k])
    assert not m.c["orphan"].any()
    assert ev["bad_headers"] == {0, 1, 2, 3, 4} and ev["lastlen_conflict"] > 0
    assert ev["lost_last"] > 0 and ev["lost_first"] > 0 and ev["parity_first"] > 0
    assert ev["surplus_after_delivery"] > 0 and ev["surplus_after_crc_fail"] > 0 and ev["crc_fail_decoded"] > 0 and ev["crc_fail_plain"] > 0
    assert ev["no_sync_inside"] > 0 and ev["bits_without_sync"] > 0 and ev["sync_only_inside"] > 0 and ev["foreign_inside"] > 0
    assert ev["other_src"] > 0 and {254, 255, 0} <= ev["ids"] and ev["cut_inside_packet"] > 0 and ev["wraps"] > 0 and ev["short_body"] > 0
    assert ev["plain_burst"] > 0 and ev["max_m"] >= 2
    # channel 0 by hand, in one call
    m1 = fr.run_rows(pktref.one_call(chans), sh, ring_entries=100)
    ent, data = m1.packets(0)
    assert ent["length"][:9].tolist() == [1, CAP - 4, CAP - 3, CAP, 116, 60, 60, 61, 62] and ent["nfrag"][:9].tolist() == [1, 1, 2, 2, 5, 3, 3, 3, 3]
    assert ent["id"][:12].tolist() == [0, 1, 2, 3, 4, 20, 21, 22, 23, 254, 255, 0] and ent["dst"][7] == 0xFF
    assert ent["seq"].tolist() == list(range(len(ent))) and all(len(b) == n for b, n in zip(data, ent["length"]))
    assert (ent["src"] != fr.FILT).all() and {5, 6, 7} <= set(ent["src"].tolist()) and 41 in ent["id"].tolist() and 42 in ent["id"].tolist()
    assert m1.c["recovered"][0] >= 8 and m1.c["repaired"][0] > m1.c["recovered"][0] and m1.c["duplicate"][0] == 1
    # the two senders interleaved: each throws the other out, and each packet is still put together from what is left of it
    assert m1.c["incomplete"][0] == 2
    # channel 1: bursts with r + 1 losses are never delivered and are closed by the next one; channel 2: nothing lost
    assert m.c["incomplete"][1] > 0 and m.c["recovered"][1] > 0 and m.c["crc_fail"][1] > 0 and m.c["duplicate"][1] > 0
    assert m.c["delivered"][2] == 6 and not m.c["recovered"][2] and m.c["surplus"][2] >= 6
    # the ring keeps the newest
    ent4, data4 = m.packets(0)
    assert len(ent4) == fr.RING and m.c["lost"][0] == m.c["delivered"][0] - fr.RING and data4 == data[-fr.RING:]


@pytest.mark.parametrize("name", ["one", "wide"])
def test_the_other_shapes_tables(name):
    sh = fr.SHAPES[name]
    chans = fr.streams(name)
    m = fr.run_rows(pktref.one_call(chans), sh, ring_entries=100)
    if name == "one":
        assert m.c["delivered"][0] == 12 and m.c["recovered"][0] == 8 and m.c["repaired"][0] == 8 and m.c["surplus"][0] == 4
        assert all(len(b) == 1 for b in m.packets(0)[1]) and m.ev["lost_last"] >= 8 and m.ev["parity_first"] >= 8
    else:
        assert fr.r_of(84, 16, 100) == 16
        assert m.c["delivered"][0] == 3 and m.c["recovered"][0] == 3 and m.c["repaired"][0] >= 12 + 2 and m.ev["max_m"] >= 12
        assert [len(b) for b in m.packets(0)[1]] == [2012, 2011, 2010] and not m.c["surplus"][0]


@pytest.mark.parametrize("name,how", [("small", "between_fragments"), ("small", "seed2"), ("small", "one_per_call"), ("one", "between_fragments"),
                                      ("one", "seed3"), ("wide", "between_fragments"), ("wide", "seed2")])
def test_the_same_rows_cut_into_other_calls_give_the_same_ring(name, how):
    sh = fr.SHAPES[name]
    chans = fr.streams(name)
    ref = fr.run_rows(pktref.one_call(chans), sh)
    if how == "between_fragments":
        calls = fr.between_fragments(chans)
        assert tuple(calls[0][0][1][-1, [0, 2, 4]]) == tuple(calls[1][0][1][0, [0, 2, 4]])
    elif how == "one_per_call":
        n = max(len(st) for st, _ in chans)
        calls = [[(st[i:i + 1], pl[i:i + 1]) for st, pl in chans] for i in range(n)]
    else:
        calls = pktref.cut(chans, int(how[-1]), 12)
    m = fr.run_rows(calls, sh)
    assert name == "one" or m.ev["cut_inside_packet"] > 0
    for c in range(len(chans)):
        assert _same_packets(m.packets(c), ref.packets(c), but_call_and_row=True), c
    assert all(np.array_equal(m.c[k], ref.c[k]) for k in ref.c)


def test_one_call_of_4096_rows():
    big = fr.big_call()
    assert [len(st) for st, _ in big[0]] == [4096, 4095, 1]
    m = fr.run_rows(big, fr.SHAPES["small"], ring_entries=5000)
    assert m.c["delivered"][0] > 500 and m.c["recovered"][0] > 100 and m.c["crc_fail"][0] > 0 and m.c["incomplete"][0] > 0 and m.ev["max_rows"] == 4096


# ---------------------------------------------------------------- the binding and the library, without a device

def test_structures_have_the_headers_layout(tmp_path):
    """pirip_pkt_fec_config / pirip_pkt_fec_info: the ctypes twins against what gcc makes of the header"""
    from pirip_amd import binding
    twins = {"pirip_pkt_fec_config": binding.PktFecConfig, "pirip_pkt_fec_info": binding.PktFecInfo}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pirip_hip.h"', "int main(void) {"]
    for name, T in twins.items():
        lines.append(f'    printf("S {name} %zu\\n", sizeof({name}));')
        lines += [f'    printf("F {name} {f} %zu %zu\\n", offsetof({name}, {f}), sizeof((({name} *)0)->{f}));' for f, *_ in T._fields_]
    lines += ["    return 0;", "}"]
    (tmp_path / "l.c").write_text("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "l"), str(tmp_path / "l.c")], check=True)
    size, fields = {}, {n: [] for n in twins}
    for ln in subprocess.run([str(tmp_path / "l")], check=True, capture_output=True, text=True).stdout.split("\n"):
        w = ln.split()
        if w and w[0] == "S":
            size[w[1]] = int(w[2])
        elif w:
            fields[w[1]].append((w[2], int(w[3]), int(w[4])))
    for name, T in twins.items():
        assert C.sizeof(T) == size[name]
        assert [(n, getattr(T, n).offset, getattr(T, n).size) for n, *_ in T._fields_] == fields[name]
    # the header's field lists are the twins' (a field added to the header alone would pass the offsets above)
    src = open(os.path.join(ROOT, "include", "pirip_hip.h")).read()
    for name, T in twins.items():
        body = re.sub(r"/\*.*?\*/", " ", src.split("struct %s {" % name)[1].split("};")[0], flags=re.S)
        names = [d.strip().split()[-1] for decl in body.split(";") if decl.strip() for d in decl.split(",")]
        assert names == [n for n, *_ in T._fields_], (name, names)


def test_the_library_refuses_null_handles_without_a_device(built_lib):
    import pirip_amd
    from pirip_amd import binding
    BAD_ARG = -1
    out = C.c_void_p(0x1234)
    cfg, fec = binding.PktConfig(4, 1, 1, 7, 5, 12, 4), binding.PktFecConfig(3, 50)
    assert built_lib.pirip_hip_pkt_create_fec(None, None, None, C.byref(cfg), C.byref(fec), C.byref(out)) == BAD_ARG and out.value is None
    out = C.c_void_p(0x1234)
    assert built_lib.pirip_hip_pkt_create_fec(None, None, None, C.byref(cfg), None, C.byref(out)) == BAD_ARG and out.value is None
    assert built_lib.pirip_hip_pkt_create_fec(None, None, None, None, C.byref(fec), C.byref(out)) == BAD_ARG
    assert built_lib.pirip_hip_pkt_create_fec(None, None, None, C.byref(cfg), C.byref(fec), None) == BAD_ARG
    assert built_lib.pirip_hip_pkt_get_fec_info(None, None) == BAD_ARG and built_lib.pirip_hip_pkt_get_fec_counters(None, None, None, None, None) == BAD_ARG
    assert issubclass(pirip_amd.HipPacketFec, pirip_amd.HipPacket) and pirip_amd.HipPacketFec._c == "pirip_hip_pkt"
