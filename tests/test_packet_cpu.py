"""include/pirip_hip.h section R without a GPU: the host model tests/pktref.py that tests/test_packet.py holds the device to. Its records
are frames the framer accepts, its tables reach every corner they claim, and the same rows cut into other calls give the same packets.
Also: the lane-parallel CRC-32 of pirip_amd/csrc/pkt_device.hpp against zlib, the structures' layouts, the library's refusal of NULL
handles and packet_channels' argument validation."""
import ctypes as C
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

import pktref
import sigutil
from test_tools_cli_cpu import BIN, CODE, NO_OUTPUT, RX, TXC, run_case, workdir  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KB, CAP = pktref.KB, pktref.cap(pktref.KB)
PRE, FRAME, GAP = 50, 544, 7                   # the stand-in code with M = 2: preamble and frame in bits; the gap the framer is given


# ---------------------------------------------------------------- the wire format

def test_sizes():
    assert (KB, CAP, pktref.max_packet(KB, 5), pktref.max_packet(KB, 100)) == (32, 24, 116, 2396)
    assert pktref.MAX_FRAMES == 100


@pytest.mark.parametrize("L", [1, CAP - 4, CAP - 3, CAP, 116])
def test_a_packets_records_are_frames_the_framer_accepts(built_lib, L):
    rng = np.random.default_rng(L)
    packet = rng.integers(0, 256, L).astype(np.uint8).tobytes()
    rec = pktref.segment(packet, 0x21, 0x42, 300 + L, KB, 5)
    n = {1: 1, CAP - 4: 1, CAP - 3: 2, CAP: 2, 116: 5}[L]
    assert rec.shape == (n + 1, 1 + KB) and rec[:, 0].tolist() == [1] + [0] * (n - 1) + [2] and not rec[n, 1:].any()
    assert rec[:n, 1].tolist() == [0x21] * n and rec[:n, 2].tolist() == [0x42] * n and rec[:n, 3].tolist() == [(300 + L) & 0xFF] * n
    assert rec[:n, 4].tolist() == list(range(n)) and rec[:n, 5].tolist() == [n] * n
    assert rec[:n, 6].tolist() == [CAP] * (n - 1) + [L + 4 - (n - 1) * CAP] and not rec[:n, KB - 1:].any()
    body = b"".join(rec[f, 7:7 + rec[f, 6]].tobytes() for f in range(n))
    assert body == packet + zlib.crc32(packet).to_bytes(4, "little")
    # the framer: one bit per byte, preamble, then per frame the unique word and the systematic codeword, then the gap's zeros
    bits = sigutil.run_framer(["-m", "2", "--packed", "--gap", str(GAP), "-", "-"], rec.tobytes())
    assert bits.size == PRE + n * FRAME + GAP
    for f in range(n):
        data = np.packbits(bits[PRE + f * FRAME + 32:PRE + f * FRAME + 32 + 8 * KB])
        assert np.array_equal(data[:KB - 2], rec[f, 1:KB - 1]), f       # the frame's bytes as given, the CRC16 behind them


def test_a_length_outside_the_range_is_refused():
    for L in (0, 117):
        with pytest.raises(ValueError):
            pktref.segment(bytes(L), 1, 2, 3, KB, 5)
    assert pktref.segment(bytes(116), 1, 2, 3, KB, 5).shape[0] == 6
    m = pktref.Link(1, 1, KB, 5, 12, 10 ** 6, 100, PRE, FRAME, GAP)
    assert m.send([[(bytes(116), 2), (bytes(117), 2), (bytes(1), 2)]]) == [1] and m.c["bad"].tolist() == [1] and m.c["sent"].tolist() == [1]


def test_lane_parallel_crc32_is_zlibs(tmp_path):
    exe = str(tmp_path / "pkt_crc_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", os.path.join(ROOT, "pirip_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "cprog", "pkt_crc_check.cpp")], check=True)
    msg = np.random.default_rng(1).integers(0, 256, 3000).astype(np.uint8).tobytes()
    Ls = [0, 1, 2, 5, 20, 63, 64, 65, 116, 127, 128, 129, 300, 2396, 3000]
    out = subprocess.run([exe] + [str(L) for L in Ls], input=msg, capture_output=True, check=True).stdout.decode().splitlines()
    assert out[:-1] == ["%d %08x" % (L, zlib.crc32(msg[:L])) for L in Ls]
    assert out[-1] == "sizes 24 2396 1 2"


# ---------------------------------------------------------------- reassembly

def _same_packets(a, b, but_call_and_row=False):
    (ea, ba), (eb, bb) = a, b
    same = pktref.same_but_call_and_row(ea, eb) if but_call_and_row else ea.tobytes() == eb.tobytes()
    return same and ba == bb


def test_the_tables_raise_every_counter_and_reach_every_corner():
    chans = pktref.streams()
    m = pktref.run_rows(pktref.cut(chans, 1, 7))
    ev = m.ev
    assert all(m.c[k][0] > 0 for k in pktref.RX_COUNTERS), m.c
    assert ev["bad_headers"] == {0, 1, 2, 3} and ev["interrupted_by_first"] > 0 and ev["duplicate"] > 0 and ev["other_src"] > 0 and ev["no_open"] > 0
    assert ev["short_body"] > 0 and ev["bits_without_sync"] > 0 and ev["sync_only_inside"] > 0 and ev["foreign_inside"] > 0
    assert ev["wraps"] > 0 and {254, 255, 0} <= ev["ids"] and ev["cut_inside_packet"] > 0
    assert m.c["crc_fail"][0] >= 2 and m.c["crc_fail"][1] > 0 and m.c["orphan"][1] > 0 and m.c["delivered"][2] == 6
    # channel 0 by hand, in one call: the first seven packets arrive whole, in order, with the lengths and ids they were given
    m1 = pktref.run_rows(pktref.one_call(chans), ring_entries=100)
    ent, data = m1.packets(0)
    assert ent["length"][:7].tolist() == [1, CAP - 4, CAP - 3, CAP, 116, 30, 30] and ent["nfrag"][:7].tolist() == [1, 1, 2, 2, 5, 2, 2]
    assert ent["id"][:7].tolist() == [0, 1, 2, 3, 254, 255, 0] and ent["dst"][:5].tolist() == [pktref.ADDR] * 4 + [0xFF] and not m1.c["lost"].any()
    assert ent["seq"].tolist() == list(range(len(ent))) and all(len(b) == n for b, n in zip(data, ent["length"]))
    assert (ent["src"] != pktref.FILT).all() and 5 in ent["src"].tolist()      # the row with BITS but no SYNC delivered its packet
    # the ring keeps the newest
    ent4, data4 = m.packets(0)
    assert len(ent4) == pktref.RING and m.c["lost"][0] == m.c["delivered"][0] - pktref.RING and data4 == data[-pktref.RING:]
    assert _same_packets(m.packets(0, 2), (ent4[-2:], data4[-2:]))
    # no filter and no address: the same rows deliver more
    m0 = pktref.run_rows(pktref.one_call(chans), filt=None, address=None)
    assert not m0.c["filtered"].any() and not m0.c["foreign"].any() and m0.c["delivered"][0] > m1.c["delivered"][0]


@pytest.mark.parametrize("how", ["between_fragments", "seed2", "seed3", "one_per_call"])
def test_the_same_rows_cut_into_other_calls_give_the_same_ring(how):
    chans = pktref.streams()
    ref = pktref.run_rows(pktref.one_call(chans))
    if how == "between_fragments":
        calls = pktref.between_fragments(chans)
        st, pl = calls[0][0]
        assert pl[-1, 3] == 0 and pl[-1, 4] > 1 and calls[1][0][1][0, 3] == 1 and calls[1][0][1][0, 2] == pl[-1, 2]
    elif how == "one_per_call":
        n = max(len(st) for st, _ in chans)
        calls = [[(st[i:i + 1], pl[i:i + 1]) for st, pl in chans] for i in range(n)]
    else:
        calls = pktref.cut(chans, int(how[-1]), 9)
    m = pktref.run_rows(calls)
    assert m.ev["cut_inside_packet"] > 0
    for c in range(3):
        assert _same_packets(m.packets(c), ref.packets(c), but_call_and_row=True), c
    assert all(np.array_equal(m.c[k], ref.c[k]) for k in ref.c)
    assert any(m.packets(c)[0]["call"].tolist() != ref.packets(c)[0]["call"].tolist() for c in range(3))


def test_one_call_of_4096_rows():
    big = pktref.big_call()
    assert [len(st) for st, _ in big[0]] == [4096, 4095, 1]
    m = pktref.run_rows(big, ring_entries=5000)
    assert m.c["delivered"][0] > 500 and m.c["crc_fail"][0] > 0 and m.c["orphan"][0] > 0 and m.ev["max_rows"] == 4096


# ---------------------------------------------------------------- send and offer

def test_link_model_prefix_bad_length_and_a_burst_that_waits():
    one = PRE + 5 * FRAME + 64
    m = pktref.Link(4, 1, KB, 5, 12, one, 1000, PRE, FRAME, 64)
    script = pktref.send_script()
    taken, offered = [], []
    for packets in script:
        taken.append(m.send(packets))
        offered.append(m.call())
    assert taken[0] == [2, 1, 2, 0] and taken[1] == [0, 1, 1, 1]
    assert m.c["refused"].tolist() == [1, 0, 0, 0] and m.c["bad"].tolist() == [0, 2, 0, 0] and m.c["sent"].tolist() == [3, 2, 4, 4]
    assert m.ev["blocked"] > 0 and m.ev["wraps"] > 0 and m.ev["max_bursts_per_offer"] >= 2 and not m.counters()["pending"].any()
    assert [len(r) for r in offered[0]] == [6, 2, 6, 0]                      # the queue holds one largest burst: the second one waits
    assert sum(len(o[0]) for o in offered) == 6 + 6 + 2
    for t in range(4):                                                       # what was offered is the accepted packets' bursts, in order
        rec = np.concatenate([o[t] for o in offered])
        sent = [p for n, packets in enumerate(script) for p in packets[t][:taken[n][t]]]
        want = [pktref.segment(b, 1, d, i, KB, 5) for i, (b, d) in enumerate(sent)]
        assert np.array_equal(rec, np.concatenate(want)), t


def test_an_id_passes_255():
    m = pktref.Link(1, 9, KB, 5, 12, 10 ** 9, 10 ** 6, PRE, FRAME, 0)
    ids = []
    for i in range(260):
        assert m.send([[(bytes([i & 0xFF]), 3)]]) == [1]
        ids.append(int(m.call()[0][0, 3]))
    assert ids == [i % 256 for i in range(260)]
    rows = pktref.rows_of([("pkt", bytes([i & 0xFF]), 9, 3, i) for i in range(260)])
    r = pktref.run_rows(pktref.one_call([rows]), ring_entries=300, filt=None, address=3)
    assert r.packets(0)[0]["id"].tolist() == ids and r.packets(0)[1] == [bytes([i & 0xFF]) for i in range(260)]


# ---------------------------------------------------------------- the binding and the library, without a device

def test_structures_have_the_headers_layout(tmp_path):
    """pirip_pkt_config / pirip_pkt_entry / pirip_pkt_info: the ctypes twins and the numpy dtype against what gcc makes of the header"""
    import pirip_amd
    from pirip_amd import binding
    twins = {"pirip_pkt_config": binding.PktConfig, "pirip_pkt_entry": binding.PktEntry, "pirip_pkt_info": binding.PktInfo}
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
    for dt in (np.dtype(pirip_amd.PKT_ENTRY_DTYPE), pktref.ENTRY):
        assert dt.itemsize == size["pirip_pkt_entry"] == 24
        assert [(n, dt.fields[n][1], dt.fields[n][0].itemsize) for n in dt.names] == fields["pirip_pkt_entry"]
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
    cfg = binding.PktConfig(4, 1, 1, 7, 5, 12, 4)
    assert built_lib.pirip_hip_pkt_create(None, None, None, C.byref(cfg), C.byref(out)) == BAD_ARG and out.value is None
    assert built_lib.pirip_hip_pkt_create(None, None, None, None, C.byref(out)) == BAD_ARG
    assert built_lib.pirip_hip_pkt_create(None, None, None, C.byref(cfg), None) == BAD_ARG
    for name, args in (("pirip_hip_pkt_destroy", ()), ("pirip_hip_pkt_get_info", (None,)), ("pirip_hip_pkt_reset", (None,)),
                       ("pirip_hip_pkt_send", (None, 0, 0, None, 0, None, None, None, None)),
                       ("pirip_hip_pkt_push_records", (None, 0, None, 0, None, 0, None, 0, None)), ("pirip_hip_pkt_process", (None, 0, None)),
                       ("pirip_hip_pkt_push", (None, 0, None, 0, None)), ("pirip_hip_pkt_records", (None,) * 5),
                       ("pirip_hip_pkt_offered", (None,) * 3), ("pirip_hip_pkt_get_counters", (None,) * 12),
                       ("pirip_hip_pkt_get_packets", (0, None, None, 0, None))):
        assert getattr(built_lib, name)(None, *args) == BAD_ARG, name
    assert pirip_amd.HipPacket._c == "pirip_hip_pkt" and issubclass(pirip_amd.HipPacket, binding._Terminal)


# ---------------------------------------------------------------- packet_channels' arguments

PKT = TXC + ["--source", "1", "--block", "24000", "-o", "-"]
USAGE = ("packet_channels (pirip_hip): --code NAME|FILE -s wideFs -a modemFs -r Rs [-m M] [--mask spacing] [--fsk_lower Hz] [--fsk_upper Hz]\n"
         "        -c off1,off2,... --f1 Hz --shift Hz [--gain g | --gains g1,g2,...] [--linear] [--gap BITS] --block N [--queue SYMS]\n"
         "        --source A [--filter A] [--address A] [--max-frags N] [--pending RECORDS] [--ring PACKETS] [--send FILE] [--deliver FILE]\n"
         "        [-i <u8 IQ file|->] -o <file|-> [-q]\n")
CLI = [
    ("no-args", [], 1, USAGE),
    ("unknown-option", PKT + ["-c", "0", "--bogus"], 1, "packet_channels: unrecognized option '--bogus'\n" + USAGE),
    ("m3", PKT + ["-c", "0", "-m", "3"], 1, USAGE),
    ("wide-not-multiple-of-modem", ["--code", CODE, "-s", "240000", "-a", "70000", "-r", "1000", "--f1", "1000", "--shift", "2000", "--source", "1",
                                    "--block", "24000", "-o", "-", "-c", "0"], 1,
     "packet_channels: the wideband rate 240000 must be a multiple of the modem rate 70000\n"),
    ("c-empty-token", PKT + ["-c", "1,,2"], 1, "packet_channels: -c wants integer offsets in Hz, comma separated\n"),
    ("gains-wrong-count", PKT + ["-c", "0,1000,2000", "--gains", "0.1,0.2"], 1, "packet_channels: one gain, or one per channel\n"),
    ("gap-1-with-m4", PKT + ["-c", "0", "-m", "4", "--gap", "1"], 1, "packet_channels: --gap is whole symbols\n"),
    ("block-not-multiple-of-d-ts", TXC + ["--source", "1", "--block", "1000", "-o", "-", "-c", "0"], 1,
     "packet_channels: --block must be a multiple of D * Ts = 240 wideband samples\n"),
    ("source-missing", TXC + ["--block", "24000", "-o", "-", "-c", "0"], 1,
     "packet_channels: --source A (0 .. 255) is needed; --filter A and --address A likewise\n"),
    ("address-300", PKT + ["-c", "0", "--address", "300"], 1, "packet_channels: --source A (0 .. 255) is needed; --filter A and --address A likewise\n"),
    ("max-frags-0", PKT + ["-c", "0", "--max-frags", "0"], 1, "packet_channels: --max-frags 1 .. 100, --ring >= 1\n"),
    ("max-frags-101", PKT + ["-c", "0", "--max-frags", "101"], 1, "packet_channels: --max-frags 1 .. 100, --ring >= 1\n"),
    ("ring-0", PKT + ["-c", "0", "--ring", "0"], 1, "packet_channels: --max-frags 1 .. 100, --ring >= 1\n"),
    ("pending-too-small", PKT + ["-c", "0", "--max-frags", "5", "--pending", "5"], 1, "packet_channels: --pending holds at least one packet, 6 records\n"),
    ("code-nowhere", ["--code", "nosuch"] + RX + ["--f1", "1000", "--shift", "2000", "--source", "1", "--block", "24000", "-o", "-", "-c", "0"], 2,
     "packet_channels: no table for --code nosuch (format: pirip_amd/csrc/fsk_ldpc.hpp; $PIRIP_CODE_DIR or a file path)\n"),
    ("cannot-open", PKT + ["-c", "0", "-i", "missing.iq8"], 1, "packet_channels: can't open missing.iq8\n"),
    ("send-cannot-open", PKT + ["-c", "0", "--send", "missing.pkt"], 1, "packet_channels: can't open missing.pkt\n"),
    ("send-other-channel", PKT + ["-c", "0", "--send", "chan1.pkt"], 1,
     "packet_channels: --send: a record for channel 1 of 3 bytes is not one of this link's\n"),
    ("send-cut-short", PKT + ["-c", "0", "--send", "short.pkt"], 1, "packet_channels: --send ends inside a record\n"),
]


@pytest.mark.parametrize("name,args,code,err", CLI, ids=[c[0] for c in CLI])
def test_packet_channels_answers_its_arguments(built_lib, workdir, name, args, code, err):  # noqa: F811
    with open(os.path.join(workdir, "chan1.pkt"), "wb") as f:
        f.write(bytes([1, 7, 3, 0, 1, 2, 3]))
    with open(os.path.join(workdir, "short.pkt"), "wb") as f:
        f.write(bytes([0, 7, 3, 0, 1, 2, 3, 0, 7]))
    assert run_case(BIN, workdir, "packet_channels", args, {}) == (code, err, NO_OUTPUT)


def test_packet_channels_without_a_device(built_lib, workdir):  # noqa: F811
    import pirip_amd
    if pirip_amd.device_count() > 0:
        pytest.skip("a HIP device is present")
    assert run_case(BIN, workdir, "packet_channels", PKT + ["-c", "-90000,30001"], {}) == \
        (2, "packet_channels: channelizer: no usable HIP device\n", NO_OUTPUT)
