"""The medium-access layer without a device (include/pirip_hip.h section T): tests/macref.py, the model tests/test_mac.py
holds the device to, shown to do what the header says and to reach what its scripts claim; pirip_amd/csrc/mac_device.hpp against the
model's tables in a stand-alone program (built once more with the host sanitizers); the structures' layouts; the library's refusal of NULL
handles; and the model alone on a modelled shared medium, where two ARQ terminals with equal timers lose everything without the gate and
nothing with it."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import macref as m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the draw and the gate by hand

def test_the_draw_by_hand():
    assert m.draw(0, 0, 0, 1024) == 0                                     # x = 0 stays 0 through the mixer
    # key 1, t 0, a 0 by the header's lines, written out
    x = 1
    x ^= x >> 16
    x = x * 0x7FEB352D & m.M32
    x ^= x >> 15
    x = x * 0x846CA68B & m.M32
    x ^= x >> 16
    assert m.draw(1, 0, 0, 1024) == x * 1024 >> 32 and m.draw(1, 0, 0, 1) == 0
    assert m.draw(7, 3, 2 ** 32 + 5, 8) == m.draw(7, 3, 5, 8)             # a is truncated to 32 bits
    for cw in m.DRAW_CWS:
        got = [m.draw(k, t, a, cw) for k in m.DRAW_KEYS for t in range(8) for a in m.DRAW_AS]
        assert min(got) == 0 and max(got) <= cw - 1 and (cw > 8 or max(got) == cw - 1)          # inside [0, cw), both ends reached
    # uniform enough to be a backoff: 4096 draws of cw = 8 fill every slot within 20 % of the mean
    hist = np.bincount([m.draw(0xC0FFEE, 1, a, 8) for a in range(4096)], minlength=8)
    assert hist.min() > 0.8 * 512 and hist.max() < 1.2 * 512


def test_the_gate_by_hand():
    rules = dict(slot_calls=2, cw=8, ifs_calls=1, txop_bursts=2, key=9)
    b = m.draw(9, 3, 0, 8)
    g = m.new_gate()
    assert m.gate_step(g, rules, 3, False, False, 5) == 0 and g == m.new_gate()                # nothing due: nothing happens
    # due on a busy medium: the access begins, the countdown does not run (idle 1 is not more than ifs_calls)
    assert m.gate_step(g, rules, 3, True, False, 1) == 0
    assert (g["phase"], g["counter"], g["accesses"], g["deferred"], g["backoff"]) == (m.CONTEND, 2 * b, 1, 1, 0)
    for left in range(2 * b, 0, -1):
        assert m.gate_step(g, rules, 3, True, False, 2) == 0 and g["counter"] == left - 1
    assert g["backoff"] == 2 * b and g["phase"] == m.CONTEND
    assert m.gate_step(g, rules, 3, True, False, 0) == 0 and g["deferred"] == 2               # carrier at counter 0: wait
    assert m.gate_step(g, rules, 3, True, False, 2) == 2 and (g["phase"], g["run"], g["won"]) == (m.HOLD, 0, 1)
    g["run"] = 1                                                          # the offer took one burst
    assert m.gate_step(g, rules, 3, True, True, 0) == 1                   # HOLD does not listen
    g["run"] = 2
    assert m.gate_step(g, rules, 3, True, True, 9) == 0 and g["phase"] == m.HOLD               # the access is used up while the queue drains
    # the queue is empty: IDLE, and the burst that is due starts the next access in the same call, with the next draw
    assert m.gate_step(g, rules, 3, True, False, 0) == 0
    assert (g["phase"], g["accesses"], g["counter"]) == (m.CONTEND, 2, 2 * m.draw(9, 3, 1, 8))
    # cw = 1 on an idle medium: IDLE -> CONTEND -> HOLD in one call
    g = m.new_gate()
    assert m.gate_step(g, dict(rules, cw=1, ifs_calls=0), 0, True, False, 1) == 2 and (g["phase"], g["won"], g["backoff"]) == (m.HOLD, 1, 0)
    assert m.run_next(m.RUN_MAX, False) == m.RUN_MAX and m.run_next(7, True) == 0


# ---------------------------------------------------------------- mac_device.hpp on the host

def _build(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", os.path.join(ROOT, "pirip_amd", "csrc")] + flags +
                   ["-o", exe, os.path.join(ROOT, "tests", "cprog", "mac_gate_check.cpp")], check=True)
    return exe


def test_mac_device_hpp_is_the_models_arithmetic_also_under_the_host_sanitizers(tmp_path):
    """draw: cw in {1, 2, 3, 8, 1024}, t 0 .. 7, a in {0 .. 63, 2^32 - 1}, four keys; the gate: every combination of phase, counter 0 .. 3,
    run 0 .. 2, due, queued, idle 0 .. 3, ifs_calls 0 .. 2, txop_bursts 1 .. 2"""
    table = tmp_path / "table.txt"
    table.write_text(m.table_text())
    assert len(m.draw_lines()) == 4 * 5 * 8 * 65 and len(m.gate_lines()) == 3 * 2 * 3 * 4 * 3 * 2 * 2 * 4
    for name, flags in (("mac_gate_check", []), ("mac_gate_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        r = subprocess.run([_build(tmp_path, name, flags), str(table)], capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", (name, r.returncode, r.stderr[-2000:])
        assert r.stdout == "draws %d gates %d\n" % (len(m.draw_lines()), len(m.gate_lines())), name
    # the program does compare: one changed draw and one changed limit are found
    lines = m.table_text().splitlines()
    for i in (5, len(lines) - 3):
        w = lines[i].split()
        bad = lines[:i] + [" ".join(w[:-1] + [str(int(w[-1]) + 1)])] + lines[i + 1:]
        table.write_text("\n".join(bad) + "\n")
        r = subprocess.run([str(tmp_path / "mac_gate_check"), str(table)], capture_output=True, text=True)
        assert r.returncode == 1 and "differs" in r.stderr, i


# ---------------------------------------------------------------- the scripts reach what they claim

def test_the_sense_scripts_reach_every_edge():
    t = m.terminal(mac=dict(cw=1))
    seen = []
    for rows, stats, note in m.sense_script():
        t.call(rows, stats)
        seen.append((note, list(t.mac.last_carrier)))
    sizes = {len(rows[0][0]) for rows, _, _ in m.sense_script()}
    assert sizes == set(m.SENSE_SIZES)
    for note, car in seen:
        want = note.startswith("SYNC at")
        assert sum(car) == want, note
    assert {n for n, _ in seen} >= {"SYNC at 0 of 1", "SYNC at 63 of 64", "SYNC at 64 of 65", "SYNC at 4095 of 4096", "SYNC at 63 of 4096", "nothing in 0 rows"}
    # the idle run restarts at a carrier and counts otherwise
    assert t.mac.idle[1] == len(seen) and t.mac.idle[0] < len(seen)
    for mask, want in ((1, dict(at=0, under=0, nan=0, inf=0)), (2, dict(at=1, under=0, nan=0, inf=1)), (3, dict(at=1, under=0, nan=0, inf=1))):
        t = m.terminal(mac=dict(cw=1, sense_mask=mask, sense_snr=m.SNR_T))
        for rows, stats, note in m.snr_script():
            t.call(rows, stats)
            if note.split()[0] in want:
                assert t.mac.last_carrier == [want[note.split()[0]], 0, 0, 0], (mask, note)
            elif note == "SYNC under weak stats":
                assert t.mac.last_carrier[0] == (mask & 1), mask
            else:
                assert not any(t.mac.last_carrier), note
        assert (t.mac.ev["nan_rows"] > 0) == bool(mask & 2)


@pytest.mark.parametrize("fec", [None, (2, 50)], ids=["plain", "fec"])
def test_the_mute_script_mutes_what_the_own_burst_produced(fec):
    M = 2
    t = m.terminal(mac=dict(cw=1, mute_calls=M), fec=fec)
    m.run_script(t, m.mute_script(M, fec))
    c, r = t.mac.counters(), t.rasm.counters()
    air = [(m.PRE + (1 + (1 if fec else 0)) * m.FRAME + m.GAP + m.REC_S - 1) // m.REC_S]
    air.append(-(-(m.PRE + (m.MAX_FRAGS + (2 if fec else 0)) * m.FRAME + m.GAP) // m.REC_S))
    ncalls = M + 7
    # own for the calls on air and mute_calls - 1 more (quiet 0 .. mute_calls - 1); every packet outside them is delivered
    assert c["own"].tolist()[:3] == [air[0] + M - 1, air[1] + M - 1, 0] and c["won"].tolist() == [1, 1, 0, 1]
    assert r["delivered"].tolist()[:3] == [ncalls - 1 - c["own"][0], ncalls - 1 - c["own"][1], ncalls - 1]
    assert c["muted"][0] == c["own"][0] * (2 if fec else 1) and c["muted"][2] == 0 and c["muted"][3] == 1
    assert t.mac.ev["mute_kept_sync"] > 0 and (fec or t.mac.ev["muted_open_packet"] > 0)
    # the packet that was open across the muted calls: lost on the plain handle, rebuilt from parity on the FEC handle
    assert r["delivered"][3] == (1 if fec else 0) and (fec or (r["orphan"][3], r["incomplete"][3]) == (1, 1))
    # mute_calls = 0: nothing is ever muted
    t0 = m.terminal(mac=dict(cw=1, mute_calls=0), fec=fec)
    m.run_script(t0, m.mute_script(0, fec))
    assert not t0.mac.counters()["own"].any() and t0.rasm.counters()["delivered"].tolist() == [6, 6, 6, 1]


GATE_CASES = {"cw1": dict(cw=1, ifs_calls=0, txop_bursts=1), "cw8_ifs2_txop2": dict(cw=8, slot_calls=2, ifs_calls=2, txop_bursts=2),
              "cw8_ifs0_txop1": dict(cw=8, ifs_calls=0, txop_bursts=1, mute_calls=2)}


@pytest.mark.parametrize("case", sorted(GATE_CASES))
def test_the_gate_script_reaches_every_rule(case):
    kw = dict(GATE_CASES[case], rx_of_tx=[0, -1, 3, 2], key=5)
    t, plain = m.terminal(mac=kw), m.terminal()
    off = m.run_script(t, [(s, r, None) for s, r in m.gate_script(3)])
    ref = m.run_script(plain, [(s, r, None) for s, r in m.gate_script(3)])
    # the ungated channel is offered exactly as without the layer; the gated ones are not
    assert all(np.array_equal(a[1], b[1]) for a, b in zip(off, ref)) and any(not np.array_equal(a[0], b[0]) for a, b in zip(off, ref))
    c, ev = t.mac.counters(), t.mac.ev
    for t_ in (0, 2, 3):
        assert c["accesses"][t_] > 3 and c["won"][t_] > 3 and c["deferred"][t_] > 0 and c["bursts"][t_] >= c["won"][t_]
    assert c["accesses"][1] == c["bursts"][1] == 0 and t.mac.state(1)["idle"] == -1
    assert ev["limited"] > 0 and ev["hold_exhausted"] > 0 and ev["due_while_hold"] > 0
    assert (c["backoff"].sum() > 0) == (kw["cw"] > 1) and (ev["contend_to_hold_same_call"] > 0) == (kw["cw"] == 1)
    if kw["txop_bursts"] == 2:
        assert c["bursts"][0] > c["won"][0]                               # some access took two bursts
    else:
        assert (c["bursts"] <= c["won"]).all()                            # an access puts one burst on air at the most


# ---------------------------------------------------------------- the structures and the library, without a device

def test_structures_have_the_headers_layout(tmp_path):
    import pirip_amd
    from pirip_amd import binding
    twins = {"pirip_mac_config": binding.MacConfig, "pirip_mac_info": binding.MacInfo}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pirip_hip.h"', "int main(void) {"]
    for name, T in twins.items():
        lines.append(f'    printf("S {name} %zu\\n", sizeof({name}));')
        lines += [f'    printf("F {name} {f} %zu %zu\\n", offsetof({name}, {f}), sizeof((({name} *)0)->{f}));' for f, *_ in T._fields_]
    lines += ['    printf("P %d %d %d\\n", PIRIP_MAC_IDLE, PIRIP_MAC_CONTEND, PIRIP_MAC_HOLD);', "    return 0;", "}"]
    (tmp_path / "l.c").write_text("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "l"), str(tmp_path / "l.c")], check=True)
    size, fields, phases = {}, {n: [] for n in twins}, None
    for ln in subprocess.run([str(tmp_path / "l")], check=True, capture_output=True, text=True).stdout.split("\n"):
        w = ln.split()
        if w and w[0] == "S":
            size[w[1]] = int(w[2])
        elif w and w[0] == "F":
            fields[w[1]].append((w[2], int(w[3]), int(w[4])))
        elif w:
            phases = tuple(int(x) for x in w[1:])
    for name, T in twins.items():
        assert C.sizeof(T) == size[name]
        assert [(n, getattr(T, n).offset, getattr(T, n).size) for n, *_ in T._fields_] == fields[name]
    assert phases == (pirip_amd.MAC_IDLE, pirip_amd.MAC_CONTEND, pirip_amd.MAC_HOLD) == (m.IDLE, m.CONTEND, m.HOLD)
    assert binding.MacConfig.sense_snr.size == 4 and dict(binding.MacConfig._fields_)["sense_snr"] is C.c_float
    assert dict(binding.MacConfig._fields_)["key"] is C.c_uint32
    src = open(os.path.join(ROOT, "include", "pirip_hip.h")).read()
    for name, T in twins.items():
        body = re.sub(r"/\*.*?\*/", " ", src.split("struct %s {" % name)[1].split("};")[0], flags=re.S)
        names = [d.strip().split()[-1] for decl in body.split(";") if decl.strip() for d in decl.split(",")]
        assert names == [n for n, *_ in T._fields_], (name, names)
    assert pirip_amd.HipMac.TX_COUNTERS == m.TX_COUNTERS and pirip_amd.HipMac.RX_COUNTERS == m.RX_COUNTERS and pirip_amd.HipMac.STATE == m.STATE


def test_the_library_refuses_null_handles_without_a_device(built_lib):
    import pirip_amd
    from pirip_amd import binding
    BAD_ARG = -1
    out = C.c_void_p(0x1234)
    cfg = binding.MacConfig(1, 0.0, 1, 8, 0, 1, 1, 7)
    rt = (C.c_int32 * 4)(0, 1, 2, 3)
    assert built_lib.pirip_hip_mac_create(None, C.byref(cfg), rt, C.byref(out)) == BAD_ARG and out.value is None
    assert built_lib.pirip_hip_mac_create(None, C.byref(cfg), rt, None) == BAD_ARG
    for name, args in (("pirip_hip_mac_destroy", ()), ("pirip_hip_mac_get_info", (None,)), ("pirip_hip_mac_reset", (None,)),
                       ("pirip_hip_mac_set_stats", (None, 0)), ("pirip_hip_mac_stats", (None, None)), ("pirip_hip_mac_get_counters", (None,) * 8),
                       ("pirip_hip_mac_get_state", (0,) + (None,) * 5)):
        assert getattr(built_lib, name)(None, *args) == BAD_ARG, name
    assert pirip_amd.HipMac._c == "pirip_hip_mac" and issubclass(pirip_amd.HipMac, binding._Handle)
    assert "HipMac" not in vars(binding)                                 # a module of its own, as HipPacket and HipArq are


# ---------------------------------------------------------------- the model alone on a modelled shared medium

def test_the_air_keys_draw_differently_on_every_channel():
    """a condition on the inputs of the air runs, here and in tests/test_mac.py: for accesses 0 .. 7 the two ends never draw alike"""
    assert m.keys_differ(m.AIR_KEYS, m.AIR_CW, accesses=8, nchan=4)
    assert not m.keys_differ((5, 5)) and m.AIR_KEYS[0] != m.AIR_KEYS[1]


@pytest.mark.parametrize("lag", [1, 2, 3])
def test_without_the_gate_every_burst_collides_and_with_it_every_segment_arrives(lag):
    """two terminals submit in the same call with equal timers; sensing lags by `lag` calls; slot_calls = lag + 1"""
    med = m.air_pair(False, lag)
    ta, tb = m.air_traffic(med.nodes[0].max_payload)
    rto = m.air_rto(lag + 1)
    m.run_air(med, ta, tb, 2 + m.AIR_TRIES * rto + 5)
    a, b = (n.counters() for n in med.nodes)
    assert med.arrived == [0, 0] and med.collided[0] == med.collided[1] == 4 * m.AIR_W * m.AIR_TRIES
    assert a["broken"].tolist() == b["broken"].tolist() == [1] * 4 and not a["delivered"].any() and not b["delivered"].any()
    assert (a["sent"] + a["retransmitted"]).tolist() == [m.AIR_W * m.AIR_TRIES] * 4
    med = m.air_pair(True, lag)
    m.run_air(med, ta, tb, 300 * (lag + 1))                               # (the horizon: long enough for the last ACK at every lag)
    a, b = (n.counters() for n in med.nodes)
    assert not a["broken"].any() and not b["broken"].any() and not a["inflight"].any() and not b["inflight"].any()
    for c in range(4):
        assert med.nodes[1].sess[c].delivered()[1] == ta[c] and med.nodes[0].sess[c].delivered()[1] == tb[c], c
        assert med.nodes[1].sess[c].delivered()[0]["seq"].tolist() == list(range(m.AIR_SEGMENTS))
    for nd in med.nodes:
        mc = nd.mac.counters()
        assert mc["won"].min() >= m.AIR_SEGMENTS and mc["deferred"].min() > 0 and mc["backoff"].min() > 0
        # every row with BITS that the terminal's own air produced was muted: nothing of its own reached the reassembly's filter
        assert mc["muted"].min() > 0 and not nd.rasm.counters()["filtered"].any()
    assert med.arrived[0] > 0 and med.arrived[1] > 0
