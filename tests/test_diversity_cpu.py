"""The diversity receiver's model (include/pirip_hip.h section Q) without a device: tests/divref.py, the numpy
restatement the device tests hold the kernels to, against the rule's own text.

  1. the reference does not depend on how the branches' rows were cut into calls (whole, one row per call, ragged);
  2. the closure rule at its edges (tests/divshapes.py: BOUNDARY) and the combination by value (SPECIAL), on explicit tags and words;
  3. on oracle-demodulated input a frame is recovered that no branch decodes alone;
  4. what the binding and the library refuse without a device, and the three structures' layouts against the header."""
import ctypes as C
import gc
import os
import subprocess

import numpy as np
import pytest

import divref
import divshapes
import sigutil

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODE = os.path.join(ROOT, "pirip_amd", "data", "standin_256_512_4.code")
RX_BITS = 4


def pending_capacity(B, max_rows, Nbits, bpf):
    """pirip_hip_div_create's sizing, restated: 3 (max_rows Nbits / bpf + 2) + 2 candidates per branch"""
    return B * (3 * (max_rows * Nbits // bpf + 2) + 2)


@pytest.fixture(scope="module")
def rescue_rows(oracle, built_lib):
    """two branches of one transmission through the CPU oracle: per branch dict(llr, status, payload, info, stats), and the pieces"""
    r = divshapes.RESCUE
    code = oracle.parse_code_file(CODE)
    c = dict(sigutil.CFG1, P=6)
    p = subprocess.run([os.path.join(ROOT, "pirip_amd", "bin", "fsk_ldpc_framer"), "--code", CODE, "--testframes", str(r["frames"]), "--bursts", "1",
                        "--seq", "/dev/zero", "-"], input=b"", capture_output=True)
    assert p.returncode == 0, p.stderr
    bits = np.frombuffer(p.stdout, dtype=np.uint8)
    rows = []
    for u8 in divshapes.branch_copies(oracle, c, 2, [bits] * r["bursts"], r["ebno_db"], r["seed"], r["delays"]):
        dem = oracle.OracleFsk(c["Fs"], c["Rs"], 2, P=6, est_min=500, est_max=25000)
        d = dem.demod(u8, oracle.IN_CU8_CSDR)
        st, pl, info = oracle.OracleLdpc(code, 2).rx(d["rx_filt"])
        rows.append(dict(llr=oracle.OracleLdpc(code, 2).llr(d["rx_filt"]), status=st, payload=pl, info=info, stats=d["stats"]))
    return dict(rows=rows, code=code, Ts=c["Fs"] // c["Rs"], nin0=dem.N, want=np.packbits(bits[50 + 32:][:256]))


def _ref(oracle, rr, max_rows):
    o = oracle.OracleLdpc(rr["code"], 2)
    return divref.DivRef(2, 1, rr["Ts"], 512, 50, rr["nin0"], divshapes.RESCUE["skew"], divref.oracle_decoder(o),
                         pending_capacity=pending_capacity(2, max_rows, 50, 544))


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert {k: x[k] for k in divref.ENTRY_FIELDS} == {k: y[k] for k in divref.ENTRY_FIELDS}
        assert np.array_equal(x["payload"], y["payload"]) and x["taus"] == y["taus"]


def test_reference_does_not_depend_on_the_cutting_into_calls(oracle, rescue_rows):
    rows = rescue_rows["rows"]
    total = max(len(r["status"]) for r in rows)
    whole = _ref(oracle, rescue_rows, total)
    for b in range(2):
        divshapes.feed_rows(whole, b, rows[b])
    whole.close(); whole.flush()
    single = _ref(oracle, rescue_rows, 1)
    for f in range(total):
        for b in range(2):
            divshapes.feed_rows(single, b, rows[b], f, f + 1)
        single.close()
    single.flush()
    ragged = _ref(oracle, rescue_rows, 7)                      # branch 0 a call ahead of branch 1 at every boundary
    for i in range(total // 7 + 3):
        divshapes.feed_rows(ragged, 0, rows[0], 7 * i, 7 * i + 7)
        divshapes.feed_rows(ragged, 1, rows[1], 7 * (i - 1), 7 * i) if i else None
        ragged.close()
    ragged.flush()
    assert len(whole.entries) >= 15
    _same(whole.entries, single.entries)
    _same(whole.entries, ragged.entries)
    assert [whole.dropped, single.dropped, ragged.dropped] == [0, 0, 0]          # the ring sized from max_rows holds every cutting
    print("pending at most", whole.max_pending, single.max_pending, ragged.max_pending, "of",
          [pending_capacity(2, m, 50, 544) for m in (total, 1, 7)])
    # a call's clusters are all closed: nothing emitted before a flush lies above the horizon
    assert all(max(e["taus"]) - min(e["taus"]) <= whole.K for e in whole.entries)


def _tag_ref(K, B=2, n=8):
    seen = []

    def decoder(llr):
        seen.append(np.asarray(llr, dtype=np.float16).copy())
        return np.zeros(2, dtype=np.uint8), 0, 0, 0, divref.RX_SYNC
    ref = divref.DivRef(B, 1, 8, n, 8, 0, K, decoder)
    return ref, seen


@pytest.mark.parametrize("name", sorted(divshapes.BOUNDARY))
def test_closure_rule_at_its_edges(name):
    K, cands, H, want_call, want_flush = divshapes.BOUNDARY[name]
    ref, seen = _tag_ref(K)
    for i, (tau, b) in enumerate(cands):
        ref.add(tau, b, np.full(8, 2.0 ** i, dtype=np.float16), False)       # candidate i carries 2^i: a cluster's sum names its members
    got_call = ref.close(H=H)
    got_flush = ref.flush()
    for got, want in ((got_call, want_call), (got_flush, want_flush)):
        assert len(got) == len(want), (name, got, want)
        for e, idx in zip(got, want):
            assert e["members"] == sum(1 << cands[i][1] for i in idx)
            assert e["t_samples"] == min((cands[i][0], cands[i][1]) for i in idx)[0]
            assert sorted(e["taus"]) == sorted(cands[i][0] for i in idx)
    sums = [float(s[0]) for s in seen]
    assert sums == [float(sum(2.0 ** i for i in idx)) for idx in want_call + want_flush]
    assert not ref.pending


@pytest.mark.parametrize("name", sorted(divshapes.SPECIAL))
def test_combination_by_value(name):
    vals, want = divshapes.SPECIAL[name]
    got = divref.combine([np.full(3, v, dtype=np.float16) for v in vals])
    assert divshapes.same_f16(got, np.full(3, want, dtype=np.float16)), (name, got)
    for v in vals:                                                         # every operand is a binary16 value as written
        assert np.isnan(v) or float(np.float16(v)) == v


def test_a_cluster_of_one_reproduces_its_word():
    w = np.array(divshapes.SINGLE, dtype=np.float16)
    assert divshapes.same_f16(divref.combine([w]), w)
    assert divshapes.same_f16(divref.combine([np.array([np.nan], dtype=np.float16)]), np.zeros(1, dtype=np.float16))


def test_a_frame_no_branch_decodes_alone_is_rescued(oracle, rescue_rows):
    rows, r = rescue_rows["rows"], divshapes.RESCUE
    total = max(len(x["status"]) for x in rows)
    ref = _ref(oracle, rescue_rows, total)
    for b in range(2):
        divshapes.feed_rows(ref, b, rows[b])
    ref.close(); ref.flush()
    frames = r["frames"] * r["bursts"]
    assert 2 * frames <= 40                                              # the whole input: 20 frames on each of two branches
    solo = [int(((x["status"] & RX_BITS) != 0).sum()) for x in rows]
    cnt = ref.counters(256)
    rescued = [e for e in ref.entries if e["solo_ok"] == 0 and e["members"] == 3 and e["status"] & RX_BITS]
    print("decoded alone", solo, "of", frames, "each; clusters", cnt["clusters"], "with BITS", cnt["bits"], "rescued", cnt["rescued"])
    assert len(rescued) >= 1 and cnt["rescued"] >= len(rescued)
    want = rescue_rows["want"]
    assert all(np.array_equal(e["payload"][2:30], want[2:30]) for e in rescued)        # the test frame, 0 coded errors
    assert cnt["bits"] > max(solo)
    # conditions on the input, checked on the reference: nothing dropped, every cluster's members within K
    assert ref.dropped == 0 and cnt["dropped"] == 0
    assert all(max(e["taus"]) - min(e["taus"]) <= ref.K for e in ref.entries)
    assert divshapes.RESCUE["delays"][1] % rescue_rows["Ts"] != 0
    # a cluster of one is the branch's own record
    for e in ref.entries:
        if e["members"] in (1, 2):
            x = rows[e["members"] - 1]
            hit = [f for f in range(len(x["status"])) if x["info"][f, 6] >= 0 and np.array_equal(x["payload"][f], e["payload"])]
            assert any(int(x["status"][f]) == e["status"] and x["info"][f, 4] == e["iters"] and x["info"][f, 5] == e["pcc"] and
                       x["info"][f, 8] == e["eraw"] for f in hit), e


# ---------------------------------------------------------------- without a device: the binding, the library's argument checks, layouts

def test_structures_have_the_headers_layout(tmp_path):
    """pirip_div_config / pirip_div_entry / pirip_div_info: the ctypes twins and the numpy dtype against what gcc makes of the header"""
    import pirip_amd
    from pirip_amd import binding
    twins = {"pirip_div_config": binding.DivConfig, "pirip_div_entry": binding.DivEntry, "pirip_div_info": binding.DivInfo}
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
    dt = np.dtype(pirip_amd.DIV_ENTRY_DTYPE)
    assert dt.itemsize == size["pirip_div_entry"] == 24
    assert [(n, dt.fields[n][1], dt.fields[n][0].itemsize) for n in dt.names] == fields["pirip_div_entry"]
    # the header's field lists are the twins' (a field added to the header alone would pass the offsets above)
    src = open(os.path.join(ROOT, "include", "pirip_hip.h")).read()
    for name, T in twins.items():
        body = src.split("struct %s {" % name)[1].split("};")[0]
        import re
        body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
        names = [d.strip().split()[-1] for decl in body.split(";") if decl.strip() for d in decl.split(",")]
        assert names == [n for n, *_ in T._fields_], (name, names)


def test_the_library_refuses_null_handles_without_a_device(built_lib):
    import pirip_amd
    from pirip_amd import binding
    BAD_ARG = -1
    assert built_lib.pirip_hip_strerror(BAD_ARG)
    out = C.c_void_p(0x1234)
    cfg = binding.DivConfig(2, 24, 1200, 80, 64, 16)
    assert built_lib.pirip_hip_div_create(None, C.byref(cfg), C.byref(out)) == BAD_ARG and out.value is None
    assert built_lib.pirip_hip_div_create(None, None, C.byref(out)) == BAD_ARG
    assert built_lib.pirip_hip_div_create(None, C.byref(cfg), None) == BAD_ARG
    for name, args in (("pirip_hip_div_destroy", ()), ("pirip_hip_div_get_info", (None,)), ("pirip_hip_div_reset", (None,)),
                       ("pirip_hip_div_collect", (None, 0, None, 0, None, 0, None, 1, None)),
                       ("pirip_hip_div_push_candidates", (None, None, None, None, 0, None, None)), ("pirip_hip_div_flush", (None,)),
                       ("pirip_hip_div_last", (None,) * 5), ("pirip_hip_div_get_log", (0, None, None, 0, None)),
                       ("pirip_hip_div_get_counters", (None,) * 6), ("pirip_hip_div_get_combined", (0, 0, None))):
        assert getattr(built_lib, name)(None, *args) == BAD_ARG, name
    assert pirip_amd.HipDiversity._c == "pirip_hip_div" and issubclass(pirip_amd.HipDiversity, binding._Handle)


class _Stub:
    """tests/test_binding_handles_cpu.py's stub in the place of the loaded library"""
    def __init__(self, fail=()):
        self.calls, self.fail = [], set(fail)

    def __getattr__(self, name):
        from pirip_amd import binding
        if name not in binding.SIGNATURES:
            raise AttributeError(name)

        def fn(*args):
            assert len(args) == len(binding.SIGNATURES[name][1]), (name, args)
            self.calls.append((name, args))
            if name == "pirip_hip_strerror":
                return b"stub"
            if name in self.fail:
                return -3
            if "create" in name:
                args[-1]._obj.value = 0x1000 + len(self.calls)
            return 0
        return fn


def test_handle_life_cycle_on_the_common_base(monkeypatch):
    import pirip_amd
    from pirip_amd import binding
    stub = _Stub()
    monkeypatch.setattr(binding, "_lib", stub)
    ld = binding.HipLdpc("no.code", 2, nstreams=4)
    dv = pirip_amd.HipDiversity(ld, 2, 24, 1200, 80, 64)
    assert isinstance(dv.info, binding.DivInfo) and dv.h is not None
    h = dv.h
    dv.collect(11, 13, 15, nframes=17, ncalls=18, status_stride=12, info_stride=14, stats_stride=16, stream=19)
    dv.push_candidates(21, 22, 23, 24, 26, ncand=25, stream=27)
    dv.flush(stream=31)
    assert stub.calls[-3:] == [("pirip_hip_div_collect", (h, 11, 12, 13, 14, 15, 16, 17, 18, 19)),
                               ("pirip_hip_div_push_candidates", (h, 21, 22, 23, 24, 25, 26, 27)), ("pirip_hip_div_flush", (h, 31))]
    with pytest.raises(ValueError):
        dv.collect(11, 13, 15)                                     # raw pointers need the sizes
    dv.close(); dv.close()
    assert dv.h is None and [c for c in stub.calls if c[0] == "pirip_hip_div_destroy"] == [("pirip_hip_div_destroy", (h,))]
    n = len(stub.calls)
    with pytest.raises(pirip_amd.PiripError, match="closed"):
        dv.flush()
    assert len(stub.calls) == n
    ld.close()
    with pytest.raises(pirip_amd.PiripError, match="closed"):
        pirip_amd.HipDiversity(ld, 2, 24, 1200, 80, 64)            # the parent must be open
    stub2 = _Stub(fail=["pirip_hip_div_create"])
    monkeypatch.setattr(binding, "_lib", stub2)
    ld = binding.HipLdpc("no.code", 2, nstreams=4)
    bad = pirip_amd.HipDiversity.__new__(pirip_amd.HipDiversity)
    with pytest.raises(pirip_amd.PiripError, match=r"\(-3\)"):
        bad.__init__(ld, 2, 24, 1200, 80, 64)
    assert bad.h is None
    del bad
    gc.collect()
    assert not [c for c in stub2.calls if c[0] == "pirip_hip_div_destroy"]
