"""tests/streamshapes.py held to the header and the sources, without a GPU: every entry point that takes a hip_stream is called by a
gated test or exempt in the header's own words; every launch on a literal stream and every blocking call under pirip_amd/csrc is listed
with a reason; every family's decoy differs from its real input, and where the family has a host model the model gives another result
on the decoy -- the condition under which tests/test_stream_order.py's comparisons can fail at all."""
import ast
import inspect
import os
import re

import numpy as np
import pytest

import streamshapes as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pirip_amd", "csrc")
HEADERS = [os.path.join(ROOT, "include", n) for n in ("pirip_hip.h", "pirip_hip_rccl.h")]


# ---------------------------------------------------------------- the header
def _strip_comments(text):
    """comments replaced by blanks, line structure kept"""
    text = re.sub(r"/\*.*?\*/", lambda m: re.sub(r"[^\n]", " ", m.group(0)), text, flags=re.S)
    return re.sub(r"//[^\n]*", lambda m: " " * len(m.group(0)), text)


def stream_entry_points(text):
    """names of the declared functions with a `void *hip_stream` parameter"""
    out = []
    for m in re.finditer(r"\b(pirip_hip_\w+)\s*\(([^;{}]*?)\)\s*;", _strip_comments(text), flags=re.S):
        if re.search(r"\bvoid\s*\*\s*hip_stream\b", m.group(2)):
            out.append(m.group(1))
    return out


def _header_text():
    return "\n".join(open(h).read() for h in HEADERS)


def _words(text):
    """a comment's words: line breaks, comment stars and runs of blanks are one blank"""
    return re.sub(r"[\s*]+", " ", text)


def test_parser_on_synthetic_declarations():
    text = """/* int pirip_hip_in_a_comment(void *hip_stream); */
    int pirip_hip_one(pirip_hip_x *h, const uint8_t *d, size_t n,
                      void *hip_stream);
    int pirip_hip_two(pirip_hip_x *h, int hip_streams);       // void *hip_stream in a line comment
    int64_t pirip_hip_three(void* hip_stream);
    int pirip_hip_four(const pirip_hip_x *h);"""
    assert stream_entry_points(text) == ["pirip_hip_one", "pirip_hip_three"]


def test_entry_points_are_the_headers():
    declared = stream_entry_points(_header_text())
    assert len(declared) == len(set(declared)) and len(declared) > 50
    assert sorted(ss.ENTRY_POINTS) == sorted(declared), (sorted(set(declared) - set(ss.ENTRY_POINTS)), sorted(set(ss.ENTRY_POINTS) - set(declared)))


def _test_functions():
    tree = ast.parse(open(os.path.join(ROOT, "tests", "test_stream_order.py")).read())
    return {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}


def _family_calls(fam):
    return set(ss.FAMILIES[fam]["sequence"]) | set(ss.FAMILIES[fam]["reset"])


def test_every_entry_point_has_a_gated_test_or_the_headers_word():
    have = _test_functions()
    header = _words(_header_text())
    for name, (kind, what) in ss.ENTRY_POINTS.items():
        assert kind in ("test", "exempt"), name
        if kind == "test":
            assert what.startswith(ss.T), name
            fn = what[len(ss.T):]
            assert fn in have, (name, fn)
            m = re.fullmatch(r"test_(\w+)_gated", fn)
            assert m and m.group(1) in ss.FAMILIES, (name, fn)
            assert name in _family_calls(m.group(1)), f"{fn}'s family does not call {name}"
        else:
            quotes = re.findall(r'"([^"]+)"', what)
            if what.startswith("the header:"):
                assert quotes, name
            for q in quotes:
                assert _words(q) in header, (name, q)
            assert quotes or len(what.split()) > 12, f"{name}: an exemption without the header's words needs a sentence"


def test_families_are_whole():
    have = _test_functions()
    for fam, f in ss.FAMILIES.items():
        assert "test_%s_gated" % fam in have and "test_%s_pairs" % fam in have, fam
        assert 3 <= len(f["sequence"]) <= 9, fam
        for name in _family_calls(fam):
            assert name in ss.ENTRY_POINTS and ss.ENTRY_POINTS[name][0] == "test", (fam, name)
        assert f["decoy"] and f["handles"], fam
        assert f["gate_ms"] >= 4 * f["enqueue_ms"] > 0, (fam, f["gate_ms"], f["enqueue_ms"])
    assert "test_gate_catches_a_step_on_another_stream" in have
    # every handle the contract is stated for appears in a family
    named = " ".join(f["handles"] for f in ss.FAMILIES.values())
    for h in ("HipRx", "HipChan", "HipDecim", "HipMux", "HipTx", "HipTxStream", "HipTestBits", "HipRepeater", "HipPing", "HipAir", "HipSpectrum",
              "HipDiversity", "HipPacket", "HipPacketFec", "HipArq", "HipMac", "HipDemod", "HipLdpc"):
        assert re.search(r"\b%s\b" % h, named), h


# ---------------------------------------------------------------- the sources
STREAM_ARG = {"hipLaunchKernelGGL": 4, "hipMemsetAsync": 3, "hipMemcpyAsync": 4, "hipMemcpy2DAsync": 7, "hipMemcpyToSymbolAsync": 5}
BLOCKING_CALLS = ("hipMemcpy", "hipMemset", "hipMemcpyToSymbol", "hipDeviceSynchronize", "hipStreamSynchronize")
LITERALS = ("0", "nullptr", "NULL")


def call_args(text, at):
    """the arguments of the call whose opening parenthesis is text[at], split at the commas of its own level -- what the preprocessor
    takes a macro's arguments to be: (kernel<A, B>) in parentheses is one argument"""
    depth, args, start = 0, [], at + 1
    for i in range(at, len(text)):
        ch = text[i]
        if ch in "([{":
            depth += 1
        elif ch in ")]}":
            depth -= 1
            if depth == 0:
                args.append(text[start:i].strip())
                return args
        elif ch == "," and depth == 1:
            args.append(text[start:i].strip())
            start = i + 1
    raise ValueError("unbalanced call")


def literal_stream_lines(text):
    """line numbers (from 0) of the calls of STREAM_ARG whose stream argument is a literal"""
    code = _strip_comments(text)
    out = []
    for m in re.finditer(r"\b(%s)\s*\(" % "|".join(STREAM_ARG), code):
        args = call_args(code, m.end() - 1)
        at = STREAM_ARG[m.group(1)]
        assert len(args) > at, (m.group(1), args)
        if re.sub(r"^\(\s*hipStream_t\s*\)\s*", "", args[at]) in LITERALS:
            out.append(code.count("\n", 0, m.start()))
    return out


def blocking_lines(text):
    """line numbers (from 0), one per occurrence, of the blocking calls -- not of their Async forms, not inside comments"""
    code = _strip_comments(text)
    return [code.count("\n", 0, m.start()) for m in re.finditer(r"\b(%s)\s*\(" % "|".join(BLOCKING_CALLS), code)]


def test_scanners_on_synthetic_lines():
    text = """
    hipLaunchKernelGGL((kernel<A, B,
                        C>), dim3(g, 1), dim3(256),
                       lds_bytes(a, b), stream, args, 0);
    hipLaunchKernelGGL((kernel<A, B>), grid, block, 0,
                       nullptr, a, stream);                 // literal, two lines down from the name
    hipLaunchKernelGGL(k, g, b, 0, 0, x);
    hipLaunchKernelGGL(k, g, b, 0, (hipStream_t)0, x);
    hipLaunchKernelGGL(k, g, b, 0, st, 0, nullptr);         // literals behind the stream are arguments
    PIRIP_HIPCHK(hipMemsetAsync(p, 0, n, st));
    PIRIP_HIPCHK(hipMemsetAsync(p, 0, n, NULL));
    hipMemcpyAsync(d, s, n, hipMemcpyDeviceToDevice, 0);
    hipMemcpy2DAsync(d, dp, s, sp, w, h, hipMemcpyDeviceToDevice, nullptr);
    hipMemcpyToSymbolAsync(HIP_SYMBOL(sym), &v, sizeof(v), 0, hipMemcpyHostToDevice, stream);
    // hipLaunchKernelGGL(k, g, b, 0, 0, x);  hipMemcpy(a, b, n, kind);
    /* hipDeviceSynchronize(); */
    hipMemcpy(a, b, n, kind); hipMemset(a, 0, n);
    (void)hipStreamSynchronize(st);
    my_hipMemcpy(a); hipMemcpyAsync(a, b, n, k, st); hipMemcpyToSymbol(HIP_SYMBOL(s), &v, 4);
    """
    assert literal_stream_lines(text) == [4, 6, 7, 10, 11, 12]
    assert blocking_lines(text) == [16, 16, 17, 18]
    assert call_args("f((k<A, B>), g[1, 2], {3, 4}, x)", 1) == ["(k<A, B>)", "g[1, 2]", "{3, 4}", "x"]


def _sources():
    return sorted(n for n in os.listdir(CSRC) if n.endswith((".hip", ".hpp", ".cpp", ".h")))


def _hold(table, finder, reasons=None):
    """one to one: every occurrence the finder sees is named by exactly one entry (the longest whose text begins the line), every entry
    names as many occurrences as it says"""
    seen = {}
    assert len({(f, s) for f, s, _, _ in table}) == len(table), "an entry twice"
    for name in _sources():
        text = open(os.path.join(CSRC, name)).read()
        lines = text.split("\n")
        for n in finder(text):
            line = lines[n].strip()
            fits = [s for f, s, _, _ in table if f == name and line.startswith(s)]
            assert fits, f"{name}:{n + 1}: not listed in tests/streamshapes.py with a reason: {line[:100]}"
            key = (name, max(fits, key=len))
            seen[key] = seen.get(key, 0) + 1
    for f, s, count, why in table:
        assert seen.get((f, s), 0) == count, f"{f}: {s!r} is listed {count} times and found {seen.get((f, s), 0)} times"
        assert why and (reasons is None or all(w in reasons for w in why.split())), (f, s, why)


def test_literal_streams_are_the_listed_ones():
    _hold(ss.LITERAL_STREAM, literal_stream_lines)


def test_blocking_calls_are_the_listed_ones():
    _hold(ss.BLOCKING, blocking_lines, ss.WHY)


def test_a_new_blocking_call_or_literal_stream_is_seen(tmp_path, monkeypatch):
    """a scratch copy of the sources with one hipMemset( and one launch on stream 0 more fails both checks"""
    import shutil
    scratch = tmp_path / "csrc"
    shutil.copytree(CSRC, scratch, ignore=shutil.ignore_patterns("*.o", "*.so"))
    with open(scratch / "mux_kernels.hip", "a") as f:
        f.write("\nstatic void extra(float *p) { (void)hipMemset(p, 0, 4); hipLaunchKernelGGL(k, dim3(1), dim3(1), 0, 0, p); }\n")
    monkeypatch.setattr(__import__(__name__), "CSRC", str(scratch))
    with pytest.raises(AssertionError, match="not listed"):
        test_blocking_calls_are_the_listed_ones()
    with pytest.raises(AssertionError, match="not listed"):
        test_literal_streams_are_the_listed_ones()
    monkeypatch.setattr(ss, "BLOCKING", ss.BLOCKING[1:])
    monkeypatch.setattr(__import__(__name__), "CSRC", CSRC)
    with pytest.raises(AssertionError, match="not listed"):
        test_blocking_calls_are_the_listed_ones()


# ---------------------------------------------------------------- decoys
def _inputs(fam, seed, oracle):
    fn = ss.FAMILIES[fam]["inputs"]
    return fn(seed, oracle) if "oracle" in inspect.signature(fn).parameters else fn(seed)


@pytest.mark.parametrize("fam", sorted(ss.FAMILIES))
def test_decoys_differ_from_the_real_inputs_and_the_seeds_from_each_other(oracle, built_lib, fam):
    a, b = _inputs(fam, 0, oracle), _inputs(fam, 1, oracle)
    assert a and sorted(a) == sorted(b)
    for name, (real, decoy) in a.items():
        assert real.shape == decoy.shape and real.dtype == decoy.dtype, (fam, name)
        assert not np.array_equal(real, decoy), (fam, name)
    assert any(not np.array_equal(a[k][0], b[k][0]) for k in a), fam


def _variant(inputs, decoy):
    return {k: v[1 if decoy else 0] for k, v in inputs.items()}


def _rows(status, payload, ncalls):
    return [(status[c, :ncalls[c]], payload[c, :ncalls[c]]) for c in range(status.shape[0])]


def _model_tx(x, oracle):
    import txref
    t = ss.TX
    return [txref.repeater_replay(x["status"][s], x["payload"][s], t["source"]).tobytes() for s in range(len(t["f1"]))] + [x["nrec"].tobytes()]


def _model_txs(x, oracle):
    import txsref
    sh = txsref.SHAPES[ss.TXS["shape"]]
    lens = txsref.record_lens(ss.TXS["plan"], 50 * (sh["M"] // 2), 32 + txsref.CODE_N, txsref.GAP_SYMS)
    K = len(sh["f1"])
    m = txsref.Model(K, ss.TXS["S"], sum(lens) + ss.TXS["S"] + 3)
    out = []
    for step in ("S0", "P", "P", "S1", "P", "P"):
        if step[0] == "S":
            i = int(step[1])
            offers = [None if x["nrec"][i, c] == 0 else (x["records"][i, c, :, 1].repeat(200)[:sum(lens)], np.zeros(sum(lens), np.int8),
                                                        np.zeros(sum(lens), np.int64)) for c in range(K)]
            out.append(m.send(offers).tobytes())
        else:
            out.append(m.process().tobytes())
    return out


def _model_tbits(x, oracle):
    import pirip_amd
    import tbitsref
    import tbitsshapes as ts
    rows = np.concatenate([x["rows"], np.unpackbits(x["packed"], axis=-1)[..., :ts.SYN["row_bits"]]], axis=1)
    nf = x["nframes"] + x["nframes_packed"]
    got = tbitsref.count_streams(rows, list(nf), ts.default_frame(), ts.SYN["thresh"])
    tally = tbitsref.record_tally(x["status"], x["payload"], x["info"], x["ncalls"], pirip_amd.testframe_payload(8 * ts.REC_DB))
    return [got[k].tobytes() for k in tbitsref.NAMES] + [tally[k].tobytes() for k in tbitsref.REC_NAMES]


def _model_spec(x, oracle):
    import specref
    nfft, hop, fmt, avg = ss.SPEC["case"]
    return [specref.rows(x["iq"][0], specref.U8, nfft, hop, avg).tobytes()]


def _model_chan(x, oracle):
    import chanref
    import muxshapes as ms
    from test_channelizer_cpu import _taps
    return [chanref.channel(x["iq"][0], _taps(ss.CHAN["D"]), ss.CHAN["D"], ss.CHAN["Fs"], ms.LOOP["offsets"][0], ss.CHAN["t0"][0]).tobytes()]


def _model_mux(x, oracle):
    import muxref
    import muxshapes as ms
    Fs, D, tbw, offsets, outputs, noutputs, branch, _ = ms.SHAPES[ss.MUX["shape"]]
    z = x["z"][0]
    _, g = ms.inputs(ss.MUX["shape"], z.shape[1])
    return [muxref.mux(z[:2], muxref.linear_taps(D), D, Fs, offsets[:2], g[:2], ss.MUX["m0"][0]).tobytes()]


def _model_air(x, oracle):
    import airref
    import airshapes as sh
    _, paths = sh.inputs(ss.AIR["Fs"], "u8", seed=0)
    xw = airref.widen(x["iq"][:, :600], airref.U8)
    return [airref.receive(xw, ss.AIR["Fs"], paths, 2, ss.AIR["n0"]).tobytes()]


def _model_pkt(x, oracle):
    import pktref
    m = pktref.run_rows([_rows(x["status"], x["payload"], x["ncalls"])], filt=ss.LINK["own"], address=ss.LINK["own"], max_frags=ss.LINK["max_frags"])
    return [m.counters()[k].tobytes() for k in pktref.RX_COUNTERS] + [x["lengths"].tobytes()]


def _model_fec(x, oracle):
    import pktfecref as fr
    import pktref
    m = fr.run_rows([_rows(x["status"], x["payload"], x["ncalls"])], fr.SHAPES[ss.FEC_SHAPE], filt=ss.LINK["own"], address=ss.LINK["own"])
    return [m.counters()[k].tobytes() for k in pktref.RX_COUNTERS] + [m.fec_counters()[k].tobytes() for k in fr.FEC_COUNTERS] + [x["lengths"].tobytes()]


def _model_arq(x, oracle):
    nd = ss.arq_node()
    nd.submit([[x["segments"][c, j, :x["lengths"][c, j]].tobytes() for j in range(x["nseg"][c])] for c in range(4)])
    for k in range(ss.ARQ["calls"]):
        nd.call(_rows(x["status"][k], x["payload"][k], x["ncalls"][k]))
    return nd.counters()


def _model_mac(x, oracle):
    import macref as m
    out = []
    for mask in ss.MAC["masks"]:
        term = m.terminal(mac=dict(cw=ss.MAC["cw"], sense_mask=mask, sense_snr=m.SNR_T, key=7))
        term.link.send([[(x["raw"][c, 0, :x["lengths"][c, 0]].tobytes(), m.ADDR)] if x["lengths"][c, 0] else [] for c in range(4)])
        for k in range(ss.MAC["calls"]):
            rows = _rows(x["status"][k], x["payload"][k], x["ncalls"][k])
            term.call(rows, [x["stats"][k, c, :x["ncalls"][k, c]] for c in range(4)])
        out.append(term.mac.counters())
    return out


def _model_rpt(x, oracle):
    import txref
    return [txref.repeater_replay(x["status"][c, :x["ncalls"][c]], x["payload"][c, :x["ncalls"][c]], 2).tobytes() for c in range(4)]


def _model_ping(x, oracle):
    import pingref
    import pirip_amd
    rows = [(x["status"][c, :x["ncalls"][c]], x["payload"][c, :x["ncalls"][c]], x["info"][c, :x["ncalls"][c]], x["stats"][c, :x["ncalls"][c]])
            for c in range(4)]
    m = pingref.run_log([rows], pirip_amd.testframe_payload(8 * pingref.KB))
    return [m.counters()[k].tobytes() for k in pingref.RX_COUNTERS]


def _model_div(x, oracle):
    import divref
    llr = x["llr"].view(np.float16)
    return [np.asarray(divref.combine([llr[0], llr[1]])).tobytes()]


MODELS = dict(tx=_model_tx, txs=_model_txs, tbits=_model_tbits, spec=_model_spec, chan=_model_chan, mux=_model_mux, air=_model_air, pkt=_model_pkt,
              fec=_model_fec, arq=_model_arq, mac=_model_mac, rpt=_model_rpt, ping=_model_ping, div=_model_div)


def _flat(v):
    if isinstance(v, dict):
        return [np.asarray(v[k]).tobytes() for k in sorted(v)]
    if isinstance(v, (list, tuple)):
        return [b for e in v for b in _flat(e)]
    return [v]


@pytest.mark.parametrize("fam", sorted(MODELS))
def test_the_host_model_tells_the_decoy_from_the_real_input(oracle, built_lib, fam):
    x = _inputs(fam, 0, oracle)
    x = {k: v for k, v in x.items() if k != "records" or fam in ("tx", "txs")}
    real, decoy = _flat(MODELS[fam](_variant(x, False), oracle)), _flat(MODELS[fam](_variant(x, True), oracle))
    assert len(real) == len(decoy) and real != decoy, fam


def test_the_arq_sequence_retransmits_and_is_acknowledged_in_the_model():
    x = _variant(ss.arq_inputs(0), False)
    c = _model_arq(x, None)
    for k in ("sent", "retransmitted", "acked", "acks_sent", "delivered"):
        assert c[k][0] > 0, k


def test_the_mac_sequence_senses_and_sends_in_the_model():
    for c in _model_mac(_variant(ss.mac_inputs(0), False), None):
        assert c["carrier"].sum() > 0 and c["bursts"].sum() > 0, c
