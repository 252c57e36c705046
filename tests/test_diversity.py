"""The diversity receiver on the device (include/pirip_hip.h section Q) against tests/divref.py, the model in numpy:

  1. exact against the reference on the device's own branch outputs, fused and unfused receive chains, once per decoder;
  2. cut independence: the same soft decisions in one call, in calls of 1 and 7 rows and with ragged row counts, and through the
     streaming receiver with two block sizes -- the rings are byte-identical;
  3. special values and the closure rule's edges through push_candidates (tests/divshapes.py: SPECIAL, SINGLE, BOUNDARY);
  4. a cluster of one equals the branch's own record;
  5. end to end: one HipTx burst through HipAir's independent fades onto two groups of two receivers, against the reference;
  6. life cycle: a collect without a fresh batch, reset, two handles on two HIP streams, no candidate dropped.
G = 2 groups throughout; B = 2 and B = 3."""
import os

import numpy as np
import pytest

import divref
import divshapes
import ldpcshapes
import sigutil

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODE = os.path.join(ROOT, "pirip_amd", "data", "standin_256_512_4.code")
BAD_ARG = r"\(-1\)"
SKEW = 80


def _crc_bits(data):
    """the last 16 data bits: CRC-16/CCITT-FALSE of the bytes before them (ldpcshapes.stream_recording's framing)"""
    crc = 0xFFFF
    for byte in np.packbits(data[:-16]):
        x = ((crc >> 8) ^ int(byte)) & 0xFF
        x ^= x >> 4
        crc = ((crc << 8) ^ (x << 12) ^ (x << 5) ^ x) & 0xFFFF
    data[-16:] = [(crc >> (15 - i)) & 1 for i in range(16)]


def _shape(oracle, tmp_path, M, Nsym, n, k, frames, seed):
    """code (the oracle's dict), its file, the modem configuration and one burst's bits (50 preamble bits, then frames)"""
    cfg = dict(sigutil.CFG1 if M == 2 else sigutil.CFG4, P=6 if M == 2 else 8)
    rng = np.random.default_rng(seed)
    if (n, k) == (512, 256):
        code, path = oracle.parse_code_file(CODE), CODE
    else:
        path = str(tmp_path / ("ra_%d_%d.code" % (n, k)))
        ldpcshapes._write_random_code(path, n, k, 3, 77 + n)
        code = oracle.parse_code_file(path)
    data = rng.integers(0, 2, (frames, k)).astype(np.uint8)
    for d in data:
        _crc_bits(d)
    cw = ldpcshapes.ra_encode(code["rows"], k, data)
    assert not (ldpcshapes.dense_h(code["rows"], n).astype(np.int64) @ cw.T.astype(np.int64) & 1).any()
    bits = np.concatenate([np.tile(np.array([0, 1], dtype=np.uint8), 25)] + [np.concatenate([np.array(ldpcshapes.UW, dtype=np.uint8), c]) for c in cw])
    if M == 4 and bits.size % 2:
        bits = np.concatenate([bits, np.zeros(1, dtype=np.uint8)])
    return dict(code=code, path=path, cfg=cfg, M=M, Nsym=Nsym, n=n, k=k, bits=bits, Ts=cfg["Fs"] // cfg["Rs"], bps=1 if M == 2 else 2,
                Nbits=Nsym * (1 if M == 2 else 2), per=M * Nsym, kb=k // 8)


def _inputs(oracle, S, G, B, ebno, seed, silent=()):
    """u8 IQ [G B, nsamp, 2]: every group its own transmission, every branch its own delay (no whole symbol) and noise"""
    delays = [0, 37, 13, 61, 29, 50, 7, 44][:B]
    out = []
    for g in range(G):
        out += divshapes.branch_copies(oracle, S["cfg"], S["M"], [S["bits"]] * 2, ebno, seed + 10 * g, delays, silence=3000)
    n = min(len(x) for x in out)
    u8 = np.stack([x[:n] for x in out])
    for r in silent:
        u8[r] = 127
    return u8


class _Rows:
    """the device buffers of one receive call of R receivers and max_frames rows"""
    def __init__(self, torch, pirip_amd, R, maxf, kb, per=0):
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
        self.status, self.payload = z((R, maxf), torch.uint8), z((R, maxf, kb), torch.uint8)
        self.info, self.stats = z((R, maxf, pirip_amd.LDPC_INFO_PER_CALL), torch.int32), z((R, maxf, pirip_amd.STATS_PER_FRAME), torch.float32)
        self.nframes, self.consumed = z((R,), torch.int32), z((R,), torch.int64)
        self.filt = z((R, maxf, per), torch.float32) if per else None
        self.maxf = maxf

    def host(self):
        return dict(status=self.status.cpu().numpy(), payload=self.payload.cpu().numpy(), info=self.info.cpu().numpy(),
                    stats=self.stats.cpu().numpy(), nframes=self.nframes.cpu().numpy(), filt=None if self.filt is None else self.filt.cpu().numpy())


def _demod(pirip_amd, S, R):
    c = S["cfg"]
    return pirip_amd.HipDemod(c["Fs"], c["Rs"], S["M"], P=c["P"], Nsym=S["Nsym"], est_min=500, est_max=c["est_max"], in_format=pirip_amd.IN_CU8_CSDR,
                              nstreams=R)


def _receive(torch, pirip_amd, S, u8, chain, B, log_entries=64):
    """one receive call over the whole input, then collect: (handles, rows, diversity handle). chain: pirip_hip_fsk_ldpc_rx_batch; else
    pirip_hip_demod_batch + pirip_hip_ldpc_rx_batch, which keeps the magnitudes"""
    R, nsamp = u8.shape[0], u8.shape[1]
    d_in = torch.from_numpy(u8).cuda()
    dem = _demod(pirip_amd, S, R)
    maxf = dem.max_frames_for(nsamp)
    ld = pirip_amd.HipLdpc(S["path"], S["M"], Nsym=S["Nsym"], nstreams=R)
    rows = _Rows(torch, pirip_amd, R, maxf, S["kb"], 0 if chain else S["per"])
    dv = pirip_amd.HipDiversity(ld, B, S["Ts"], dem.N, SKEW, maxf, log_entries=log_entries)
    if chain:
        ld.chain_batch(dem, d_in.data_ptr(), nsamp * 2, nsamp, rows.status.data_ptr(), rows.payload.data_ptr(), rows.info.data_ptr(),
                       rows.nframes.data_ptr(), rows.consumed.data_ptr(), maxf, rows.stats.data_ptr(), maxf * pirip_amd.STATS_PER_FRAME)
    else:
        dem.demod_batch(d_in.data_ptr(), nsamp * 2, nsamp, 0, 0, rows.filt.data_ptr(), maxf * S["per"], rows.stats.data_ptr(),
                        maxf * pirip_amd.STATS_PER_FRAME, rows.nframes.data_ptr(), rows.consumed.data_ptr(), maxf)
        ld.rx_batch(rows.filt.data_ptr(), maxf * S["per"], rows.nframes.data_ptr(), maxf, rows.status.data_ptr(), rows.payload.data_ptr(),
                    rows.info.data_ptr())
    dv.collect(rows.status, rows.info, rows.stats, nframes=rows.nframes, stream=0)
    torch.cuda.synchronize()
    return (dem, ld), rows, dv


def _capacity(B, max_rows, S):
    return B * (3 * (max_rows * S["Nbits"] // (32 + S["n"]) + 2) + 2)


def _reference(oracle, S, G, B, h, nin0, max_rows):
    """one DivRef per group fed with the device's own rows (host dict h) as one call; returns the refs and what that call emitted"""
    refs, first = [], []
    for g in range(G):
        ref = divref.DivRef(B, S["bps"], S["Ts"], S["n"], S["Nbits"], nin0, SKEW, divref.oracle_decoder(oracle.OracleLdpc(S["code"], S["M"], S["Nsym"])),
                            pending_capacity=_capacity(B, max_rows, S))
        for b in range(B):
            r, nf = g * B + b, int(h["nframes"][g * B + b])
            llr = oracle.OracleLdpc(S["code"], S["M"], S["Nsym"]).llr(h["filt"][r, :nf]) if nf else np.zeros((0, S["Nbits"]), dtype=np.float32)
            divshapes.feed_rows(ref, b, dict(llr=llr, info=h["info"][r, :nf], status=h["status"][r, :nf], stats=h["stats"][r, :nf]))
        first.append(len(ref.close()))
        refs.append(ref)
    return refs, first


def _check_against(dv, refs, first, G, log_entries=64):
    """collect's clusters, then the flush's: entries, payloads, combined soft bits and counters, field for field and word for word"""
    import torch
    for g in range(G):
        for slot in range(first[g]):
            assert divshapes.same_f16(dv.combined(g, slot), refs[g].combined[slot]), (g, slot)
    dv.flush(stream=0)
    torch.cuda.synchronize()
    cnt = dv.counters()
    for g in range(G):
        tail = refs[g].flush()
        for slot in range(len(tail)):
            assert divshapes.same_f16(dv.combined(g, slot), refs[g].combined[first[g] + slot]), (g, "flush", slot)
        e, p = dv.log(g)
        msg = divref.entries_equal(e, p, refs[g].entries[-log_entries:])
        assert msg is None, (g, msg)
        want = refs[g].counters(log_entries)
        assert {k: int(cnt[k][g]) for k in want} == want, g
    return cnt


SHAPES = divshapes.DEVICE_SHAPES               # (M, Nsym, n, k, B)


@pytest.mark.parametrize("decoder", ["generic", "fast", "bank"])
@pytest.mark.parametrize("M,Nsym,n,k,B", SHAPES)
def test_exact_against_the_reference_on_the_devices_branch_outputs(oracle, built_lib, tmp_path, monkeypatch, M, Nsym, n, k, B, decoder):
    import torch
    import pirip_amd
    monkeypatch.setenv("PIRIP_LDPC_DECODER", decoder)
    G = 2
    S = _shape(oracle, tmp_path, M, Nsym, n, k, frames=4 if n == 512 else 12, seed=n + Nsym)
    u8 = _inputs(oracle, S, G, B, 5.0 if M == 2 else 5.5, seed=3 + M)
    # the chain as a caller runs it (fused where the shape has a fused instance) ...
    (dem_a, ld_a), rows_a, dv_a = _receive(torch, pirip_amd, S, u8, True, B)
    # ... and on the same soft decisions with the magnitudes kept, which the reference reads
    (dem_b, ld_b), rows_b, dv_b = _receive(torch, pirip_amd, S, u8, False, B)
    ha, hb = rows_a.host(), rows_b.host()
    for key in ("status", "payload", "info", "stats", "nframes"):
        assert np.array_equal(ha[key], hb[key]), key
    refs, first = _reference(oracle, S, G, B, hb, dem_b.N, rows_b.maxf)
    ncand = sum(len(r.entries) + len(r.pending) for r in refs)
    assert ncand >= 4 * G, "the input gives the branches nothing to combine"
    assert max(int((hb["info"][r, :, 6] >= 0).sum()) for r in range(G * B)) > 1              # several jobs per receiver and call
    for dv in (dv_b, dv_a):
        cnt = _check_against(dv, [divref_copy(r) for r in refs], first, G)
    print("fused" if ld_a.last_path_fused() else "unfused", {k: v.tolist() for k, v in cnt.items()})
    assert not cnt["dropped"].any()


def divref_copy(ref):
    import copy
    c = copy.copy(ref)
    c.pending, c.entries, c.combined = list(ref.pending), list(ref.entries), list(ref.combined)
    return c


def _cut_run(torch, pirip_amd, S, G, B, h, nin0, cuts, max_rows):
    """the rows of host dict h (magnitudes and stats of every receiver) through pirip_hip_ldpc_rx_batch + collect call by call; cuts: per
    call the valid rows per receiver. Returns the groups' logs as bytes and the counters."""
    R = G * B
    ld = pirip_amd.HipLdpc(S["path"], S["M"], Nsym=S["Nsym"], nstreams=R)
    dv = pirip_amd.HipDiversity(ld, B, S["Ts"], nin0, SKEW, max_rows, log_entries=64)
    at = [0] * R
    for valid in cuts:
        nc = max(max(valid), 1)
        rows = _Rows(torch, pirip_amd, R, nc, S["kb"], S["per"])
        filt, stats = np.full((R, nc, S["per"]), 123.0, dtype=np.float32), np.zeros((R, nc, 10), dtype=np.float32)
        for r in range(R):
            v = valid[r]
            filt[r, :v], stats[r, :v] = h["filt"][r, at[r]:at[r] + v], h["stats"][r, at[r]:at[r] + v]
            at[r] += v
        rows.filt.copy_(torch.from_numpy(filt)); rows.stats.copy_(torch.from_numpy(stats))
        rows.nframes.copy_(torch.from_numpy(np.array(valid, dtype=np.int32)))
        ld.rx_batch(rows.filt.data_ptr(), nc * S["per"], rows.nframes.data_ptr(), nc, rows.status.data_ptr(), rows.payload.data_ptr(), rows.info.data_ptr())
        dv.collect(rows.status, rows.info, rows.stats, nframes=rows.nframes, stream=0)
        torch.cuda.synchronize()
    assert at == [int(x) for x in h["nframes"]]
    dv.flush(stream=0)
    torch.cuda.synchronize()
    logs = [dv.log(g) for g in range(G)]
    return [(e.tobytes(), p.tobytes()) for e, p in logs], dv.counters()


def _cuts(nframes, size, ragged=False):
    left, out, call = [int(x) for x in nframes], [], 0
    while any(left):
        valid = [min(l, size - ((r + call) % 3 if ragged else 0)) for r, l in enumerate(left)]
        left = [l - v for l, v in zip(left, valid)]
        out.append(valid); call += 1
    return out


@pytest.mark.parametrize("M,Nsym,n,k,B", [SHAPES[0], SHAPES[4]])
def test_rings_do_not_depend_on_the_cutting_into_calls(oracle, built_lib, tmp_path, M, Nsym, n, k, B):
    import torch
    import pirip_amd
    G = 2
    S = _shape(oracle, tmp_path, M, Nsym, n, k, frames=3 if n == 512 else 10, seed=n)
    u8 = _inputs(oracle, S, G, B, 5.0, seed=11)
    (dem, _), rows, dv0 = _receive(torch, pirip_amd, S, u8, False, B)
    h = rows.host()
    nf = h["nframes"]
    whole, cw = _cut_run(torch, pirip_amd, S, G, B, h, dem.N, [[int(x) for x in nf]], int(nf.max()))
    assert cw["clusters"].min() >= 3
    for name, cuts, mr in (("1 row", _cuts(nf, 1), 1), ("7 rows", _cuts(nf, 7), 7), ("ragged", _cuts(nf, 7, True), 7)):
        got, c = _cut_run(torch, pirip_amd, S, G, B, h, dem.N, cuts, mr)
        assert got == whole, name
        assert all(np.array_equal(c[key], cw[key]) for key in cw), name
        assert not c["dropped"].any()


def test_rings_do_not_depend_on_the_streaming_receivers_block_size(oracle, built_lib, tmp_path):
    import torch
    import pirip_amd
    G, B = 2, 2
    S = _shape(oracle, tmp_path, 2, 50, 512, 256, frames=3, seed=5)
    u8 = _inputs(oracle, S, G, B, 5.0, seed=21)
    n = (u8.shape[1] // 12000) * 12000
    d_in = torch.from_numpy(np.ascontiguousarray(u8[:, :n])).cuda()
    out = []
    for block in (4000, 12000):
        dem = _demod(pirip_amd, S, G * B)
        ld = pirip_amd.HipLdpc(S["path"], 2, nstreams=G * B)
        rx = pirip_amd.HipRx(dem, ldpc=ld, block=block)
        rows = _Rows(torch, pirip_amd, G * B, rx.max_frames, S["kb"])
        dv = pirip_amd.HipDiversity(ld, B, S["Ts"], dem.N, SKEW, rx.max_frames, log_entries=64)
        for i in range(n // block):
            rx.push(d_in.data_ptr() + i * block * 2, n * 2, d_status=rows.status.data_ptr(), d_payload=rows.payload.data_ptr(), d_info=rows.info.data_ptr(),
                    d_stats=rows.stats.data_ptr(), stats_stride=rx.max_frames * pirip_amd.STATS_PER_FRAME, d_nframes=rows.nframes.data_ptr())
            dv.collect(rows.status, rows.info, rows.stats, nframes=rows.nframes, stream=0)
        dv.flush(stream=0)
        torch.cuda.synchronize()
        c = dv.counters()
        assert not c["dropped"].any() and c["clusters"].min() >= 3
        out.append([(e.tobytes(), p.tobytes()) for e, p in (dv.log(g) for g in range(G))])
    assert out[0] == out[1]


# ---------------------------------------------------------------- push_candidates: values and tags under exact control

def _push(torch, dv, cands, H, back, n, R):
    """cands: (llr value or row, tau, receiver); every branch's clock at its group's H + 2 bpf Ts (H: one horizon, or one per group)"""
    Hs = list(H) if isinstance(H, (list, tuple)) else [H]
    units = [Hs[r * len(Hs) // R] + back for r in range(R)]
    llr = np.stack([np.broadcast_to(np.asarray(v, dtype=np.float16), (n,)) for v, _, _ in cands]) if cands else np.zeros((0, n), dtype=np.float16)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.array(a, dtype=dt))).cuda()
    bufs = (torch.from_numpy(np.ascontiguousarray(llr).view(np.int16)).cuda(), t([c[1] for c in cands], np.int64), t([c[2] for c in cands], np.int32),
            t([0] * len(cands), np.uint8), t(units, np.int64))
    dv.push_candidates(bufs[0] if cands else 0, bufs[1] if cands else 0, bufs[2] if cands else 0, bufs[3] if cands else 0, bufs[4], ncand=len(cands), stream=0)
    torch.cuda.synchronize()


def test_special_values_and_the_rules_edges_through_push_candidates(oracle, built_lib):
    import torch
    import pirip_amd
    G, B, n, Ts = 2, 8, 512, 8
    ld = pirip_amd.HipLdpc(CODE, 2, nstreams=G * B)
    back = 2 * 544 * Ts
    with pytest.raises(pirip_amd.PiripError, match=BAD_ARG):
        pirip_amd.HipDiversity(ld, B, Ts, 400, 544 * Ts // 2, 8)            # K = bpf Ts / 2 is refused, one below is not
    pirip_amd.HipDiversity(ld, B, Ts, 400, 544 * Ts // 2 - 1, 8).close()
    for bad in (1, 9, 3):                                                    # branches outside 2 .. 8, or no divisor of 16 receivers
        with pytest.raises(pirip_amd.PiripError, match=BAD_ARG):
            pirip_amd.HipDiversity(ld, bad, Ts, 400, 10, 8)
    dv = pirip_amd.HipDiversity(ld, B, Ts, 400, 100, 8, log_entries=64)
    # sums: case i in group i % 2, one position of the word per case would do -- every position holds the case, so the vector path's
    # eight lanes and the words past lane 0 are held to it as well
    names = sorted(divshapes.SPECIAL)
    for i, name in enumerate(names):
        vals, want = divshapes.SPECIAL[name]
        g = i % 2
        _push(torch, dv, [(v, 5000 * (i + 1), g * B + b) for b, v in enumerate(vals)], 10 ** 9, back, n, G * B)
        assert divshapes.same_f16(dv.combined(g, 0), np.full(n, want, dtype=np.float16)), name
        assert divshapes.same_f16(dv.combined(g, 0), divref.combine([np.full(n, v, dtype=np.float16) for v in vals])), name
        e, _ = dv.log(g)
        assert int(e[-1]["members"]) == (1 << len(vals)) - 1 and int(e[-1]["t_samples"]) == 5000 * (i + 1), name
    # a word of its own in every position, summed over all eight branches in ascending order: the reference's float32 walk
    rng = np.random.default_rng(8)
    words = (rng.normal(0, 6, (B, n)) * 2.0 ** rng.integers(-6, 7, (B, n))).astype(np.float16)
    words[rng.random((B, n)) < 0.02] = np.float16(np.nan)
    words[rng.random((B, n)) < 0.02] = np.float16(np.inf)
    words[rng.random((B, n)) < 0.02] = np.float16(-np.inf)
    _push(torch, dv, [(words[b], 10 ** 6, 1 * B + (B - 1 - b)) for b in range(B)], 10 ** 9, back, n, G * B)       # pushed in descending branch order
    assert divshapes.same_f16(dv.combined(1, 0), divref.combine([words[B - 1 - b] for b in range(B)]))
    # a single member reproduces its input
    single = np.resize(np.array(divshapes.SINGLE, dtype=np.float16), n)
    _push(torch, dv, [(single, 2 * 10 ** 6, 3)], 10 ** 9, back, n, G * B)
    assert divshapes.same_f16(dv.combined(0, 0), single)
    # the closure rule's edges, both groups at once: group 1 gets the case shifted by 7 units so that a slip between groups shows
    for K in (100, 0):
        dk = pirip_amd.HipDiversity(ld, B, Ts, 400, K, 8, log_entries=64)
        for name in sorted(divshapes.BOUNDARY):
            k, cands, H, want_call, want_flush = divshapes.BOUNDARY[name]
            if k != K:
                continue
            dk.reset(stream=0)
            push = [(2.0 ** i, tau + 7 * g, g * B + b) for g in range(G) for i, (tau, b) in enumerate(cands)]
            _push(torch, dk, push, [H, H + 7], back, n, G * B)             # (every group has its own horizon: its branches' clocks)
            for g in range(G):
                e, _ = dk.log(g)
                assert len(e) == len(want_call), (name, g)
                for slot, idx in enumerate(want_call):
                    assert float(dk.combined(g, slot)[0]) == sum(2.0 ** i for i in idx), (name, g, slot)
                    assert int(e[slot]["members"]) == sum(1 << cands[i][1] for i in idx)
                    assert int(e[slot]["t_samples"]) == min((cands[i][0], cands[i][1]) for i in idx)[0] + 7 * g
            dk.flush(stream=0)
            torch.cuda.synchronize()
            for g in range(G):
                e, _ = dk.log(g)
                assert len(e) == len(want_call) + len(want_flush), (name, g)
                for slot, idx in enumerate(want_flush):
                    assert float(dk.combined(g, slot)[0]) == sum(2.0 ** i for i in idx), (name, g, slot)
            assert not dk.counters()["dropped"].any()


def test_a_cluster_of_one_equals_the_branchs_own_record(oracle, built_lib, tmp_path):
    import torch
    import pirip_amd
    G, B = 2, 2
    S = _shape(oracle, tmp_path, 2, 50, 512, 256, frames=4, seed=9)
    u8 = _inputs(oracle, S, G, B, 7.0, seed=31, silent=(3,))              # group 1's second branch hears silence
    _, rows, dv = _receive(torch, pirip_amd, S, u8, True, B)
    dv.flush(stream=0)
    torch.cuda.synchronize()
    h = rows.host()
    e, p = dv.log(1)
    own = [f for f in range(int(h["nframes"][2])) if h["info"][2, f, 6] >= 0]
    assert int((h["info"][3, :, 6] >= 0).sum()) == 0 and len(own) >= 4 and len(e) == len(own)
    for i, f in enumerate(own):
        assert int(e[i]["members"]) == 1 and int(e[i]["solo_ok"]) == (1 if h["status"][2, f] & 4 else 0)
        assert np.array_equal(p[i], h["payload"][2, f])
        assert (int(e[i]["iters"]), int(e[i]["pcc"]), int(e[i]["eraw"]), int(e[i]["status"])) == \
               (int(h["info"][2, f, 4]), int(h["info"][2, f, 5]), int(h["info"][2, f, 8]), int(h["status"][2, f]))
    assert (e["status"] & 4).any()


def test_end_to_end_through_the_channels_independent_fades(oracle, built_lib, tmp_path):
    """One HipTx burst -> HipAir, one transmitter onto four receivers (two groups of two branches), every path with its own integer
    delay and its own fade (tests/fadeshapes.py's demodulator row: 20 Hz, Rayleigh and Rician K = 4 in turn, a key per path) and every
    receiver with its own noise -> receive chain -> collect -> flush: equal to the reference on the device's own branch outputs. How
    many frames the combination rescues is printed, not asserted: the device demodulator's soft decisions are not the oracle's."""
    import torch
    import pirip_amd
    import fadeshapes as fs
    G, B, nfr = 2, 2, 6
    S = _shape(oracle, tmp_path, 2, 50, 512, 256, frames=1, seed=0)
    c = S["cfg"]
    tx = pirip_amd.HipTx(CODE, c["Fs"], c["Rs"], 2, nstreams=1, f1=c["f1"], shift=c["shift"], lead=200, gap=700)
    rec = np.zeros((1, nfr + 1, 1 + tx.data_bytes), dtype=np.uint8)
    rec[:, :, 0] = [1] + [0] * (nfr - 1) + [2]
    rec[:, :nfr, 1:] = pirip_amd.testframe_payload(8 * tx.data_bytes)
    rec[0, :nfr, 1], rec[0, :nfr, 2] = 0x21, np.arange(1, nfr + 1)
    nsym = 200 + tx.preamble_syms + nfr * tx.frame_syms + 700
    nsamp = nsym * S["Ts"]
    d_rec = torch.from_numpy(rec).cuda()
    iq = torch.zeros((1, nsamp * 2), dtype=torch.uint8, device="cuda")
    tx.records_to_iq(d_rec.data_ptr(), rec[0].size, nfr + 1, nsym, iq.data_ptr(), nsamp * 2, amp=14.0)       # u8 IQ around 127: the channel reads b / 127.5 - 1
    delays = [0, 37, 13, 61]
    paths = [(r, 0, 1.0, delays[r], 0) for r in range(G * B)]
    fades = [(r, fs.DEMOD_HZ, fs.DEMOD_FADES[r % 2][2], 11 + r) for r in range(G * B)]
    air = pirip_amd.HipAir(c["Fs"], paths, 1, G * B, sigma=0.1, seed=5, fades=fades)
    heard = torch.zeros((G * B, nsamp * 2), dtype=torch.uint8, device="cuda")
    air.push(iq, nsamp * 2, nsamp, heard, nsamp * 2, stream=0)
    torch.cuda.synchronize()
    u8 = heard.cpu().numpy().reshape(G * B, nsamp, 2)
    assert len({u8[r].tobytes() for r in range(G * B)}) == G * B
    (dem_a, ld_a), rows_a, dv_a = _receive(torch, pirip_amd, S, u8, True, B)
    (dem_b, ld_b), rows_b, dv_b = _receive(torch, pirip_amd, S, u8, False, B)
    ha, hb = rows_a.host(), rows_b.host()
    for key in ("status", "payload", "info", "stats", "nframes"):
        assert np.array_equal(ha[key], hb[key]), key
    refs, first = _reference(oracle, S, G, B, hb, dem_b.N, rows_b.maxf)
    solo = [int(((hb["status"][r] & 4) != 0).sum()) for r in range(G * B)]
    assert sum(len(r.entries) + len(r.pending) for r in refs) >= 2 * G, "the channel left the branches nothing to combine"
    for dv in (dv_b, dv_a):
        cnt = _check_against(dv, [divref_copy(r) for r in refs], first, G)
    print("frames sent", nfr, "decoded alone per receiver", solo, {k: v.tolist() for k, v in cnt.items()})
    assert not cnt["dropped"].any()


def test_life_cycle(oracle, built_lib, tmp_path):
    import torch
    import pirip_amd
    G, B = 2, 2
    S = _shape(oracle, tmp_path, 2, 50, 512, 256, frames=3, seed=2)
    u8 = _inputs(oracle, S, G, B, 6.0, seed=41)
    (dem, ld), rows, dv = _receive(torch, pirip_amd, S, u8, True, B)
    with pytest.raises(pirip_amd.PiripError, match=BAD_ARG):                 # no fresh batch behind the last collect
        dv.collect(rows.status, rows.info, rows.stats, nframes=rows.nframes, stream=0)
    dv.flush(stream=0)
    torch.cuda.synchronize()
    first = [(e.tobytes(), p.tobytes()) for e, p in (dv.log(g) for g in range(G))]
    c1 = dv.counters()
    assert c1["clusters"].min() >= 3 and not c1["dropped"].any() and not c1["lost"].any()
    # reset returns to call 0: the same input again gives the same rings
    d_in = torch.from_numpy(u8).cuda()
    nsamp = u8.shape[1]

    def again(dem, ld, dv, rows, stream):
        dem.reset(stream); ld.reset(stream); dv.reset(stream=stream)
        ld.chain_batch(dem, d_in.data_ptr(), nsamp * 2, nsamp, rows.status.data_ptr(), rows.payload.data_ptr(), rows.info.data_ptr(),
                       rows.nframes.data_ptr(), rows.consumed.data_ptr(), rows.maxf, rows.stats.data_ptr(), rows.maxf * pirip_amd.STATS_PER_FRAME, stream)
        dv.collect(rows.status, rows.info, rows.stats, nframes=rows.nframes, stream=stream)
        dv.flush(stream=stream)
    with pytest.raises(pirip_amd.PiripError, match=BAD_ARG):
        dv.reset(stream=0)
        dv.collect(rows.status, rows.info, rows.stats, nframes=rows.nframes, stream=0)          # a reset does not make the old batch fresh
    with pytest.raises(pirip_amd.PiripError, match=BAD_ARG):
        dv.collect(rows.status, rows.info, rows.stats, nframes=rows.nframes, ncalls=rows.maxf + 1, stream=0)
    again(dem, ld, dv, rows, 0)
    torch.cuda.synchronize()
    assert [(e.tobytes(), p.tobytes()) for e, p in (dv.log(g) for g in range(G))] == first
    assert all(np.array_equal(dv.counters()[k], c1[k]) for k in c1)
    # two handles on two HIP streams do not meet
    (dem2, ld2), rows2, dv2 = _receive(torch, pirip_amd, S, u8, True, B)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    for _ in range(2):
        again(dem, ld, dv, rows, s1.cuda_stream)
        again(dem2, ld2, dv2, rows2, s2.cuda_stream)
    torch.cuda.synchronize()
    for d in (dv, dv2):
        assert [(e.tobytes(), p.tobytes()) for e, p in (d.log(g) for g in range(G))] == first
    # a ring shorter than what a call emits keeps the newest entries and counts the rest as lost
    _, _, dv3 = _receive(torch, pirip_amd, S, u8, True, B, log_entries=2)
    dv3.flush(stream=0)
    torch.cuda.synchronize()
    c3 = dv3.counters()
    assert np.array_equal(c3["clusters"], c1["clusters"]) and np.array_equal(c3["lost"], c1["clusters"] - 2)
    for g in range(G):
        e, p = dv3.log(g)
        e1, p1 = dv.log(g)
        assert e.tobytes() == e1[-2:].tobytes() and p.tobytes() == p1[-2:].tobytes()
    last = dv.last()
    assert last["entries"] and last["payload"] and last["count"] and last["entry_stride"] == dv.slots and last["payload_stride"] == dv.slots * dv.data_bytes
