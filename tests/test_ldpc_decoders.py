"""The three LDPC decoders of pirip_amd/csrc/ldpc_decode.hip against the mirror oracle (oracle/ldpc_oracle.c) on every path they can take:
every shape of tests/ldpcshapes.py under every PIRIP_LDPC_DECODER setting, soft bits at the clamp ends / zeros / infinities / NaN,
max_iter 1, 2, 3 and 50, batches of more frames than one round of workgroups, the stream path with 1, 2 and 3 job chunks per stream,
and the bytes next to an unaligned status array. Everything goes through pirip_hip_ldpc_decode_llr / pirip_hip_ldpc_rx_batch and is
compared with np.array_equal: there is no tolerance here. tests/test_ldpc_decoders_cpu.py holds what keeps these from passing vacuously
(which kernel each case reaches, what the word sets contain).

Kernels reached (ldpcshapes.launch_path; W waves per workgroup, REGIDX / row-weight build):
  test_decoder_shape_matrix           every name of ldpcshapes.SHAPES x generic | fast | bank | auto: decode_kernel<8|4|2, true>,
                                      decode_kernel<8|4|2|1, false>, decode_fast_kernel<4, 6>, <2, 8>, decode_bank_kernel<8, 6>, <8, 8>
  test_generic_decoder_records        decode_kernel<8, true> through the receiver (job lists, CRC, records)
  test_soft_bit_edges, test_max_iter  decode_kernel<8, true>, decode_fast_kernel<4, 6> / <2, 8>, decode_bank_kernel<8, 6> / <8, 8>
  test_more_frames_than_one_round     decode_kernel<8, true>, decode_fast_kernel<4, 6>, decode_bank_kernel<8, 6> (cps = num_cu + 2)
  test_stream_path_chunks_per_stream, test_status_neighbours    the same three, stream mode, cps = 1, 2, 3"""
import os

import numpy as np
import pytest

import ldpcshapes as ls

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODE = os.path.join(ROOT, "pirip_amd", "data", "standin_256_512_4.code")
DEC3 = ("generic", "fast", "bank")
RX_SYNC, RX_BITS, RX_BIT_ERRORS = 2, 4, 8
_codes, _want = {}, {}


@pytest.fixture(scope="module")
def code_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("ldpc_shapes")


def _code(oracle, code_dir, name, max_iter=15):
    """(parsed code, path of its code file); the shipped code at its own max_iter is the shipped file itself."""
    key = (name, max_iter)
    if key not in _codes:
        if name == ls.SHIPPED and max_iter == 15:
            _codes[key] = (oracle.parse_code_file(CODE), CODE)
        else:
            c = ls.shape_code(name, oracle.parse_code_file(CODE)["rows"], max_iter)
            path = str(code_dir / ("%s_%d.code" % (name, max_iter)))
            ls.write_code(path, c["n"], c["k"], c["rows"], max_iter)
            parsed = oracle.parse_code_file(path)
            assert parsed["rows"] == c["rows"] and parsed["max_iter"] == max_iter
            _codes[key] = (parsed, path)
    return _codes[key]


def _oracle_decode(oracle, key, code, llr):
    """The oracle's (bits, iter / pcc) for a word set, computed once and shared by the decoder settings."""
    if key not in _want:
        bits, ip = oracle.OracleLdpc(code, 2).decode(llr)
        bits.setflags(write=False); ip.setflags(write=False)
        _want[key] = (bits, ip)
    return _want[key]


def _handle(monkeypatch, decoder, path, M=2, Nsym=50, nstreams=1):
    import pirip_amd
    monkeypatch.delenv("PIRIP_LDPC_GENERIC", raising=False)
    monkeypatch.setenv("PIRIP_LDPC_DECODER", decoder)
    return pirip_amd.HipLdpc(path, M, Nsym=Nsym, nstreams=nstreams)


def _decode(h, llr):
    """pirip_hip_ldpc_decode_llr on zero-filled outputs (a skipped slot shows as iter 0)."""
    import torch
    import pirip_amd
    ncw, n = llr.shape
    dl = torch.from_numpy(np.ascontiguousarray(llr, dtype=np.float32)).cuda()
    bits = torch.zeros((ncw, n), dtype=torch.uint8, device="cuda")
    ip = torch.zeros((ncw, 2), dtype=torch.int32, device="cuda")
    pirip_amd.binding._chk(h.L.pirip_hip_ldpc_decode_llr(h.h, dl.data_ptr(), ncw, bits.data_ptr(), ip.data_ptr(), 0), "decode")
    torch.cuda.synchronize()
    return bits.cpu().numpy(), ip.cpu().numpy()


def _num_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _assert_equal(got_bits, got_ip, want_bits, want_ip, what):
    bad = np.where((got_ip != want_ip).any(1))[0]
    assert bad.size == 0, (what, "iterations / parity counts differ at words", bad[:8], got_ip[bad[:8]].tolist(), want_ip[bad[:8]].tolist())
    bad = np.where((got_bits != want_bits).any(1))[0]
    assert bad.size == 0, (what, "decoded bits differ at words", bad[:8])


# ---- a. decoder x shape matrix, direct decode ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("decoder", DEC3 + ("auto",))
@pytest.mark.parametrize("name", list(ls.SHAPES))
def test_decoder_shape_matrix(oracle, built_lib, code_dir, monkeypatch, name, decoder):
    """Bits, iterations and parity counts equal the oracle's; the device's own parity count is what numpy counts on the dense H; converged
    easy words are the transmitted ones. Shapes without the fast layout run under fast / bank too and must equal the generic decoder."""
    code, path = _code(oracle, code_dir, name)
    H = ls.dense_h(code["rows"], code["n"])
    cw, llr, easy = ls.matrix_words(name, code)
    wb, wip = _oracle_decode(oracle, ("matrix", name), code, llr)
    h = _handle(monkeypatch, decoder, path)
    gb, gip = _decode(h, llr)
    print(name, decoder, ls.launch_path(code, decoder, llr.shape[0], 1, _num_cu())["kernel"], "iterations", np.bincount(gip[:, 0], minlength=16))
    _assert_equal(gb, gip, wb, wip, (name, decoder))
    assert np.array_equal(gip[:, 1], ls.parity_ok_count(H, gb))
    conv = gip[:, 1] == H.shape[0]
    assert conv[easy].sum() >= easy.sum() // 2
    if ls.comes_back(name):
        assert np.array_equal(gb[easy & conv], cw[easy & conv])


def test_a_code_over_the_lds_limit_is_refused_at_creation(oracle, built_lib, code_dir, monkeypatch):
    import pirip_amd
    n, k, wcol = ls.OVER_LIMIT
    for w, refused in ((wcol, True), (wcol - 1, False)):
        rows = ls.ra_rows(n, k, w, 1)
        path = str(code_dir / ("limit_%d.code" % w))
        ls.write_code(path, n, k, rows)
        assert ls.create_refused(dict(n=n, k=k, rows=rows)) == refused
        if refused:
            with pytest.raises(pirip_amd.binding.PiripError, match=r"\(%d\)" % ls.ERR_UNSUPPORTED):
                _handle(monkeypatch, "auto", path)
        else:
            assert _handle(monkeypatch, "auto", path).n == n


def test_generic_decoder_records(oracle, built_lib, monkeypatch):
    """decode_kernel<8, true> behind the receiver: PIRIP_LDPC_DECODER=generic on the shipped code, one rx_host pass over a two-burst
    recording -- status, payload and info equal the oracle's."""
    import pirip_amd
    import sigutil
    import test_ldpc as tl
    code = oracle.parse_code_file(CODE)
    c = dict(sigutil.CFG1, P=6)
    bits = sigutil.run_framer(["--testframes", "4", "--bursts", "1", "--seq", "--source", "0x6", "/dev/zero", "-"])
    u8 = tl._bursts(oracle, c, 2, [bits, bits], ebno_db=6.0, seed=61)
    dem = pirip_amd.HipDemod(c["Fs"], c["Rs"], 2, P=6, est_min=500, est_max=c["est_max"], in_format=pirip_amd.IN_CU8_CSDR, nstreams=1)
    filt = dem.demod_host(u8)["rx_filt"]
    ws, wp, wi = oracle.OracleLdpc(code, 2).rx(filt)
    gs, gp, gi = _handle(monkeypatch, "generic", CODE).rx_host(filt)
    assert np.array_equal(gs, ws), np.where(gs != ws)
    assert np.array_equal(gp, wp)
    assert np.array_equal(gi, wi), np.where(gi != wi)
    ok = (ws & RX_BITS) != 0
    assert ok.sum() >= 4 and (wi[ok, 4] > 1).any()               # (a false lock in the gap / > 10 % raw errors can cost a frame)


# ---- b. soft-bit edges ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decoder", DEC3)
@pytest.mark.parametrize("name", [ls.SHIPPED, "unbalanced6"])
def test_soft_bit_edges(oracle, built_lib, code_dir, monkeypatch, name, decoder):
    """One word per edge value of ldpcshapes.EDGE_VALUES (every magnitude equal: the first iteration's q is exactly it), the zero words,
    contradicted infinities, rounding ties, and NaN with either sign bit in 1 and in 50 places: a NaN soft bit is an erasure (+0 where
    soft bits enter), so all three decoders and the oracle agree.
    Before that rule (NaN passed on as binary16 NaN) the sign-set NaN words split the decoders: decode_kernel reads "q < 0" (hard bit 0 in
    those places), decode_fast_kernel and decode_bank_kernel the sign bit (1). Measured on the shipped code, (iter, pcc): "-NaN x 1" generic
    (15, 252), fast and bank (2, 256); "-NaN x 50" (15, 200) everywhere but 27 against 29 bits off the erasure result; on the unbalanced
    code "-NaN x 1" generic (15, 254), fast and bank (2, 256); "-NaN x 50" generic (15, 215), fast and bank (15, 196)."""
    code, path = _code(oracle, code_dir, name)
    H = ls.dense_h(code["rows"], code["n"])
    labels, w = ls.edge_words(name, code)
    wb, wip = _oracle_decode(oracle, ("edges", name), code, w)
    gb, gip = _decode(_handle(monkeypatch, decoder, path), w)
    for i, lab in enumerate(labels):
        print("%-26s device iter %2d pcc %3d | oracle iter %2d pcc %3d | bits differ %d" % (lab, gip[i, 0], gip[i, 1], wip[i, 0], wip[i, 1], int((gb[i] != wb[i]).sum())))
    bad = [labels[i] for i in range(len(labels)) if not (np.array_equal(gb[i], wb[i]) and np.array_equal(gip[i], wip[i]))]
    assert not bad, (name, decoder, bad)
    assert np.array_equal(gip[:, 1], ls.parity_ok_count(H, gb))
    i = labels.index("+-inf, one contradicted")
    assert gip[i, 0] == code["max_iter"] and 0 < gip[i, 1] < H.shape[0]


@pytest.mark.parametrize("llr_map", ["upstream", "rician"])
@pytest.mark.parametrize("M", [2, 4])
def test_llr_stage_erases_nan_from_nan_and_infinite_magnitudes(oracle, built_lib, tmp_path, M, llr_map):
    """pirip_hip_ldpc_llr: an infinite magnitude makes the call's noise term inf - inf and a NaN magnitude every sum of its call; the LLR
    clamps pass NaN (both comparisons false). Such soft bits are erasures, +0, on the device and in the oracle; the other calls of the
    batch are untouched."""
    import torch
    import pirip_amd
    import sigutil
    path = sigutil.code_variant(CODE, tmp_path, llr_map)
    code = oracle.parse_code_file(path)
    rng = np.random.default_rng(5 + M)
    ncalls, nsym = 40, 50
    filt = np.zeros((ncalls, M, nsym), dtype=np.float32)
    for i in range(ncalls):
        sym = rng.integers(0, M, nsym)
        z = (rng.normal(size=(M, nsym)) + 1j * rng.normal(size=(M, nsym))) / np.sqrt(2)
        z[sym, np.arange(nsym)] += np.sqrt(4.0)
        filt[i] = np.abs(z)
    filt[3, 0, 7] = np.inf
    filt[9, M - 1, 0] = np.nan
    filt[10, 1, 49] = ls.NAN_NEG
    filt[20, :, 5] = np.inf
    filt[33, 0, :] = np.nan
    filt[34] = np.inf
    o = oracle.OracleLdpc(code, M)
    want = o.llr(filt)
    h = pirip_amd.HipLdpc(path, M)
    d = torch.from_numpy(filt).cuda()
    out = torch.full((ncalls, o.Nbits), 77.0, dtype=torch.float32, device="cuda")
    pirip_amd.binding._chk(h.L.pirip_hip_ldpc_llr(h.h, d.data_ptr(), ncalls, out.data_ptr(), 0), "llr")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert not np.isnan(want).any() and not np.isnan(got).any()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.where(got.view(np.uint32) != want.view(np.uint32))
    clean = np.isfinite(filt).all(axis=(1, 2))
    assert (want[clean] != 0).mean() > 0.9 and not want[34].any()


# ---- c. max_iter 1, 2, 3, 50 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decoder", DEC3)
@pytest.mark.parametrize("max_iter", ls.MAX_ITERS)
@pytest.mark.parametrize("name", ls.ITER_SHAPES)
def test_max_iter(oracle, built_lib, code_dir, monkeypatch, name, max_iter, decoder):
    """The same rows with max_iter 1, 2, 3 and 50 (the persistent decoder checks parity one iteration late and leaves on it > max_iter):
    a word that converges exactly at max_iter reports iter == max_iter and pcc == m, one that does not iter == max_iter and the last
    iteration's pcc -- both as the oracle has them (test_ldpc_decoders_cpu.py: the word set holds both kinds)."""
    code, path = _code(oracle, code_dir, name, max_iter)
    m = code["n"] - code["k"]
    _, llr = ls.iter_words(name, code)
    wb, wip = _oracle_decode(oracle, ("iter", name, max_iter), code, llr)
    gb, gip = _decode(_handle(monkeypatch, decoder, path), llr)
    _assert_equal(gb, gip, wb, wip, (name, max_iter, decoder))
    at_max = gip[:, 0] == max_iter
    assert (at_max & (gip[:, 1] == m)).any() and (at_max & (gip[:, 1] != m)).sum() >= 3 and (gip[~at_max, 1] == m).all()
    assert np.array_equal(gip[:, 1], ls.parity_ok_count(ls.dense_h(code["rows"], code["n"]), gb))


# ---- d. more frames than one round ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decoder", DEC3)
def test_more_frames_than_one_round(oracle, built_lib, code_dir, monkeypatch, decoder):
    """(56,24) code: 16 num_cu + 17 words under bank (workgroups walk several units, chunks per stream = num_cu + 2: the magic division),
    4 x 8192 + 5 under fast and 8 x 8192 + 5 under generic (the grid is capped at 8192 workgroups: slot strides). Most words are one of
    16 clean ones, every 97th and the last five are noisy; outputs are zero-filled first. The oracle decodes each DISTINCT word once
    (np.unique by content) -- a decode depends on the word alone."""
    code, path = _code(oracle, code_dir, "ra56")
    num_cu = _num_cu()
    count = {"bank": 16 * num_cu + 17, "fast": 4 * 8192 + 5, "generic": 8 * 8192 + 5}[decoder]
    p = ls.launch_path(code, decoder, count, 1, num_cu)
    assert p["family"] == decoder and (p["cps"] == num_cu + 2 if decoder == "bank" else count > p["grid"][0] * p["wpb"])
    rng = np.random.default_rng(count)
    pool = ls.codewords("ra56", code, 16, rng)
    cw = pool[rng.integers(0, 16, count)]
    llr = ((1.0 - 2.0 * cw) * 8.0).astype(np.float32)
    noisy = np.arange(count) % 97 == 0
    noisy[-5:] = True
    llr[noisy] = ls.bpsk_llrs(cw[noisy], np.full(int(noisy.sum()), 0.9), rng)
    uniq, inv = np.unique(llr, axis=0, return_inverse=True)
    ub, uip = oracle.OracleLdpc(code, 2).decode(uniq)
    inv = inv.reshape(-1)
    gb, gip = _decode(_handle(monkeypatch, decoder, path), llr)
    assert (gip[:, 0] >= 1).all(), ("slots never decoded", np.where(gip[:, 0] < 1)[0][:8])
    _assert_equal(gb, gip, ub[inv], uip[inv], decoder)
    assert uniq.shape[0] > int(noisy.sum()) and (uip[:, 1] != 32).sum() >= 3


# ---- e. the stream path with 1, 2 and 3 chunks of jobs per stream --------------------------------------------------------------------
def _stream_want(oracle, code, rec_idx, recs, valid):
    """The oracle's records of one stream: STREAM_PRIME calls, then `valid` more, of recording rec_idx -- once per distinct pair."""
    key = ("stream", rec_idx, valid)
    if key not in _want:
        _want[key] = oracle.OracleLdpc(code, ls.STREAM_M, Nsym=ls.STREAM_NSYM).rx(recs[rec_idx][:ls.STREAM_PRIME + valid])
    return _want[key]


def _recordings(oracle):
    if "recs" not in _want:
        code = oracle.parse_code_file(CODE)
        _want["recs"] = [ls.stream_recording(code, 40 + i) for i in range(8)]
        for r in _want["recs"]:
            r.setflags(write=False)
    return _want["recs"]


def _run_stream_batches(h, recs, nstreams, ncalls, valid, carve=None):
    """A priming batch of STREAM_PRIME calls (every stream), then the measured batch of ncalls calls with ragged valid counts, through
    pirip_hip_ldpc_rx_batch. carve: byte offset at which the output arrays start inside 0xA5-filled buffers (None: arrays of their own).
    Returns per batch (status, payload, info) as numpy and, with carve, the guard regions."""
    import torch
    per = ls.STREAM_M * ls.STREAM_NSYM
    out = []
    for first, nc, val in ((0, ls.STREAM_PRIME, np.full(nstreams, ls.STREAM_PRIME, dtype=np.int32)), (ls.STREAM_PRIME, ncalls, valid)):
        host = np.full((nstreams, nc, per), 123.0, dtype=np.float32)             # beyond the valid calls: must not be read
        for s in range(nstreams):
            host[s, :val[s]] = recs[s % len(recs)][first:first + val[s]]
        d = torch.from_numpy(host).cuda()
        dv = torch.from_numpy(np.ascontiguousarray(val)).cuda()
        nst, npl, ninf = nstreams * nc, nstreams * nc * 32, nstreams * nc * 10 * 4
        if carve is None:
            st = torch.zeros(nst, dtype=torch.uint8, device="cuda")
            pl = torch.zeros(npl, dtype=torch.uint8, device="cuda")
            inf = torch.zeros(ninf, dtype=torch.uint8, device="cuda")
            ptrs = (st.data_ptr(), pl.data_ptr(), inf.data_ptr())
            bufs = ((st, 0, nst), (pl, 0, npl), (inf, 0, ninf))
        else:
            pad = 64
            bufs = []
            for size, off in ((nst, pad + carve), (npl, pad + carve), (ninf, pad + 4)):      # (info is int32: it stays 4-byte aligned)
                b = torch.full((size + 2 * pad + 8,), 0xA5, dtype=torch.uint8, device="cuda")
                assert b.data_ptr() % 4 == 0
                bufs.append((b, off, size))
            ptrs = tuple(b.data_ptr() + off for b, off, _ in bufs)
        h.rx_batch(d.data_ptr(), nc * per, dv.data_ptr(), nc, ptrs[0], ptrs[1], ptrs[2], 0)
        torch.cuda.synchronize()
        host_bufs = [(b.cpu().numpy(), off, size) for b, off, size in bufs]
        guards = [np.concatenate([b[:off], b[off + size:]]) for b, off, size in host_bufs]
        st_h, pl_h, inf_h = (b[off:off + size] for b, off, size in host_bufs)
        out.append((st_h.reshape(nstreams, nc), pl_h.reshape(nstreams, nc, 32), inf_h.copy().view(np.int32).reshape(nstreams, nc, 10), guards))
    return out


def _check_streams(oracle, code, recs, nstreams, ncalls, valid, out, what):
    P = ls.STREAM_PRIME
    (s1, p1, i1, _), (s2, p2, i2, _) = out
    for s in range(nstreams):
        v = int(valid[s])
        ws, wp, wi = _stream_want(oracle, code, s % len(recs), recs, v)
        gs, gp, gi = np.concatenate([s1[s], s2[s, :v]]), np.concatenate([p1[s], p2[s, :v]]), np.concatenate([i1[s], i2[s, :v]])
        assert np.array_equal(gs, ws), (what, s, v, np.where(gs != ws))
        assert np.array_equal(gp, wp), (what, s, v)
        assert np.array_equal(gi, wi), (what, s, v, np.where(gi != wi))
        assert not s2[s, v:].any() and not p2[s, v:].any() and (i2[s, v:] == -1).all(), (what, s, v)
    return int((i2[0, :, 6] >= 0).sum())                                         # frames listed for stream 0 (all its calls valid)


@pytest.mark.parametrize("decoder", DEC3)
@pytest.mark.parametrize("ncalls,more_than", list(zip(ls.STREAM_NCALLS, (0, 16, 32))))
def test_stream_path_chunks_per_stream(oracle, built_lib, monkeypatch, ncalls, more_than, decoder):
    """Synthetic soft decisions of one continuous 40-frame burst per stream (4-FSK, 50 symbols per call, shipped code) through
    pirip_hip_ldpc_rx_batch: batches of 60, 100 and 180 calls have max_jobs = 13, 20, 35, i.e. 1, 2, 3 chunks of 16 job slots per stream
    in the persistent decoder (its magic division) and more than one round of slots in the other two; 1, 3 and num_cu + 1 streams, ragged
    valid-call counts with 0 among them, 8 distinct recordings cycled. A batch from the reset state cannot list more than 32 frames in
    180 calls (a frame is listed 989 .. 1088 bits after its first), so every case primes the receivers with 11 calls first: stream 0
    then lists more than 16 / 32 frames in the measured batch (asserted from info). Every stream's records equal those of an oracle
    receiver fed its valid calls."""
    code = oracle.parse_code_file(CODE)
    recs = _recordings(oracle)
    num_cu = _num_cu()
    for nstreams in (1, 3, num_cu + 1):
        valid = ls.stream_valid_counts(nstreams, ncalls)
        h = _handle(monkeypatch, decoder, CODE, M=ls.STREAM_M, Nsym=ls.STREAM_NSYM, nstreams=nstreams)
        out = _run_stream_batches(h, recs, nstreams, ncalls, valid)
        listed = _check_streams(oracle, code, recs, nstreams, ncalls, valid, out, (decoder, ncalls, nstreams))
        assert listed > more_than, (nstreams, listed)
        h.close()


# ---- f. the bytes next to the status array -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decoder", ["bank", "fast"])
@pytest.mark.parametrize("offset", [1, 2, 3])
def test_status_neighbours(oracle, built_lib, monkeypatch, offset, decoder):
    """The persistent decoder ORs a frame's status bits into the 32-bit word that holds the status byte. Three streams, 101 calls (odd:
    rows start unaligned), status and payload carved out of 0xA5-filled buffers at byte offset 1, 2, 3: the records equal the oracle's
    and those of aligned arrays, and every guard byte before and after the three arrays is unchanged. The status array is written by the
    library alone (its sync stage, then the decoder)."""
    code = oracle.parse_code_file(CODE)
    recs = _recordings(oracle)
    nstreams, ncalls = 3, 101
    valid = np.array([ncalls, 0, 64], dtype=np.int32)
    assert ls.launch_path(code, "bank", ncalls * 100 // 544 + 2, nstreams, _num_cu())["cps"] == 2
    outs = []
    for carve in (offset, None):
        h = _handle(monkeypatch, decoder, CODE, M=ls.STREAM_M, Nsym=ls.STREAM_NSYM, nstreams=nstreams)
        out = _run_stream_batches(h, recs, nstreams, ncalls, valid, carve=carve)
        assert _check_streams(oracle, code, recs, nstreams, ncalls, valid, out, (decoder, offset, carve)) > 16
        outs.append(out)
        h.close()
    for (sa, pa, ia, guards), (sb, pb, ib, _) in zip(*outs):
        assert np.array_equal(sa, sb) and np.array_equal(pa, pb) and np.array_equal(ia, ib)
        for g in guards:
            assert g.size >= 128 and (g == 0xA5).all(), np.where(g != 0xA5)
