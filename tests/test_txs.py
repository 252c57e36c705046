"""include/pirip_hip.h section K: the streaming transmitter (pirip_hip_txs_*, pirip_amd.HipTxStream) and fsk_ldpc_tx_channels --block.

The contract has no tolerance: the concatenated blocks equal, byte for byte, section I's modulator (complex float, no noise, a fresh
handle) followed by section J's multiplexer (Q - 1 zeros in front, m0 = -(Q - 1)) on each channel's symbol timeline. The timeline, and
what every send takes and every call dequeues, come from the host model tests/txsref.py; tests/test_txs_cpu.py shows that its schedules
reach a refused send, an underrun inside a gap, a ring wrap and a call that starts inside a frame on every shape."""
import os
import subprocess

import numpy as np
import pytest

import muxshapes as ms
import txref
import txsref
from test_tx_shapes import write_code

pytestmark = pytest.mark.gpu

CANARY = 0xA5
BAD_ARG = -1


@pytest.fixture(scope="module")
def code(tmp_path_factory):
    return write_code(tmp_path_factory.mktemp("txs"), txsref.CODE_N, txsref.CODE_K)


def _handles(sh, fmt, code, lead=5):
    """(borrowed tx -- with a lead, which a stream must not apply --, a fresh tx of the same settings without one, mux)"""
    import pirip_amd
    K, mFs = len(sh["f1"]), sh["Fs"] // sh["D"]
    kw = dict(nstreams=K, f1=sh["f1"], shift=sh["shift"], gap=txsref.GAP_SYMS)
    tx = pirip_amd.HipTx(code, mFs, sh["Rs"], sh["M"], lead=lead, **kw)
    ref = pirip_amd.HipTx(code, mFs, sh["Rs"], sh["M"], lead=0, **kw)
    gains = [0.6 / K * (1 + c % 3) / 3 * (-1) ** c for c in range(K)]
    mux = pirip_amd.HipMux(sh["Fs"], sh["D"], sh["offsets"], outputs=sh["outputs"], gains=gains, kind=sh["kind"], transition_bw=sh["tbw"],
                           noutputs=sh["noutputs"], out_format=pirip_amd.IN_CF32 if fmt == "cf32" else pirip_amd.IN_CU8_CSDR)
    return tx, ref, mux


def _records(plans, kb, seed):
    rng = np.random.default_rng(seed)
    return [txref.records(rng, p, kb) for p in plans]


def _symbols(ref, recs, lens):
    """each channel's symbols, record after record, from section I's framer on a handle without lead"""
    import torch
    K, max_rec = len(recs), max(len(r) for r in recs)
    host = np.zeros((K, max_rec, recs[0].shape[1]), np.uint8)
    for c, r in enumerate(recs):
        host[c, :len(r)] = r
    nrec = torch.tensor([len(r) for r in recs], dtype=torch.int32, device="cuda")
    cap = ref.max_syms(max_rec)
    d_rec = torch.from_numpy(host).cuda()
    syms = torch.zeros((K, cap), dtype=torch.uint8, device="cuda")
    nsym = torch.zeros(K, dtype=torch.int32, device="cuda")
    ref.frame(d_rec.data_ptr(), host[0].size, max_rec, syms.data_ptr(), cap, cap, d_nrec=nrec.data_ptr(), d_nsym=nsym.data_ptr())
    torch.cuda.synchronize()
    syms, nsym = syms.cpu().numpy(), nsym.cpu().numpy()
    assert nsym.tolist() == [sum(l) for l in lens]
    return [syms[c, :nsym[c]] for c in range(K)]


def _one_shot(ref, mux, timeline):
    """uint8 [noutputs, T Ts D * bytes per sample]: modulate (cf32, sigma 0, from phase 0) and multiplex the whole timeline"""
    import torch
    import pirip_amd
    K, T = timeline.shape
    Q, bs = mux.Q, mux.bytes_per_sample
    nmod = T * ref.Ts
    ref.reset()
    rows = torch.zeros((K, Q - 1 + nmod, 2), dtype=torch.float32, device="cuda")
    d_tl = torch.from_numpy(np.ascontiguousarray(timeline)).cuda()
    ref.modulate(d_tl.data_ptr(), T, T, rows.data_ptr() + (Q - 1) * 8, rows[0].numel() * 4, out_format=pirip_amd.IN_CF32, sigma=0.0)
    n_wide = nmod * mux.D
    wide = torch.zeros((mux.noutputs, n_wide * bs), dtype=torch.uint8, device="cuda")
    mux.batch(rows.data_ptr(), rows[0].numel() * 4, Q - 1 + nmod, wide.data_ptr(), n_wide * bs, m0=-(Q - 1))
    torch.cuda.synchronize()
    return wide


class _Run:
    """a schedule on the device: every send's records staged up front, every call's block written behind the one before it"""

    def __init__(self, txs, steps, recs, pad=0):
        import torch
        self.txs, self.steps = txs, steps
        K, rl = txs.nchan, recs[0].shape[1]
        sends = [s[1] for s in steps if s[0] == "S"]
        self.ncalls = sum(1 for s in steps if s[0] == "P")
        self.max_rec = max([mk[1] - mk[0] for s in sends for mk in s if mk is not None] + [1])
        stage = np.full((max(len(sends), 1), K, self.max_rec, rl), 3, np.uint8)
        nrec = np.zeros((max(len(sends), 1), K), np.int32)
        for i, marks in enumerate(sends):
            for c, mk in enumerate(marks):
                if mk is not None:
                    stage[i, c, :mk[1] - mk[0]] = recs[c][mk[0]:mk[1]]
                    nrec[i, c] = mk[1] - mk[0]
        self.d_stage, self.d_nrec = torch.from_numpy(stage).cuda(), torch.from_numpy(nrec).cuda()
        self.taken = torch.full(nrec.shape, -7, dtype=torch.int32, device="cuda")
        self.sent = torch.full((self.ncalls, K), -7, dtype=torch.int32, device="cuda")
        self.want_taken = nrec
        bs = txs.bytes_per_sample
        self.blk = txs.block * bs
        self.pad = pad * bs
        self.stride = (self.ncalls * self.blk + 32 + 15) // 16 * 16 + self.pad
        self.out = torch.full((txs.noutputs * self.stride + 64,), CANARY, dtype=torch.uint8, device="cuda")
        assert self.out.data_ptr() % 16 == 0

    def go(self, between=None):
        i = k = 0
        for n, st in enumerate(self.steps):
            if st[0] == "S":
                self.txs.send(self.d_stage[i].data_ptr(), self.d_stage[i, 0].numel(), self.max_rec, d_nrec=self.d_nrec[i].data_ptr(),
                              d_taken=self.taken[i].data_ptr())
                i += 1
            else:
                self.txs.process(self.out.data_ptr() + self.pad + k * self.blk, self.stride, d_sent=self.sent[k].data_ptr())
                k += 1
            if between is not None and n == len(self.steps) // 2:
                between()
        return self

    def rows(self):
        """uint8 [noutputs, ncalls * block * bytes per sample] after checking that nothing was stored around them"""
        import torch
        torch.cuda.synchronize()
        o, n = self.out, self.ncalls * self.blk
        assert (o[:self.pad] == CANARY).all() and (o[self.pad + self.txs.noutputs * self.stride:] == CANARY).all()
        body = o[self.pad:self.pad + self.txs.noutputs * self.stride].reshape(self.txs.noutputs, self.stride)
        assert (body[:, n:] == CANARY).all(), "bytes stored past a block"
        return body[:, :n]


def _case(name, fmt, code, seed=5):
    import pirip_amd
    sh = txsref.SHAPES[name]
    plans, lens, tags, cap = txsref.shape_plans(name)
    tx, ref, mux = _handles(sh, fmt, code)
    Ts = tx.Ts
    recs = _records(plans, tx.data_bytes, seed)
    syms = _symbols(ref, recs, lens)
    steps = txsref.make_schedule(plans, lens, tags, sh["S"], cap)
    txs = pirip_amd.HipTxStream(tx, mux, sh["S"] * sh["D"] * Ts, cap)
    assert (txs.S, txs.H, txs.queue_syms, txs.nchan, txs.noutputs) == (sh["S"], sh["H"], cap, len(plans), sh["noutputs"])
    assert mux.Q == sh["Q"] and txs.info.out_format == mux.out_format
    return sh, plans, lens, tags, cap, tx, ref, mux, recs, syms, steps, txs


CASES = [(n, "u8") for n in sorted(txsref.SHAPES)] + [("h1_d6_outs", "cf32"), ("h10_d1", "cf32"), ("tile_d30", "cf32")]


@pytest.mark.parametrize("name,fmt", CASES, ids=[f"{n}-{f}" for n, f in CASES])
def test_blocks_equal_one_shot_and_counters_equal_the_model(built_lib, code, name, fmt):
    import torch
    sh, plans, lens, tags, cap, tx, ref, mux, recs, syms, steps, txs = _case(name, fmt, code)
    taken, sent = [], []
    m = txsref.replay(steps, plans, lens, tags, syms, sh["S"], cap, on_send=lambda mk, t: taken.append(t.copy()),
                      on_process=lambda s: sent.append(s.copy()))
    run = _Run(txs, steps, recs, pad=sh["pad"]).go()
    got = run.rows()
    want = _one_shot(ref, mux, m.timelines())
    assert got.shape == want.shape
    bad = (got != want).nonzero()
    assert torch.equal(got, want), (name, fmt, bad[:4].tolist(), int(bad.shape[0]))
    if sh["noutputs"] > len(set(sh["outputs"] or [0])):
        empty = [i for i in range(sh["noutputs"]) if i not in sh["outputs"]][0]
        assert (got[empty] == (128 if fmt == "u8" else 0)).all()
    # what each send took and each call dequeued, and the counters
    assert np.array_equal(run.taken.cpu().numpy()[:len(taken)], np.where(np.array(taken), run.want_taken[:len(taken)], 0))
    assert np.array_equal(run.sent.cpu().numpy(), np.array(sent))
    c = txs.counters()
    assert np.array_equal(c["sent"], m.sent) and np.array_equal(c["underrun"], m.underrun) and np.array_equal(c["refused"], m.refused)
    assert np.array_equal(c["queued"], m.queued()) and m.refused.all() and m.underrun.all()
    # after reset the handle is as created: the same schedule gives the same bytes and counters
    txs.reset()
    assert not any(v.any() for v in txs.counters().values())
    again = _Run(txs, steps, recs, pad=0).go()
    assert torch.equal(again.rows(), got)
    assert np.array_equal(txs.counters()["refused"], m.refused)


def test_same_timeline_in_blocks_of_1_3_and_7_symbols(built_lib, code):
    """queues fed ahead, no underrun: wherever the timelines coincide, the bytes do"""
    import torch
    import pirip_amd
    sh = txsref.SHAPES["h1_d6_outs"]
    plans, lens, tags, _ = txsref.shape_plans("h1_d6_outs")
    tx, ref, mux = _handles(sh, "u8", code)
    recs = _records(plans, tx.data_bytes, 8)
    total = min(sum(l) for l in lens)
    outs = []
    for S in (1, 3, 7):
        txs = pirip_amd.HipTxStream(tx, mux, S * sh["D"] * tx.Ts, max(sum(l) for l in lens))
        ncalls = total // S
        steps = [("S", [(0, len(p)) for p in plans])] + [("P",)] * ncalls
        run = _Run(txs, steps, recs).go()
        outs.append(run.rows())
        c = txs.counters()
        assert not c["underrun"].any() and not c["refused"].any() and (c["sent"] == ncalls * S).all()
    n = min(o.shape[1] for o in outs)
    assert n > 200 * sh["D"] * tx.Ts * 2
    assert torch.equal(outs[0][:, :n], outs[1][:, :n]) and torch.equal(outs[0][:, :n], outs[2][:, :n])


def test_more_than_fs_samples_past_zero_and_reset(built_lib, code):
    """a small Fs: the absolute sample index passes Fs several times (the rotation's m0 mod Fs wraps), then reset and the same again"""
    import torch
    import pirip_amd
    sh = dict(Fs=2400, D=6, kind=txsref.FIR, tbw=0.05, Rs=50, M=2, f1=[50, -150], shift=50, offsets=[-700, 501], outputs=None, noutputs=1)
    plans = txsref.PLANS[:2]
    tx, ref, mux = _handles(sh, "u8", code)
    lens = [txsref.record_lens(p, tx.preamble_syms, tx.frame_syms, txsref.GAP_SYMS) for p in plans]
    tags = [txsref.record_tags(p, tx.preamble_syms, tx.frame_syms, txsref.GAP_SYMS) for p in plans]
    recs = _records(plans, tx.data_bytes, 9)
    syms = _symbols(ref, recs, lens)
    S, cap = 5, 400
    steps = txsref.make_schedule(plans, lens, tags, S, cap)
    m = txsref.replay(steps, plans, lens, tags, syms, S, cap)
    txs = pirip_amd.HipTxStream(tx, mux, S * sh["D"] * tx.Ts, cap)
    got = _Run(txs, steps, recs).go().rows()
    assert got.shape[1] // 2 > 3 * sh["Fs"] and m.calls * S * tx.Ts > sh["Fs"]        # wideband samples, and modem samples: m0 itself passes Fs
    want = _one_shot(ref, mux, m.timelines())
    assert torch.equal(got, want)
    txs.reset()
    assert torch.equal(_Run(txs, steps, recs).go().rows(), got)


def test_a_call_on_the_borrowed_transmitter_changes_nothing(built_lib, code):
    import torch
    sh, plans, lens, tags, cap, tx, ref, mux, recs, syms, steps, txs = _case("h2_ts8", "u8", code, seed=6)
    first = _Run(txs, steps, recs).go().rows().clone()
    sy = torch.randint(0, sh["M"], (len(plans), 37), dtype=torch.uint8, device="cuda")
    scratch = torch.zeros((len(plans), 37 * tx.Ts * 2), dtype=torch.uint8, device="cuda")
    txs.reset()
    disturbed = _Run(txs, steps, recs).go(between=lambda: tx.modulate(sy.data_ptr(), 37, 37, scratch.data_ptr(), scratch[0].numel())).rows()
    assert scratch.any() and torch.equal(disturbed, first)


def test_create_refuses_what_the_header_names(built_lib, code):
    import pirip_amd
    sh = txsref.SHAPES["h1_d6_outs"]
    tx, ref, mux = _handles(sh, "u8", code)
    Ts, D, K = tx.Ts, sh["D"], len(sh["f1"])

    def fails(*a):
        with pytest.raises(pirip_amd.PiripError, match=rf"\({BAD_ARG}\)"):
            pirip_amd.HipTxStream(*a)

    pirip_amd.HipTxStream(tx, mux, 2 * D * Ts, 2).close()
    fails(tx, mux, 2 * D * Ts + D, 10)                             # block no multiple of D Ts
    fails(tx, mux, 2 * D * Ts + Ts, 10)
    fails(tx, mux, 0, 10)
    fails(tx, mux, 2 * D * Ts, 1)                                  # queue_syms < S
    fewer = pirip_amd.HipTx(code, sh["Fs"] // D, sh["Rs"], sh["M"], nstreams=K - 1)
    fails(fewer, mux, 2 * D * Ts, 10)                              # nstreams != nchan
    slow = pirip_amd.HipTx(code, sh["Fs"] // D // 2, sh["Rs"], sh["M"], nstreams=K)
    fails(slow, mux, D * slow.Ts, 10)                              # tx.Fs * D != mux.Fs


def test_create_refuses_handles_on_different_devices(built_lib, code):
    import pirip_amd
    if pirip_amd.device_count() < 2:
        pytest.skip("needs two devices")
    sh = txsref.SHAPES["h1_d6_outs"]
    tx, ref, mux = _handles(sh, "u8", code)
    other = pirip_amd.HipTx(code, sh["Fs"] // sh["D"], sh["Rs"], sh["M"], nstreams=len(sh["f1"]), device=1)
    with pytest.raises(pirip_amd.PiripError, match=rf"\({BAD_ARG}\)"):
        pirip_amd.HipTxStream(other, mux, 2 * sh["D"] * tx.Ts, 10)


def test_loopback_block_after_block(built_lib):
    """HipTxStream (u8) -> HipRx(chan=...) with the inputs of tests/test_mux.py's loopback: every payload comes back"""
    import torch
    import pirip_amd
    from test_mux import _assert_all_back, _rx_handles
    lp = ms.LOOP
    rec = ms.loop_records()
    tx = pirip_amd.HipTx(ms.CODE, lp["mFs"], lp["Rs"], lp["M"], nstreams=4, f1=lp["f1"], shift=lp["shift"], gap=lp["tail"])
    mux = pirip_amd.HipMux(lp["Fs"], lp["D"], lp["offsets"], gains=ms.LOOP_GAINS)
    S = 100
    block = S * lp["D"] * tx.Ts
    burst = tx.preamble_syms + lp["nframes"] * tx.frame_syms + lp["tail"]
    txs = pirip_amd.HipTxStream(tx, mux, block, burst + S)
    dem, ld, ch = _rx_handles()
    rx = pirip_amd.HipRx(dem, ldpc=ld, chan=ch, block=block)
    R, nb = rx.max_frames, ld.data_bytes
    d_rec = torch.from_numpy(rec).cuda()
    taken = torch.zeros(4, dtype=torch.int32, device="cuda")
    blk = torch.zeros(block * 2, dtype=torch.uint8, device="cuda")
    outs = [[] for _ in range(4)]
    for k in range(3 + (burst + S - 1) // S):
        if k == 2:                                                   # 200 symbols of silence in front: the empty queue
            txs.send(d_rec.data_ptr(), rec[0].size, rec.shape[1], d_taken=taken.data_ptr())
        txs.process(blk.data_ptr(), block * 2)
        st = torch.zeros((4, R), dtype=torch.uint8, device="cuda")
        pl = torch.zeros((4, R, nb), dtype=torch.uint8, device="cuda")
        info = torch.zeros((4, R, 10), dtype=torch.int32, device="cuda")
        nfr = torch.zeros(4, dtype=torch.int32, device="cuda")
        rx.push(blk.data_ptr(), block * 2, d_status=st.data_ptr(), d_payload=pl.data_ptr(), d_info=info.data_ptr(), d_nframes=nfr.data_ptr())
        torch.cuda.synchronize()
        s, p, nf = st.cpu().numpy(), pl.cpu().numpy(), nfr.cpu().numpy()
        for c in range(4):
            outs[c] += [p[c, f] for f in range(nf[c]) if s[c, f] & pirip_amd.RX_BITS]
    assert taken.cpu().tolist() == [rec.shape[1]] * 4
    c = txs.counters()
    assert (c["sent"] == burst).all() and not c["queued"].any() and not c["refused"].any()
    _assert_all_back([np.array(o, dtype=np.uint8).reshape(-1, nb) for o in outs], rec)


def _cli_records():
    rec = ms.loop_records(seed=23)
    rec = np.concatenate([rec, rec[:, :2]], axis=1)                  # a second burst that the input ends in, without its `2`
    rec[1, 4:] = rec[1, 3]                                           # channel 1: ends after its first burst (three `2` records)
    return rec


def _cli(tmp_path, extra, fmt="u8", rec=None):
    lp = ms.LOOP
    rec = _cli_records() if rec is None else rec
    prefix = str(tmp_path / "rec")
    for c in range(4):
        rec[c].tofile(f"{prefix}.{c}")
    out = str(tmp_path / ("wide" + "".join(extra) + ".iq"))
    cmd = [os.path.join(ms.BIN, "fsk_ldpc_tx_channels"), "--code", ms.CODE, "-s", str(lp["Fs"]), "-a", str(lp["mFs"]), "-r", str(lp["Rs"]),
           "--f1", str(lp["f1"]), "--shift", str(lp["shift"]), "-c", ",".join(map(str, lp["offsets"])),
           "--gains", ",".join(f"{g:.9g}" for g in ms.LOOP_GAINS), "--format", fmt, "--packed", "--gap", "64", "-i", prefix, "-o", out]
    return subprocess.run(cmd + extra, capture_output=True, timeout=120), out


def test_cli_block_mode_equals_the_one_piece_mode(built_lib, tmp_path):
    lp = ms.LOOP
    p, whole = _cli(tmp_path, [])
    assert p.returncode == 0, p.stderr.decode()
    want = np.fromfile(whole, dtype=np.uint8)
    blk = 7 * lp["D"] * (lp["mFs"] // lp["Rs"])
    for extra in (["--block", str(blk)], ["--block", str(blk), "--queue", "5000"]):
        p, name = _cli(tmp_path, extra)
        assert p.returncode == 0, p.stderr.decode()
        got = np.fromfile(name, dtype=np.uint8)
        assert got.size % (2 * blk) == 0 and want.size <= got.size < want.size + 2 * blk
        assert np.array_equal(got[:want.size], want)
        Lp = 14 * lp["D"]                                            # the filter has drained ntaps_padded samples behind the last symbol
        assert (got[want.size + 2 * Lp:] == 128).all()
    p, _ = _cli(tmp_path, ["--block", str(blk), "--lead", "10"])
    assert p.returncode == 1 and p.stderr
    p, _ = _cli(tmp_path, ["--block", str(blk + 1)])
    assert p.returncode == 1 and p.stderr


def test_cli_with_a_queue_of_the_largest_burst_sends_every_symbol(built_lib, tmp_path):
    """--queue equal to the largest burst, whose length is no multiple of S: a burst waits until the queue is empty, the channel underruns
    in between, and the file is the one-shot result on the timeline the model gives for the tool's policy -- to the last symbol"""
    import pirip_amd
    lp = ms.LOOP
    one = ms.loop_records(seed=24)
    rec = np.concatenate([one, one], axis=1)                         # two bursts, each as large as the queue
    rec[1, 4:] = rec[1, 3]                                           # channel 1: one burst, then `2` records only
    S, gap = 7, 64
    ref = pirip_amd.HipTx(ms.CODE, lp["mFs"], lp["Rs"], lp["M"], nstreams=4, f1=lp["f1"], shift=lp["shift"], gap=gap)
    mux = pirip_amd.HipMux(lp["Fs"], lp["D"], lp["offsets"], gains=ms.LOOP_GAINS)
    plans = [rec[c, :, 0].tolist() for c in range(4)]
    lens = [txsref.record_lens(p, ref.preamble_syms, ref.frame_syms, gap) for p in plans]
    tags = [txsref.record_tags(p, ref.preamble_syms, ref.frame_syms, gap) for p in plans]
    cap = max(sum(l[a:b]) for p, l in zip(plans, lens) for a, b in zip([0] + txsref.burst_ends(p)[:-1], txsref.burst_ends(p)))
    assert cap % S and cap == ref.preamble_syms + 3 * ref.frame_syms + gap
    syms = _symbols(ref, [rec[c] for c in range(4)], lens)
    steps = txsref.cli_schedule(plans, lens, tags, S, cap)
    m = txsref.replay(steps, plans, lens, tags, syms, S, cap)
    total = max(sum(l) for l in lens)
    assert m.refused.all() and m.calls * S >= total + S and (m.sent == [sum(l) for l in lens]).all()      # longer than the symbols alone
    blk = S * lp["D"] * ref.Ts
    assert m.underrun.min() >= S - cap % S and -(-total // S) < m.calls          # an underrun between the bursts of every channel
    p, name = _cli(tmp_path, ["--block", str(blk), "--queue", str(cap)], rec=rec)
    assert p.returncode == 0, p.stderr.decode()
    got = np.fromfile(name, dtype=np.uint8)
    want = _one_shot(ref, mux, m.timelines())[0].cpu().numpy()
    assert got.size == want.size == m.calls * blk * 2
    assert np.array_equal(got, want)
    p, _ = _cli(tmp_path, ["--block", str(blk), "--queue", str(cap - 1)], rec=rec)
    assert p.returncode == 1 and b"largest burst" in p.stderr
