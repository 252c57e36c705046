"""include/pirip_hip.h section M: the streaming repeater (pirip_hip_rpt_*, pirip_amd.HipRepeater) and frame_repeater_channels.

Every check is exact. The records offered per call and the counters come from the host model tests/rptref.py, which
tests/test_repeater_stream_cpu.py pins to frame_repeater's own output and whose schedules it shows to reach every corner; the IQ must be
what a fresh HipTxStream makes when the host sends it the model's records call by call. The closed loop runs a terminal's bursts through
the repeater and a checking receiver, and feeds the repeater its own output to see that it repeats none of it."""
import os
import subprocess

import numpy as np
import pytest

import muxshapes as ms
import rptref
import sigutil

pytestmark = pytest.mark.gpu

CANARY = 0xA5
BAD_ARG, UNSUPPORTED = -1, -6
MFS, RS = 40000, 5000                          # Ts = 8, the smallest of tests/test_txs.py's shapes; D = 1, linear: wideband = modem rate


def _modem(M):
    return (50, 544) if M == 2 else (100, 272)  # preamble and frame of the stand-in code, in symbols


def _tx_side(ntx, M):
    import pirip_amd
    f1 = [1000 + 13 * (c % 7) for c in range(ntx)]
    tx = pirip_amd.HipTx(ms.CODE, MFS, RS, M, nstreams=ntx, f1=f1, shift=RS, gap=rptref.GAP_SYMS)
    offsets = [int(-19000 + 38000 * (c + 0.5) / ntx) for c in range(ntx)]
    gains = [0.8 / ntx * (1 + c % 3) / 3 * (-1) ** c for c in range(ntx)]
    mux = pirip_amd.HipMux(MFS, 1, offsets, gains=gains, kind=pirip_amd.MUX_LINEAR)
    assert (tx.preamble_syms, tx.frame_syms) == _modem(M) and tx.data_bytes == rptref.KB
    return tx, mux


class _Run:
    """a schedule's calls staged on the device; go() pushes them through a HipRepeater and keeps what every call offered"""

    def __init__(self, sched, M=2):
        import torch
        import pirip_amd
        self.s, self.M = sched, M
        self.tx, self.mux = _tx_side(sched["ntx"], M)
        self.block = sched["S"] * self.tx.Ts
        self.txs = pirip_amd.HipTxStream(self.tx, self.mux, self.block, sched["queue_syms"])
        self.rpt = pirip_amd.HipRepeater(self.tx, self.txs, sched["route"], sched["source"], filter=sched["filter"], holdoff=sched["holdoff"],
                                         max_burst=sched["max_burst"], pending=sched["pending"])
        calls, nrx, kb = sched["calls"], len(sched["route"]), rptref.KB
        self.ncalls, self.nrx = len(calls), nrx
        self.w = max([len(st) for call in calls for st, _ in call] + [1])
        hst = np.full((self.ncalls, nrx, self.w), 6, np.uint8)       # unused slots: a status that would start a burst, were it read
        hpl = np.full((self.ncalls, nrx, self.w, kb), 0x5A, np.uint8)
        hnc = np.zeros((self.ncalls, nrx), np.int32)
        for n, call in enumerate(calls):
            for c, (st, pl) in enumerate(call):
                hst[n, c, :len(st)], hpl[n, c, :len(st)], hnc[n, c] = st, pl, len(st)
        self.hst, self.hpl = hst, hpl
        self.d_st, self.d_pl, self.d_nc = torch.from_numpy(hst).cuda(), torch.from_numpy(hpl).cuda(), torch.from_numpy(hnc).cuda()
        self.blk = self.block * 2
        self.P, self.rl = sched["pending"], 1 + kb

    def go(self, upto=None):
        """the first `upto` calls (None: all) -> (IQ uint8 [calls * block * 2], offered uint8 [calls, ntx, P, rl], counts int32 [calls, ntx])"""
        import torch
        rt = sigutil.hip_runtime()
        ntx = self.s["ntx"]
        ncalls = self.ncalls if upto is None else upto
        out = torch.full((ncalls * self.blk + 64,), CANARY, dtype=torch.uint8, device="cuda")
        off = torch.full((ncalls, ntx, self.P, self.rl), 0xEE, dtype=torch.uint8, device="cuda")
        cnt = torch.full((ncalls, ntx), -7, dtype=torch.int32, device="cuda")
        p_rec, stride, p_n = self.rpt.offered()
        assert stride == self.P * self.rl
        for n in range(ncalls):
            self.rpt.push_records(self.d_st[n], self.d_pl[n], out.data_ptr() + 32 + n * self.blk, self.blk, ncalls=self.d_nc[n])
            sigutil.d2d(rt, off[n].data_ptr(), p_rec, ntx * stride)
            sigutil.d2d(rt, cnt[n].data_ptr(), p_n, ntx * 4)
        torch.cuda.synchronize()
        assert (out[:32] == CANARY).all() and (out[32 + ncalls * self.blk:] == CANARY).all()
        assert np.array_equal(self.d_st.cpu().numpy(), self.hst) and np.array_equal(self.d_pl.cpu().numpy(), self.hpl)   # the records are only read
        return out[32:32 + ncalls * self.blk], off.cpu().numpy(), cnt.cpu().numpy()

    def host_driven(self, offered):
        """a fresh HipTxStream of the same configuration, sent the model's records call by call -> IQ"""
        import torch
        import pirip_amd
        ntx = self.s["ntx"]
        txs = pirip_amd.HipTxStream(self.tx, self.mux, self.block, self.s["queue_syms"])
        stage = np.full((self.ncalls, ntx, self.P, self.rl), 3, np.uint8)
        nrec = np.zeros((self.ncalls, ntx), np.int32)
        for n, per in enumerate(offered):
            for t, r in enumerate(per):
                stage[n, t, :len(r)], nrec[n, t] = r, len(r)
        d_stage, d_nrec = torch.from_numpy(stage).cuda(), torch.from_numpy(nrec).cuda()
        out = torch.zeros(self.ncalls * self.blk, dtype=torch.uint8, device="cuda")
        for n in range(self.ncalls):
            txs.send(d_stage[n].data_ptr(), self.P * self.rl, self.P, d_nrec=d_nrec[n].data_ptr())
            txs.process(out.data_ptr() + n * self.blk, self.blk)
        torch.cuda.synchronize()
        assert not txs.counters()["refused"].any()
        return out


def _check_offered(sched, offered, off, cnt):
    """every call's rows against the model; records behind a count are what the rows held before the call"""
    prev = np.zeros_like(off[0])
    for n, per in enumerate(offered):
        assert cnt[n].tolist() == [len(r) for r in per], (sched["name"], n)
        for t, r in enumerate(per):
            assert np.array_equal(off[n, t, :len(r)], r), (sched["name"], n, t)
            assert np.array_equal(off[n, t, len(r):], prev[t, len(r):]), (sched["name"], n, t)
        prev = off[n]


SCHEDULES = {s["name"]: s for s in rptref.schedules(*_modem(2))}
CASES = [(n, 2) for n in SCHEDULES] + [("corners_holdoff1", 4), ("fixture_permuted", 4)]


@pytest.mark.parametrize("name,M", CASES, ids=["%s-M%d" % c for c in CASES])
def test_records_path_equals_the_model_and_a_host_driven_transmitter(built_lib, name, M):
    import torch
    pre, frame = _modem(M)
    sched = {s["name"]: s for s in rptref.schedules(pre, frame)}[name]
    offered, m = rptref.run(sched, pre, frame)
    run = _Run(sched, M)
    iq, off, cnt = run.go()
    _check_offered(sched, offered, off, cnt)
    got, want = run.rpt.counters(), m.counters()
    for k in want:
        assert np.array_equal(got[k], want[k]), (k, got[k], want[k])
    c = run.txs.counters()
    assert not c["refused"].any()
    assert np.array_equal(c["queued"], np.array(m.queued))
    ref = run.host_driven(offered)
    assert torch.equal(iq, ref), (name, M, int((iq != ref).sum()))
    if name.startswith("corners"):
        assert (iq != 128).any()                                     # and it is not silence


def test_cutting_the_records_differently_gives_the_same_records(built_lib):
    """the fixture's streams in one call, one record per call, and in five pieces with per-channel counts: the concatenation per transmit
    channel is the same, and in one piece it is the model's"""
    base = SCHEDULES["fixture_one_call"]
    streams = base["calls"][0]
    rng = np.random.default_rng(91)
    longest = max(len(st) for st, _ in streams)
    cuts = [base["calls"], rptref.one_per_call(streams, extra=1), rptref.cut_calls(rng, streams, 5) + [[(st[:0], pl[:0]) for st, pl in streams]]]
    assert len(cuts[1]) == longest + 1
    cat = []
    for calls in cuts:
        sched = dict(base, calls=calls)
        run = _Run(sched)
        _, off, cnt = run.go()
        cat.append([np.concatenate([off[n, t, :cnt[n, t]] for n in range(len(calls))]) for t in range(base["ntx"])])
        assert not run.rpt.counters()["dropped"].any() and not run.rpt.counters()["pending"].any()
    offered, _ = rptref.run(base, *_modem(2))
    for t in range(base["ntx"]):
        want = np.concatenate([o[t] for o in offered])
        for k in range(3):
            assert cat[k][t].shape == want.shape and np.array_equal(cat[k][t], want), (k, t)


def test_reset_forgets_open_bursts_and_pending_rings(built_lib):
    import torch
    sched = SCHEDULES["corners_holdoff3"]
    first, off1, cnt1 = _Run(sched).go()
    # stop in the middle: a burst is open on channel 0 and records wait in the rings
    _, m = rptref.run(dict(sched, calls=sched["calls"][:14]), *_modem(2))
    assert any(x.size for x in m.open_st) and m.counters()["pending"].any()
    run = _Run(sched)
    run.go(upto=14)
    assert np.array_equal(run.rpt.counters()["pending"], m.counters()["pending"])
    run.rpt.reset()
    assert not any(v.any() for v in run.rpt.counters().values()) and not any(v.any() for v in run.txs.counters().values())
    # the whole schedule on the handle that was reset: the bytes and records of a fresh one
    again, off2, cnt2 = run.go()
    assert torch.equal(again, first) and np.array_equal(cnt1, cnt2)
    for n in range(run.ncalls):
        for t in range(sched["ntx"]):
            assert np.array_equal(off1[n, t, :cnt1[n, t]], off2[n, t, :cnt2[n, t]])


def test_argument_limits_as_the_header_states_them(built_lib):
    import torch
    import pirip_amd
    pre, frame = _modem(2)
    tx, mux = _tx_side(3, 2)
    one = rptref.burst_cost(1, pre, frame, rptref.GAP_SYMS)
    txs = pirip_amd.HipTxStream(tx, mux, 3 * tx.Ts, 4 * one)

    def fails(code, **kw):
        args = dict(route=[0, 1, 2], source=1, max_burst=4, pending=5)
        args.update(kw)
        with pytest.raises(pirip_amd.PiripError, match=rf"\({code}\)"):
            pirip_amd.HipRepeater(tx, args.pop("txs", txs), **args)

    pirip_amd.HipRepeater(tx, txs, [0, 1, 2], 1, max_burst=4, pending=5).close()
    pirip_amd.HipRepeater(tx, txs, [2, -1, -1, 0], 1, max_burst=4, pending=5).close()       # several unrouted channels are no duplicates
    fails(BAD_ARG, route=[0, 1, 1])                                  # duplicate route
    fails(BAD_ARG, route=[0, 1, 3])                                  # route >= nchan
    fails(BAD_ARG, pending=4)                                        # pending < max_burst + 1
    fails(BAD_ARG, max_burst=0)
    fails(BAD_ARG, max_burst=101, pending=200)
    fails(BAD_ARG, max_burst=5, pending=6)                           # five frames need pre + 5 frame + gap > 4 (pre + frame + gap) symbols
    small = pirip_amd.HipTxStream(tx, mux, 3 * tx.Ts, one - 1)
    fails(BAD_ARG, txs=small, max_burst=1, pending=2)                # a queue smaller than one burst
    other = pirip_amd.HipTx(ms.CODE, MFS, RS, 2, nstreams=3)
    with pytest.raises(pirip_amd.PiripError, match=rf"\({BAD_ARG}\)"):
        pirip_amd.HipRepeater(other, txs, [0, 1, 2], 1, max_burst=1, pending=2)             # txs was not created on this tx
    rpt = pirip_amd.HipRepeater(tx, txs, [0, 1, 2], 1, max_burst=4, pending=5)
    out = torch.zeros(3 * tx.Ts * 2, dtype=torch.uint8, device="cuda")
    L = rpt.L

    def push(ncalls):
        st = torch.zeros((3, max(ncalls, 1)), dtype=torch.uint8, device="cuda")
        pl = torch.zeros((3, max(ncalls, 1), rptref.KB), dtype=torch.uint8, device="cuda")
        rc = L.pirip_hip_rpt_push_records(rpt.h, st.data_ptr(), ncalls, pl.data_ptr(), ncalls * rptref.KB, 0, ncalls, out.data_ptr(), out.numel(), 0)
        torch.cuda.synchronize()
        return rc

    assert push(4097) == UNSUPPORTED and push(4096) == 0 and push(0) == 0
    assert L.pirip_hip_rpt_process(rpt.h, out.data_ptr(), out.numel(), 0) == BAD_ARG         # no rx
    assert L.pirip_hip_rpt_push(rpt.h, out.data_ptr(), out.numel(), out.data_ptr(), out.numel(), 0) == BAD_ARG
    assert L.pirip_hip_rpt_push_records(rpt.h, 0, 0, 0, 0, 0, 0, out.data_ptr(), out.numel(), 0) == BAD_ARG
    assert (out == 128).all()                                        # the calls that ran sent silence
    assert not rpt.counters()["bursts_in"].any()


def test_4096_records_in_one_call(built_lib):
    """the largest call table: independently drawn status bytes (short bursts), against the model"""
    import torch
    rng = np.random.default_rng(12)
    pre, frame = _modem(2)
    st = [rng.choice([0, 2, 4, 6, 8, 0xA, 0xC, 0xE, 1], 4096).astype(np.uint8) for _ in range(2)]
    pl = [rng.integers(0, 256, (4096, rptref.KB)).astype(np.uint8) for _ in range(2)]
    empty = [(s[:0], p[:0]) for s, p in zip(st, pl)]
    sched = dict(name="table", calls=[list(zip(st, pl)), empty], route=[1, 0], ntx=2, source=0x42, filter=0x17, holdoff=0, max_burst=6,
                 pending=256, queue_syms=rptref.burst_cost(6, pre, frame, rptref.GAP_SYMS) * 2, S=2)
    offered, m = rptref.run(sched, pre, frame)
    assert m.counters()["bursts_in"].min() > 200 and m.counters()["dropped"].all() and m.counters()["filtered"].all()
    run = _Run(sched)
    iq, off, cnt = run.go()
    _check_offered(sched, offered, off, cnt)
    got = run.rpt.counters()
    for k, v in m.counters().items():
        assert np.array_equal(got[k], v), k
    assert torch.equal(iq, run.host_driven(offered))


def test_the_intake_writes_the_records_of_the_record_conversion(built_lib, tmp_path):
    """The two users of the one repeater body, held to each other on frame_repeater's own cases with 13-byte frames (bursts open across
    calls, bursts of more than 100 frames, BITS without SYNC): every case is a receive channel routed to the transmit channel of its index,
    cut into the same random pieces for HipTx.repeat_records and for HipRepeater.push_records. A pending ring holds every record of the
    largest case and a queue every symbol of a channel, so a burst is offered in the call in which it ends and nothing is dropped."""
    import torch
    import pirip_amd
    import txref
    from test_tx_repeater import _call, _code_for, _cuts
    kb, src, pieces, drain = 13, 0x31, 5, 2
    cases = [c for c in txref.repeater_cases() if c["kb"] == kb]
    B, total = len(cases), sum(c["out"].shape[0] for c in cases)
    assert B > 80 and total > 2000
    tx = pirip_amd.HipTx(_code_for(kb, tmp_path), MFS, RS, 2, nstreams=B, f1=1000, shift=RS, gap=rptref.GAP_SYMS)
    assert tx.data_bytes == kb
    rng = np.random.default_rng(1300)
    cuts = [_cuts(rng, c["status"].size, pieces) for c in cases]
    parts = [([c["status"][cuts[s][p][0]:cuts[s][p][1]] for s, c in enumerate(cases)],
              [c["payload"][cuts[s][p][0]:cuts[s][p][1]] for s, c in enumerate(cases)]) for p in range(pieces)]
    parts += [([c["status"][:0] for c in cases], [c["payload"][:0] for c in cases])] * drain
    # path one: the record conversion, call by call
    got = [_call(tx, kb, src, st, pl) for st, pl in parts[:pieces]]
    one = [np.concatenate([g[s] for g in got]) for s in range(B)]
    for s, c in enumerate(cases):
        want = c["out"].copy()
        want[want[:, 0] != 2, 1] = src                               # the fixture's records with this test's source byte
        assert np.array_equal(one[s], want), c["name"]
    # path two: the streaming repeater's intake, and what it offers call by call
    ctl = [r[:, 0] for r in one]
    syms = [int((x == 1).sum() * tx.preamble_syms + (x <= 1).sum() * tx.frame_syms + (x == 2).sum() * rptref.GAP_SYMS) for x in ctl]
    P = max(max(r.shape[0] for r in one), 101)
    mux = pirip_amd.HipMux(MFS, 1, [int(-19000 + 38000 * (c + 0.5) / B) for c in range(B)], gains=[0.5 / B] * B, kind=pirip_amd.MUX_LINEAR)
    block = 2 * tx.Ts
    txs = pirip_amd.HipTxStream(tx, mux, block, max(max(syms), rptref.burst_cost(100, tx.preamble_syms, tx.frame_syms, rptref.GAP_SYMS)))
    rpt = pirip_amd.HipRepeater(tx, txs, list(range(B)), src, filter=None, holdoff=0, max_burst=100, pending=P)
    rt = sigutil.hip_runtime()
    rl = 1 + kb
    p_rec, stride, p_n = rpt.offered()
    assert stride == P * rl
    out = torch.zeros(block * 2, dtype=torch.uint8, device="cuda")
    off = torch.full((len(parts), B, P, rl), 0xEE, dtype=torch.uint8, device="cuda")
    cnt = torch.full((len(parts), B), -7, dtype=torch.int32, device="cuda")
    staged = []
    for n, (st, pl) in enumerate(parts):
        w = max(max(x.size for x in st), 1)
        hst, hpl = np.full((B, w), 6, np.uint8), np.full((B, w, kb), 0x5A, np.uint8)
        for s in range(B):
            hst[s, :st[s].size], hpl[s, :st[s].size] = st[s], pl[s]
        staged.append([torch.from_numpy(x).cuda() for x in (hst, hpl, np.array([x.size for x in st], np.int32))])
        rpt.push_records(staged[n][0], staged[n][1], out, block * 2, ncalls=staged[n][2])
        sigutil.d2d(rt, off[n].data_ptr(), p_rec, B * stride)
        sigutil.d2d(rt, cnt[n].data_ptr(), p_n, B * 4)
    torch.cuda.synchronize()
    off, cnt = off.cpu().numpy(), cnt.cpu().numpy()
    compared = 0
    for t in range(B):
        two = np.concatenate([off[n, t, :cnt[n, t]] for n in range(len(parts))])
        assert two.shape == one[t].shape and np.array_equal(two, one[t]), cases[t]["name"]
        compared += two.shape[0]
    assert compared == total
    c = rpt.counters()
    assert not c["dropped"].any() and not c["unrouted"].any() and not c["pending"].any() and not c["filtered"].any()
    assert c["frames_in"].sum() == sum(int((x <= 1).sum()) for x in ctl) and not txs.counters()["refused"].any()


# ---------------------------------------------------------------- the closed loop (tests/muxshapes.py's LOOP)

ROUTE = [1, 0, 3, 2]
LOOP_S, LOOP_GAP, LOOP_CALLS = 100, 64, 80


def _terminal_records():
    rec = ms.loop_records(seed=31)
    rec[:, :ms.LOOP["nframes"], 1] = 1                               # the terminal's source byte
    return rec


def _terminal_blocks():
    """the terminal's wideband u8 IQ, uint8 tensor [LOOP_CALLS, block * 2]: its bursts go in before call 2"""
    import torch
    import pirip_amd
    lp = ms.LOOP
    rec = _terminal_records()
    tx = pirip_amd.HipTx(ms.CODE, lp["mFs"], lp["Rs"], lp["M"], nstreams=4, f1=lp["f1"], shift=lp["shift"], gap=LOOP_GAP)
    mux = pirip_amd.HipMux(lp["Fs"], lp["D"], lp["offsets"], gains=ms.LOOP_GAINS)
    block = LOOP_S * lp["D"] * tx.Ts
    txs = pirip_amd.HipTxStream(tx, mux, block, tx.preamble_syms + lp["nframes"] * tx.frame_syms + LOOP_GAP)
    d_rec = torch.from_numpy(rec).cuda()
    out = torch.zeros((LOOP_CALLS, block * 2), dtype=torch.uint8, device="cuda")
    for k in range(LOOP_CALLS):
        if k == 2:
            txs.send(d_rec.data_ptr(), rec[0].size, rec.shape[1])
        txs.process(out[k].data_ptr(), block * 2)
    torch.cuda.synchronize()
    assert not txs.counters()["refused"].any()
    return out


class _Repeater:
    """HipRepeater(rx=HipRx(chan=...)) of the LOOP shapes; the handles it borrows live as long as it does"""

    def __init__(self, holdoff, filt=2):
        import pirip_amd
        from test_mux import _rx_handles
        lp = ms.LOOP
        self.tx = pirip_amd.HipTx(ms.CODE, lp["mFs"], lp["Rs"], lp["M"], nstreams=4, f1=lp["f1"], shift=lp["shift"], gap=LOOP_GAP)
        self.mux = pirip_amd.HipMux(lp["Fs"], lp["D"], lp["offsets"], gains=ms.LOOP_GAINS)
        self.block = LOOP_S * lp["D"] * self.tx.Ts
        burst = self.tx.preamble_syms + lp["nframes"] * self.tx.frame_syms + LOOP_GAP
        self.txs = pirip_amd.HipTxStream(self.tx, self.mux, self.block, burst)
        self.dem, self.ld, self.ch = _rx_handles()
        self.rx = pirip_amd.HipRx(self.dem, ldpc=self.ld, chan=self.ch, block=self.block)
        self.rpt = pirip_amd.HipRepeater(self.tx, self.txs, ROUTE, 2, filter=filt, holdoff=holdoff, max_burst=lp["nframes"],
                                         pending=lp["nframes"] + 1, rx=self.rx)
        assert self.rpt.rx_rows == self.rx.max_frames and self.rpt.info.has_rx == 1

    def run(self, blocks, tbits=None):
        """-> uint8 tensor like blocks: the repeated wideband IQ. With tbits every call's records() go to that counter, chained on the
        same stream with nothing waiting for anything, and copies of them are kept in self.seen (status, payload, info, nframes per call)"""
        import torch
        out = torch.zeros_like(blocks)
        K, R, kb = blocks.shape[0], self.rpt.rx_rows, rptref.KB
        if tbits is not None:
            rt = sigutil.hip_runtime()
            st = torch.zeros((K, 4, R), dtype=torch.uint8, device="cuda")
            pl = torch.zeros((K, 4, R, kb), dtype=torch.uint8, device="cuda")
            info = torch.zeros((K, 4, R, 10), dtype=torch.int32, device="cuda")
            nfr = torch.zeros((K, 4), dtype=torch.int32, device="cuda")
        for k in range(K):
            self.rpt.push(blocks[k], self.block * 2, out[k], self.block * 2)
            if tbits is not None:
                r = self.rpt.records()
                assert (r["status_stride"], r["payload_stride"], r["info_stride"]) == (R, R * kb, R * 10)
                tbits.push_records(r["status"], r["payload"], r["info"], ncalls=r["nframes"], max_calls=R,
                                   status_stride=r["status_stride"], payload_stride=r["payload_stride"], info_stride=r["info_stride"])
                sigutil.d2d(rt, st[k].data_ptr(), r["status"], 4 * R)
                sigutil.d2d(rt, pl[k].data_ptr(), r["payload"], 4 * R * kb)
                sigutil.d2d(rt, info[k].data_ptr(), r["info"], 4 * R * 10 * 4)
                sigutil.d2d(rt, nfr[k].data_ptr(), r["nframes"], 4 * 4)
        torch.cuda.synchronize()
        if tbits is not None:
            self.seen = [x.cpu().numpy() for x in (st, pl, info, nfr)]
        return out


@pytest.fixture(scope="module")
def loop(built_lib):
    """the terminal's blocks, and what the repeater with holdoff 1 made of them, with its counters and the test-frame counter's"""
    import pirip_amd
    blocks = _terminal_blocks()
    rp = _Repeater(holdoff=1)
    tb = pirip_amd.HipTestBits(nstreams=4)
    tb.set_payload(rptref.KB)
    out = rp.run(blocks, tbits=tb)
    return dict(blocks=blocks, out=out, rp=rp, counters=rp.rpt.counters(), tb=tb.record_counters(), txs=rp.txs.counters(), seen=rp.seen)


def _receive(blocks):
    """a checking HipRx on wideband blocks -> per channel the payloads of the frames with BITS"""
    import torch
    import pirip_amd
    from test_mux import _rx_handles
    dem, ld, ch = _rx_handles()
    block = blocks.shape[1] // 2
    rx = pirip_amd.HipRx(dem, ldpc=ld, chan=ch, block=block)
    R, nb = rx.max_frames, ld.data_bytes
    K = blocks.shape[0]
    st = torch.zeros((K, 4, R), dtype=torch.uint8, device="cuda")
    pl = torch.zeros((K, 4, R, nb), dtype=torch.uint8, device="cuda")
    info = torch.zeros((K, 4, R, 10), dtype=torch.int32, device="cuda")
    nfr = torch.zeros((K, 4), dtype=torch.int32, device="cuda")
    for k in range(K):
        rx.push(blocks[k].data_ptr(), block * 2, d_status=st[k].data_ptr(), d_payload=pl[k].data_ptr(), d_info=info[k].data_ptr(),
                d_nframes=nfr[k].data_ptr())
    torch.cuda.synchronize()
    s, p, nf = st.cpu().numpy(), pl.cpu().numpy(), nfr.cpu().numpy()
    outs = [[p[k, c, f] for k in range(K) for f in range(nf[k, c]) if s[k, c, f] & pirip_amd.RX_BITS] for c in range(4)]
    return [np.array(o, dtype=np.uint8).reshape(-1, nb) for o in outs]


def test_closed_loop_every_payload_comes_back_on_the_routed_channel(loop):
    nfr = ms.LOOP["nframes"]
    rec = _terminal_records()
    c = loop["counters"]
    assert c["bursts_in"].tolist() == [1] * 4 and c["frames_in"].tolist() == [nfr] * 4 and not c["filtered"].any() and not c["unrouted"].any()
    assert c["bursts_out"].tolist() == [1] * 4 and not c["pending"].any() and not c["dropped"].any()
    assert not loop["txs"]["refused"].any() and not loop["txs"]["queued"].any()
    # the counter chained on records() counted what records() showed, call after call, and every frame passed its CRC
    import pirip_amd
    import tbitsref
    st, pl, info, nf = loop["seen"]
    want = {k: np.zeros(4, np.int64) for k in tbitsref.REC_NAMES}
    for k in range(st.shape[0]):
        for name, v in tbitsref.record_tally(st[k], pl[k], info[k], nf[k], pirip_amd.testframe_payload(8 * rptref.KB)).items():
            want[name] += v
    for name in want:
        assert np.array_equal(loop["tb"][name], want[name]), (name, loop["tb"][name], want[name])
    assert loop["tb"]["crc_ok"].tolist() == [nfr] * 4 and (loop["tb"]["frames"] >= nfr).all()
    back = _receive(loop["out"])
    for cch, t in enumerate(ROUTE):
        got = back[t]
        assert got.shape[0] == nfr, (t, got.shape)
        assert (got[:, 0] == 2).all()                                # the repeater's source byte
        assert np.array_equal(got[:, 1:-2], rec[cch, :nfr, 2:-2]), (cch, t)   # the rest unchanged (the CRC is the new frame's own)


def test_no_echo_the_repeaters_own_output_is_filtered(loop):
    rp = loop["rp"]
    rp.rpt.reset()
    assert not any(v.any() for v in rp.rpt.counters().values())
    out = rp.run(loop["out"])
    c = rp.rpt.counters()
    assert c["filtered"].tolist() == [ms.LOOP["nframes"]] * 4        # every frame carries the repeater's source byte
    assert not c["bursts_in"].any() and not c["frames_in"].any() and not c["bursts_out"].any() and not c["pending"].any()
    assert (out == 128).all()                                        # carrier off only


def test_reset_with_a_receiver_repeats_the_first_run(loop):
    import torch
    rp = loop["rp"]
    rp.rpt.reset()
    assert torch.equal(rp.run(loop["blocks"]), loop["out"])
    got = rp.rpt.counters()
    assert all(np.array_equal(got[k], loop["counters"][k]) for k in got)


def _cli(tmp_path, blocks, holdoff):
    lp = ms.LOOP
    src, dst = str(tmp_path / "in.iq"), str(tmp_path / ("out%d.iq" % holdoff))
    blocks.cpu().numpy().tofile(src)
    cmd = [os.path.join(ms.BIN, "frame_repeater_channels"), "--code", ms.CODE, "-s", str(lp["Fs"]), "-a", str(lp["mFs"]), "-r", str(lp["Rs"]),
           "-m", str(lp["M"]), "--fsk_lower", str(lp["est_min"]), "--fsk_upper", str(lp["est_max"]), "-q",
           "-c", ",".join(map(str, lp["offsets"])), "--f1", str(lp["f1"]), "--shift", str(lp["shift"]),
           "--gains", ",".join(f"{g:.9g}" for g in ms.LOOP_GAINS), "--gap", str(LOOP_GAP), "--block", str(blocks.shape[1] // 2),
           "--source", "2", "--filter", "2", "--route", ",".join(map(str, ROUTE)), "--holdoff", str(holdoff), "--max-burst", str(lp["nframes"]),
           "--pending", str(lp["nframes"] + 1), "--queue", str(50 + lp["nframes"] * 544 + LOOP_GAP), "-i", src, "-o", dst]
    return subprocess.run(cmd, capture_output=True, timeout=120), dst


@pytest.mark.parametrize("holdoff", [0, 2])
def test_cli_equals_the_binding(loop, tmp_path, holdoff):
    rp = _Repeater(holdoff=holdoff)
    want = rp.run(loop["blocks"]).cpu().numpy().reshape(-1)
    c = rp.rpt.counters()
    p, name = _cli(tmp_path, loop["blocks"], holdoff)
    assert p.returncode == 0, p.stderr.decode()
    got = np.fromfile(name, dtype=np.uint8)
    assert got.size == want.size and np.array_equal(got, want)
    assert (want != 128).any() and not np.array_equal(want, loop["out"].cpu().numpy().reshape(-1))     # the hold-off moves the bursts
    lines = [ln for ln in p.stderr.decode().splitlines() if ln.startswith("rx ") or ln.startswith("tx ")]
    assert lines == ["rx %d: bursts %d frames %d filtered %d unrouted %d" % (i, c["bursts_in"][i], c["frames_in"][i], c["filtered"][i], c["unrouted"][i])
                     for i in range(4)] + \
                    ["tx %d: bursts %d pending %d dropped %d" % (t, c["bursts_out"][t], c["pending"][t], c["dropped"][t]) for t in range(4)]
