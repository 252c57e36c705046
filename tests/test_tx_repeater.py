"""pirip_hip_tx_repeat_records (include/pirip_hip.h section I) against what the reference's own frame_repeater wrote: every case of
tests/golden/repeater_cases.npz is one stream of a handle, its status and payload arrays go straight to the kernel -- in one call and
cut into random pieces with per-stream call counts -- and the concatenated Tx records must be the program's stdout, byte for byte.
tests/test_tx_repeater_cpu.py pins the fixture and the replay; this file never reads the reference or oracle/_ref."""
import os

import numpy as np
import pytest

import txref
from test_ldpc import _write_random_code

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODE = os.path.join(ROOT, "pirip_amd", "data", "standin_256_512_4.code")
CODES = {13: (136, 104), 32: None, 37: (600, 296)}                  # kb -> (n, k) of an accumulator code with k / 8 = kb; None: the stand-in
BAD_ARG, UNSUPPORTED = -1, -6
FILL = 0xEE
pytestmark = pytest.mark.gpu


def _code_for(kb, tmp_path):
    if CODES[kb] is None:
        return CODE
    n, k = CODES[kb]
    path = str(tmp_path / ("kb%d.code" % kb))
    _write_random_code(path, n, k, 3, seed=n)
    return path


def _call(tx, kb, src, status, payload, check_tail=True):
    """one pirip_hip_tx_repeat_records call: status[s] uint8 [n_s], payload[s] uint8 [n_s, kb] per stream -> list of record arrays.
    Unused call slots hold status 6 and rows behind the capacity a fill pattern: neither may be touched."""
    import torch
    B = len(status)
    ncalls = max(len(st) for st in status)
    w = max(ncalls, 1)
    hst = np.full((B, w), 6, dtype=np.uint8)
    hpl = np.full((B, w, kb), 0x5A, dtype=np.uint8)
    for s in range(B):
        hst[s, :len(status[s])] = status[s]
        hpl[s, :len(status[s])] = payload[s]
    cap = tx.repeat_max_records(ncalls)
    assert cap == txref.REPEAT_MAX_FRAMES + 2 * ncalls
    d_st, d_pl = torch.from_numpy(hst).cuda(), torch.from_numpy(hpl).cuda()
    d_nc = torch.tensor([len(st) for st in status], dtype=torch.int32, device="cuda")
    out = torch.full((B, cap + 2, 1 + kb), FILL, dtype=torch.uint8, device="cuda")
    cnt = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    tx.repeat_records(d_st.data_ptr(), w, d_pl.data_ptr(), w * kb, ncalls, src, out.data_ptr(), (cap + 2) * (1 + kb), cap,
                      d_ncalls=d_nc.data_ptr(), d_nrec=cnt.data_ptr())
    torch.cuda.synchronize()
    o, c = out.cpu().numpy(), cnt.cpu().numpy()
    res = []
    for s in range(B):
        assert 0 <= c[s] <= cap, (s, c[s])
        if check_tail:
            assert (o[s, c[s]:] == FILL).all(), s                    # bytes behind d_nrec keep their fill pattern
        res.append(o[s, :c[s]].copy())
    return res


def _cuts(rng, n, pieces):
    """n records into `pieces` consecutive slices, some of them empty, some of one record"""
    if rng.random() < 0.3:
        cut = np.sort(rng.integers(0, min(n, 3) + 1, pieces - 1))   # pieces of 0 and 1 records in front, the rest in one
    else:
        cut = np.sort(rng.integers(0, n + 1, pieces - 1))
    cut = np.concatenate([[0], cut, [n]])
    return [(int(cut[i]), int(cut[i + 1])) for i in range(pieces)]


@pytest.mark.parametrize("kb", [13, 32, 37])
def test_every_fixture_case_in_one_call_and_in_pieces_equals_frame_repeater(built_lib, tmp_path, kb):
    import pirip_amd
    cases = [c for c in txref.repeater_cases() if c["kb"] == kb]
    B = len(cases)
    assert B > 80
    tx = pirip_amd.HipTx(_code_for(kb, tmp_path), 240000, 10000, 2, nstreams=B, f1=10000, shift=10000)
    assert tx.data_bytes == kb
    rng = np.random.default_rng(4000 + kb)
    nrec_total = 0
    for src in sorted({c["source"] for c in cases}):
        active = [c["source"] == src for c in cases]
        # streams of another source byte get no records in this pass (d_ncalls[s] = 0): they must write nothing and keep no state
        st = [c["status"] if a else c["status"][:0] for c, a in zip(cases, active)]
        pl = [c["payload"] if a else c["payload"][:0] for c, a in zip(cases, active)]
        tx.reset()
        one = _call(tx, kb, src, st, pl)
        for s, c in enumerate(cases):
            want = c["out"] if active[s] else c["out"][:0]
            assert one[s].shape == want.shape and np.array_equal(one[s], want), (c["name"], src)     # d_nrec is the record count
            nrec_total += one[s].shape[0]
        for pieces in (2, 3, 9):
            cuts = [_cuts(rng, len(x), pieces) for x in st]
            tx.reset()
            got = [[] for _ in range(B)]
            for p in range(pieces):
                part = _call(tx, kb, src, [x[cuts[s][p][0]:cuts[s][p][1]] for s, x in enumerate(st)],
                             [x[cuts[s][p][0]:cuts[s][p][1]] for s, x in enumerate(pl)])
                for s in range(B):
                    got[s].append(part[s])
            for s, c in enumerate(cases):
                want = c["out"] if active[s] else c["out"][:0]
                cat = np.concatenate(got[s])
                assert cat.shape == want.shape and np.array_equal(cat, want), (c["name"], src, pieces, cuts[s])
    assert nrec_total == sum(c["out"].shape[0] for c in cases)
    # one record per call: every burst is open across as many calls as it has records
    short = [c for c in cases if c["status"].size <= 40][:B]
    tx.reset()
    src = 0x31
    got = [[] for _ in range(B)]
    pad = [short[s % len(short)] for s in range(B)]
    for i in range(40):
        part = _call(tx, kb, src, [c["status"][i:i + 1] for c in pad], [c["payload"][i:i + 1] for c in pad])
        for s in range(B):
            got[s].append(part[s])
    for s, c in enumerate(pad):
        want = c["out"].copy()
        want[want[:, 0] != 2, 1] = src                               # the fixture's records with this pass's source byte
        assert np.array_equal(np.concatenate(got[s]), want), c["name"]


def test_reset_forgets_an_open_burst(built_lib):
    import pirip_amd
    kb, B = 32, 3
    rng = np.random.default_rng(5)
    tx = pirip_amd.HipTx(CODE, 240000, 10000, 2, nstreams=B, f1=10000, shift=10000)
    st = [np.array([6, 6, 6], dtype=np.uint8)] * B
    pl = [rng.integers(0, 256, (3, kb)).astype(np.uint8) for _ in range(B)]
    fl = [np.array([4], dtype=np.uint8)] * B                         # BITS without SYNC: appended and flushed if a burst is open, nothing if not
    fp = [rng.integers(0, 256, (1, kb)).astype(np.uint8) for _ in range(B)]
    assert all(r.shape[0] == 0 for r in _call(tx, kb, 9, st, pl))
    got = _call(tx, kb, 9, fl, fp)                                   # without a reset the held frames come out
    for s in range(B):
        assert np.array_equal(got[s], txref.repeater_replay(np.concatenate([st[s], fl[s]]), np.concatenate([pl[s], fp[s]]), 9))
        assert list(got[s][:, 0]) == [1, 0, 0, 0, 2]
    assert all(r.shape[0] == 0 for r in _call(tx, kb, 9, st, pl))
    tx.reset()
    assert all(r.shape[0] == 0 for r in _call(tx, kb, 9, fl, fp))    # after a reset there is no burst to append to
    got = _call(tx, kb, 9, [np.array([6, 0], dtype=np.uint8)] * B, [p[:2] for p in pl])
    assert all(list(g[:, 0]) == [1, 2] for g in got)                 # and the next burst holds its own frame only


def test_argument_limits_of_the_record_conversion(built_lib):
    """Stated from include/pirip_hip.h: ncalls <= 4096 (PIRIP_ERR_UNSUPPORTED above), rows of at least repeat_max_records records
    (PIRIP_ERR_BAD_ARG below), at most PIRIP_TX_REPEAT_MAX_FRAMES frames per burst: further frames are dropped."""
    import torch
    import pirip_amd
    kb, B = 32, 2
    rng = np.random.default_rng(8)
    tx = pirip_amd.HipTx(CODE, 240000, 10000, 2, nstreams=B, f1=10000, shift=10000)
    L = tx.L

    def raw(ncalls, max_rec, rows):
        st = torch.zeros((B, ncalls), dtype=torch.uint8, device="cuda")
        pl = torch.zeros((B, ncalls, kb), dtype=torch.uint8, device="cuda")
        out = torch.zeros((B, rows, 1 + kb), dtype=torch.uint8, device="cuda")
        rc = L.pirip_hip_tx_repeat_records(tx.h, st.data_ptr(), ncalls, pl.data_ptr(), ncalls * kb, 0, ncalls, 1, out.data_ptr(), rows * (1 + kb),
                                           max_rec, 0, 0)
        torch.cuda.synchronize()
        return rc

    assert tx.repeat_max_records(4097) == 100 + 2 * 4097
    assert raw(4097, 100 + 2 * 4097, 100 + 2 * 4097) == UNSUPPORTED
    assert raw(4096, 100 + 2 * 4096, 100 + 2 * 4096) == 0
    assert raw(50, 199, 200) == BAD_ARG and raw(50, 200, 200) == 0
    # 4096 calls of independently drawn status bytes (short bursts): the largest call table, against the replay
    tx.reset()
    st = [rng.choice([0, 2, 4, 6, 8, 0xA, 0xC, 0xE, 1], 4096).astype(np.uint8) for _ in range(B)]
    st[1][-3:] = [6, 6, 4]
    pl = [rng.integers(0, 256, (4096, kb)).astype(np.uint8) for _ in range(B)]
    got = _call(tx, kb, 0x42, st, pl)
    for s in range(B):
        want = txref.repeater_replay(st[s], pl[s], 0x42)
        assert want.shape[0] > 500 and np.array_equal(got[s], want), s
    # a burst of 130 frames: the first 100 and the end record, in one call and cut inside the dropped part
    long_st = np.array([6] * 130 + [0], dtype=np.uint8)
    long_pl = rng.integers(0, 256, (131, kb)).astype(np.uint8)
    want = txref.repeater_replay(np.concatenate([long_st[:100], long_st[-1:]]), np.concatenate([long_pl[:100], long_pl[-1:]]), 3)
    assert want.shape[0] == 101
    tx.reset()
    got = _call(tx, kb, 3, [long_st, long_st[:0]], [long_pl, long_pl[:0]])
    assert np.array_equal(got[0], want) and got[1].shape[0] == 0
    tx.reset()
    a = _call(tx, kb, 3, [long_st[:70], long_st[:0]], [long_pl[:70], long_pl[:0]])
    b = _call(tx, kb, 3, [long_st[70:115], long_st[:0]], [long_pl[70:115], long_pl[:0]])
    c = _call(tx, kb, 3, [long_st[115:], long_st[:0]], [long_pl[115:], long_pl[:0]])
    assert a[0].shape[0] == 0 and b[0].shape[0] == 0 and np.array_equal(c[0], want)
