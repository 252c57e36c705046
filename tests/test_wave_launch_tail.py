"""Launch tail of the wave kernel ("Launch tail"): pirip_hip_set_launch_tail_first makes the workgroups of a launch's
last residency start at a raised wave priority. Priority only changes the order in which the hardware issues the waves' instructions, so
the setter must leave every word where it was: the launches here are compared word for word between the setter off (nothing raised)
and on, and eight streams of each, strided across the batch, with the oracle.

Stream counts, with R = the workgroups resident at once as the library reports them (four streams per workgroup in both instances): 1
stream; 5 (a partial second workgroup); 4 R (one residency: nothing raised); 4 R + 4 (one workgroup more: all but the first raised);
4 R + 1027 (a ragged tail, the last workgroup partial); 8 R + 8 (two residencies and two workgroups: about 6150 streams x 7.3 KB). Each
stream holds three frames (3600 + 48 samples); a first call takes two of them and a second, chunked one the rest from every stream's own
position, which is how the state block a call saves (raw tail, tone rows, last frame's length: no accessor of its own) shows.
"""
import ctypes as C

import numpy as np
import pytest

import sigutil
from parity import _compare, _oracle_field_Sf

pytestmark = pytest.mark.gpu

NSAMP = 3600 + 48
SHAPES = {
    "headline": dict(sigutil.CFG1, fmt=0),
    "4fsk_p8": dict(sigutil.CFG4, fmt=0),
}
NBASE, NOFF = 8, 24                      # stream s: base signal s % 8 read from sample (s // 8) % 24 on


def _handle(c, B):
    import pirip_amd
    h = pirip_amd.HipDemod(c["Fs"], c["Rs"], c["M"], P=c["P"], est_min=c["est_min"], est_max=c["est_max"], in_format=c["fmt"], nstreams=B)
    assert h.kernel() == "wave"
    return h


@pytest.fixture(scope="module")
def resident(built_lib):
    """R per shape, from the library"""
    out = {}
    for name, c in SHAPES.items():
        h = _handle(c, 1)
        out[name] = h.launch_resident_blocks()
        h.close()
        assert out[name] > 0 and out[name] % 3 == 0, out        # three workgroups of four waves per CU
    return out


@pytest.fixture(scope="module")
def bases(oracle):
    """per shape: NBASE signals of NSAMP + NOFF samples -- other bits, tone plans a bin apart, two of them noisy"""
    out = {}
    for name, c in SHAPES.items():
        nb = 50 * (1 if c["M"] == 2 else 2)
        rows = []
        for k in range(NBASE):
            u8, _ = sigutil.make_u8_stream(oracle, c, 5 * nb, seed=100 + k, tone_bins=(k % 3) - 1, ebno_db=12.0 if k in (3, 6) else None,
                                           random_bits=True)
            rows.append(u8[5 * k:5 * k + NSAMP + NOFF])
        out[name] = np.stack(rows)
    return out


def stream_counts(R):
    return [1, 5, 4 * R, 4 * R + 4, 4 * R + 1027, 8 * R + 8]


def _host(base, B):
    host = np.empty((B, NSAMP, 2), dtype=np.uint8)
    for k in range(min(NBASE * NOFF, B)):
        off = (k // NBASE) % NOFF
        host[k::NBASE * NOFF] = base[k % NBASE, off:off + NSAMP]
    return host


def _stream_of(base, s):
    off = (s // NBASE) % NOFF
    return base[s % NBASE, off:off + NSAMP]


def _watch(B, R):
    """streams whose Sf, scalars and state are read back one by one: eight strided ones and those next to the window's edges"""
    w = set(np.linspace(0, B - 1, min(B, 8)).astype(int).tolist())
    first = (B + 3) // 4 - R
    if first > 0:
        for blk in (first - 1, first, first + R // 2):
            w.update(s for s in (4 * blk, 4 * blk + 3) if 0 <= s < B)
    w.add(B - 1)
    return sorted(w)


def run(c, host, on, watch, packed=False):
    """two calls (two frames, then the rest from every stream's own position) of all B streams with the setter on or off"""
    import torch
    import pirip_amd
    B = host.shape[0]
    h = _handle(c, B)
    h.set_launch_tail_first(on)
    if packed:
        h.set_bit_packing(True)
    nb = (h.Nbits + 7) // 8 if packed else h.Nbits
    nf, ns = c["M"] * 50, pirip_amd.STATS_PER_FRAME
    st = torch.cuda.current_stream().cuda_stream
    pos = np.zeros(B, dtype=np.int64)
    out = {"bits": [], "rx_filt": [], "stats": [], "nframes": [], "consumed": []}
    for k in (2, 2):
        n = int(NSAMP - pos.max())
        piece = host if not pos.any() else host[np.arange(B)[:, None], pos[:, None] + np.arange(n)[None, :]]
        dev = torch.from_numpy(np.ascontiguousarray(piece)).cuda()
        bits = torch.zeros((B, k, nb), dtype=torch.uint8, device="cuda")
        filt = torch.zeros((B, k, nf), dtype=torch.float32, device="cuda")
        stats = torch.zeros((B, k, ns), dtype=torch.float32, device="cuda")
        nfr = torch.zeros(B, dtype=torch.int32, device="cuda"); cons = torch.zeros(B, dtype=torch.int64, device="cuda")
        h.demod_batch(dev.data_ptr(), n * 2, n, bits.data_ptr(), k * nb, filt.data_ptr(), k * nf, stats.data_ptr(), k * ns,
                      nfr.data_ptr(), cons.data_ptr(), k, st)
        torch.cuda.synchronize()
        out["bits"].append(bits.cpu().numpy()); out["rx_filt"].append(filt.cpu().numpy()); out["stats"].append(stats.cpu().numpy())
        out["nframes"].append(nfr.cpu().numpy()); out["consumed"].append(cons.cpu().numpy())
        pos += out["consumed"][-1]
    assert (out["nframes"][0] == 2).all() and (out["nframes"][1] == 1).all(), "two frames, then the third"
    per = {}
    for s in watch:
        sc = np.zeros(8, dtype=np.float32)
        assert h.L.pirip_hip_get_scalars(h.h, s, sc.ctypes.data) == 0
        per[s] = {"Sf": h.get_Sf(s), "scalars": sc, "state": np.frombuffer(h.stream_state(s), dtype=np.uint32)}
    h.close()
    return out, per


def _words(x):
    return x.view(np.uint8 if x.dtype == np.uint8 else np.uint32) if x.dtype != np.int64 else x


def same_words(a, b, what):
    (oa, pa), (ob, pb) = a, b
    for k in oa:
        for call, (x, y) in enumerate(zip(oa[k], ob[k])):
            if not np.array_equal(_words(x), _words(y)):
                bad = np.unique(np.argwhere(_words(x) != _words(y))[:, 0])
                raise AssertionError((what, k, "call %d" % call, "%d streams differ, first" % len(bad), bad[:8].tolist()))
    for s in pa:
        for k in pa[s]:
            assert np.array_equal(_words(pa[s][k]), _words(pb[s][k])), (what, "stream %d" % s, k)


def against_oracle(oracle, c, base, res, streams):
    out, per = res
    for s in streams:
        x = _stream_of(base, s)
        o = oracle.OracleFsk(c["Fs"], c["Rs"], c["M"], P=c["P"], est_min=c["est_min"], est_max=c["est_max"])
        consumed = int(out["consumed"][0][s] + out["consumed"][1][s])
        ro = o.demod(x[:consumed], c["fmt"])
        rh = {"nframes": 3, "consumed": consumed, **{k: np.concatenate([out[k][0][s], out[k][1][s][:1]]) for k in ("bits", "rx_filt", "stats")}}
        _compare(ro, rh, M=c["M"], allow_near_tie_flips=(s % NBASE) in (3, 6))
        Sf_o = np.ctypeslib.as_array(C.cast(_oracle_field_Sf(oracle, o), C.POINTER(C.c_float)), shape=(256,))
        assert np.array_equal(per[s]["Sf"], Sf_o), ("Sf", s)


@pytest.mark.parametrize("which", range(6), ids=["1", "5", "4R", "4R+4", "4R+1027", "8R+8"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_raised_tail_moves_no_word(oracle, built_lib, resident, bases, name, which):
    import pirip_amd
    c, R = SHAPES[name], resident[name]
    B = stream_counts(R)[which]
    nblocks = (B + 3) // 4
    first = pirip_amd.launch_first_tail_block(nblocks, 12, 4, R // 3)
    assert first == (nblocks - R if nblocks > R else nblocks)                           # the launch under test raises what the case is named for
    host = _host(bases[name], B)
    watch = _watch(B, R)
    off = run(c, host, False, watch)
    against_oracle(oracle, c, bases[name], off, np.linspace(0, B - 1, min(B, 8)).astype(int).tolist())
    same_words(off, run(c, host, True, watch), "setter on")
    poff = run(c, host, False, [], packed=True)
    assert np.array_equal(np.unpackbits(poff[0]["bits"][0], axis=2)[:, :, :off[0]["bits"][0].shape[2]], off[0]["bits"][0])
    same_words(poff, run(c, host, True, [], packed=True), "packed bits, setter on")
