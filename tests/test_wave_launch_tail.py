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
import numpy as np
import pytest

import sigutil
from demodrun import make_handle, make_oracle, run_calls, same_results
from parity import _compare, oracle_Sf

pytestmark = pytest.mark.gpu

NSAMP = 3600 + 48
SHAPES = {
    "headline": dict(sigutil.CFG1, fmt=0),
    "4fsk_p8": dict(sigutil.CFG4, fmt=0),
}
NBASE, NOFF = 8, 24                      # stream s: base signal s % 8 read from sample (s // 8) % 24 on


def _handle(c, B):
    h = make_handle(c, B)
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
        nb = sigutil.frame_bits(c)
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
    """two calls (two frames, then the third -- all that is left -- from every stream's own position) of all B streams with the setter on or off"""
    h = _handle(c, host.shape[0])
    h.set_launch_tail_first(on)
    res = run_calls(h, host, [2, (2, 1)], watch=watch, packed=packed)
    h.close()
    return res


def against_oracle(oracle, c, base, res, streams):
    for s in streams:
        rh = res[s]
        o = make_oracle(oracle, c)
        ro = o.demod(_stream_of(base, s)[:rh["consumed"]], c["fmt"])
        _compare(ro, rh, M=c["M"], allow_near_tie_flips=(s % NBASE) in (3, 6))
        assert np.array_equal(rh["Sf"], oracle_Sf(oracle, o)), ("Sf", s)


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
    same_results(off, run(c, host, True, watch), "setter on")
    poff = run(c, host, False, [], packed=True)
    bits = np.stack([r["bits"] for r in off])
    assert np.array_equal(np.unpackbits(np.stack([r["bits"] for r in poff]), axis=2)[:, :, :bits.shape[2]], bits)
    same_results(poff, run(c, host, True, [], packed=True), "packed bits, setter on")
