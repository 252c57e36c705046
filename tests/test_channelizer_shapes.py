"""The channelizer (include/pirip_hip.h section H) away from the three geometries tests/test_channelizer.py visits: every tile geometry
the host rule can pick (D from 1 to 4095, filters of 8 to 324 padded taps, full tiles, partial-wave tiles, one output per workgroup, the
64 KiB LDS window), channel groups of 1 to 8 per lane, Fs at the limit of the rotation's integer arithmetic (2^24), negative and
wrapping t0, captures of one output, of none, and captures no channel listens to. Everything is held to tests/chanref.py's float64
formula on the same bytes and taps (contract 1, the bound derived there) and, where two calls must agree, bit for bit (contract 2).
Every run fills the input slack and the output rows' padding with 0xA5 and checks that the padding comes back untouched.

GEOMETRY, GROUPS and FS_LIMIT are plain data: tests/test_channelizer_cpu.py checks without a GPU that they reach the paths named here."""
import numpy as np
import pytest

import chanref

pytestmark = pytest.mark.gpu

UNSUPPORTED = -6
FS = 2400000
FILL = 0xA5
OUT_PAD = 64                              # bytes past n_out in every output row
IN_PAD = 6                                # the first tile of every capture takes the unaligned-head path

# negative, 0, +-1, not multiples of any output rate here, next to +-Fs/2
OFFS_A = [-700003, 0, 1, 123457, 1199999]
OFFS_B = [-1199999, -1, 0, 333333, 250001]
# name: (D, transition_bw, Lp, offsets, n_out) -- n_out is two full tiles and a partial one (T = 1 has no partial tile)
GEOMETRY = {
    "D1": (1, 0.05, 80, OFFS_A, 700),                   # P = 1: every row one sample; Lp > 4 D
    "D2": (2, 0.05, 80, OFFS_B, 700),                   # D < 8: a 16-byte staging chunk spans 3-4 rows; P = 3 for both
    "D3": (3, 0.05, 80, OFFS_A, 701),
    "D6_Lp320": (6, 0.0125, 320, OFFS_B, 700),          # Lp >> D: 54 rows past the tile; the long-filter bound
    "D6_Lp324": (6, 0.0124, 324, OFFS_A, 650),
    "D30_Lp84": (30, 0.049, 84, OFFS_A, 300),           # the longest filter under the 1e-5 bound
    "D30_Lp12": (30, 0.5, 12, OFFS_A, 700),             # Lp < D
    "D30_Lp8": (30, 1.0, 8, OFFS_B, 700),               # Lp < D, the shortest filter
    "D125": (125, 0.05, 80, OFFS_A, 2 * 64 + 37),       # the largest full tile; 65000 bytes of LDS
    "D127": (127, 0.05, 80, OFFS_B, 2 * 63 + 31),       # first T < Tpad, odd D
    "D128": (128, 0.05, 80, OFFS_A, 2 * 62 + 30),       # even D, P = 129
    "D200": (200, 0.05, 80, OFFS_B, 2 * 39 + 22),       # partial-wave tiles throughout
    "D1000": (1000, 0.05, 80, OFFS_A, 2 * 7 + 3),
    "D4095": (4095, 0.05, 80, OFFS_B, 5),               # one output per workgroup, the largest D accepted
}

# 17 distinct offsets, negatives among them; a case listens to the first K
GROUP_OFFSETS = [-700003, 0, 1, 123457, -250001, 1159999, -1159999, 333333, -1, 5, -77777, 900001, -480000, 40000, -40000, 600007, -3]
# (D, K, the group sizes the host rule makes of them)
GROUP_NOUT = 500
GROUPS = [(6, 6, [6]), (6, 7, [7]), (6, 8, [8]), (6, 9, [5, 4]), (6, 16, [8, 8]), (6, 17, [6, 6, 5]), (30, 16, [8, 8]), (45, 17, [5, 4, 4, 4])]

FS_LIMIT = [(Fs, D) for Fs in (1 << 24, (1 << 24) - 1, 16000000) for D in (6, 30)]
FS_T0 = [0, 2 ** 33 + 5]
FS_NOUT = 700
FS_SPLITS = [0, 1, 37, 255, 256, 257, 600, FS_NOUT]


def fs_offsets(Fs):
    """a small negative f_c makes S = f_c D mod Fs close to Fs, so that B + k S climbs to 255 Fs, the top of the rotation's 32 bits"""
    return [-1, -3, -1000001, 1, 1234567, Fs // 2 - 1, -(Fs // 2 - 1)]


def capture_len(n_out, D, Lp):
    """n_out outputs and as long a tail as leaves it at that"""
    return (n_out - 1) * D + Lp + min(D - 1, 37)


def random_capture(seed, W, n):
    return np.random.default_rng(seed).integers(0, 256, (W, n, 2), dtype=np.uint8)


def run(ch, host, t0=0, in_pad=IN_PAD, raw=False):
    """host [W, n, 2] uint8 -> [K, nout] complex128 (cf32) or int64 [K, nout, 2] (s16); raw: the rows' bytes instead. Slack and padding
    are FILL; asserts that no byte of an output row past nout was written."""
    import torch
    W, n = host.shape[0], host.shape[1]
    stride = 2 * n + in_pad + 2
    flat = np.full(W * stride + 64, FILL, dtype=np.uint8)
    for w in range(W):
        flat[in_pad + w * stride: in_pad + w * stride + 2 * n] = host[w].reshape(-1)
    buf = torch.from_numpy(flat).cuda()
    no = ch.nout(n)
    assert no == chanref.nout(n, ch.Lp, ch.D)
    bps = ch.bytes_per_sample
    out = torch.full((ch.nchan, no * bps + OUT_PAD), FILL, dtype=torch.uint8, device="cuda")
    ch.batch(buf.data_ptr() + in_pad, stride, n, out.data_ptr(), out.shape[1], t0=t0)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[:, no * bps:] == FILL).all(), "a store past n_out"
    o = np.ascontiguousarray(o[:, :no * bps])
    if raw:
        return o
    if ch.out_s16:
        return o.view(np.int16).reshape(ch.nchan, no, 2).astype(np.int64)
    v = o.view(np.float32).reshape(ch.nchan, no, 2).astype(np.float64)
    return v[..., 0] + 1j * v[..., 1]


def check_contract_1(got, want, h, out_s16, what, vanish=True):
    """one channel: every component within chanref.bound(h) of float64, s16 within one LSB; returns the largest cf32 component error"""
    if out_s16:
        d = np.abs(got - chanref.to_s16(want))
        assert d.max() <= 1, (what, d.max())
        return 0.0
    b = chanref.bound(h)
    e = max(np.abs(got.real - want.real).max(), np.abs(got.imag - want.imag).max())
    print("chan %s: max component error %.3e, bound %.3e" % (what, e, b))
    assert e <= b, (what, e, b)
    if vanish:
        assert np.abs(want).max() > 10 * b, "the test signal should not vanish in the bound"
    return e


# ---- 1. geometry sweep -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_s16", [False, True])
@pytest.mark.parametrize("shape", list(GEOMETRY))
def test_geometry_matches_float64(built_lib, shape, out_s16):
    import pirip_amd
    D, tbw, Lp, offsets, n_out = GEOMETRY[shape]
    ch = pirip_amd.HipChan(FS, D, offsets, transition_bw=tbw, out_s16=out_s16)
    try:
        assert ch.Lp == Lp
        h = ch.taps()
        assert chanref.lp_of(h) == Lp
        n = capture_len(n_out, D, Lp)
        assert ch.nout(n) == n_out
        host = random_capture(list(GEOMETRY).index(shape), 1, n)
        got = run(ch, host)
        for c, fc in enumerate(offsets):
            check_contract_1(got[c], chanref.channel(host[0], h, D, FS, fc), h, out_s16, (shape, fc))
    finally:
        ch.close()


def test_decimation_4096_is_unsupported(built_lib):
    """P = 4097: two rows no longer fit 64 KiB"""
    import pirip_amd
    with pytest.raises(pirip_amd.PiripError, match=r"\(%d\)" % UNSUPPORTED):
        pirip_amd.HipChan(FS, 4096, [0, 1])


# ---- 2. group sizes --------------------------------------------------------------------------------------------------------------------
_alone = {}


def alone(D, n):
    """GROUP_OFFSETS, each computed by a one-channel handle of its own on the capture of group_capture(D, n): raw rows, computed once"""
    import pirip_amd
    if D not in _alone:
        host = group_capture(D, n)
        rows = []
        for fc in GROUP_OFFSETS:
            ch = pirip_amd.HipChan(FS, D, [fc])
            rows.append(run(ch, host, t0=99, raw=True)[0])
            ch.close()
        _alone[D] = np.stack(rows)
    return _alone[D]


def group_capture(D, n):
    return random_capture(100 + D, 1, n)


@pytest.mark.parametrize("D,K,sizes", GROUPS)
def test_group_sizes_match_float64_and_the_channel_alone(built_lib, D, K, sizes):
    import pirip_amd
    offsets = GROUP_OFFSETS[:K]
    ch = pirip_amd.HipChan(FS, D, offsets)
    try:
        assert chanref.group_sizes(K, chanref.tile_geometry(D, ch.Lp)[1]) == sizes
        h = ch.taps()
        n = capture_len(GROUP_NOUT, D, ch.Lp)
        host = group_capture(D, n)
        raw = run(ch, host, t0=99, raw=True)
        assert np.array_equal(raw, alone(D, n)[:K]), np.nonzero((raw != alone(D, n)[:K]).any(axis=1))[0]
        v = raw.view(np.float32).reshape(K, -1, 2).astype(np.float64)
        for c, fc in enumerate(offsets):
            check_contract_1(v[c, :, 0] + 1j * v[c, :, 1], chanref.channel(host[0], h, D, FS, fc, 99), h, False, (D, K, fc))
    finally:
        ch.close()


# ---- 3. Fs at the limit ----------------------------------------------------------------------------------------------------------------
def constant_capture(n):
    """byte 255 throughout: x = 1 + 1j, so the output is the rotation times H(f_c) (1 + 1j)"""
    return np.full((1, n, 2), 255, dtype=np.uint8)


def in_passband(fc, Fs, D):
    return 2 * D * abs(fc) < Fs


@pytest.mark.parametrize("out_s16", [False, True])
@pytest.mark.parametrize("Fs,D", FS_LIMIT)
def test_fs_limit_matches_float64(built_lib, Fs, D, out_s16):
    """(a) random bytes; (b) a constant capture, where a rotation error is not buried under the filter sum and s16 clamps"""
    import pirip_amd
    offsets = fs_offsets(Fs)
    ch = pirip_amd.HipChan(Fs, D, offsets, out_s16=out_s16)
    try:
        h = ch.taps()
        n = capture_len(FS_NOUT, D, ch.Lp)
        rnd, const = random_capture(Fs % 1000 + D, 1, n), constant_capture(n)
        for t0 in FS_T0:
            got = run(ch, rnd, t0=t0)
            for c, fc in enumerate(offsets):
                check_contract_1(got[c], chanref.channel(rnd[0], h, D, Fs, fc, t0), h, out_s16, ("random", Fs, D, t0, fc))
            got = run(ch, const, t0=t0)
            for c, fc in enumerate(offsets):
                if in_passband(fc, Fs, D):
                    want = chanref.channel(const[0], h, D, Fs, fc, t0)
                    assert np.abs(want).min() > 0.5 * np.sqrt(2.0) and np.ptp(np.abs(want)) < 1e-9
                    if out_s16 and abs(fc) <= 3:
                        assert (np.abs(chanref.to_s16(want)) >= 32767).any(), "a component should clamp"
                    check_contract_1(got[c], want, h, out_s16, ("constant", Fs, D, t0, fc))
    finally:
        ch.close()


@pytest.mark.parametrize("Fs,D", FS_LIMIT)
def test_fs_limit_blocks_equal_one_shot(built_lib, Fs, D):
    """tests/test_channelizer.py's test_channelizer_blocks_equal_one_shot at these Fs: split points that are no multiples of T"""
    import pirip_amd
    ch = pirip_amd.HipChan(Fs, D, fs_offsets(Fs))
    try:
        n = (FS_NOUT - 1) * D + ch.Lp
        host = random_capture(Fs % 1000 + D + 1, 1, n)
        for t_base in FS_T0:
            whole = run(ch, host, t0=t_base, raw=True).reshape(ch.nchan, FS_NOUT, 8)
            for pad_i, (ja, jb) in enumerate(zip(FS_SPLITS[:-1], FS_SPLITS[1:])):
                part = host[:, ja * D: (jb - 1) * D + ch.Lp]
                got = run(ch, part, t0=t_base + ja * D, in_pad=2 * (pad_i % 8), raw=True).reshape(ch.nchan, jb - ja, 8)
                assert np.array_equal(got, whole[:, ja:jb]), (t_base, ja, jb, np.nonzero((got != whole[:, ja:jb]).any(axis=(1, 2)))[0])
    finally:
        ch.close()


def test_fs_above_2_to_24_is_unsupported(built_lib):
    import pirip_amd
    with pytest.raises(pirip_amd.PiripError, match=r"\(%d\)" % UNSUPPORTED):
        pirip_amd.HipChan((1 << 24) + 1, 6, [0, 1])


# ---- 4. time base ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t0", [-1, -(2 ** 40) - 7, FS - 3])
def test_time_base(built_lib, t0):
    """negative t0 and a t0 whose phase index wraps inside the first tile: within the bound, and a negative t0 is t0 + m Fs bit for bit"""
    import pirip_amd
    D = 30
    ch = pirip_amd.HipChan(FS, D, OFFS_A + OFFS_B[:2])
    try:
        h = ch.taps()
        n = capture_len(300, D, ch.Lp)
        host = random_capture(7, 1, n)
        raw = run(ch, host, t0=t0, raw=True)
        v = raw.view(np.float32).reshape(ch.nchan, -1, 2).astype(np.float64)
        for c, fc in enumerate(ch.offsets.tolist()):
            check_contract_1(v[c, :, 0] + 1j * v[c, :, 1], chanref.channel(host[0], h, D, FS, fc, t0), h, False, (t0, fc))
        if t0 < 0:
            m = -(t0 // FS) + 3
            assert t0 + m * FS >= 0
            assert np.array_equal(raw, run(ch, host, t0=t0 + m * FS, raw=True))
    finally:
        ch.close()


def test_s16_saturates_both_ways(built_lib):
    """x = +-(1 + 1j) turned by 45 degrees: a component of +-1.414, clamped to 32767 and -32768"""
    import pirip_amd
    D = 30
    ch = pirip_amd.HipChan(FS, D, [1], out_s16=True)
    try:
        h = ch.taps()
        n = capture_len(40, D, ch.Lp)
        for byte, clamp in ((255, 32767), (0, -32768)):
            host = np.full((1, n, 2), byte, dtype=np.uint8)
            got = run(ch, host, t0=FS // 8)
            want = chanref.to_s16(chanref.channel(host[0], h, D, FS, 1, FS // 8))
            assert (want[:, 0] == clamp).all() and np.abs(got[0] - want).max() <= 1 and (got[0][:, 0] == clamp).all()
    finally:
        ch.close()


# ---- 5. degenerate sizes and an idle capture -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_s16", [False, True])
def test_one_output_and_none(built_lib, out_s16):
    import torch
    import pirip_amd
    D = 30
    ch = pirip_amd.HipChan(FS, D, OFFS_A, out_s16=out_s16)
    try:
        h = ch.taps()
        host = random_capture(8, 1, ch.Lp)
        got = run(ch, host, t0=12345)
        assert got.shape[1] == 1
        for c, fc in enumerate(OFFS_A):
            check_contract_1(got[c], chanref.channel(host[0], h, D, FS, fc, 12345), h, out_s16, ("one output", fc), vanish=False)
        # no output: the call succeeds and writes nothing (run() checks every byte of the rows, all of them padding)
        for n in (ch.Lp - 1, 0):
            assert ch.nout(n) == 0
            assert run(ch, host[:, :n], raw=True).shape == (len(OFFS_A), 0)
        # n_in = 0 with a buffer that holds nothing else either
        buf = torch.full((64,), FILL, dtype=torch.uint8, device="cuda")
        out = torch.full((len(OFFS_A), OUT_PAD), FILL, dtype=torch.uint8, device="cuda")
        ch.batch(buf.data_ptr(), 2, 0, out.data_ptr(), OUT_PAD)
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == FILL).all()
    finally:
        ch.close()


def test_idle_capture_is_never_read_into_a_channel(built_lib):
    """three captures, channels on 0 and 2 only: the outputs of a two-capture handle on those two, bit for bit, whatever capture 1 holds"""
    import pirip_amd
    D = 30
    offsets, inputs = [-700003, 0, 1, 123457, 1199999, -1], [0, 2, 2, 0, 2, 0]
    ch3 = pirip_amd.HipChan(FS, D, offsets, inputs=inputs)
    ch2 = pirip_amd.HipChan(FS, D, offsets, inputs=[w // 2 for w in inputs])
    try:
        assert ch3.ninputs == 3 and ch2.ninputs == 2
        h = ch3.taps()
        n = capture_len(300, D, ch3.Lp)
        host = random_capture(9, 3, n)
        want = run(ch2, host[[0, 2]], t0=5, raw=True)
        for middle in (host[1], 255 - host[1]):
            host3 = np.stack([host[0], middle, host[2]])
            assert np.array_equal(run(ch3, host3, t0=5, raw=True), want)
        v = want.view(np.float32).reshape(len(offsets), -1, 2).astype(np.float64)
        for c, (w, fc) in enumerate(zip(inputs, offsets)):
            check_contract_1(v[c, :, 0] + 1j * v[c, :, 1], chanref.channel(host[w], h, D, FS, fc, 5), h, False, ("idle capture", w, fc))
    finally:
        ch3.close()
        ch2.close()
