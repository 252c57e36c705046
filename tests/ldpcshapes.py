"""Code shapes for the three LDPC decoders (pirip_amd/csrc/ldpc_decode.hip) and the host's launch rule RESTATED.

launch_path() restates make_decoder_layout's admission test (fsk_ldpc.cpp) and launch_decode's choice (ldpc_decode.hip) in plain
Python -- it does not call the library. tests/test_ldpc_decoders_cpu.py asserts which kernel every shape below reaches, so a shape
that silently stops reaching its kernel fails without a GPU.

The code writers are deterministic from a seed and write the code-file format of fsk_ldpc.hpp. None of these is a good code: each is
a SHAPE -- row and column weights, sizes against the wave width and the LDS budget -- for a run-time path of the decoders.

Which n reaches which workgroup size of decode_kernel (80 KB rule, column weight 3, n = 2 k): 560: 8 waves (82 032 bytes at (600,296):
that code of test_ldpc.py already runs with 4); 800: 4 waves; 1200: 2 waves; 4096: 1 wave. Register-resident rows (REGIDX) need
m <= 256 and row weight <= 8, which caps E at 2048 and the LDS of two waves at 52 KB: decode_kernel<1, true> cannot be reached by any loadable code; <4, true> and <2, true> are reached by codes of
column weight 1 with m = 256 ((1280,1024) and (1792,1536) below)."""
import numpy as np

# ---- constants of the product, restated (fsk_ldpc.hpp, ldpc_device.hpp, ldpc_decode.hip) --------------------------------------------
FAST_ROWS, FAST_VARS, FAST_ROW_DEG, FAST_COL_DEG = 256, 512, 8, 4
WAVE, ROWS_PER_LANE, DEG_FAST, PHI_N, BANK_CHUNK = 64, 4, 8, 576, 16
ERR_UNSUPPORTED = -6
UW = [(0x1ACFFC1D >> (31 - i)) & 1 for i in range(32)]


def _al16(x):
    return (x + 15) & ~15


def dec_lds_bytes(m, n, E, wpb):
    """decode_kernel's dynamic LDS: index lists (u16), the phi table, per wave Q, messages (f32) and hard bits (u8)."""
    return _al16((m + 1 + n + 1 + 2 * E) * 2) + PHI_N * 4 + wpb * _al16((n + E) * 4 + n)


def fast_lds_bytes(deg, wpb):
    return wpb * ((FAST_VARS + 4) * 4 + (deg * FAST_ROWS + 4) * 4 + FAST_VARS * 2) + (PHI_N + 4) * 4 + 16


def bank_lds_bytes(deg, wpb):
    return PHI_N * 32 * 4 + 16 + wpb * ((FAST_VARS + 4) * 4 + (deg * FAST_ROWS + 4) * 4)


def code_dims(code):
    rows = code["rows"]
    n, k = code["n"], code["k"]
    colw = np.zeros(n, dtype=np.int64)
    for r in rows:
        colw[r] += 1
    return dict(n=n, k=k, m=n - k, E=sum(len(r) for r in rows), maxdeg=max(len(r) for r in rows), maxcol=int(colw.max()))


def admitted(code):
    """make_decoder_layout's admission test: the fast / persistent decoders' storage layout exists."""
    d = code_dims(code)
    return d["m"] <= FAST_ROWS and d["n"] <= FAST_VARS and d["maxdeg"] <= FAST_ROW_DEG and d["maxcol"] <= FAST_COL_DEG


def create_refused(code):
    """pirip_hip_ldpc_create's limit: E > 65535 or the generic decoder's LDS for ONE wave above 160 KB -> PIRIP_ERR_UNSUPPORTED."""
    d = code_dims(code)
    return d["E"] > 65535 or dec_lds_bytes(d["m"], d["n"], d["E"], 1) > 160 * 1024


def _grid_x(slots, wpb, ny):
    gx, want = (slots + wpb - 1) // wpb, 8192 // max(ny, 1)
    return gx if gx <= want else max(want, 1)


def launch_path(code, decoder, slots, nstreams, num_cu, fast_static_lds=0):
    """launch_decode's choice for `slots` job slots (direct mode: codewords) of `nstreams` streams (direct mode: 1) under
    PIRIP_LDPC_DECODER=decoder: dict(family, regidx, wpb, build, grid, cps, kernel). build: the fast / persistent decoders' row-weight
    build (6 | 8), None for the generic decoder; regidx: its register-resident rows, None for the others; cps: the persistent
    decoder's chunks per stream."""
    assert decoder in ("auto", "generic", "fast", "bank")
    d = code_dims(code)
    ok = admitted(code)
    build = (6 if d["maxdeg"] <= 6 else FAST_ROW_DEG) if ok else None
    if ok and (decoder == "bank" or (decoder == "auto" and slots * nstreams >= num_cu * 8 * 4)):
        cps = (slots + BANK_CHUNK - 1) // BANK_CHUNK
        units = cps * nstreams
        assert (units + min(units, num_cu)) * cps < 1 << 32
        assert bank_lds_bytes(build, 8) <= 160 * 1024
        return dict(family="bank", regidx=None, wpb=8, build=build, grid=(min(units, num_cu), 1), cps=cps,
                    kernel="decode_bank_kernel<8, %d>" % build)
    if ok and decoder != "generic" and fast_static_lds == 0:
        wpb = 4
        while wpb > 1 and fast_lds_bytes(build, wpb) > 40 * 1024:
            wpb >>= 1
        return dict(family="fast", regidx=None, wpb=wpb, build=build, grid=(_grid_x(slots, wpb, nstreams), nstreams), cps=None,
                    kernel="decode_fast_kernel<%d, %d>" % (wpb, build))
    wpb = 8
    while wpb > 1 and dec_lds_bytes(d["m"], d["n"], d["E"], wpb) > 80 * 1024:
        wpb >>= 1
    while wpb > 1 and dec_lds_bytes(d["m"], d["n"], d["E"], wpb) > 160 * 1024:
        wpb >>= 1
    assert dec_lds_bytes(d["m"], d["n"], d["E"], wpb) <= 160 * 1024
    regidx = d["m"] <= WAVE * ROWS_PER_LANE and d["maxdeg"] <= DEG_FAST
    return dict(family="generic", regidx=regidx, wpb=wpb, build=None, grid=(_grid_x(slots, wpb, nstreams), nstreams), cps=None,
                kernel="decode_kernel<%d, %s>" % (wpb, "true" if regidx else "false"))


# ---- code writers --------------------------------------------------------------------------------------------------------------------
def write_code(path, n, k, rows, max_iter=15):
    with open(path, "w") as f:
        f.write("# test code\nname TEST_%d_%d\nn %d\nk %d\nmax_iter %d\n" % (k, n, n, k, max_iter))
        f.write("uw " + " ".join(str(b) for b in UW) + "\n")
        f.write("uw_thresh1 4\nuw_thresh2 6\nbad_uw_thresh 1\nrows %d\n" % (n - k))
        for r in rows:
            f.write(" ".join(str(c) for c in sorted(r)) + "\n")


def dense_h(rows, n):
    H = np.zeros((len(rows), n), dtype=np.uint8)
    for r, cols in enumerate(rows):
        H[r, cols] = 1
    return H


def _staircase(rows, k):
    for p in range(len(rows)):
        if p:
            rows[p].append(k + p - 1)
        rows[p].append(k + p)
    return [sorted(r) for r in rows]


def ra_rows(n, k, wcol, seed):
    """A small repeat-accumulate code: every data column in its wcol least-loaded rows (balanced degrees), staircase parity part."""
    rng = np.random.default_rng(seed)
    m = n - k
    rows = [[] for _ in range(m)]
    load = np.zeros(m, dtype=np.int64)
    for c in range(k):
        order = np.lexsort((rng.random(m), load))                  # least-loaded rows first, ties at random: balanced degrees
        for r in order[:wcol]:
            rows[r].append(c)
        load[order[:wcol]] += 1
    return _staircase(rows, k)


def _write_random_code(path, n, k, wcol, seed, max_iter=15):
    """ra_rows as a code file (not a good code: a different SHAPE for the decoder's run-time paths -- row degrees above and below the
    register fast path, a frame length that is not a multiple of 32). Returns the largest row weight."""
    rows = ra_rows(n, k, wcol, seed)
    write_code(path, n, k, rows, max_iter)
    return max(len(r) for r in rows)


def ra_unbalanced_rows(n, k, top, seed):
    """Repeat-accumulate with UNBALANCED weights: data columns of weight 1, 2, 3 and 4 mixed; row 0 holds its own parity column only
    (weight 1: the file format asks for a non-empty row, no more), rows 1 .. top - 1 have weights 2 .. top, the others anything in
    2 .. top; the largest row weight is exactly `top` (6: the weight-6 build with neutral slots; 7: the weight-8 build with one).
    Every column keeps at least one check. Rows get their data-column counts first, then the columns are placed heaviest first, each
    into the rows with the most room left (the greedy realisation of a bipartite degree sequence)."""
    rng = np.random.default_rng(seed)
    m = n - k
    cap = top - 2                                                    # data columns of a row below the staircase's two
    colw = np.array([1 + (c % 4) for c in range(k)])
    rng.shuffle(colw)
    want = np.array([0] + [(p - 1) % (cap + 1) for p in range(1, m)])           # row 0: none; then 0 .. cap cycling
    pinned = top                                                     # rows 0 .. top - 1 keep weights 1, 2 .. top
    while want.sum() != colw.sum():
        p = int(rng.integers(pinned, m))
        if want.sum() < colw.sum() and want[p] < cap:
            want[p] += 1
        elif want.sum() > colw.sum() and want[p] > 0:
            want[p] -= 1
    room = want.copy()
    rows = [[] for _ in range(m)]
    for c in sorted(range(k), key=lambda c: (-colw[c], c)):
        order = sorted(range(m), key=lambda r: (-room[r], rng.random()))
        pick = order[:colw[c]]
        assert all(room[r] > 0 for r in pick), "degree sequence not realisable"
        for r in pick:
            rows[r].append(c); room[r] -= 1
    assert not room.any()
    rows = _staircase(rows, k)
    w = [len(r) for r in rows]
    assert w[0] == 1 and max(w) == top and set(range(1, top + 1)) <= set(w)
    cw = dense_h(rows, n).sum(0)
    assert cw.min() >= 1 and set(cw[:k]) == {1, 2, 3, 4}
    return rows


def random_h_rows(n, k, seed, wcol=3):
    """A NON-accumulator H: every one of the n columns, the last n - k included, sits in wcol least-loaded rows; the parity part is
    not the staircase, so there is no encoder here -- words for it are the all-zero codeword plus noise."""
    rng = np.random.default_rng(seed)
    m = n - k
    rows = [[] for _ in range(m)]
    load = np.zeros(m, dtype=np.int64)
    for c in rng.permutation(n):
        order = np.lexsort((rng.random(m), load))
        for r in order[:wcol]:
            rows[r].append(int(c))
        load[order[:wcol]] += 1
    rows = [sorted(r) for r in rows]
    assert any(k + p not in rows[p] for p in range(m)), "parity part came out as a staircase"
    return rows


def ra_encode(rows, k, data):
    """The accumulator's encoder: parity p = (row p's data bits + parity p - 1) mod 2. data: [.., k] bits -> [.., n] codewords."""
    data = np.atleast_2d(np.asarray(data, dtype=np.uint8))
    m = len(rows)
    par = np.zeros((data.shape[0], m), dtype=np.uint8)
    prev = np.zeros(data.shape[0], dtype=np.uint8)
    for p, cols in enumerate(rows):
        d = [c for c in cols if c < k]
        prev = (data[:, d].sum(1).astype(np.uint8) + prev) & 1
        par[:, p] = prev
    return np.concatenate([data, par], axis=1)


# ---- the shapes ----------------------------------------------------------------------------------------------------------------------
# name -> (n, k, kind, argument, admitted by the fast layout, kernels reached under generic / fast / bank in a 64-word direct decode)
SHIPPED = "shipped"
SHAPES = {
    SHIPPED:          (512, 256, "file", None, True, ("decode_kernel<8, true>", "decode_fast_kernel<4, 6>", "decode_bank_kernel<8, 6>")),
    "ra56":           (56, 24, "ra", 3, True, ("decode_kernel<8, true>", "decode_fast_kernel<4, 6>", "decode_bank_kernel<8, 6>")),
    "ra448":          (448, 192, "ra", 3, True, ("decode_kernel<8, true>", "decode_fast_kernel<4, 6>", "decode_bank_kernel<8, 6>")),
    "unbalanced6":    (512, 256, "unbalanced", 6, True, ("decode_kernel<8, true>", "decode_fast_kernel<4, 6>", "decode_bank_kernel<8, 6>")),
    "unbalanced7":    (200, 104, "unbalanced", 7, True, ("decode_kernel<8, true>", "decode_fast_kernel<2, 8>", "decode_bank_kernel<8, 8>")),
    "random_h":       (512, 256, "random_h", 3, True, ("decode_kernel<8, true>", "decode_fast_kernel<4, 6>", "decode_bank_kernel<8, 6>")),
    "ra560":          (560, 280, "ra", 3, False, ("decode_kernel<8, false>",) * 3),
    "ra800":          (800, 400, "ra", 3, False, ("decode_kernel<4, false>",) * 3),
    "ra1200":         (1200, 600, "ra", 3, False, ("decode_kernel<2, false>",) * 3),
    "ra4096":         (4096, 2048, "ra", 3, False, ("decode_kernel<1, false>",) * 3),
    "ra1280_regidx":  (1280, 1024, "ra", 1, False, ("decode_kernel<4, true>",) * 3),
    "ra1792_regidx":  (1792, 1536, "ra", 1, False, ("decode_kernel<2, true>",) * 3),
}
OVER_LIMIT = (4096, 2048, 6)             # the smallest column weight at n = 4096 whose one-wave LDS passes 160 KB (5 still fits)


def shape_rows(name, shipped_rows=None):
    n, k, kind, arg = SHAPES[name][:4]
    seed = 1000 + n + 7 * k
    if kind == "file":
        return [list(r) for r in shipped_rows]
    if kind == "ra":
        return ra_rows(n, k, arg, seed)
    if kind == "unbalanced":
        return ra_unbalanced_rows(n, k, arg, seed)
    return random_h_rows(n, k, seed, arg)


def shape_code(name, shipped_rows=None, max_iter=15):
    """The parsed-code dict the oracle takes (oracle.binding.parse_code_file's keys), without going through a file."""
    n, k = SHAPES[name][:2]
    rows = shape_rows(name, shipped_rows)
    row_ptr = np.zeros(len(rows) + 1, dtype=np.int32)
    row_ptr[1:] = np.cumsum([len(r) for r in rows])
    return dict(name=name, n=n, k=k, max_iter=max_iter, uw=np.array(UW, dtype=np.uint8), uw_thresh1=4, uw_thresh2=6, bad_uw_thresh=1,
                row_ptr=row_ptr, col_idx=np.array([c for r in rows for c in r], dtype=np.int32), rows=rows, llr_map="upstream")


def is_ra(name):
    return SHAPES[name][2] != "random_h"


def comes_back(name):
    """Whether a converged easy word must be the transmitted one. Not a property of the two codes of column weight 1: two data bits of
    one row and weight 1 are a codeword of weight 2, and the decoder rightly converges on the nearer neighbour."""
    return is_ra(name) and not (SHAPES[name][2] == "ra" and SHAPES[name][3] == 1)


# ---- words ---------------------------------------------------------------------------------------------------------------------------
EASY_SIGMAS = (0.2, 0.3, 0.4)            # Q(1/0.4) = 0.6 % channel errors at most: words the decoder must give back as sent
EDGE_SIGMAS = (0.6, 0.7, 0.8, 0.9, 1.0, 1.3)          # across the decoding edge of a rate-1/2 code


def codewords(name, code, count, rng):
    if not is_ra(name):
        return np.zeros((count, code["n"]), dtype=np.uint8)
    return ra_encode(code["rows"], code["k"], rng.integers(0, 2, (count, code["k"])).astype(np.uint8))


def bpsk_llrs(cw, sigmas, rng):
    """BPSK-like channel LLRs of codewords cw [count, n], word i at noise sigmas[i], clipped to +-24 like the receiver's."""
    sig = np.asarray(sigmas, dtype=np.float64)[:, None]
    y = (1.0 - 2.0 * cw) + rng.normal(0.0, 1.0, cw.shape) * sig
    return np.clip(2.0 * y / sig ** 2, -24, 24).astype(np.float32)


def matrix_words(name, code):
    """Section (a)'s words: half easy, half across the decoding edge; 4 words for n = 4096 so the CPU oracle stays quick.
    Returns (transmitted codewords, LLRs, easy mask)."""
    count = 4 if code["n"] == 4096 else 64
    rng = np.random.default_rng(code["n"] * 31 + code["k"])
    cw = codewords(name, code, count, rng)
    easy = np.arange(count) % 2 == 0
    sig = [EASY_SIGMAS[(i // 2) % 3] if easy[i] else EDGE_SIGMAS[(i // 2) % 6] for i in range(count)]
    return cw, bpsk_llrs(cw, sig, rng), easy


def parity_ok_count(H, bits):
    """Rows of the dense H that each word of bits [count, n] satisfies -- numpy alone, no oracle."""
    return (((bits.astype(np.int64) @ H.T.astype(np.int64)) & 1) == 0).sum(1)


# ---- section (c): max_iter sweeps, vetted by the CPU test ----------------------------------------------------------------------------
MAX_ITERS = (1, 2, 3, 50)
ITER_SHAPES = (SHIPPED, "unbalanced7")
ITER_SIGMAS = (0.3, 0.45, 0.55, 0.62, 0.68, 0.74, 0.8, 0.86, 0.92, 1.0, 1.2, 1.6)
ITER_WORDS = 192
# a word that converges at exactly 50 iterations is one in ~15 000 on the (200,104) code: a block of 64 words, seed found by search, holds one
ITER_LATE_SEED = {"unbalanced7": 256}
ITER_LATE_SIGMAS = (0.7, 0.75, 0.8, 0.85, 0.9, 0.95, 1.0, 0.8)


def iter_words(name, code):
    """The same words for every max_iter of a shape: a sigma sweep from clean to hopeless."""
    rng = np.random.default_rng(code["n"] * 17 + 5)
    cw = codewords(name, code, ITER_WORDS, rng)
    sig = [ITER_SIGMAS[i % len(ITER_SIGMAS)] for i in range(ITER_WORDS)]
    llr = bpsk_llrs(cw, sig, rng)
    if name in ITER_LATE_SEED:
        rng = np.random.default_rng(ITER_LATE_SEED[name])
        cw2 = codewords(name, code, 64, rng)
        cw, llr = np.concatenate([cw, cw2]), np.concatenate([llr, bpsk_llrs(cw2, np.tile(ITER_LATE_SIGMAS, 8), rng)])
    return cw, llr


# ---- section (b): soft-bit edge values -----------------------------------------------------------------------------------------------
PHI_X_LO = np.float32(9.08e-5)
EDGE_VALUES = [2.0 ** -24, 2.0 ** -15, 2.0 ** -14, 1523 * 2.0 ** -24, 9.08e-5, 1524 * 2.0 ** -24, 9.99, 10.0, 10.01, 15.99, 16.0, 31.9, 32.0,
               65504.0, 1e6]
# what each becomes as binary16 (round to nearest even): asserted by the CPU test
EDGE_ROUNDED = [2.0 ** -24, 2.0 ** -15, 2.0 ** -14, 1523 * 2.0 ** -24, 1523 * 2.0 ** -24, 1524 * 2.0 ** -24, 9.9921875, 10.0, 10.0078125,
                15.9921875, 16.0, 31.90625, 32.0, 65504.0, np.inf]
NAN_POS = np.uint32(0x7FC00000).view(np.float32)
NAN_NEG = np.uint32(0xFFC00000).view(np.float32)


def edge_words(name, code):
    """One word per case: signs from a codeword with ~3 % flips, every magnitude the case value (the first iteration's q is then exactly
    it); then the zero, infinity, rounding-tie and NaN words. Returns (labels, LLRs [count, n] float32)."""
    n = code["n"]
    rng = np.random.default_rng(n + 99)
    cw = codewords(name, code, 1, rng)[0]
    flips = rng.random(n) < 0.03
    sign = np.where((cw ^ flips) != 0, -1.0, 1.0).astype(np.float32)
    clean = np.where(cw != 0, -1.0, 1.0).astype(np.float32)
    labels, words = [], []
    for v in EDGE_VALUES:
        labels.append("mag %g" % v); words.append(sign * np.float32(v))
    labels.append("all +0"); words.append(np.zeros(n, dtype=np.float32))
    labels.append("all -0"); words.append(-np.zeros(n, dtype=np.float32))
    w = np.where(rng.random(n) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    strong = rng.choice(n, 12, replace=False)
    w[strong] = clean[strong] * np.float32(20.0)
    labels.append("mixed +-0, 12 strong"); words.append(w)
    w = clean * np.float32(1e6)                                    # +-inf as binary16, one bit against its checks
    w[n // 3] = -w[n // 3]
    labels.append("+-inf, one contradicted"); words.append(w)
    tie = np.where(np.arange(n) % 2 == 0, np.float32(1.0 + 2.0 ** -11), np.float32(1.0 + 3 * 2.0 ** -11))
    labels.append("rounding ties"); words.append(sign * tie.astype(np.float32))
    base = sign * np.float32(3.0)
    for nan, tag in ((NAN_POS, "+NaN"), (NAN_NEG, "-NaN")):
        for cnt in (1, 50):
            w = base.copy()
            w[rng.choice(n, cnt, replace=False)] = nan
            labels.append("%s x %d" % (tag, cnt)); words.append(w)
    out = np.stack(words).astype(np.float32)
    assert np.signbit(out[labels.index("all -0")]).all() and np.signbit(out[labels.index("-NaN x 50")]).sum() >= 50
    return labels, out


# ---- sections (e), (f): synthetic soft decisions of a continuous burst -----------------------------------------------------------------
STREAM_M, STREAM_NSYM, STREAM_FRAMES, STREAM_PRIME = 4, 50, 40, 11
STREAM_NCALLS = (60, 100, 180)           # max_jobs = ncalls * 100 / 544 + 2 = 13, 20, 35: cps = 1, 2, 3


def stream_recording(code, seed, ebno_db=6.5):
    """Rician magnitudes [calls, M * Nsym] of STREAM_FRAMES back-to-back frames (unique word + codeword) of the accumulator code
    `code`, 4-FSK, 50 symbols per call -- what fsk_demod_sd would hand over; no demodulator involved."""
    rng = np.random.default_rng(seed)
    M, Nsym = STREAM_M, STREAM_NSYM
    data = rng.integers(0, 2, (STREAM_FRAMES, code["k"])).astype(np.uint8)
    for d in data:                                                   # the last 16 data bits: CRC-16/CCITT-FALSE of the bytes before them
        crc = 0xFFFF
        for byte in np.packbits(d[:-16]):
            x = ((crc >> 8) ^ int(byte)) & 0xFF
            x ^= x >> 4
            crc = ((crc << 8) ^ (x << 12) ^ (x << 5) ^ x) & 0xFFFF
        d[-16:] = [(crc >> (15 - i)) & 1 for i in range(16)]
    cw = ra_encode(code["rows"], code["k"], data)
    bits = np.concatenate([np.concatenate([np.array(UW, dtype=np.uint8), c]) for c in cw])
    nsym = bits.size // 2
    sym = bits[:nsym * 2].reshape(nsym, 2)
    sym = sym[:, 0] * 2 + sym[:, 1]
    ncalls = nsym // Nsym
    sym = sym[:ncalls * Nsym].reshape(ncalls, Nsym)
    esn0 = 2 * 10 ** (ebno_db / 10.0)
    z = (rng.normal(size=(ncalls, M, Nsym)) + 1j * rng.normal(size=(ncalls, M, Nsym))) / np.sqrt(2)
    ci, si = np.meshgrid(np.arange(ncalls), np.arange(Nsym), indexing="ij")
    z[ci, sym, si] += np.sqrt(esn0)
    return (np.abs(z) * 0.37).astype(np.float32).reshape(ncalls, M * Nsym)


def stream_valid_counts(nstreams, ncalls):
    """Ragged valid-call counts of the measured batch: all, none and a shorter one, cycled (3 against the 8 recordings: 24 pairs)."""
    pat = [ncalls, 0, ncalls - 37]
    return np.array([pat[s % 3] if nstreams > 1 else ncalls for s in range(nstreams)], dtype=np.int32)
