"""Conditions that the CPU side alone must meet so that tests/test_ldpc_decoders.py (GPU) cannot pass vacuously: every shape of
tests/ldpcshapes.py reaches the kernel its table says (the host's launch rule restated, not called), the word sets really hold the
iteration counts and failures the max_iter tests are about, the mirror oracle's parity-check counts are what numpy counts on the dense
H, the soft-bit edge values land where they are meant to after binary16 rounding, and the stream recordings list more than 16 / 32
frames per batch. No GPU."""
import os

import numpy as np
import pytest

import ldpcshapes as ls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODE = os.path.join(ROOT, "pirip_amd", "data", "standin_256_512_4.code")
DECODERS = ("generic", "fast", "bank", "auto")
_cache = {}


def _code(oracle, name, max_iter=15):
    key = (name, max_iter)
    if key not in _cache:
        _cache[key] = ls.shape_code(name, oracle.parse_code_file(CODE)["rows"], max_iter)
    return _cache[key]


@pytest.mark.parametrize("name", list(ls.SHAPES))
def test_every_shape_reaches_the_kernel_its_table_says(oracle, name):
    code = _code(oracle, name)
    n, k, _, _, adm, kernels = ls.SHAPES[name]
    assert (code["n"], code["k"]) == (n, k) and k % 8 == 0 and k >= 24 and n - k >= k // 8 and n <= 4096       # the loader's rules
    assert all(len(r) and len(set(r)) == len(r) and max(r) < n for r in code["rows"]) and ls.dense_h(code["rows"], n).sum(0).min() >= 1
    assert ls.admitted(code) == adm and not ls.create_refused(code)
    words = 4 if n == 4096 else 64
    for num_cu in (256, 304, 64):
        got = {d: ls.launch_path(code, d, words, 1, num_cu) for d in DECODERS}
        assert tuple(got[d]["kernel"] for d in ("generic", "fast", "bank")) == kernels
        assert got["auto"]["kernel"] == (kernels[1] if words < num_cu * 32 else kernels[2])
        # a forced fast / bank on a shape without the layout falls through to the generic decoder, the same launch
        if not adm:
            assert got["fast"] == got["bank"] == got["generic"] == got["auto"]


def test_the_shapes_cover_every_reachable_instantiation_and_the_creation_limit(oracle):
    reached = set()
    for name in ls.SHAPES:
        reached |= set(ls.SHAPES[name][5])
    # the codes of test_ldpc.py: (600,296) is 112 bytes over the 80 KB of eight waves, (136,104) has rows above weight 8 (the two-pass loop);
    # decode_kernel<1, true> is unreachable (ldpcshapes.py says why)
    code600 = dict(n=600, k=296, rows=ls.ra_rows(600, 296, 3, 600))
    assert ls.launch_path(code600, "auto", 8, 1, 256)["kernel"] == "decode_kernel<4, false>"
    code136 = dict(n=136, k=104, rows=ls.ra_rows(136, 104, 3, 136))
    assert ls.launch_path(code136, "bank", 8, 1, 256)["kernel"] == "decode_kernel<8, false>" and ls.code_dims(code136)["maxdeg"] > 8
    assert reached >= {"decode_kernel<8, true>", "decode_kernel<8, false>", "decode_kernel<4, true>", "decode_kernel<2, true>", "decode_kernel<4, false>",
                       "decode_kernel<2, false>", "decode_kernel<1, false>", "decode_fast_kernel<4, 6>", "decode_fast_kernel<2, 8>",
                       "decode_bank_kernel<8, 6>", "decode_bank_kernel<8, 8>"}
    n, k, wcol = ls.OVER_LIMIT
    assert ls.create_refused(dict(n=n, k=k, rows=ls.ra_rows(n, k, wcol, 1)))
    assert not ls.create_refused(dict(n=n, k=k, rows=ls.ra_rows(n, k, wcol - 1, 1)))


@pytest.mark.parametrize("num_cu", [256, 304, 64])
def test_the_big_batches_walk_more_than_one_round(oracle, num_cu):
    code = _code(oracle, "ra56")
    p = ls.launch_path(code, "bank", 16 * num_cu + 17, 1, num_cu)
    assert p["kernel"] == "decode_bank_kernel<8, 6>" and p["cps"] == num_cu + 2 > 1 and p["grid"] == (num_cu, 1)      # units > workgroups
    p = ls.launch_path(code, "fast", 4 * 8192 + 5, 1, num_cu)
    assert p["kernel"] == "decode_fast_kernel<4, 6>" and p["grid"] == (8192, 1) and 4 * 8192 + 5 > p["grid"][0] * p["wpb"]
    p = ls.launch_path(code, "generic", 8 * 8192 + 5, 1, num_cu)
    assert p["kernel"] == "decode_kernel<8, true>" and p["grid"] == (8192, 1) and 8 * 8192 + 5 > p["grid"][0] * p["wpb"]
    # the stream path: max_jobs = ncalls * Nbits / bpf + 2 -> chunks per stream 1, 2, 3
    ship = _code(oracle, ls.SHIPPED)
    for ncalls, jobs, cps in zip(ls.STREAM_NCALLS, (13, 20, 35), (1, 2, 3)):
        assert ncalls * 100 // 544 + 2 == jobs
        for ns in (1, 3, num_cu + 1):
            p = ls.launch_path(ship, "bank", jobs, ns, num_cu)
            assert p["cps"] == cps and p["grid"][0] == min(cps * ns, num_cu)
            assert ls.launch_path(ship, "fast", jobs, ns, num_cu)["grid"] == ((jobs + 3) // 4, ns)
            assert ls.launch_path(ship, "generic", jobs, ns, num_cu)["grid"] == ((jobs + 7) // 8, ns)


@pytest.mark.parametrize("name", list(ls.SHAPES))
def test_oracle_parity_counts_are_numpys_and_easy_words_come_back(oracle, name):
    code = _code(oracle, name)
    H = ls.dense_h(code["rows"], code["n"])
    cw, llr, easy = ls.matrix_words(name, code)
    assert not (ls.parity_ok_count(H, cw) != H.shape[0]).any()                 # the encoder's words are codewords of H
    bits, ip = oracle.OracleLdpc(code, 2).decode(llr)
    assert np.array_equal(ip[:, 1], ls.parity_ok_count(H, bits))
    conv = ip[:, 1] == H.shape[0]
    assert conv[easy].sum() >= easy.sum() // 2 and (ip[:, 0] > 1).any()
    if ls.comes_back(name):
        assert np.array_equal(bits[easy & conv], cw[easy & conv])
    print(name, "iterations", np.bincount(ip[:, 0], minlength=16), "unconverged", int((~conv).sum()))


@pytest.mark.parametrize("max_iter", ls.MAX_ITERS)
@pytest.mark.parametrize("name", ls.ITER_SHAPES)
def test_the_max_iter_word_sets_hold_what_they_are_for(oracle, name, max_iter):
    code = _code(oracle, name, max_iter)
    H = ls.dense_h(code["rows"], code["n"])
    m = H.shape[0]
    _, llr = ls.iter_words(name, code)
    bits, ip = oracle.OracleLdpc(code, 2).decode(llr)
    assert np.array_equal(ip[:, 1], ls.parity_ok_count(H, bits))
    conv = ip[:, 1] == m
    hist = np.bincount(ip[conv, 0], minlength=max_iter + 1)
    print(name, max_iter, "converged at", hist[:12], "unconverged", int((~conv).sum()))
    assert all(hist[i] > 0 for i in range(1, min(max_iter, 6) + 1))            # every count 1 .. min(max_iter, 6)
    assert hist[max_iter] > 0                                                  # a word that converges exactly at max_iter
    assert (~conv).sum() >= 3 and (ip[~conv, 0] == max_iter).all()             # ... and words that do not


def test_soft_bit_edge_values_land_on_both_sides_of_every_boundary():
    with np.errstate(over="ignore"):                                          # 1e6 -> inf is the point
        r = np.array(ls.EDGE_VALUES, dtype=np.float32).astype(np.float16).astype(np.float32)
    assert np.array_equal(r, np.array(ls.EDGE_ROUNDED, dtype=np.float32))
    lo = ls.PHI_X_LO
    # below / at / above the lower clamp 9.08e-5 (binary16 has no 9.08e-5: it rounds to the neighbour below); 2^-14 is the table's first bin
    assert r[0] < r[1] < r[2] < r[3] == r[4] < lo < r[5]
    assert r[6] < 10.0 == r[7] < r[8] and r[9] < 16.0 == r[10] and r[11] < 32.0 == r[12]       # the upper clamp, the table's end, the old range's end
    assert r[13] == 65504.0 and np.isinf(r[14])
    ties = np.array([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11], dtype=np.float32).astype(np.float16).astype(np.float32)
    assert ties[0] == 1.0 and ties[1] == 1.0 + 2.0 ** -9                        # ties go to the even mantissa
    for name in (ls.SHIPPED, "unbalanced6"):
        labels, w = ls.edge_words(name, dict(n=512, k=256, rows=[list(range(256 + p, 257 + p)) for p in range(256)]))
        assert len(labels) == w.shape[0] == len(ls.EDGE_VALUES) + 9
        assert np.isnan(w[-4:]).sum(1).tolist() == [1, 50, 1, 50] and np.signbit(w[-2:][np.isnan(w[-2:])]).all()
        assert not np.signbit(w[-4:-2][np.isnan(w[-4:-2])]).any()


@pytest.mark.parametrize("name", [ls.SHIPPED, "unbalanced6"])
def test_oracle_on_the_edge_words(oracle, name):
    """The edge words through the mirror oracle: the parity count stays numpy's, NaN soft bits are erasures (same result as the word with
    +0 in their place), the contradicted infinities end unconverged at max_iter with a finite parity count."""
    code = _code(oracle, name)
    H = ls.dense_h(code["rows"], code["n"])
    labels, w = ls.edge_words(name, code)
    o = oracle.OracleLdpc(code, 2)
    bits, ip = o.decode(w)
    assert np.array_equal(ip[:, 1], ls.parity_ok_count(H, bits))
    b0, ip0 = o.decode(np.where(np.isnan(w), np.float32(0.0), w))
    assert np.array_equal(bits, b0) and np.array_equal(ip, ip0)
    i = labels.index("+-inf, one contradicted")
    assert ip[i, 0] == code["max_iter"] and 0 < ip[i, 1] < H.shape[0]
    for lab in ("all +0", "all -0"):
        assert not bits[labels.index(lab)].any()


def test_stream_recordings_list_more_than_16_and_32_frames(oracle):
    """A batch from the reset state lists a frame once it has slid to the head of the two-frame window, 989 to 1088 bits after its first:
    180 calls of 100 bits list at most 32. The measured batch therefore follows a priming batch of STREAM_PRIME calls, and then holds 33."""
    code = _code(oracle, ls.SHIPPED)
    rec = ls.stream_recording(code, 0)
    assert rec.shape[0] >= ls.STREAM_PRIME + max(ls.STREAM_NCALLS)
    for ncalls, more_than in zip(ls.STREAM_NCALLS, (0, 16, 32)):
        st, _, info = oracle.OracleLdpc(code, ls.STREAM_M, Nsym=ls.STREAM_NSYM).rx(rec[:ls.STREAM_PRIME + ncalls])
        jobs = int((info[ls.STREAM_PRIME:, 6] >= 0).sum())
        print(ncalls, "calls:", jobs, "frames listed; iterations", np.bincount(info[info[:, 6] >= 0, 4]))
        assert jobs > more_than and jobs <= ncalls * 100 // 544 + 2
        assert ((st & 4) != 0).sum() >= jobs - 3 and (info[info[:, 6] >= 0, 4] > 1).any()
