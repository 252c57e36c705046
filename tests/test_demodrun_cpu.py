"""tests/demodrun.py without a GPU: the shared comparators are as strict as the device tests need them, the resampler's body and the
host read loop do what their callers rely on."""
import copy

import numpy as np
import pytest

from demodrun import host_chunks, resample_at, same_results, same_words, words

ARRAYS = ("bits", "rx_filt", "stats", "Sf", "scalars", "state")


def _nan(payload):
    return np.array([0x7FC00000 | payload], dtype=np.uint32).view(np.float32)


def _result(seed=1):
    rng = np.random.default_rng(seed)
    f = lambda *shape: rng.normal(size=shape).astype(np.float32)
    return {"nframes": 3, "consumed": 3600, "bits": rng.integers(0, 2, (3, 50)).astype(np.uint8), "rx_filt": f(3, 100), "stats": f(3, 10),
            "Sf": f(256), "scalars": f(8), "state": rng.integers(0, 2 ** 32, 13, dtype=np.uint64).astype(np.uint32)}


def _flip(a, i):
    words(a).reshape(-1)[i] ^= 1            # (a view of the array's own memory: the arrays here are contiguous)


def test_words_are_unsigned_words_of_the_item_size():
    assert words(np.zeros(3, np.float32)).dtype == np.uint32 and words(np.zeros(3, np.uint8)).dtype == np.uint8
    assert words(np.zeros(3, np.int64)).dtype == np.uint64 and words(np.zeros((4, 6), np.float32)[:, ::2]).shape == (4, 3)


@pytest.mark.parametrize("case", ["one word", "signed zero", "shape", "dtype", "nan payload"])
def test_same_words_fails_on(case):
    a = np.linspace(1.0, 2.0, 12, dtype=np.float32).reshape(3, 4)
    b = a.copy()
    if case == "one word":
        _flip(b, 7)
    elif case == "signed zero":
        a[1, 2], b[1, 2] = 0.0, -0.0
        assert np.array_equal(a, b)                      # equal by value
    elif case == "shape":
        b = b.reshape(4, 3)
    elif case == "dtype":
        b = b.view(np.uint32)
    else:
        a[0, 0], b[0, 0] = _nan(1)[0], _nan(2)[0]
    assert a.tobytes() == b.tobytes() or case in ("one word", "signed zero", "nan payload")
    with pytest.raises(AssertionError) as e:
        same_words(a, b, "what is compared")
    assert "what is compared" in str(e.value)
    if case == "one word":
        assert "1 of 12 words differ" in str(e.value) and "[1, 3]" in str(e.value), str(e.value)


def test_same_words_passes_on_equal_words_nan_included():
    a = np.linspace(1.0, 2.0, 12, dtype=np.float32)
    a[5] = _nan(5)[0]
    b = a.copy()
    assert not np.array_equal(a, b)                      # (by value a NaN equals nothing)
    same_words(a, b, "nan of equal payload")
    same_words(a[::2], b[::2], "strided views")


def test_same_results_passes_on_a_deep_copy():
    r = _result()
    same_results(r, copy.deepcopy(r), "one result")
    same_results([r, _result(2)], copy.deepcopy([r, _result(2)]), "per stream")


@pytest.mark.parametrize("key", ARRAYS)
def test_same_results_fails_on_one_word_of(key):
    a = [_result(), _result(2)]
    b = copy.deepcopy(a)
    _flip(b[1][key], 3)
    with pytest.raises(AssertionError) as e:
        same_results(a, b, "two runs")
    assert key in str(e.value) and "1 of" in str(e.value)
    same_results(a, b, "the other arrays", keys=[k for k in ARRAYS if k != key])
    with pytest.raises(AssertionError):
        same_results(a, b, "that array alone", keys=[key])


@pytest.mark.parametrize("key", ["consumed", "nframes"])
def test_same_results_fails_on_a_count(key):
    a, b = _result(), _result()
    b[key] += 1
    with pytest.raises(AssertionError):
        same_results(a, b, "counts")
    with pytest.raises(AssertionError):
        same_results(a, b, "counts hold under keys too", keys=("bits",))


@pytest.mark.parametrize("side", [0, 1])
def test_same_results_fails_on_a_key_on_one_side_only(side):
    pair = [_result(), _result()]
    del pair[side]["state"]
    with pytest.raises(AssertionError) as e:
        same_results(pair[0], pair[1], "a lost entry")
    assert "state" in str(e.value)
    with pytest.raises(AssertionError):
        same_results(pair[0], pair[1], "a lost entry, narrowed", keys=("bits",))
    with pytest.raises(AssertionError):
        same_results([_result()], [_result(), _result()], "a lost stream")


def test_resample_at_integer_and_half_positions():
    rng = np.random.default_rng(3)
    x = rng.normal(size=(40, 2)).astype(np.float32)
    i = np.arange(40)
    y = resample_at(x, i.astype(np.float64))
    assert y.dtype == np.float32
    same_words(y, x, "integer positions")
    half = resample_at(x, i[:-1] + 0.5)
    same_words(half, np.float32(0.5) * x[:-1] + np.float32(0.5) * x[1:], "half-way: the float32 mean")
    same_words(resample_at(x[:, 0], np.array([39.0, 2.25])), np.array([x[39, 0], np.float32(0.75) * x[2, 0] + np.float32(0.25) * x[3, 0]]), "1-D, last sample")


class _FakeHandle:
    """demod_host consumes whole frames of FRAME samples and returns the consumed samples as bits"""
    FRAME = 7

    def __init__(self):
        self.seen = []

    def demod_host(self, buf):
        self.seen.append(buf.copy())
        n = buf.shape[0] // self.FRAME
        used = buf[:n * self.FRAME]
        return {"nframes": n, "consumed": n * self.FRAME, "bits": used.reshape(n, 2 * self.FRAME), "stats": np.full((n, 2), len(self.seen), dtype=np.float32)}


@pytest.mark.parametrize("cuts", [[], [3], [7, 14], [1, 2, 20, 33], [10, 10, 45], [50]], ids=lambda c: "-".join(map(str, c)) or "whole")
def test_host_chunks_carries_the_unconsumed_tail(cuts):
    buf = np.arange(2 * 53, dtype=np.uint8).reshape(53, 2)
    h = _FakeHandle()
    r = host_chunks(h, buf, cuts)
    # the pieces it saw: the carry of the call before, then the next chunk
    carry, last = 0, 0
    for piece, cut in zip(h.seen, list(cuts) + [53]):
        same_words(piece, buf[last - carry:cut], "carry + next chunk")
        carry, last = piece.shape[0] % h.FRAME, cut
    assert len(h.seen) == len(cuts) + 1
    assert r["consumed"] == 53 - carry == 49 and r["nframes"] == 7
    # the joined output does not depend on the cuts
    whole = host_chunks(_FakeHandle(), buf, [])
    same_results(r, whole, "cuts", keys=("bits",))
    same_words(r["bits"].reshape(-1, 2), buf[:49], "bits")
    assert r["stats"].shape == (7, 2)
