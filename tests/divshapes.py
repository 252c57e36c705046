"""Rows the diversity tests share (tests/test_diversity_cpu.py holds the reference to them, tests/test_diversity.py the device).

BOUNDARY: the closure rule at its edges, on explicit tags. A case: skew K (bps = 1: K in samples), candidates (tau, branch) in the order
they are pushed, the horizon H of the one call, the clusters that call emits as lists of candidate indices (each in ascending branch
order, clusters in emission order) and the candidates a flush then still emits.

SPECIAL: sums by value. A case: the members' binary16 values in ascending branch order and the binary16 sum -- worked out by hand
from the rule (float32 adds left to right from the first value, one rounding, NaN -> +0), not taken from any implementation."""
import numpy as np

BOUNDARY = {
    # name: (K, [(tau, branch)], H, clusters of the call, clusters of the flush)
    "tag at anchor + K joins": (100, [(1000, 0), (1100, 1)], 10000, [[0, 1]], []),
    "tag at anchor + K + 1 does not": (100, [(1000, 0), (1101, 1)], 10000, [[0], [1]], []),
    "anchor + K == H closes": (100, [(1000, 0), (1050, 1)], 1100, [[0, 1]], []),
    "anchor + K == H + 1 waits": (100, [(1000, 0), (1050, 1)], 1099, [], [[0, 1]]),
    "equal tags order by branch": (100, [(1000, 1), (1000, 0)], 10000, [[1, 0]], []),
    "two of one branch: the later stays and anchors": (100, [(1000, 0), (1040, 0), (1060, 1)], 10000, [[0, 2], [1]], []),
    "the later one waits for its own horizon": (100, [(1000, 0), (1040, 0), (1060, 1)], 1100, [[0, 2]], [[1]]),
    "K = 0": (0, [(1000, 0), (1000, 1), (1001, 1)], 10000, [[0, 1], [2]], []),
    "negative tags": (100, [(-3000, 1), (-2950, 0)], -2850, [[1, 0]], []),
}

F16 = np.float16
INF, NAN = float("inf"), float("nan")
# Eight members whose float32 sum depends on the order. float32's ulp at 2^14 is 2^-9, so 16384 + 2^-10 is a tie and rounds to the even
# 16384. Left to right: 16384 four times over, - 16384 = 0, + 1 = 1, + 2^-10 = 1 + 2^-10 (a binary16 value). The pairwise tree instead:
# (16384 + 2^-10) + (2^-10 + 2^-10) = 16384 + 2^-9; (2^-10 - 16384) + (1 + 2^-10) = -16384 + 1 + 2^-10; total 1 + 3 * 2^-10.
ORDER8 = [16384.0, 2.0 ** -10, 2.0 ** -10, 2.0 ** -10, 2.0 ** -10, -16384.0, 1.0, 2.0 ** -10]
# four members: left to right ((16384 + 2^-10) - 16384) + 2^-10 = 2^-10, the tree (16384 + 2^-10) + (-16384 + 2^-10) = 0
CANCEL4 = [16384.0, 2.0 ** -10, -16384.0, 2.0 ** -10]
# all exact in float32: 2048 + 7 = 2055, a binary16 tie that rounds to the even 2056 -- accumulating in binary16 would stay at 2048
EXACT8 = [2048.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]
SPECIAL = {
    # name: (values in ascending branch order, the binary16 result)
    "inf + -inf is an erasure": ([INF, -INF], 0.0),
    "-inf + -inf stays": ([-INF, -INF], -INF),
    "a sum past 65504 is inf": ([40000.0, 40000.0], INF),
    "a sum just inside stays finite": ([32768.0, 32736.0], 65504.0),
    "-0 + +0 is +0": ([-0.0, 0.0], 0.0),
    "-0 + -0 is -0": ([-0.0, -0.0], -0.0),
    "a NaN member is an erasure": ([NAN, 3.0], 0.0),
    "eight members in ascending order": (ORDER8, 1.0 + 2.0 ** -10),
    "eight members accumulated in float": (EXACT8, 2056.0),
    "left to right, not a tree": (CANCEL4, 2.0 ** -10),
    "one rounding, to nearest even": ([1.0, 2.0 ** -11], 1.0),
    "one rounding, above the tie": ([1.0, 2.0 ** -11, 2.0 ** -20], 1.0 + 2.0 ** -10),
}
SINGLE = [-0.0, 0.0, -INF, INF, 65504.0, 2.0 ** -24, -3.25]      # a cluster of one reproduces its input word for word (NaN aside: erasure)


def same_f16(a, b):
    """binary16 words equal, the sign of zero included"""
    return np.array_equal(np.asarray(a, dtype=F16).view(np.uint16), np.asarray(b, dtype=F16).view(np.uint16))


# ---- branches of one transmission: the same bursts, independently noised, each copy delayed by its own number of samples ---------------
def branch_copies(ob, cfg, M, bursts, ebno_db, seed, delays, silence=4000, amp=14.0):
    """tests/test_ldpc.py's _bursts with len(delays) receivers: u8 IQ [copies][n, 2]. Copy i starts delays[i] samples late and has
    its own noise (seed + i); every copy has the same length."""
    import sigutil
    ts = cfg["Fs"] // cfg["Rs"]
    rng = np.random.default_rng(seed)
    segs = [np.zeros((silence + int(rng.integers(0, ts)), 2), dtype=np.float32)]
    for b in bursts:
        segs.append(sigutil.mod_complex(ob, cfg, b))
        segs.append(np.zeros((silence * 3, 2), dtype=np.float32))
    segs.append(np.zeros((silence * 2, 2), dtype=np.float32))
    x = np.concatenate(segs)
    eb = 4.0 * ts / np.log2(M)
    sigma = np.sqrt(eb / (10 ** (ebno_db / 10.0)) / 2.0)
    out = []
    for i, d in enumerate(delays):
        xi = np.concatenate([np.zeros((d, 2), dtype=np.float32), x, np.zeros((max(delays) - d, 2), dtype=np.float32)])
        noise = np.random.default_rng(seed * 1000 + i).normal(0.0, sigma, xi.shape).astype(np.float32)
        out.append(ob.quantise_cu8(xi + noise, amp=amp))
    return out


def feed_rows(ref, b, rows, lo=0, hi=None):
    """rows lo .. hi - 1 of a branch's rows dict(llr, info, status, stats) into DivRef ref as one call"""
    hi = len(rows["status"]) if hi is None else min(hi, len(rows["status"]))
    if hi > lo:
        ref.feed(b, rows["llr"][lo:hi], rows["info"][lo:hi, 6], rows["status"][lo:hi], rows["stats"][lo:hi, 6])


# the rescue demonstration of tests/test_diversity_cpu.py: found by a search over seeds on the CPU oracle (2-FSK, config 1 with P = 6)
# (seeds 0 .. 5 at 3.8, 4.2 and 4.6 dB all show rescued frames but one; this row: 3 + 3 of 20 frames decode alone, 15 combined, 9 of them rescued;
#  the members' tags lie 36 .. 60 apart around the 37 samples of delay: the demodulators' timing moves in steps of Ts / 4)
RESCUE = dict(ebno_db=4.2, seed=0, frames=10, bursts=2, delays=(0, 37), skew=80)


# The device test's receivers: (M, Nsym, n, k, B); (512,256) is the stand-in code file, the others repeat-accumulate codes that
# ldpcshapes writes. Nsym 272 goes with the stand-in code and the (56,24) code with Nsym 33: pirip_hip_ldpc_create refuses a call of
# more bits than a frame (272 > 88), so that pair cannot be made; (56,24) at 33 bits per call lists several frames per receive call.
# (124,56): n is no multiple of the combine kernel's eight values per lane.
DEVICE_SHAPES = [(2, 50, 512, 256, 2), (4, 50, 512, 256, 3), (2, 33, 512, 256, 3), (2, 272, 512, 256, 2), (2, 33, 56, 24, 2), (2, 50, 124, 56, 3)]
