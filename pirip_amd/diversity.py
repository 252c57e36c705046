"""HipDiversity: include/pirip_hip.h section Q on the binding's one handle base (pirip_amd/binding.py: _Handle, SIGNATURES, DivConfig,
DivEntry, DivInfo). It never computes on the CPU: every method is one C call."""
import ctypes as C

import numpy as np

from .binding import DIV_ENTRY_DTYPE, DivConfig, DivEntry, DivInfo, _Handle, _dev, _hip_stream


class HipDiversity(_Handle):
    """Diversity receiver (include/pirip_hip.h section Q): the receivers of HipLdpc `ldpc` in groups of `branches` branches; behind every
    receive call collect() turns the frames the branches listed into candidates tagged on the sample timeline, clusters the candidates of
    one frame (first unique-word bits at most max_skew_samples apart), adds their soft bits and decodes the sum once with ldpc's own
    decoder. One entry per cluster goes to the group's ring. samples_per_symbol: Fs / Rs of the branches' demodulator; nin0: what its
    first call consumes; max_rows: rows per receiver and call (sizes everything). ldpc must outlive the handle; pointer arguments take
    torch tensors or raw device pointers, streams default to torch's current stream."""
    _c, _Info = "pirip_hip_div", DivInfo

    COUNTERS = ("clusters", "bits", "rescued", "members", "lost", "dropped")

    def __init__(self, ldpc, branches, samples_per_symbol, nin0, max_skew_samples, max_rows, log_entries=256):
        self.ldpc = ldpc
        cfg = DivConfig(int(branches), int(samples_per_symbol), int(nin0), int(max_skew_samples), int(max_rows), int(log_entries))
        name = "pirip_hip_div_create"
        self._create(name, ldpc._ptr(name), C.byref(cfg))
        i = self.info
        self.groups, self.branches, self.pending, self.slots, self.n, self.data_bytes = i.groups, i.branches, i.pending, i.slots, i.n, i.data_bytes
        self.log_entries, self.max_rows = i.log_entries, i.max_rows

    def collect(self, status, info, stats, nframes=None, ncalls=None, status_stride=None, info_stride=None, stats_stride=None, stream=None):
        """behind a receive call of ldpc with the same ncalls: status uint8 [nstreams, ncalls], info int32 [nstreams, ncalls, 10], stats
        float32 [nstreams, ncalls, 10] (tensors, per-receiver rows contiguous; or raw pointers with ncalls and the strides in elements),
        nframes int32 [nstreams] or None."""
        if hasattr(status, "shape"):
            ncalls = int(status.shape[1]) if ncalls is None else int(ncalls)
            status_stride = int(status.stride(0)) if status_stride is None else int(status_stride)
            info_stride = int(info.stride(0)) if info_stride is None else int(info_stride)
            stats_stride = int(stats.stride(0)) if stats_stride is None else int(stats_stride)
        elif None in (ncalls, status_stride, info_stride, stats_stride):
            raise ValueError("raw pointers need ncalls and the three strides")
        self._call("pirip_hip_div_collect", _dev(status), status_stride, _dev(info), info_stride, _dev(stats), stats_stride, _dev(nframes),
                   int(ncalls), _hip_stream(stream))

    def push_candidates(self, llr_h16, tag, group_branch, solo_ok, clock_units, ncand=None, stream=None):
        """the layer under collect: llr_h16 float16 [ncand, n], tag int64 [ncand], group_branch int32 [ncand] (g * branches + b),
        solo_ok uint8 [ncand], clock_units int64 [groups * branches] (each branch's clock, samples * bits per symbol)."""
        if ncand is None:
            ncand = int(tag.shape[0]) if tag is not None else 0
        self._call("pirip_hip_div_push_candidates", _dev(llr_h16), _dev(tag), _dev(group_branch), _dev(solo_ok), int(ncand), _dev(clock_units),
                   _hip_stream(stream))

    def flush(self, stream=None):
        """emit everything pending (the horizon at +inf)"""
        self._call("pirip_hip_div_flush", _hip_stream(stream))

    def reset(self, stream=None):
        self._call("pirip_hip_div_reset", _hip_stream(stream))

    def last(self):
        """dict of device pointers to what the last call emitted: entries, entry_stride (entries), payload, payload_stride (bytes), count"""
        pe, pp, pc = C.c_void_p(), C.c_void_p(), C.c_void_p()
        se, sp = C.c_size_t(0), C.c_size_t(0)
        self._call("pirip_hip_div_last", C.byref(pe), C.byref(se), C.byref(pp), C.byref(sp), C.byref(pc))
        return dict(entries=int(pe.value), entry_stride=int(se.value), payload=int(pp.value), payload_stride=int(sp.value), count=int(pc.value))

    def log(self, group, max_entries=None):
        """(entries, payloads) of group `group`, the newest, oldest first: a numpy structured array of DIV_ENTRY_DTYPE and uint8
        [entries, data_bytes]. Synchronises."""
        n = self.log_entries if max_entries is None else int(max_entries)
        out = np.zeros(max(n, 1), dtype=np.dtype(DIV_ENTRY_DTYPE))
        pl = np.zeros((max(n, 1), self.data_bytes), dtype=np.uint8)
        assert out.dtype.itemsize == C.sizeof(DivEntry) == 24
        got = C.c_int(0)
        self._call("pirip_hip_div_get_log", int(group), out.ctypes.data, pl.ctypes.data, n, C.byref(got))
        return out[:got.value].copy(), pl[:got.value].copy()

    def counters(self):
        """dict of int64 arrays [groups]: clusters, bits, rescued, members, lost, dropped. Synchronises."""
        out = {k: np.zeros(self.groups, dtype=np.int64) for k in self.COUNTERS}
        self._call("pirip_hip_div_get_counters", *(out[k].ctypes.data for k in self.COUNTERS))
        return out

    def combined(self, group, slot):
        """the n combined soft bits (float16) of cluster `slot` of group `group` of the last call. Synchronises."""
        out = np.zeros(self.n, dtype=np.float16)
        self._call("pirip_hip_div_get_combined", int(group), int(slot), out.ctypes.data)
        return out
