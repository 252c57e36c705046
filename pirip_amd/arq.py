"""HipArq: include/pirip_hip.h section S on the binding's one handle base (pirip_amd/binding.py: _Handle, SIGNATURES, ArqConfig, ArqEntry,
ArqInfo). It never computes on the CPU: submit() with lists of bytes stages them on the device, everything else is one C call."""
import ctypes as C

import numpy as np

from .binding import ARQ_ENTRY_DTYPE, ArqConfig, ArqEntry, ArqInfo, _dev, _Handle, _hip_stream


class HipArq(_Handle):
    """Selective-repeat ARQ sessions (include/pirip_hip.h section S) over one HipPacket or HipPacketFec `pkt` that has a transmitter and as
    many receive as transmit channels: transmit channel t and receive channel t form one session with the peer address peers[t] (0 .. 255,
    or None / -1 for whoever answers; one value for all channels or one per channel). window: segments in flight, 1 .. 32; rto: calls after
    which an unacknowledged segment is sent again; max_tries: transmissions of one segment before the session is broken; queue_entries:
    segments of a channel's submit queue (default: 2 * window); out_entries: segments of a channel's output ring. While the HipArq lives
    its pkt must not be driven directly, and pkt must outlive it. Pointer arguments take torch tensors or raw device pointers, streams
    default to torch's current stream."""
    _c, _Info = "pirip_hip_arq", ArqInfo

    SENDER_COUNTERS = ("sent", "retransmitted", "acked", "acks_sent", "deferred", "refused", "bad", "broken", "waiting", "inflight")
    RECEIVER_COUNTERS = ("delivered", "duplicate", "outside", "stale", "alien", "stranger", "malformed", "overrun", "lost")

    def __init__(self, pkt, peers, window=8, rto=16, max_tries=8, queue_entries=None, out_entries=64):
        self.pkt = pkt
        nchan = int(pkt.nchan)
        pr = np.ascontiguousarray([-1 if p is None else int(p) for p in (peers if hasattr(peers, "__len__") else [peers] * nchan)], dtype=np.intc)
        if pr.size != nchan:
            raise ValueError("peers: one value, or one per channel")
        if queue_entries is None:
            queue_entries = 2 * int(window)
        cfg = ArqConfig(int(window), int(rto), int(max_tries), int(queue_entries), int(out_entries))
        name = "pirip_hip_arq_create"
        self._create(name, pkt._ptr(name), C.byref(cfg), pr.ctypes.data)
        i = self.info
        self.nchan, self.window, self.rto, self.max_tries = i.nchan, i.window, i.rto_calls, i.max_tries
        self.queue_entries, self.out_entries, self.max_payload, self.acklen = i.queue_entries, i.out_entries, i.max_payload, i.acklen
        self._staged = None

    def submit(self, segments, lengths=None, nseg=None, taken=None, stream=None):
        """Hand segments to the sessions. Either segments is a list with one list of bytes objects per channel -- they are staged on the
        device here, and the int32 [nchan] tensor of the counts taken is returned --; or segments is a uint8 tensor [nchan, max_seg, row
        bytes], lengths int32 [nchan, max_seg], nseg int32 [nchan] or None (every row is a segment) and taken int32 [nchan] or None, all on
        the device. Enqueued on `stream`; does not synchronise."""
        if not hasattr(segments, "data_ptr"):
            import torch
            if len(segments) != self.nchan:
                raise ValueError("segments: one list per channel")
            max_seg = max([len(q) for q in segments] + [1])
            row = max([len(b) for q in segments for b in q] + [1])
            st, ln, n = np.zeros((self.nchan, max_seg, row), np.uint8), np.zeros((self.nchan, max_seg), np.int32), np.zeros(self.nchan, np.int32)
            for t, q in enumerate(segments):
                n[t] = len(q)
                for j, b in enumerate(q):
                    st[t, j, :len(b)] = np.frombuffer(bytes(b), np.uint8)
                    ln[t, j] = len(b)
            segments, lengths, nseg = (torch.from_numpy(x).cuda() for x in (st, ln, n))
            taken = torch.zeros(self.nchan, dtype=torch.int32, device="cuda")
            self._staged = (segments, lengths, nseg, taken)              # alive until the next submit: the call is only enqueued
        if segments.dim() != 3 or segments.shape[0] != self.nchan or segments.element_size() != 1 or (segments.shape[2] > 1 and segments.stride(2) != 1):
            raise ValueError("segments: uint8 [nchan, max_seg, row bytes]")
        if lengths is None:
            raise ValueError("segments on the device need lengths")
        self._call("pirip_hip_arq_submit", _dev(segments), int(segments.stride(0)), int(segments.stride(1)), _dev(nseg), int(segments.shape[1]),
                   _dev(lengths), _dev(taken), _hip_stream(stream))
        return taken

    def push_records(self, status, payload, out=None, out_stride=0, ncalls=None, max_calls=None, status_stride=None, payload_stride=None, stream=None):
        """HipPacket.push_records' arguments: one call of the sessions around the packet handle's."""
        if hasattr(status, "shape"):
            max_calls = int(status.shape[1]) if max_calls is None else int(max_calls)
            status_stride = int(status.stride(0)) if status_stride is None else int(status_stride)
            payload_stride = int(payload.stride(0)) if payload_stride is None else int(payload_stride)
        elif None in (max_calls, status_stride, payload_stride):
            raise ValueError("raw pointers need max_calls and the two strides")
        self._call("pirip_hip_arq_push_records", _dev(status), status_stride, _dev(payload), payload_stride, _dev(ncalls), int(max_calls),
                   _dev(out), int(out_stride), _hip_stream(stream))

    def process(self, out, out_stride, stream=None):
        """the block at pkt.rx.input() -> one call, one block per output (pkt needs rx)"""
        self._call("pirip_hip_arq_process", _dev(out), int(out_stride), _hip_stream(stream))

    def push(self, d_in, in_stride, out, out_stride, stream=None):
        """process() after copying the block from d_in (rows in_stride bytes apart) into pkt.rx's input"""
        self._call("pirip_hip_arq_push", _dev(d_in), int(in_stride), _dev(out), int(out_stride), _hip_stream(stream))

    def counters(self):
        """dict of int64 arrays [nchan]: SENDER_COUNTERS and RECEIVER_COUNTERS. Synchronises."""
        names = self.SENDER_COUNTERS + self.RECEIVER_COUNTERS
        out = {k: np.zeros(self.nchan, dtype=np.int64) for k in names}
        self._call("pirip_hip_arq_get_counters", *(out[k].ctypes.data for k in names))
        return out

    def delivered(self, chan, max=None):
        """the newest segments of channel chan, oldest first: (numpy structured array of ARQ_ENTRY_DTYPE, list of bytes). Synchronises."""
        n = self.out_entries if max is None else int(max)
        ent = np.zeros(n if n > 1 else 1, dtype=np.dtype(ARQ_ENTRY_DTYPE))
        assert ent.dtype.itemsize == C.sizeof(ArqEntry) == 16
        data = np.zeros((ent.size, self.max_payload), dtype=np.uint8)
        got = C.c_int(0)
        self._call("pirip_hip_arq_get_delivered", int(chan), ent.ctypes.data, data.ctypes.data, n, C.byref(got))
        ent = ent[:got.value].copy()
        return ent, [data[i, :int(e["length"])].tobytes() for i, e in enumerate(ent)]

    def state(self, chan):
        """checking aid: dict sub_nxt, snd_nxt, snd_una, rcv_nxt (absolute), held (bit i: segment rcv_nxt + 1 + i), ack_pending.
        Synchronises."""
        v = [C.c_int64(0) for _ in range(4)]
        held, pend = C.c_uint32(0), C.c_int(0)
        self._call("pirip_hip_arq_get_state", int(chan), *(C.byref(x) for x in v), C.byref(held), C.byref(pend))
        return dict(sub_nxt=v[0].value, snd_nxt=v[1].value, snd_una=v[2].value, rcv_nxt=v[3].value, held=held.value, ack_pending=pend.value)

    def reset(self, stream=None):
        """forgets the sessions and resets pkt too"""
        self._call("pirip_hip_arq_reset", _hip_stream(stream))
