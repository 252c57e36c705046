"""HipPacket: include/pirip_hip.h section R on the binding's one handle base (pirip_amd/binding.py: _Terminal, SIGNATURES, PktConfig,
PktEntry, PktInfo). It never computes on the CPU: send() with lists of bytes stages them on the device, everything else is one C call."""
import ctypes as C

import numpy as np

from .binding import PKT_ENTRY_DTYPE, PktConfig, PktEntry, PktFecConfig, PktFecInfo, PktInfo, _dev, _hip_stream, _ptr_of, _Terminal


class HipPacket(_Terminal):
    """Packet link (include/pirip_hip.h section R): send() cuts packets of up to max_packet bytes into bursts of FSK_LDPC frames that
    wait in a pending ring per transmit channel; per call the received records -- the caller's, or with a HipRx `rx` created with an ldpc
    those of the wideband block -- are put back together into packets in a ring per receive channel, and whole bursts go out through
    HipTxStream `txs` (created on HipTx `tx`). Without tx / txs the handle only receives and every call's out is None. source: src of
    every frame sent; filter: None, or the byte 0 of frames that are not looked at (the terminal's own); address: None (every frame is
    accepted) or the dst that is, besides 0xFF; max_frags: fragments per packet; pending: records of each pending ring (default: two
    packets of max_frags); ring_entries: packets of each receive ring. The handles must outlive the link; pointer arguments take torch
    tensors or raw device pointers, streams default to torch's current stream."""
    _c, _Info = "pirip_hip_pkt", PktInfo

    RX_COUNTERS = ("delivered", "filtered", "foreign", "malformed", "orphan", "incomplete", "crc_fail", "lost")
    TX_COUNTERS = ("sent", "refused", "bad", "pending")

    def __init__(self, rx=None, tx=None, txs=None, nrx=None, source=1, filter=None, address=None, max_frags=100, pending=None, ring_entries=64):
        self.rx, self.tx, self.txs = rx, tx, txs
        if nrx is None:
            nrx = rx.nstreams if rx is not None else 0
        if pending is None:
            pending = 2 * (self._burst_frames(int(max_frags)) + 1)
        cfg = PktConfig(int(nrx), int(source), -1 if filter is None else int(filter), -1 if address is None else int(address), int(max_frags),
                        int(pending), int(ring_entries))
        self._create_link(rx, tx, txs, cfg)
        i = self.info
        self.nrx, self.nchan, self.rx_rows, self.data_bytes, self.ring_entries = i.nrx, i.nchan, i.rx_rows, i.data_bytes, i.ring_entries
        self.cap, self.max_packet, self.max_frags, self.pending = i.cap, i.max_packet, i.max_frags, i.pending_records
        self._staged = None

    def _burst_frames(self, max_frags):
        """frames of the largest burst"""
        return max_frags

    def _create_link(self, rx, tx, txs, cfg):
        name = "pirip_hip_pkt_create"
        self._create(name, _ptr_of(rx, name), _ptr_of(tx, name), _ptr_of(txs, name), C.byref(cfg))

    def send(self, packets, dst, lengths=None, npk=None, taken=None, stream=None):
        """Hand packets to the transmit channels. Either packets is a list with one list of bytes objects per channel and dst an int or a
        matching list of lists -- they are staged on the device here, and the int32 [nchan] tensor of the counts taken is returned --; or
        packets is a uint8 tensor [nchan, max_pk, row bytes], lengths int32 [nchan, max_pk], dst uint8 [nchan, max_pk], npk int32 [nchan]
        or None (every row is a packet) and taken int32 [nchan] or None, all on the device. Enqueued on `stream`; does not synchronise."""
        if not hasattr(packets, "data_ptr"):
            import torch
            if len(packets) != self.nchan:
                raise ValueError("packets: one list per transmit channel")
            max_pk = max([len(q) for q in packets] + [1])
            row = max([len(b) for q in packets for b in q] + [1])
            st = np.zeros((self.nchan, max_pk, row), np.uint8)
            ln, ds, n = np.zeros((self.nchan, max_pk), np.int32), np.zeros((self.nchan, max_pk), np.uint8), np.zeros(self.nchan, np.int32)
            for t, q in enumerate(packets):
                n[t] = len(q)
                for j, b in enumerate(q):
                    st[t, j, :len(b)] = np.frombuffer(bytes(b), np.uint8)
                    ln[t, j] = len(b)
                    ds[t, j] = dst if np.isscalar(dst) else dst[t][j]
            packets, lengths, dst, npk = (torch.from_numpy(x).cuda() for x in (st, ln, ds, n))
            taken = torch.zeros(self.nchan, dtype=torch.int32, device="cuda")
            self._staged = (packets, lengths, dst, npk, taken)           # alive until the next send: the call is only enqueued
        if packets.dim() != 3 or packets.shape[0] != self.nchan or packets.element_size() != 1 or (packets.shape[2] > 1 and packets.stride(2) != 1):
            raise ValueError("packets: uint8 [nchan, max_pk, row bytes]")
        if lengths is None:
            raise ValueError("packets on the device need lengths")
        self._call("pirip_hip_pkt_send", _dev(packets), int(packets.stride(0)), int(packets.stride(1)), _dev(npk), int(packets.shape[1]), _dev(lengths),
                   _dev(dst), _dev(taken), _hip_stream(stream))
        return taken

    def push_records(self, status, payload, out=None, out_stride=0, ncalls=None, max_calls=None, status_stride=None, payload_stride=None, stream=None):
        """status uint8 [nrx, max_calls], payload uint8 [nrx, max_calls, data_bytes] (tensors, per-channel rows contiguous; or raw pointers
        with max_calls and the strides in elements), ncalls int32 [nrx] or None -> the packets, and with tx one block per output at out +
        i * out_stride."""
        if hasattr(status, "shape"):
            max_calls = int(status.shape[1]) if max_calls is None else int(max_calls)
            status_stride = int(status.stride(0)) if status_stride is None else int(status_stride)
            payload_stride = int(payload.stride(0)) if payload_stride is None else int(payload_stride)
        elif None in (max_calls, status_stride, payload_stride):
            raise ValueError("raw pointers need max_calls and the two strides")
        self._call("pirip_hip_pkt_push_records", _dev(status), status_stride, _dev(payload), payload_stride, _dev(ncalls), int(max_calls),
                   _dev(out), int(out_stride), _hip_stream(stream))

    def process(self, out=None, out_stride=0, stream=None):
        """the block at rx.input() -> the packets, and with tx one block per output (needs rx)"""
        super().process(out, out_stride, stream)

    def push(self, d_in, in_stride, out=None, out_stride=0, stream=None):
        """process() after copying the block from d_in (rows in_stride bytes apart) into rx's input"""
        super().push(d_in, in_stride, out, out_stride, stream)

    def records(self):
        """dict of the last call's rows: device pointers status, payload, nframes and the strides in elements"""
        return self._records(("status", "payload"))

    def counters(self):
        """dict of int64 arrays -- [nrx]: delivered, filtered, foreign, malformed, orphan, incomplete, crc_fail, lost; [nchan]: sent,
        refused, bad, pending. Synchronises."""
        out = {k: np.zeros(self.nrx, dtype=np.int64) for k in self.RX_COUNTERS}
        out.update({k: np.zeros(self.nchan, dtype=np.int64) for k in self.TX_COUNTERS})
        self._call("pirip_hip_pkt_get_counters", *(out[k].ctypes.data for k in self.RX_COUNTERS + self.TX_COUNTERS))
        return out

    def packets(self, chan, max=None):
        """the newest packets of receive channel chan, oldest first: (numpy structured array of PKT_ENTRY_DTYPE, list of bytes).
        Synchronises."""
        n = self.ring_entries if max is None else int(max)
        ent = np.zeros(n if n > 1 else 1, dtype=np.dtype(PKT_ENTRY_DTYPE))
        assert ent.dtype.itemsize == C.sizeof(PktEntry) == 24
        data = np.zeros((ent.size, self.max_packet), dtype=np.uint8)
        got = C.c_int(0)
        self._call("pirip_hip_pkt_get_packets", int(chan), ent.ctypes.data, data.ctypes.data, n, C.byref(got))
        ent = ent[:got.value].copy()
        return ent, [data[i, :int(e["length"])].tobytes() for i, e in enumerate(ent)]


class HipPacketFec(HipPacket):
    """HipPacket with parity fragments (include/pirip_hip.h section R, pirip_hip_pkt_create_fec): behind the k data fragments of a packet
    go r(k) = max(1, min(max_parity, ceil(k * parity_pct / 100))) parity fragments, and any k of the k + r put the packet together. Both
    ends are created alike. pending defaults to two bursts of max_frags + r(max_frags) frames; txs must hold one such burst."""

    FEC_COUNTERS = ("recovered", "repaired", "duplicate", "surplus")

    def __init__(self, rx=None, tx=None, txs=None, nrx=None, source=1, filter=None, address=None, max_frags=84, pending=None, ring_entries=64,
                 max_parity=16, parity_pct=20):
        self._fec = PktFecConfig(int(max_parity), int(parity_pct))
        super().__init__(rx, tx, txs, nrx, source, filter, address, max_frags, pending, ring_entries)
        self.max_parity, self.parity_pct, self.max_burst_frames = int(max_parity), int(parity_pct), self.fec_info().max_burst_frames

    def _burst_frames(self, max_frags):
        r = -(-max_frags * self._fec.parity_pct // 100)
        return max_frags + max(1, min(self._fec.max_parity, r))

    def _create_link(self, rx, tx, txs, cfg):
        name = "pirip_hip_pkt_create_fec"
        self._create(name, _ptr_of(rx, name), _ptr_of(tx, name), _ptr_of(txs, name), C.byref(cfg), C.byref(self._fec))

    def fec_info(self):
        """PktFecInfo: enabled, max_parity, parity_pct, max_burst_frames"""
        info = PktFecInfo()
        self._call("pirip_hip_pkt_get_fec_info", C.byref(info))
        return info

    def fec_counters(self):
        """dict of int64 arrays [nrx]: recovered (packets delivered that needed a decode), repaired (data fragments rebuilt in them),
        duplicate, surplus. Synchronises."""
        out = {k: np.zeros(self.nrx, dtype=np.int64) for k in self.FEC_COUNTERS}
        self._call("pirip_hip_pkt_get_fec_counters", *(out[k].ctypes.data for k in self.FEC_COUNTERS))
        return out
