"""The diversity receiver's model (include/pirip_hip.h section Q) RESTATED in numpy: one group of B branches.

Branch clock: {samples = 0, next_nin = nin0}; per row: samples += next_nin; next_nin = (int)stats[6].
Candidate: every row with info[6] = loc >= 0: the n soft bits (binary16) 32 behind window position loc of that call, the branch,
solo_ok = the row's RX_BITS, and tau = t_end * bps - (2 * bpf - loc) * Ts (int, units of 1 / bps sample).
Horizon: H = min over the branches of samples * bps - 2 * bpf * Ts.
Clusters, K = max_skew_samples * bps, repeated: anchor = the pending candidate of smallest (tau, branch); if tau_a + K <= H the cluster
is every pending candidate with tau <= tau_a + K, the earliest of each branch; emitted and removed; stop at the first open anchor.
Combination: float32 adds in ascending branch order from the first member's value, one rounding to float16, NaN -> +0.
Decode: the caller's decoder (oracle_decoder below: OracleLdpc.decode + crc16).

The soft-bit stream of a branch is [2 * bpf zeros | every row's Nbits values]: row c's window starts at (c + 1) * Nbits, so the
codeword of a frame found at loc in row c is stream[(c + 1) * Nbits + loc + 32 :][:n] whatever the cutting into calls was."""
import numpy as np

RX_SYNC, RX_BITS, RX_BIT_ERRORS = 2, 4, 8
ENTRY_FIELDS = ("t_samples", "iters", "pcc", "eraw", "members", "solo_ok", "status")


def combine(rows):
    """rows: float16 arrays in ascending branch order -> their sum as the device forms it"""
    acc = np.asarray(rows[0], dtype=np.float16).astype(np.float32)
    with np.errstate(all="ignore"):
        for r in rows[1:]:
            acc = (acc + np.asarray(r, dtype=np.float16).astype(np.float32)).astype(np.float32)
        out = acc.astype(np.float16)
    out[np.isnan(out)] = np.float16(0.0)
    return out


def oracle_decoder(o):
    """o: oracle.OracleLdpc -> decoder(llr float16 [n]) = (payload uint8 [k / 8], iters, pcc, eraw, status)"""
    k, m = o.code["k"], o.code["n"] - o.code["k"]

    def dec(llr):
        x = np.asarray(llr, dtype=np.float16).astype(np.float32)
        bits, ip = o.decode(x)
        bits = bits[0]
        payload = np.packbits(bits[:k])
        crc_ok = o.crc16(payload[:-2]) == ((int(payload[-2]) << 8) | int(payload[-1]))
        eraw = int(((x < 0) != (bits != 0)).sum())
        status = RX_SYNC | (RX_BITS if crc_ok else 0) | (RX_BIT_ERRORS if int(ip[0, 1]) != m else 0)
        return payload, int(ip[0, 0]), int(ip[0, 1]), eraw, status
    return dec


class DivRef:
    """One group. feed() a call's rows of each branch, then close(); flush() at the end. self.entries: one dict per cluster, in order."""

    def __init__(self, B, bps, Ts, n, Nbits, nin0, max_skew_samples, decoder, pending_capacity=None):
        self.B, self.bps, self.Ts, self.n, self.Nbits, self.bpf = B, bps, Ts, n, Nbits, 32 + n
        self.K = max_skew_samples * bps
        assert 0 <= self.K and 2 * self.K < self.bpf * Ts
        self.decoder, self.cap = decoder, pending_capacity
        self.samples, self.next_nin, self.rows = [0] * B, [nin0] * B, [0] * B
        self.stream = [[np.zeros(2 * self.bpf, dtype=np.float16)] for _ in range(B)]
        self.pending, self.entries, self.combined = [], [], []
        self.dropped = self.max_pending = 0

    # ---- candidates
    def add(self, tau, branch, llr, solo_ok):
        if self.cap is not None and len(self.pending) >= self.cap:
            self.dropped += 1
            return
        self.pending.append(dict(tau=int(tau), branch=int(branch), llr=np.asarray(llr, dtype=np.float16).copy(), solo=bool(solo_ok),
                                 order=len(self.pending)))
        self.max_pending = max(self.max_pending, len(self.pending))

    def feed(self, b, llr_rows, loc, status, nin):
        """a call's valid rows of branch b: soft bits [rows, Nbits] (binary16 values), info[:, 6], status, stats[:, 6]"""
        llr_rows = np.asarray(llr_rows, dtype=np.float32).reshape(-1, self.Nbits).astype(np.float16)
        for f in range(llr_rows.shape[0]):
            self.samples[b] += self.next_nin[b]
            self.next_nin[b] = int(nin[f])
            self.stream[b].append(llr_rows[f])
            c = self.rows[b]
            self.rows[b] += 1
            if int(loc[f]) >= 0:
                s = np.concatenate(self.stream[b])
                at = (c + 1) * self.Nbits + int(loc[f]) + 32
                self.stream[b] = [s]
                tau = self.samples[b] * self.bps - (2 * self.bpf - int(loc[f])) * self.Ts
                self.add(tau, b, s[at:at + self.n], (int(status[f]) & RX_BITS) != 0)

    # ---- clusters
    def horizon(self):
        return min(self.samples) * self.bps - 2 * self.bpf * self.Ts

    def close(self, H=None, flush=False):
        """emit what the horizon closes (H: an explicit horizon, for the boundary cases); returns the new entries"""
        if H is None and not flush:
            H = self.horizon()
        new = []
        while self.pending:
            a = min(self.pending, key=lambda c: (c["tau"], c["branch"]))
            if not flush and a["tau"] + self.K > H:
                break
            members = {}
            for c in sorted(self.pending, key=lambda c: (c["tau"], c["order"])):
                if c["tau"] <= a["tau"] + self.K and c["branch"] not in members:
                    members[c["branch"]] = c
            for c in members.values():
                self.pending.remove(c)
            ms = [members[b] for b in sorted(members)]
            llr = combine([c["llr"] for c in ms])
            payload, iters, pcc, eraw, status = self.decoder(llr)
            e = dict(t_samples=a["tau"] // self.bps, iters=iters, pcc=pcc, eraw=eraw, members=sum(1 << c["branch"] for c in ms),
                     solo_ok=sum(1 << c["branch"] for c in ms if c["solo"]), status=status, payload=payload,
                     taus=[c["tau"] for c in ms])
            self.entries.append(e)
            self.combined.append(llr)
            new.append(e)
        return new

    def flush(self):
        return self.close(flush=True)

    def counters(self, log_entries):
        ok = [e for e in self.entries if e["status"] & RX_BITS]
        return dict(clusters=len(self.entries), bits=len(ok), rescued=sum(1 for e in ok if e["solo_ok"] == 0),
                    members=sum(bin(e["members"]).count("1") for e in self.entries), lost=max(0, len(self.entries) - log_entries),
                    dropped=self.dropped)


def entries_equal(dev_entries, dev_payloads, ref_entries):
    """a device log (structured array + payload rows) against reference entries, field for field; returns a message or None"""
    if len(dev_entries) != len(ref_entries):
        return "count %d != %d" % (len(dev_entries), len(ref_entries))
    for i, (d, r) in enumerate(zip(dev_entries, ref_entries)):
        for f in ENTRY_FIELDS:
            if int(d[f]) != int(r[f]):
                return "entry %d field %s: %d != %d" % (i, f, int(d[f]), int(r[f]))
        if not np.array_equal(dev_payloads[i], r["payload"]):
            return "entry %d payload" % i
    return None
