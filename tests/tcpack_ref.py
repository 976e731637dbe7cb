"""Numpy restatement of pico_tcp_ack_batch_dev's contract (include/pico_csum.h), the checker of
tests/test_gpu_tcpack.py, written from the contract and not from the kernel.  Its inputs are the
coalescing's outputs (tests/tcprx_ref.coalesce); segment parsing and sums are tcprx_ref.classify's and
the oracle's.  Pinned to the compiled reference stack's own ACK frames by tests/test_ref_tcpack.py;
shift > 0 (more than 64 KiB of receive space) and IPv6 are pinned by this restatement alone: the
reference's queue is 16 KiB and the fixture's stack speaks IPv4."""
from __future__ import annotations

import numpy as np

from oracle import oracle as O
from tests import tcprx_ref as R

V_ACCEPT, V_L4_BAD, V_MALFORMED = R.V_ACCEPT, R.V_L4_BAD, R.V_MALFORMED
V_TCP_CTRL, V_TCP_OLD, V_TCP_HELD = R.V_TCP_CTRL, R.V_TCP_OLD, R.V_TCP_HELD
DESC_DTYPE = R.DESC_DTYPE
ACK_DTYPE = np.dtype([("space", "<u4"), ("tsval", "<u4"), ("tsecr", "<u4"), ("aflags", "<u4")])
assert ACK_DTYPE.itemsize == 16
MAX_SEG = R.MAX_SEG
M32 = R.M32


def sack_prepare(queue, rcv_nxt: int):
    """tcp_sack_prepare (modules/pico_tcp.c:1597-1657) restated literally, with the reference's own
    first_segment / next_segment (:161-179): queue = [(seq, payload_len)] in tree order, unique by seq;
    returns the blocks [(left, right)] in the order tcp_add_sack_option emits them.  The quirks are the
    reference's: next_segment is peek_segment(seq + payload_len) -- the segment that starts exactly
    where this one ends, or none -- so the walk follows ONE contiguous run from the first segment and
    ends at its first gap (in practice at most one block); at most 3 blocks; each block is pushed to
    the FRONT of the list; the segment that breaks a run closes the block and is itself skipped;
    left == 0 means "no open block"; `pkt->seq < rcv_nxt` is a raw compare."""
    def next_segment(i):
        t = (queue[i][0] + queue[i][1]) & M32
        return next((k for k in range(i + 1, len(queue)) if queue[k][0] == t), None)   # (tree order: it lies ahead)

    sacks, left, right, n = [], 0, 0, 0
    i = 0 if queue else None
    while n < 3:
        if i is None:
            if left:
                sacks.insert(0, (left, right))
                n += 1
            break
        seq, pl = queue[i]
        i = next_segment(i)
        if seq < rcv_nxt:
            continue
        if not left:
            left, right = seq, (seq + pl) & M32
            continue
        if seq == right:
            right = (right + pl) & M32
            continue
        sacks.insert(0, (left, right))
        n += 1
        left = right = 0
    return sacks


def window(space: int, out_len: int, held: int):
    """tcp_set_space (:681-700) after the burst: (rwnd, shift)."""
    s, shift = max(0, space - out_len - held), 0
    while s > 0xFFFF:
        s >>= 1
        shift += 1
    return s, shift


def options(shift: int, ts_ok: bool, tsval: int, tsecr: int, blocks) -> bytes:
    """tcp_options_size (:703-731) + tcp_add_options (:582-617) for flags = ACK."""
    size = 3 + (10 if ts_ok else 0) + 1 + (2 + 8 * len(blocks) if blocks else 0)
    size = (size + 3) >> 2 << 2
    o = bytearray([1] * size)
    b = bytes([3, 3, shift])
    if ts_ok:
        b += bytes([8, 10]) + tsval.to_bytes(4, "big") + tsecr.to_bytes(4, "big")
    if blocks:
        b += bytes([5, 2 + 8 * len(blocks)]) + b"".join(l.to_bytes(4, "big") + r.to_bytes(4, "big") for l, r in blocks)
    o[:len(b)] = b
    if len(b) < size:
        o[size - 1] = 0
    return bytes(o)


def template_ok(tb: np.ndarray, off: int, ln: int):
    """The family checks in the segmentation batch's order: (N, v6) or None."""
    if off > tb.size or ln > tb.size - off or ln < 1:
        return None
    ver = int(tb[off]) >> 4
    if ver not in (4, 6):
        return None
    n = 40 if ver == 6 else 20
    if ln < n:
        return None
    if ver == 6 and int(tb[off + 6]) != 6:
        return None
    if ver == 4 and (int(tb[off]) & 15 != 5 or int(tb[off + 9]) != 6):
        return None
    if ln < n + 20:
        return None
    return n, ver == 6


def frame(t: np.ndarray, n: int, v6: bool, ack: int, rwnd: int, opts: bytes) -> np.ndarray:
    """The ACK frame from the template's n + 20 bytes."""
    thl = 20 + len(opts)
    f = np.concatenate([t[:n + 20], np.frombuffer(opts, np.uint8)]).astype(np.uint8)
    if v6:
        f[4:6] = [thl >> 8, thl & 0xFF]
        ph = np.concatenate([f[8:40], np.array([0, 0, thl >> 8, thl & 0xFF, 0, 0, 0, 6], np.uint8)])
    else:
        f[2:4] = [(20 + thl) >> 8, (20 + thl) & 0xFF]
        f[6:8] = [0x40, 0]
        f[10:12] = 0
        c = O.checksum(f[:20])
        f[10:12] = [c >> 8, c & 0xFF]
        ph = np.concatenate([f[12:20], np.array([0, 6, thl >> 8, thl & 0xFF], np.uint8)])
    x = f[n:]
    x[8:12] = list(ack.to_bytes(4, "big"))
    x[12] = ((thl << 2) | (int(x[12]) & 0x0F)) & 0xFF
    x[13] = 0x10
    x[14:16] = [rwnd >> 8, rwnd & 0xFF]
    x[16:18] = 0
    c = O.dualbuffer_checksum(ph, x)
    x[16:18] = [c >> 8, c & 0xFF]
    return f


def ack_batch(base, seg, groups, conn, out_len, seg_verdict, tmpl_base, tmpl, ack, out, out_desc, flags=0):
    """The batch on host arrays: writes every due ACK frame into `out` (uint8, writable) and nothing
    else; returns (verdict uint8[n], out_ack DESC[n], seg_verdict uint8[n_seg] -- a new array)."""
    assert flags == 0
    seg = np.ascontiguousarray(seg, dtype=DESC_DTYPE)
    td = np.ascontiguousarray(tmpl, dtype=DESC_DTYPE)
    od = np.ascontiguousarray(out_desc, dtype=DESC_DTYPE)
    ak = np.ascontiguousarray(ack, dtype=ACK_DTYPE)
    grp = np.ascontiguousarray(groups, dtype=np.uint32).reshape(-1, 2)
    cn = np.ascontiguousarray(conn, dtype=np.uint32).reshape(-1, 2)
    sv = np.array(seg_verdict, dtype=np.uint8, copy=True)
    n, n_seg = grp.shape[0], seg.shape[0]
    v, oa = np.full(n, V_MALFORMED, np.uint8), np.zeros(n, DESC_DTYPE)
    for g in range(n):
        first, cnt = int(grp[g, 0]), int(grp[g, 1])
        rcv0, cflags = int(cn[g, 0]), int(cn[g, 1])
        oo, cap = int(od["off"][g]), int(od["len"][g])
        aflags = int(ak["aflags"][g])
        if cnt == 0 or cnt > MAX_SEG or not (first <= n_seg and cnt <= n_seg - first) or cflags & ~1 or aflags & ~1:
            continue
        tk = template_ok(tmpl_base, int(td["off"][g]), int(td["len"][g]))
        if tk is None or oo > out.size or cap > out.size - oo:
            continue
        N, v6 = tk
        rcv = (rcv0 + int(out_len[g])) & M32
        new, due, queue = {}, False, []
        for j in range(first, first + cnt):
            x = int(sv[j])
            if x == V_ACCEPT:
                due = True
            if x not in (V_TCP_OLD, V_TCP_HELD):
                continue
            st, c = R.classify(base, int(seg["off"][j]), int(seg["len"][j]))
            if st != 0:
                continue                                     # not the coalescing's verdict: left alone
            sq, po, pl, ph, t = c
            if O.dualbuffer_checksum(ph, base[t:po + pl]) != 0:
                new[j] = V_L4_BAD
                continue
            due = True
            if x == V_TCP_HELD and cflags & 1 and all(q[0] != sq for q in queue):
                queue.append((sq, pl))
        flen = 0
        if due:
            queue.sort(key=lambda q: (q[0] - rcv) & M32)
            blocks = sack_prepare(queue, rcv)
            rwnd, shift = window(int(ak["space"][g]), int(out_len[g]), sum(q[1] for q in queue))
            opts = options(shift, bool(aflags & 1), int(ak["tsval"][g]), int(ak["tsecr"][g]), blocks)
            flen = N + 20 + len(opts)
            if flen > cap:
                continue
            to = int(td["off"][g])
            out[oo:oo + flen] = frame(tmpl_base[to:to + N + 20], N, v6, rcv, rwnd, opts)
            oa[g] = (oo, flen, 0)
        for j, x in new.items():
            sv[j] = x
        v[g] = V_ACCEPT
    return v, oa, sv

