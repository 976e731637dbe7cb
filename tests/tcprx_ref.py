"""Numpy restatement of pico_tcp_coalesce_batch_dev's contract (include/pico_csum.h), the checker of
tests/test_gpu_tcprx.py, written from the contract and not from the kernel.  The IPv4 network-header
outcomes are the RX oracle's (oracle.batch_ipv4: MALFORMED / NET_BAD / FRAG, in its order); sums:
oracle.checksum / oracle.dualbuffer_checksum.  Not restated from a reference run: see DESIGN.md 5
(IPv6, inconsistent overlaps, groups beyond the reference's queue)."""
from __future__ import annotations

import numpy as np

from oracle import oracle as O

V_ACCEPT, V_NET_BAD, V_L4_BAD, V_MALFORMED, V_FRAG = 1, 2, 4, 8, 16
V_TCP_CTRL, V_TCP_OLD, V_TCP_HELD = 32, 64, 128
DESC_DTYPE = O.DESC_DTYPE
MAX_SEG = 512
M32 = 0xFFFFFFFF


def seq_before(a: int, b: int) -> bool:
    """pico_seq_compare(a, b) < 0 (stack/pico_stack.c:568-591)."""
    if a > b:
        return a - b > 0x7FFFFFFF
    return a < b and b - a <= 0x7FFFFFFF


def classify(base: np.ndarray, off: int, ln: int):
    """One received frame: (verdict, None) or (0, (seq, payload offset in base, payload bytes,
    pseudo header bytes, TCP header offset in base)) for a candidate of the chain."""
    if off > base.size or ln > base.size - off or ln < 1:
        return V_MALFORMED, None
    ver = int(base[off]) >> 4
    if ver == 4:
        if ln < 20:
            return V_MALFORMED, None
        d = np.zeros(1, DESC_DTYPE)
        d["off"], d["len"] = off, ln
        v = int(O.batch_ipv4(base, d)[2][0])
        if v in (V_MALFORMED, V_NET_BAD, V_FRAG):
            return v, None
        ihl = int(base[off]) & 15
        hl = 4 * ihl
        tl = ((int(base[off + 2]) << 8 | int(base[off + 3])) - hl) & 0xFFFF
        if int(base[off + 9]) != 6:
            return V_MALFORMED, None
        ph = np.concatenate([base[off + 12:off + 20], np.array([0, 6, tl >> 8, tl & 0xFF], np.uint8)])
    elif ver == 6:
        if ln < 40 or int(base[off + 6]) != 6:
            return V_MALFORMED, None
        hl = 40
        tl = int(base[off + 4]) << 8 | int(base[off + 5])
        if 40 + tl > ln:
            return V_MALFORMED, None
        ph = np.concatenate([base[off + 8:off + 40], np.array([0, 0, tl >> 8, tl & 0xFF, 0, 0, 0, 6], np.uint8)])
    else:
        return V_MALFORMED, None
    if tl < 20:
        return V_MALFORMED, None
    t = off + hl
    thl = 4 * (int(base[t + 12]) >> 4)
    if thl < 20 or thl > tl:
        return V_MALFORMED, None
    flags, pl = int(base[t + 13]), tl - thl
    if flags not in (0x10, 0x18) or pl == 0:
        return V_TCP_CTRL, None
    return 0, (int.from_bytes(bytes(base[t + 4:t + 8]), "big"), t + thl, pl, ph, t)


def coalesce(base, seg, groups, conn, out, out_desc, flags=0):
    """The batch on host arrays: writes bytes [0, out_len) of every region into `out` (uint8,
    writable) and nothing else; returns (verdict uint8[n], out_len uint32[n], seg_verdict uint8[n_seg]
    -- 0 where no group covers the segment)."""
    assert flags == 0
    seg = np.ascontiguousarray(seg, dtype=DESC_DTYPE)
    od = np.ascontiguousarray(out_desc, dtype=DESC_DTYPE)
    grp = np.ascontiguousarray(groups, dtype=np.uint32).reshape(-1, 2)
    cn = np.ascontiguousarray(conn, dtype=np.uint32).reshape(-1, 2)
    n, n_seg = grp.shape[0], seg.shape[0]
    v, ol, sv = np.full(n, V_MALFORMED, np.uint8), np.zeros(n, np.uint32), np.zeros(n_seg, np.uint8)
    for g in range(n):
        first, cnt = int(grp[g, 0]), int(grp[g, 1])
        rcv, cflags = int(cn[g, 0]), int(cn[g, 1])
        oo, cap = int(od["off"][g]), int(od["len"][g])
        grp_in = first <= n_seg and cnt <= n_seg - first
        if cnt == 0 or cnt > MAX_SEG or not grp_in or oo > out.size or cap > out.size - oo or cflags & ~1:
            if grp_in:
                sv[first:first + cnt] = V_MALFORMED
            continue
        info = []
        for j in range(cnt):
            sv[first + j], c = classify(base, int(seg["off"][first + j]), int(seg["len"][first + j]))
            info.append(c)
        cand = [j for j in range(cnt) if info[j] is not None]
        struck, good = set(), set()
        while True:
            cur, chain, last = rcv, [], -1
            while True:
                hit = next((j for j in cand if j not in struck and (cflags & 1 or j > last) and info[j][0] == cur), None)
                if hit is None or ((cur - rcv) & M32) + info[hit][2] > cap:
                    break
                chain.append(hit)
                cur = (cur + info[hit][2]) & M32
                last = hit
            failed = False
            for j in chain:                                  # pico_tcp_checksum over header + payload
                if j not in good:
                    _, po, pl, ph, t = info[j]
                    if O.dualbuffer_checksum(ph, base[t:po + pl]) == 0:
                        good.add(j)
                    else:
                        struck.add(j)
                        failed = True
            if not failed:
                break
        for j in chain:
            _, po, pl, _, _ = info[j]
            p = oo + ((info[j][0] - rcv) & M32)
            out[p:p + pl] = base[po:po + pl]
        for j in cand:
            sv[first + j] = (V_L4_BAD if j in struck else V_ACCEPT if j in chain
                             else V_TCP_OLD if seq_before(info[j][0], cur) else V_TCP_HELD)
        v[g], ol[g] = V_ACCEPT, (cur - rcv) & M32
    return v, ol, sv


def region_tail_mask(out_size: int, out_desc, verdict, out_len) -> np.ndarray:
    """True for the bytes the contract leaves unspecified: an ACCEPT connection's region bytes past
    out_len (a MALFORMED connection's region is not written at all)."""
    m = np.zeros(out_size, bool)
    for d, v, n in zip(np.ascontiguousarray(out_desc, dtype=DESC_DTYPE), verdict, out_len):
        if int(v) == V_ACCEPT:
            m[int(d["off"]) + int(n):int(d["off"]) + int(d["len"])] = True
    return m
