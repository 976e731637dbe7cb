"""Numpy restatement of pico_tcp_segment_batch_dev's contract (include/pico_csum.h), the checker of
tests/test_gpu_tcpseg.py; tests/test_ref_tcpseg.py pins it to the data segments the compiled
reference stack itself emits for a pico_socket_write (pico_socket_xmit + pico_tcp_push + tcp_send +
pico_ipv4_frame_push).  Sums: oracle.checksum / oracle.dualbuffer_checksum.  Not restated from a
reference run: IPv6 (the frozen driver has no IPv6 link; the same split with struct
pico_ipv6_pseudo_hdr, which the IPv6 RX oracle verifies in tests/test_gpu_tcpseg.py) and segment
sizes other than the three the reference's connections negotiate."""
from __future__ import annotations

import numpy as np

from oracle import oracle as O

V_ACCEPT, V_MALFORMED = 1, 8
DESC_DTYPE = O.DESC_DTYPE


def parse(base: np.ndarray, off: int, ln: int):
    """(N, thl) of a well-formed template at base[off:off + ln], or None -- the checks in the
    contract's order, none reading past ln."""
    if off > base.size or ln > base.size - off or ln < 1:
        return None
    ver = int(base[off]) >> 4
    if ver not in (4, 6):
        return None
    N = 20 if ver == 4 else 40
    if ln < N:
        return None
    if ver == 4 and ((int(base[off]) & 15) != 5 or int(base[off + 9]) != 6):
        return None
    if ver == 6 and int(base[off + 6]) != 6:
        return None
    if ln < N + 20:
        return None
    thl = 4 * (int(base[off + N + 12]) >> 4)
    if thl < 20 or ln < N + thl:
        return None
    return N, thl


def split(P: int, per: int):
    """[(payload offset, payload bytes)] of P payload bytes at per bytes a segment."""
    return [(o, min(per, P - o)) for o in range(0, P, per)] or [(0, 0)]


def frame(tmpl: np.ndarray, N: int, payload: np.ndarray, k: int, o: int) -> np.ndarray:
    """Segment k: the template's H bytes with its own len / id / frag / seq and checksums, then
    `payload` (which starts at stream payload byte o)."""
    h = tmpl.copy()
    H, pl = h.size, payload.size
    tl = H - N + pl
    if N == 20:
        ident = ((int(h[4]) << 8 | int(h[5])) + k) & 0xFFFF
        h[2], h[3], h[4], h[5], h[6], h[7], h[10], h[11] = (H + pl) >> 8, (H + pl) & 0xFF, ident >> 8, ident & 0xFF, 0x40, 0, 0, 0
        c = O.checksum(h[:20])
        h[10], h[11] = c >> 8, c & 0xFF
        ph = np.concatenate([h[12:20], np.array([0, 6, tl >> 8, tl & 0xFF], np.uint8)])
    else:
        h[4], h[5] = tl >> 8, tl & 0xFF
        ph = np.concatenate([h[8:40], np.array([0, 0, tl >> 8, tl & 0xFF, 0, 0, 0, 6], np.uint8)])   # struct pico_ipv6_pseudo_hdr
    seq = (int.from_bytes(bytes(h[N + 4:N + 8]), "big") + o) & 0xFFFFFFFF
    h[N + 4:N + 8] = np.frombuffer(seq.to_bytes(4, "big"), np.uint8)
    h[N + 16] = h[N + 17] = 0
    c = O.dualbuffer_checksum(ph, np.concatenate([h[N:], payload]))
    h[N + 16], h[N + 17] = c >> 8, c & 0xFF
    return np.concatenate([h, payload])


def segment(base, strm, groups, n_seg, out, out_desc, stride, flags=0):
    """The batch on host arrays: writes into `out` (uint8, writable); returns (verdict uint8[n],
    count uint32[n], out_seg DESC[n_seg]).  Slots no group covers stay {0, 0, 0}."""
    assert stride >= 40 and stride % 4 == 0 and flags == 0
    strm = np.ascontiguousarray(strm, dtype=DESC_DTYPE)
    od = np.ascontiguousarray(out_desc, dtype=DESC_DTYPE)
    grp = np.ascontiguousarray(groups, dtype=np.uint32).reshape(-1, 2)
    n = grp.shape[0]
    v, cnt = np.full(n, V_MALFORMED, np.uint8), np.zeros(n, np.uint32)
    of = np.zeros(n_seg, DESC_DTYPE)
    for g in range(n):
        off, ln, per = int(strm["off"][g]), int(strm["len"][g]), int(strm["seed"][g])
        first, reserved = int(grp[g, 0]), int(grp[g, 1])
        oo, cap = int(od["off"][g]), int(od["len"][g])
        slots_in = first <= n_seg and reserved <= n_seg - first
        if slots_in:
            of[first:first + reserved] = 0
        hdr = parse(base, off, ln)
        if hdr is None or per == 0:
            continue
        N, thl = hdr
        H = N + thl
        P = ln - H
        seg0 = min(per, P)
        if (H if N == 20 else thl) + seg0 > 65535 or H + seg0 > stride:
            continue
        count = max(1, -(-P // per))
        last = P - (count - 1) * per
        need = (count - 1) * stride + H + last
        if reserved < count or not slots_in or oo > out.size or cap > out.size - oo or need > cap:
            continue
        tmpl = base[off:off + H]
        for k in range(count):
            o = k * per
            pl = min(per, P - o)
            f = frame(tmpl, N, base[off + H + o:off + H + o + pl], k, o)
            p = oo + k * stride
            out[p:p + f.size] = f
            of[first + k] = (p, f.size, 0)
        v[g], cnt[g] = V_ACCEPT, count
    return v, cnt, of
