"""Numpy restatement of pico_ipv4_fragment_batch_dev's contract (include/pico_csum.h), the checker
of tests/test_gpu_fragtx.py; tests/test_ref_fragtx.py pins it to the compiled reference stack's own
fragments (pico_socket_xmit_fragments + pico_ipv4_frame_push) at MTU 1500.  Sums: oracle.checksum /
oracle.dualbuffer_checksum.  Not restated from a reference run: the split of pico_ipv4_rebound_large
(the same rule, which the frozen oracle cannot drive) and MTUs where mtu - 20 is no multiple of 8
(the reference misplaces data there; per = (mtu - 20) & ~7 is the evident intent)."""
from __future__ import annotations

import numpy as np

from oracle import oracle as O

V_ACCEPT, V_MALFORMED = 1, 8
F_WRITE = 1
DESC_DTYPE = O.DESC_DTYPE
CRC_AT = {6: 16, 17: 6, 1: 2}


def split(length: int, mtu: int):
    """(per, [(transport offset, payload bytes)]) of a datagram of `length` bytes, header included."""
    per = (mtu - 20) & ~7
    tl = length - 20
    if length <= mtu:
        return per, [(0, tl)]
    return per, [(o, min(per, tl - o)) for o in range(0, tl, per)]


def transport_checksum(hdr: np.ndarray, t: np.ndarray):
    """(value, crc field offset or -1): the TX rule -- TCP / UDP with the pseudo header of `hdr`,
    ICMPv4 without, 0 otherwise; the crc field reads as zero when it lies inside the transport."""
    proto = int(hdr[9])
    at = CRC_AT.get(proto)
    if at is None:
        return 0, -1
    t = t.copy()
    inside = at + 2 <= t.size
    if inside:
        t[at] = t[at + 1] = 0
    if proto == 1:
        return O.checksum(t), (at if inside else -1)
    ph = np.concatenate([hdr[12:20], np.array([0, proto, t.size >> 8, t.size & 0xFF], np.uint8)])
    return O.dualbuffer_checksum(ph, t), (at if inside else -1)


def fragment(base, dgram, mtu, groups, n_frag, out, out_desc, stride, flags=0):
    """The batch on host arrays: writes into `out` (uint8, writable); returns (verdict uint8[n],
    count uint32[n], transport uint16[n], out_frag DESC[n_frag]).  Slots no group covers stay
    {0, 0, 0}."""
    assert mtu >= 28 and stride % 4 == 0 and not (flags & ~F_WRITE)
    dgram = np.ascontiguousarray(dgram, dtype=DESC_DTYPE)
    od = np.ascontiguousarray(out_desc, dtype=DESC_DTYPE)
    grp = np.ascontiguousarray(groups, dtype=np.uint32).reshape(-1, 2)
    n = grp.shape[0]
    v, cnt, l4 = np.full(n, V_MALFORMED, np.uint8), np.zeros(n, np.uint32), np.zeros(n, np.uint16)
    of = np.zeros(n_frag, DESC_DTYPE)
    for g in range(n):
        off, ln = int(dgram["off"][g]), int(dgram["len"][g])
        first, reserved = int(grp[g, 0]), int(grp[g, 1])
        oo, cap = int(od["off"][g]), int(od["len"][g])
        if first > n_frag or reserved > n_frag - first:
            continue
        of[first:first + reserved] = 0
        if off > base.size or ln > base.size - off or ln < 20 or ln > 65535 or (base[off] & 15) != 5:
            continue
        per, parts = split(ln, mtu)
        assert stride >= 20 + per
        need = (len(parts) - 1) * stride + 20 + parts[-1][1]
        if reserved < len(parts) or oo > out.size or cap > out.size - oo or need > cap:
            continue
        hdr, t = base[off:off + 20], base[off + 20:off + ln].copy()
        l4[g], at = transport_checksum(hdr, t)
        if (flags & F_WRITE) and at >= 0:
            t[at], t[at + 1] = l4[g] >> 8, l4[g] & 0xFF
        for k, (o, pl) in enumerate(parts):
            h = hdr.copy()
            fr = 0x4000 if ln <= mtu else (o >> 3) | (0x2000 if k + 1 < len(parts) else 0)
            h[2], h[3], h[6], h[7], h[10], h[11] = (20 + pl) >> 8, (20 + pl) & 0xFF, fr >> 8, fr & 0xFF, 0, 0
            c = O.checksum(h)
            h[10], h[11] = c >> 8, c & 0xFF
            p = oo + k * stride
            out[p:p + 20] = h
            out[p + 20:p + 20 + pl] = t[o:o + pl]
            of[first + k] = (p, 20 + pl, 0)
        v[g], cnt[g] = V_ACCEPT, len(parts)
    return v, cnt, l4, of
