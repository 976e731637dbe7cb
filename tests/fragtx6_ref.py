"""Numpy restatement of pico_ipv6_fragment_batch_dev's contract (include/pico_csum.h), the checker
of tests/test_gpu_fragtx6.py.  The reference cannot fragment IPv6 on the sending side
(stack/pico_socket.c:1179-1185), so nothing it emits can pin the split; its receiver pins it
instead: tests/golden/make_ref_fragtx6.py feeds this restatement's fragments to the compiled
reference's pico_ipv6_process_frag, which gives the datagram back (tests/test_ref_fragtx6.py).
Restatement only: a datagram sent whole (no fragment, no reassembly -- its header is the input's
with the payload length set), and the transport value, which is pico_ipv6_checksum_batch_dev's TX
rule (oracle.batch_ipv6 with tx: computed for TCP / UDP / ICMPv6 with a transport of at least its
header, stored as computed, 0 otherwise).  Sums: oracle.dualbuffer_checksum."""
from __future__ import annotations

import numpy as np

from oracle import oracle as O

V_ACCEPT, V_MALFORMED = 1, 8
F_WRITE = 1
DESC_DTYPE = O.DESC_DTYPE
CRC_AT = {6: 16, 17: 6, 58: 2}
MIN_HDR = {6: 20, 17: 8, 58: 4}
EXT_HDRS = (0, 43, 44, 50, 51, 60, 135)


def split(length: int, mtu: int):
    """(per, [(transport offset, payload bytes)]) of a datagram of `length` bytes, header included."""
    per = (mtu - 48) & ~7
    tl = length - 40
    if length <= mtu:
        return per, [(0, tl)]
    return per, [(o, min(per, tl - o)) for o in range(0, tl, per)]


def transport_checksum(hdr: np.ndarray, t: np.ndarray):
    """(value, crc field offset or -1): the fused IPv6 batch's TX rule on the 40 header bytes `hdr`
    and the transport `t`, the crc field read as zero."""
    proto = int(hdr[6])
    at = CRC_AT.get(proto)
    if at is None or t.size < MIN_HDR[proto]:
        return 0, -1
    t = t.copy()
    t[at] = t[at + 1] = 0
    ph = np.concatenate([hdr[8:40], np.array([0, 0, t.size >> 8, t.size & 0xFF, 0, 0, 0, proto], np.uint8)])
    return O.dualbuffer_checksum(ph, t), at


def fragment(base, dgram, mtu, groups, n_frag, out, out_desc, stride, flags=0):
    """The batch on host arrays: writes into `out` (uint8, writable); returns (verdict uint8[n],
    count uint32[n], transport uint16[n], out_frag DESC[n_frag]).  Slots no group covers stay
    {0, 0, 0}."""
    assert mtu >= 56 and stride % 4 == 0 and not (flags & ~F_WRITE)
    dgram = np.ascontiguousarray(dgram, dtype=DESC_DTYPE)
    od = np.ascontiguousarray(out_desc, dtype=DESC_DTYPE)
    grp = np.ascontiguousarray(groups, dtype=np.uint32).reshape(-1, 2)
    n = grp.shape[0]
    v, cnt, l4 = np.full(n, V_MALFORMED, np.uint8), np.zeros(n, np.uint32), np.zeros(n, np.uint16)
    of = np.zeros(n_frag, DESC_DTYPE)
    for g in range(n):
        off, ln, ident = int(dgram["off"][g]), int(dgram["len"][g]), int(dgram["seed"][g])
        first, reserved = int(grp[g, 0]), int(grp[g, 1])
        oo, cap = int(od["off"][g]), int(od["len"][g])
        if first > n_frag or reserved > n_frag - first:
            continue
        of[first:first + reserved] = 0
        if off > base.size or ln > base.size - off or ln < 40 or ln > 65535:
            continue
        if (base[off] >> 4) != 6 or int(base[off + 6]) in EXT_HDRS:
            continue
        per, parts = split(ln, mtu)
        assert stride >= 48 + per
        whole = ln <= mtu
        hb = 40 if whole else 48
        need = (len(parts) - 1) * stride + hb + parts[-1][1]
        if reserved < len(parts) or oo > out.size or cap > out.size - oo or need > cap:
            continue
        hdr, t = base[off:off + 40], base[off + 40:off + ln].copy()
        l4[g], at = transport_checksum(hdr, t)
        if (flags & F_WRITE) and at >= 0:
            t[at], t[at + 1] = l4[g] >> 8, l4[g] & 0xFF
        for k, (o, pl) in enumerate(parts):
            h = np.zeros(hb, np.uint8)
            h[:40] = hdr
            plen = pl if whole else 8 + pl
            h[4], h[5] = plen >> 8, plen & 0xFF
            if not whole:
                om = o | (1 if k + 1 < len(parts) else 0)
                h[6] = 44
                h[40:48] = [hdr[6], 0, om >> 8, om & 0xFF, ident >> 24, (ident >> 16) & 0xFF, (ident >> 8) & 0xFF, ident & 0xFF]
            p = oo + k * stride
            out[p:p + hb] = h
            out[p + hb:p + hb + pl] = t[o:o + pl]
            of[first + k] = (p, hb + pl, 0)
        v[g], cnt[g] = V_ACCEPT, len(parts)
    return v, cnt, l4, of
