"""Numpy restatement of pico_icmp6_reply_batch_dev's contract (include/pico_csum.h), the checker of
tests/test_gpu_icmp6.py, written from the contract and the reference's lines, not from the kernel; the
sums and the extension-header walk are the oracle's.  Pinned to the compiled reference stack's own answers
by tests/test_ref_icmp6.py (tests/golden/ref_icmp6_cases.npz).  Pinned by this restatement alone: Packet
Too Big (type 2: the reference sends nothing, documented difference 2), the trailer rule (difference 1) and
whatever tests/golden/make_ref_icmp6.py names as not captured."""
from __future__ import annotations

import numpy as np

from oracle import oracle as O

V_ACCEPT, V_MALFORMED, V_UNTOUCHED = 1, 8, 32
DESC_DTYPE = np.dtype([("off", "<u8"), ("len", "<u4"), ("seed", "<u4")])
REQ_DTYPE = np.dtype([("src", "u1", 16), ("arg", "<u4"), ("type", "u1"), ("code", "u1"), ("hop", "u1"), ("rsvd", "u1")])
assert REQ_DTYPE.itemsize == 24
QUOTE_MAX = 1280 - 40 - 8          # PICO_IPV6_MIN_MTU less the IPv6 header and the ICMPv6 header (pico_icmp6.c:169-170)


def icmp6_crc(src: bytes, dst: bytes, t: bytearray) -> None:
    """pico_icmp6_checksum (modules/pico_icmp6.c:38-55): crc = 0, then short_be of the dual-buffer checksum
    over struct pico_ipv6_pseudo_hdr (src, dst, long_be(len), zero[3], nxthdr 58) and the transport."""
    t[2:4] = b"\0\0"
    ps = src + dst + len(t).to_bytes(4, "big") + b"\0\0\0\x3a"
    t[2:4] = O.dualbuffer_checksum(np.frombuffer(ps, np.uint8), np.frombuffer(bytes(t), np.uint8)).to_bytes(2, "big")


def datagram(src: bytes, dst: bytes, hop: int, t: bytearray) -> bytes:
    """pico_ipv6_frame_push (modules/pico_ipv6.c:1324-1339) for an ICMPv6 answer: vtf 60 00 00 00, len, nxthdr
    58, the hop limit (:1291-1322), the checksum (:1335)."""
    icmp6_crc(src, dst, t)
    return b"\x60\0\0\0" + len(t).to_bytes(2, "big") + bytes([58, hop]) + src + dst + bytes(t)


def answer(d: bytes, req) -> tuple:
    """One record without its output region: d = the desc.len bytes from the IPv6 header on.  Returns
    (verdict, answer bytes or None)."""
    typ, hop = int(req["type"]), int(req["hop"])
    rsrc = bytes(np.asarray(req["src"], np.uint8))
    if len(d) < 40 or typ > 4 or int(req["rsvd"]) != 0:
        return V_MALFORMED, None
    plen = int.from_bytes(d[4:6], "big")
    if typ == 0:
        if d[0] >> 4 != 6 or 40 + plen > len(d):
            return V_MALFORMED, None
        kind, net_len, proto = O.ipv6_walk(np.frombuffer(d[:40 + plen], np.uint8))
        if kind == O.WALK_BAD:
            return V_MALFORMED, None
        if kind != O.WALK_PROTO or proto != 58:
            return V_UNTOUCHED, None                              # discarded, a fragment, another protocol
        if net_len + 8 > 40 + plen:
            return V_MALFORMED, None
        if d[net_len] != 128:
            return V_UNTOUCHED, None                              # :104-131: the host's business
        t = bytearray(d[net_len:40 + plen])                       # :84 (the datagram's end, not the frame's: difference 1)
        t[0], t[1] = 129, 0                                       # :80-81
        src = rsrc if d[24] == 0xFF else bytes(d[24:40])          # :89; ipv6_push_hdr_adjust, pico_ipv6.c:1283-1289
        return V_ACCEPT, datagram(src, bytes(d[8:24]), hop, t)
    # pico_icmp6_notify (:153-227) behind its wrappers (:229-293)
    if typ != 4 and d[24] == 0xFF:
        return V_UNTOUCHED, None
    q = min(40 + plen, QUOTE_MAX)                                 # :164-170
    if q > len(d):
        return V_MALFORMED, None
    word = int(req["arg"]).to_bytes(4, "big") if typ in (2, 4) else b"\0\0\0\0"   # :181, :198, :214; type 2: difference 2
    t = bytearray(bytes([typ, 0 if typ == 2 else int(req["code"]), 0, 0]) + word + d[:q])   # :221-223
    return V_ACCEPT, datagram(rsrc, bytes(d[8:24]), hop, t)       # :225


def reply_batch(base: np.ndarray, desc: np.ndarray, req: np.ndarray, out: np.ndarray, out_desc: np.ndarray):
    """The batch: answers are written into `out` (in place).  Returns (verdict uint8[n], out_ans DESC[n])."""
    n = desc.shape[0]
    v = np.zeros(n, np.uint8)
    oa = np.zeros(n, DESC_DTYPE)
    for i in range(n):
        off, ln = int(desc["off"][i]), int(desc["len"][i])
        if off > base.size or ln > base.size - off:
            v[i] = V_MALFORMED
            continue
        vi, a = answer(bytes(base[off:off + ln]), req[i])
        if vi == V_ACCEPT:
            ooff, cap = int(out_desc["off"][i]), int(out_desc["len"][i])
            if ooff > out.size or cap > out.size - ooff or len(a) > cap:
                vi = V_MALFORMED
            else:
                out[ooff:ooff + len(a)] = np.frombuffer(a, np.uint8)
                oa[i] = (ooff, len(a), 0)
        v[i] = vi
    return v, oa
