"""Numpy restatement of pico_icmp4_reply_batch_dev's contract (include/pico_csum.h), the checker of
tests/test_gpu_icmp4.py, written from the contract and the reference's lines, not from the kernel; the
sums are the oracle's.  Pinned to the compiled reference stack's own answers by tests/test_ref_icmp4.py
(tests/golden/ref_icmp4_cases.npz).  Pinned by this restatement alone, because the frozen driver's
stack does not produce them: requests with IPv4 options (documented difference 1), answers above the
MTU (difference 2), and the notices 3 / 1, 3 / 4, 3 / 13, 11 / 0, 11 / 1 and 12 / x (the driver's
device has no second route, no filter, no short-MTU hop and no reassembly timeout within a capture)."""
from __future__ import annotations

import numpy as np

from oracle import oracle as O

V_ACCEPT, V_MALFORMED, V_UNTOUCHED, V_DUPLICATE = 1, 8, 32, 64
DESC_DTYPE = np.dtype([("off", "<u8"), ("len", "<u4"), ("seed", "<u4")])
REQ_DTYPE = np.dtype([("src", "<u4"), ("id", "<u2"), ("type", "u1"), ("code", "u1")])
STATE_DTYPE = np.dtype([("seen", "<u4"), ("id", "<u2"), ("seq", "<u2")])
assert REQ_DTYPE.itemsize == 8 and STATE_DTYPE.itemsize == 8


def state() -> np.ndarray:
    """pico_icmp4_process_in's statics at their initial value (firstpkt = 1: seen = 0)."""
    return np.zeros(1, STATE_DTYPE)


def ipv4_header(length: int, ident: int, frag: bytes, src: bytes, dst: bytes) -> bytes:
    """pico_ipv4_frame_push (modules/pico_ipv4.c:1039-1079) for an ICMP answer: vhl 45 (:1039), tos =
    send_tos = 0 (:1057), len (:1040), id (:1041), frag = the frame's own (:1072-1075), ttl 64 (:1032,
    :1056), proto (:1058), pico_ipv4_checksum (:1079), src = the link's address (:1055), dst (:1054)."""
    h = bytearray(20)
    h[0], h[8], h[9] = 0x45, 64, 1
    h[2:4] = length.to_bytes(2, "big")
    h[4:6] = (ident & 0xFFFF).to_bytes(2, "big")
    h[6:8] = frag
    h[12:16], h[16:20] = src, dst
    h[10:12] = O.checksum(np.frombuffer(bytes(h), np.uint8)).to_bytes(2, "big")
    return bytes(h)


def icmp_crc(t: bytearray) -> None:
    """pico_icmp4_checksum (modules/pico_icmp4.c:30-41): crc = 0, crc = short_be(pico_checksum(hdr, transport_len))."""
    t[2:4] = b"\0\0"
    t[2:4] = O.checksum(np.frombuffer(bytes(t), np.uint8)).to_bytes(2, "big")


def answer(d: bytes, req) -> tuple:
    """One record, without the duplicate rule and the output region: d = the desc.len bytes from the IPv4
    header on.  Returns (verdict, answer bytes or None, (id, seq) as stored for an echo request or None)."""
    typ, src = int(req["type"]), int(req["src"]).to_bytes(4, "little")
    if len(d) < 20 or typ not in (0, 3, 11, 12):
        return V_MALFORMED, None, None
    tot = int.from_bytes(d[2:4], "big")
    if typ == 0:
        # the candidate rule: what reaches pico_icmp4_process_in as an echo request (:55)
        ihl = d[0] & 15
        if d[0] >> 4 != 4 or ihl < 5 or d[9] != 1 or not (4 * ihl + 8 <= tot <= len(d)):
            return V_MALFORMED, None, None
        t = bytearray(d[4 * ihl:tot])
        if t[0] != 8:
            return V_UNTOUCHED, None, None                        # :72-82: the host's business
        t[0] = 0                                                  # :56
        icmp_crc(t)                                               # :70, over the bytes as copied
        # pico_ipv4_rebound (:1512-1533): dst = hdr->src; f->frag = short_be(hdr->frag) (:402) comes back
        return V_ACCEPT, ipv4_header(20 + len(t), int(req["id"]), d[6:8], src, d[12:16]) + bytes(t), bytes(d[4 * ihl + 4:4 * ihl + 8])
    # pico_icmp4_notify (:106-141), literally
    if tot < 20:                                                  # :120-121
        return V_MALFORMED, None, None
    q = min(tot, 28)                                              # :124-126
    if q > len(d):
        return V_MALFORMED, None, None
    t = bytearray([typ, int(req["code"]), 0, 0, 0, 0, 0x05, 0xDC]) + d[:q]   # :131-137 (ipm_void 0, ipm_nmtu 1500)
    icmp_crc(t)                                                   # :138
    return V_ACCEPT, ipv4_header(20 + len(t), int(req["id"]), b"\0\0", src, d[12:16]) + bytes(t), None   # :139


def reply_batch(base: np.ndarray, desc: np.ndarray, req: np.ndarray, st, out: np.ndarray, out_desc: np.ndarray):
    """The batch: answers are written into `out` (in place), st (state() or None) is updated in place.
    Returns (verdict uint8[n], out_ans DESC[n])."""
    n = desc.shape[0]
    v = np.zeros(n, np.uint8)
    oa = np.zeros(n, DESC_DTYPE)
    last = None if st is None or not int(st["seen"][0]) else (int(st["id"][0]).to_bytes(2, "little") + int(st["seq"][0]).to_bytes(2, "little"))
    for i in range(n):
        off, ln = int(desc["off"][i]), int(desc["len"][i])
        if off > base.size or ln > base.size - off:
            v[i] = V_MALFORMED
            continue
        vi, a, idseq = answer(bytes(base[off:off + ln]), req[i])
        if vi == V_ACCEPT:
            ooff, cap = int(out_desc["off"][i]), int(out_desc["len"][i])
            if ooff > out.size or cap > out.size - ooff or len(a) > cap:
                vi = V_MALFORMED                                  # (it takes no part in the duplicate rule)
            elif idseq is not None and idseq == last:
                vi = V_DUPLICATE                                  # :61-65
            else:
                if idseq is not None:
                    last = idseq                                  # :67-69
                out[ooff:ooff + len(a)] = np.frombuffer(a, np.uint8)
                oa[i] = (ooff, len(a), 0)
        v[i] = vi
    if st is not None and last is not None:
        st["seen"][0] = 1
        st["id"][0], st["seq"][0] = int.from_bytes(last[0:2], "little"), int.from_bytes(last[2:4], "little")
    return v, oa
