"""Python restatement of pico_flow_group_batch_dev's contract (include/pico_csum.h), the checker of
tests/test_gpu_flowgroup.py, written from the contract and not from the kernels: a parse per frame, a
dict by key, the two orders (table groups in table order, the others by first arrival; members by
arrival) and the padding.  The IPv6 extension-header walk is the oracle's (oracle.ipv6_walk_frag).
Also the frame builders the flow-grouping tests share."""
from __future__ import annotations

import numpy as np

from oracle import oracle as O

V_ACCEPT, V_FRAG, V_IPV6 = 1, 16, 128
FLOW_TCP, FLOW_FRAG4, FLOW_FRAG6, FLOW_F_ETH = 1, 2, 3, 0x10
DESC_DTYPE = O.DESC_DTYPE
FLOW_KEY_DTYPE = np.dtype([("src", "u1", 16), ("dst", "u1", 16), ("sport", "<u2"), ("dport", "<u2"), ("family", "u1"),
                           ("reserved", "u1", 3)])


def _pad16(b) -> bytes:
    return bytes(b) + bytes(16 - len(b))


def _frag6_header(h: np.ndarray) -> int:
    """Offset of the last fragment header of a chain oracle.ipv6_walk_frag has accepted (WALK_FRAG)."""
    nx, ptr, at = int(h[6]), 40, -1
    while nx not in (6, 17, 58):
        step = 8 if nx == 44 else (int(h[ptr + 1]) + 1) << 3
        if nx == 44:
            at = ptr
        nx = int(h[ptr])
        ptr += step
    return at


def frame_key(base: np.ndarray, off: int, ln: int, mode_flags: int, verdict=None):
    """(key, network header offset, bytes available) of a selected frame, else None.  key = (family, src16,
    dst16, the 4 bytes of sport + dport / the id)."""
    mode, eth = mode_flags & 0xF, bool(mode_flags & FLOW_F_ETH)
    if off > base.size or ln > base.size - off:
        return None
    if eth:
        if ln < 14:
            return None
        off, ln = off + 14, ln - 14
    if verdict is not None and (int(verdict) & ~V_IPV6) != (V_ACCEPT if mode == FLOW_TCP else V_FRAG):
        return None
    if ln < 20:
        return None
    h = base[off:off + ln]
    ver = int(h[0]) >> 4
    if ver == 4 and mode in (FLOW_TCP, FLOW_FRAG4):
        ihl = int(h[0]) & 15
        frag = (int(h[6]) << 8 | int(h[7])) & 0x3FFF
        if ihl < 5:
            return None
        if mode == FLOW_TCP:
            if int(h[9]) != 6 or frag or 4 * ihl + 4 > ln:
                return None
            tail = bytes(h[4 * ihl:4 * ihl + 4])
        else:
            if not frag:
                return None
            tail = bytes(h[4:6]) + b"\0\0"
        return (4, _pad16(h[12:16]), _pad16(h[16:20]), tail), off, ln
    if ver == 6 and mode in (FLOW_TCP, FLOW_FRAG6) and ln >= 40:
        if mode == FLOW_TCP:
            if ln < 44 or int(h[6]) != 6:
                return None
            tail = bytes(h[40:44])
        else:
            if O.ipv6_walk_frag(h)[0] != O.WALK_FRAG:
                return None
            fo = _frag6_header(h)
            if fo + 8 > ln:
                return None
            tail = bytes(h[fo + 4:fo + 8])
        return (6, bytes(h[8:24]), bytes(h[24:40]), tail), off, ln
    return None


def table_key(k) -> tuple:
    """A FLOW_KEY_DTYPE record as frame_key's key (reserved is not compared)."""
    return (int(k["family"]), bytes(k["src"]), bytes(k["dst"]),
            int(k["sport"]).to_bytes(2, "little") + int(k["dport"]).to_bytes(2, "little"))


def make_known(tuples) -> np.ndarray:
    """A connection table from (family, src bytes, dst bytes, sport, dport) with the ports as host
    integers (stored in network byte order)."""
    t = np.zeros(len(tuples), FLOW_KEY_DTYPE)
    for i, (fam, src, dst, sp, dp) in enumerate(tuples):
        t["family"][i] = fam
        t["src"][i] = np.frombuffer(_pad16(src), np.uint8)
        t["dst"][i] = np.frombuffer(_pad16(dst), np.uint8)
        t["sport"][i] = int.from_bytes(int(sp).to_bytes(2, "big"), "little")
        t["dport"][i] = int.from_bytes(int(dp).to_bytes(2, "big"), "little")
    return t


def group(base: np.ndarray, desc: np.ndarray, mode_flags: int, verdict_in=None, known=None):
    """The batch on host arrays: (out_desc DESC[n], out_index uint32[n], out_groups uint32[n + n_known, 2],
    counts uint32[2])."""
    n = desc.shape[0]
    nk = 0 if known is None else known.shape[0]
    members: dict = {}
    order = []                                              # group number -> key (None: a duplicate table key's)
    for t in range(nk):
        k = table_key(known[t])
        if k in members:
            order.append(None)
        else:
            members[k] = []
            order.append(k)
    where = {}
    unsel = []
    for i in range(n):
        r = frame_key(base, int(desc["off"][i]), int(desc["len"][i]), mode_flags,
                      None if verdict_in is None else verdict_in[i])
        if r is None:
            unsel.append(i)
            continue
        k, off, ln = r
        if k not in members:
            members[k] = []
            order.append(k)
        members[k].append(i)
        where[i] = (off, ln)
    od = np.zeros(n, DESC_DTYPE)
    oi = np.zeros(n, np.uint32)
    og = np.zeros((n + nk, 2), np.uint32)
    slot = 0
    for g, k in enumerate(order):
        m = members[k] if k is not None else []
        if m:
            og[g] = (slot, len(m))
        for i in m:
            od["off"][slot], od["len"][slot] = where[i]
            oi[slot] = i
            slot += 1
    nsel = slot
    for i in unsel:
        oi[slot] = i
        slot += 1
    return od, oi, og, np.array([len(order), nsel], np.uint32)


# ---------------------------------------------------------------- frame builders

def tcp_frame(family, src, dst, sport, dport, payload: int = 8, ihl: int = 5, fill: int = 0) -> np.ndarray:
    """A TCP frame with the given tuple (addresses: 4 or 16 bytes); checksums are not computed (the
    grouping reads none)."""
    t = np.full(20 + payload, fill, np.uint8)
    t[0:4] = [sport >> 8, sport & 255, dport >> 8, dport & 255]
    t[12], t[13] = 0x50, 0x18
    if family == 4:
        h = np.zeros(4 * ihl, np.uint8)
        tot = h.size + t.size
        h[0], h[2], h[3], h[6], h[8], h[9] = 0x40 | ihl, tot >> 8, tot & 255, 0x40, 64, 6
        h[12:16], h[16:20] = list(src), list(dst)
        h[20:] = 0xEE                                       # options: not ports
    else:
        h = np.zeros(40, np.uint8)
        h[0], h[4], h[5], h[6], h[7] = 0x60, t.size >> 8, t.size & 255, 6, 64
        h[8:24], h[24:40] = list(src), list(dst)
    return np.concatenate([h, t])


def eth_wrap(frame: np.ndarray, ethertype: int | None = None) -> np.ndarray:
    """The frame behind a 14-byte Ethernet header."""
    if ethertype is None:
        ethertype = 0x0800 if (int(frame[0]) >> 4) == 4 else 0x86DD
    e = np.array([2, 0, 0x5E, 0xA, 0xB, 0xC, 2, 0, 0, 0, 0, 1, ethertype >> 8, ethertype & 255], np.uint8)
    return np.concatenate([e, frame])


def pack(frames, seed: int = 5, gap: int = 3):
    """The frames laid out in one buffer, `gap` bytes apart (odd alignments): (buf, DESC[n])."""
    off, pos = [], 7
    for f in frames:
        off.append(pos)
        pos += f.size + gap
    buf = np.random.default_rng(seed).integers(0, 256, pos + 16, dtype=np.uint8)
    for o, f in zip(off, frames):
        buf[o:o + f.size] = f
    d = np.zeros(len(frames), DESC_DTYPE)
    d["off"], d["len"] = off, [f.size for f in frames]
    return buf, d
