#!/usr/bin/env python3
"""Golden ACK frames: what the compiled reference stack itself answers to a burst's last arrival.

Run where the reference is compiled (oracle/_ref):
    make -C oracle refrx && python tests/golden/make_ref_tcpack.py

One fresh reference stack, driven as tests/golden/make_ref_tcprx.py drives it (handshake, rr_stack_rx
segment by segment with rr_tick behind each, ACKs taken with rr_tx_capture).  Per connection the
stream is cut into pieces of one size and the arrivals are a list of piece indexes (SCENARIOS); the
frame kept is the reference's ACK to the LAST arrival.  What a connection was sent before its burst
has been read from the socket and nothing is read during the burst, so the receive space before the
burst is the reference's whole queue, 16384 bytes.  The host inputs of pico_tcp_ack_batch_dev come from that captured frame
and the stack's known state: the template is the frame's first 40 bytes (addresses, tos, ttl, id,
ports, seq, the urgent pointer) with the fields the batch does not read overwritten with 0xAA;
tsval / tsecr are the frame's own.

18 connections are kept, every one of them compared in full (tests/test_ref_tcpack.py: no skip list).
Conditions asserted here: every SACK connection's last arrival is a verified held segment (only then
does the reference's last ACK carry blocks: tcp_sack_prepare runs on a high segment); injected bytes
stay at or below 12 000 per connection; the scenarios yield ACKs with no block and with one, and
held sets of 1, 2, 3 and more than 3 candidate runs (see SCENARIOS for why the reference never
reports a second run).

Output (data only): ref_tcpack_cases.npz
  buf uint8[], off uint64[n], len uint32[n], group uint32[m, 2], rcv_before uint32[m], sack_ok uint8[m]
  (the injected IPv4 datagrams, as ref_tcprx_cases.npz holds them), tmpl uint8[m, 40], space uint32[m],
  tsval uint32[m], tsecr uint32[m], ts_ok uint8[m], ack uint8[] (the reference's ACK frames back to
  back), ack_len uint32[m]
"""
from __future__ import annotations

import ctypes
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)

from tests import tcpack_ref as A  # noqa: E402
from tests import tcprx_ref as RX  # noqa: E402
from tests.golden.make_ref_tcpseg import save  # noqa: E402
from tests.golden.make_ref_tx import HOST, MAC, OPTS, a32, be16, eth, ipv4, ref_lib, tcp_seg  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
M32 = 0xFFFFFFFF
SPACE = 16384                       # PICO_DEFAULT_SOCKETQ, nothing queued before the burst
MAX_INJECTED = 12000
BAD = 100                           # piece index + BAD: that piece with a flipped payload bit

# (SYN option set of make_ref_tx.OPTS, first seq or None = seeded, pieces delivered and read BEFORE the
# burst, arrivals as piece indexes)
#   option sets 3 (SACK + timestamps) and 4 (SACK, no timestamps); 5 (timestamps), 1 and 0 without SACK
# The reference's tcp_sack_prepare starts at the input queue's FIRST segment and its next_segment follows
# one contiguous run (modules/pico_tcp.c:161-179), so (a) an ACK carries blocks only when nothing
# delivered and unread lies in front of the held segments -- every SACK burst here starts behind a hole,
# what was delivered before it has been read -- and (b) it carries at most ONE block, the lowest held run,
# however many runs are held: 2 or 3 blocks cannot be drawn from this stack.
SCENARIOS = [
    (3, None, 0, [1, 2]),                           # one block of two segments
    (4, None, 0, [2, 4, 6]),                        # three candidate runs: the walk ends at the first gap, {2}
    (3, None, 0, [2, 3, 5, 7, 8]),                  # runs of two: {2, 3}; 5, the run-breaker, is never reached
    (4, None, 0, [2, 4, 6, 8, 10, 12, 14]),         # more than 3 candidate runs
    (3, None, 0, [9, 7, 5, 3]),                     # lone held segments, descending arrival: {3}
    (4, M32 - 1499, 0, [2, 3, 5]),                  # across 2^32: {2, 3} wraps its right edge
    (3, M32 - 1499, 0, [4, 5]),                     # across 2^32: both below rcv' raw, skipped: no block
    (4, M32 - 1499, 0, [4, 2]),                     # the block before the wrap, the one behind it unreported
    (3, None, 0, [3 + BAD, 3, 5]),                  # a corrupted held segment, a good copy later
    (4, None, 0, [3 + BAD, 5, 6]),                  # a corrupted held segment never repaired: absent
    (3, None, 0, [3, 3, 4, 2]),                     # a held duplicate; the lowest arrives last
    (4, None, 2, [3, 4, 6]),                        # two pieces delivered and read before the burst
    (3, None, 3, [5, 4 + BAD, 4]),                  # likewise, with a corrupted copy
    (5, None, 0, [0, 1, 3, 2]),                     # timestamps, no SACK: the high segment is dropped
    (0, None, 0, [0, 2, 1]),                        # no options at all
    (1, None, 0, [0, 1, 2]),                        # in order
    (5, None, 0, [0, 1, 0, 1 + BAD, 2]),            # old duplicates, one corrupted
    (0, None, 1, [1, 3, 1, 2]),                     # no SACK, data read before the burst
]
SACK_OPTS = (3, 4)


def capture(seed: int = 11):
    """Drive one fresh reference stack; per connection (frames, rcv_before, sack_ok, last ACK frame)."""
    rng = np.random.default_rng(seed)
    R = ref_lib()
    assert R.rr_init() == 0 and R.rr_eth_init(MAC) == 0
    assert R.rr_ipv4_link(a32(HOST)) == 0
    R.rr_real_transport(1)
    cap = np.zeros(1 << 20, np.uint8)
    lens = np.zeros(1024, np.uint32)
    R.rr_tx_capture(cap.ctypes.data, cap.size, lens.ctypes.data, lens.size)
    R.pico_socket_read.restype = ctypes.c_int
    R.pico_socket_read.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]

    def rx(frame: bytes):
        b = np.frombuffer(frame, np.uint8).copy()
        R.rr_stack_rx(b.ctypes.data, b.size)

    def taken():
        n = R.rr_tx_capture(cap.ctypes.data, cap.size, lens.ctypes.data, lens.size)   # (restarts the buffer)
        out, o = [], 0
        for i in range(n):
            out.append(bytes(cap[o:o + lens[i]]))
            o += int(lens[i])
        return [f for f in out if f[0] >> 4 == 4 and f[9] == 6]

    lst = R.rr_socket(6, a32(HOST), be16(80), 1)
    assert lst
    ident = 1
    cases = []
    for c, (opt, x0, pre, arrivals) in enumerate(SCENARIOS):
        peer = bytes([192, 168, 7, 100 + c])
        sport = 42000 + c
        x = int(rng.integers(0, 1 << 32)) if x0 is None else x0 - 1
        rx(eth(ipv4(peer, HOST, 6, bytes(tcp_seg(peer, HOST, sport, 80, x, 0, 0x02, OPTS[opt])), ident)))
        ident += 1
        R.rr_tick(2)
        synack = [f for f in taken() if (f[33] & 0x12) == 0x12][-1]
        y = int.from_bytes(synack[24:28], "big")
        rx(eth(ipv4(peer, HOST, 6, bytes(tcp_seg(peer, HOST, sport, 80, (x + 1) & M32, (y + 1) & M32, 0x10, wnd=65535)), ident)))
        ident += 1
        R.rr_tick(2)
        child = R.rr_accept(lst)
        assert child
        taken()
        start = (x + 1) & M32
        per = 400 if x0 is not None else int(rng.integers(150, 600))
        npieces = max(a % BAD for a in arrivals) + 1
        data = rng.integers(0, 256, per * npieces, dtype=np.uint8)
        assert per * len(arrivals) <= MAX_INJECTED

        def datagram(i):
            t = tcp_seg(peer, HOST, sport, 80, (start + i * per) & M32, (y + 1) & M32, 0x10, b"",
                        data[i * per:(i + 1) * per].tobytes(), wnd=65535)
            return bytearray(ipv4(peer, HOST, 6, bytes(t), ident))

        for i in range(pre):                                                # before the burst: delivered, read
            rx(eth(bytes(datagram(i))))
            ident += 1
            R.rr_tick(2)
        if pre:
            got = np.zeros(pre * per, np.uint8)
            assert R.pico_socket_read(child, got.ctypes.data, got.size) == got.size
            taken()
        frames, last = [], None
        for a in arrivals:
            i = a % BAD
            d = datagram(i)
            ident += 1
            if a >= BAD:
                d[len(d) - 1 - int(rng.integers(0, per))] ^= 1 << int(rng.integers(8))
            frames.append(bytes(d))
            rx(eth(bytes(d)))
            R.rr_tick(2)
            acks = [f for f in taken() if int.from_bytes(f[22:24], "big") == sport and f[33] == 0x10]
            if acks:
                last = acks[-1]
        assert last is not None
        cases.append((frames, (start + pre * per) & M32, int(opt in SACK_OPTS), last))
    R.rr_tx_capture(None, 0, None, 0)
    return cases


def pack(cases):
    frames = [f for c in cases for f in c[0]]
    buf = np.frombuffer(b"".join(frames), np.uint8)
    ln = np.array([len(f) for f in frames], np.uint32)
    off = np.concatenate([[0], np.cumsum(ln[:-1].astype(np.int64))]).astype(np.uint64)
    cnt = np.array([len(c[0]) for c in cases], np.uint32)
    group = np.stack([np.concatenate([[0], np.cumsum(cnt[:-1])]).astype(np.uint32), cnt], axis=1)
    m = len(cases)
    tmpl = np.zeros((m, 40), np.uint8)
    tsval, tsecr, ts_ok = np.zeros(m, np.uint32), np.zeros(m, np.uint32), np.zeros(m, np.uint8)
    for g, c in enumerate(cases):
        a = np.frombuffer(c[3], np.uint8)
        t = a[:40].copy()
        for lo, hi in ((2, 4), (6, 8), (10, 12), (28, 32), (33, 38)):      # len, frag, crc; ack; flags, rwnd, tcp crc
            t[lo:hi] = 0xAA
        t[32] = 0xA0 | (int(t[32]) & 0x0F)                                  # thl: not read; the low nibble is
        tmpl[g] = t
        o = bytes(a[40:])
        assert o[:2] == b"\x03\x03"
        if o[3:5] == b"\x08\x0a":
            ts_ok[g], tsval[g], tsecr[g] = 1, int.from_bytes(o[5:9], "big"), int.from_bytes(o[9:13], "big")
    return dict(buf=buf, off=off, len=ln, group=group, rcv_before=np.array([c[1] for c in cases], np.uint32),
                sack_ok=np.array([c[2] for c in cases], np.uint8), tmpl=tmpl, space=np.full(m, SPACE, np.uint32),
                tsval=tsval, tsecr=tsecr, ts_ok=ts_ok, ack=np.frombuffer(b"".join(c[3] for c in cases), np.uint8),
                ack_len=np.array([len(c[3]) for c in cases], np.uint32))


def check_conditions(a) -> None:
    """The conditions of the module docstring, judged by the restatements."""
    m = a["group"].shape[0]
    seg = np.zeros(a["off"].size, RX.DESC_DTYPE)
    seg["off"], seg["len"] = a["off"], a["len"]
    conn = np.stack([a["rcv_before"], a["sack_ok"].astype(np.uint32)], axis=1)
    od = np.zeros(m, RX.DESC_DTYPE)
    od["off"], od["len"] = np.arange(m) * SPACE, SPACE
    _, ol, sv = RX.coalesce(a["buf"], seg, a["group"], conn, np.zeros(m * SPACE, np.uint8), od)
    td = np.zeros(m, RX.DESC_DTYPE)
    td["off"], td["len"] = np.arange(m) * 40, 40
    ak = np.zeros(m, A.ACK_DTYPE)
    ak["space"], ak["tsval"], ak["tsecr"], ak["aflags"] = a["space"], a["tsval"], a["tsecr"], a["ts_ok"]
    fd = np.zeros(m, RX.DESC_DTYPE)
    fd["off"], fd["len"] = np.arange(m) * 100, 100
    out = np.zeros(m * 100, np.uint8)
    _, oa, sv2 = A.ack_batch(a["buf"], seg, a["group"], conn, ol, sv, a["tmpl"].reshape(-1), td, ak, out, fd)
    nblocks = set()
    for g in range(m):
        first, cnt = (int(x) for x in a["group"][g])
        assert int(a["len"][first:first + cnt].astype(np.int64).sum()) - 40 * cnt <= MAX_INJECTED
        if a["sack_ok"][g]:
            assert sv2[first + cnt - 1] == RX.V_TCP_HELD, g
            thl = 4 * (int(out[100 * g + 32]) >> 4)
            o = bytes(out[100 * g + 40:100 * g + 20 + thl])
            k = 13 if a["ts_ok"][g] else 3
            nblocks.add((o[k + 1] - 2) // 8 if o[k] == 5 else 0)
    assert nblocks == {0, 1}, nblocks


def main() -> None:
    cases = capture()
    arrays = pack(cases)
    check_conditions(arrays)
    save(os.path.join(OUT, "ref_tcpack_cases.npz"), **arrays)
    print(f"ref_tcpack_cases.npz: {len(cases)} connections, {arrays['len'].size} segments, {arrays['buf'].size} bytes, "
          f"{arrays['ack'].size} ACK bytes")


if __name__ == "__main__":
    main()
