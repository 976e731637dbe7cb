#!/usr/bin/env python3
"""Golden TCP receive bursts: what the compiled reference stack itself acknowledges and delivers.

Run where the reference is compiled (oracle/_ref):
    make -C oracle refrx && python tests/golden/make_ref_tcprx.py

oracle/_ref/libref_rx.so is the reference stack compiled unmodified (oracle/Makefile `refrx`), linked
without a version script: the stack's public pico_socket_read is reachable on the handle
make_ref_tx.ref_lib() returns.  Per connection: make_ref_tcpseg.py's handshake with one of the six
SYN option sets (OPTS[c % 6]: 3 and 4 carry SACK-permitted), then 6-20 data segments cut from ONE
byte stream, injected with rr_stack_rx in a seeded order (each followed by rr_tick, so the stack
sees them one by one, in arrival order): in-order runs, swaps, exact duplicates, a retransmission of
a byte range with another split (connections without SACK: see `burst`), a hole, a flipped payload bit followed later by a good copy, a
flipped IPv4 header bit.  The stack's ACKs are captured (rr_tx_capture): the last ack number is the
reference's rcv_nxt; pico_socket_read then takes exactly ack - start bytes.  Every connection's
injected payload total stays at or below 12 000 bytes, so the reference's 16 KiB input queue is
never the reason for a drop (asserted).

Output (data only): ref_tcprx_cases.npz
  buf uint8[] (the injected IPv4 datagrams back to back, without their Ethernet header),
  off uint64[n], len uint32[n], group uint32[m, 2] (first, count: arrival order),
  rcv_before uint32[m], sack_ok uint8[m], rcv_after uint32[m] (from the stack's last ACK),
  read uint8[] (the bytes pico_socket_read returned, back to back), read_len uint32[m]
"""
from __future__ import annotations

import ctypes
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)

from tests.golden.make_ref_tcpseg import save  # noqa: E402
from tests.golden.make_ref_tx import HOST, MAC, OPTS, a32, be16, eth, ipv4, ref_lib, tcp_seg  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
M32 = 0xFFFFFFFF
CONNS = 24
SACK_OPTS = (3, 4)                  # the option sets that carry SACK-permitted
MAX_INJECTED = 12000


def burst(rng, P: int, c: int, sack: bool):
    """A connection's arrivals as [(a, b, kind)]: payload bytes [a, b) of its stream; kind 0 intact,
    1 a flipped payload bit, 2 a flipped IPv4 header bit."""
    per = max(100, P // int(rng.integers(5, 10)))
    arr = [(a, min(a + per, P), 0) for a in range(0, P, per)]
    for _ in range(int(rng.integers(0, 3))):                          # swaps
        i = int(rng.integers(0, len(arr) - 1))
        arr[i], arr[i + 1] = arr[i + 1], arr[i]
    for _ in range(int(rng.integers(1, 3))):                          # exact duplicates
        i = int(rng.integers(0, len(arr)))
        arr.insert(int(rng.integers(i + 1, len(arr) + 1)), arr[i])
    # a retransmission with another split -- without SACK only: with it, a queued segment that the chain
    # comes to cover entirely makes pico_tcp_read run past that segment (`FATAL TCP ERR: in_frame_off >
    # f->payload_len`, modules/pico_tcp.c:1125-1129, then a memcpy of the wrapped length): reference UB
    if c % 2 == 0 and not sack:
        a = int(rng.integers(0, P // 2))
        b = int(rng.integers(a + 2, P + 1))
        q = -(-(b - a) // int(rng.integers(2, 4)))
        at = int(rng.integers(0, len(arr) + 1))
        for k, x in enumerate(range(a, b, q)):
            arr.insert(at + k, (x, min(x + q, b), 0))
    if c % 3 == 0:                                                    # a hole: every copy that starts at one cut is lost
        a = arr[int(rng.integers(1, len(arr)))][0]
        arr = [s for s in arr if s[0] != a]
    if c % 4 != 3:                                                    # a flipped payload bit, a good copy later
        i = int(rng.integers(0, len(arr)))
        a, b, _ = arr[i]
        arr[i] = (a, b, 1)
        arr.insert(int(rng.integers(i + 1, len(arr) + 1)), (a, b, 0))
    if c % 4 != 0:                                                    # a flipped IPv4 header bit
        i = int(rng.integers(0, len(arr)))
        arr[i] = (arr[i][0], arr[i][1], 2 if arr[i][2] == 0 else arr[i][2])
    return arr


def capture(conns: int = CONNS, seed: int = 5):
    """Drive one fresh reference stack; per connection (frames, rcv_before, sack_ok, rcv_after, read)."""
    rng = np.random.default_rng(seed)
    R = ref_lib()
    R.pico_socket_read.restype = ctypes.c_int
    R.pico_socket_read.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    assert R.rr_init() == 0 and R.rr_eth_init(MAC) == 0
    assert R.rr_ipv4_link(a32(HOST)) == 0
    R.rr_real_transport(1)
    cap = np.zeros(1 << 20, np.uint8)
    lens = np.zeros(1024, np.uint32)
    R.rr_tx_capture(cap.ctypes.data, cap.size, lens.ctypes.data, lens.size)

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
    for c in range(conns):
        peer = bytes([192, 168, 7, 100 + c])
        sport = 41000 + c
        # every fifth connection's stream crosses 2^32
        x = int(rng.integers(0, 1 << 32)) if c % 5 else M32 - int(rng.integers(100, 2000))
        rx(eth(ipv4(peer, HOST, 6, bytes(tcp_seg(peer, HOST, sport, 80, x, 0, 0x02, OPTS[c % len(OPTS)])), ident)))
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
        P = int(rng.integers(1500, 5000))
        data = rng.integers(0, 256, P, dtype=np.uint8)
        arr = burst(rng, P, c, c % len(OPTS) in SACK_OPTS)
        while not (6 <= len(arr) <= 20 and sum(b - a for a, b, _ in arr) <= MAX_INJECTED):
            arr = burst(rng, P, c, c % len(OPTS) in SACK_OPTS)     # (seeded: the same draws every run)
        assert 6 <= len(arr) <= 20 and sum(b - a for a, b, _ in arr) <= MAX_INJECTED
        frames, acks = [], []
        for a, b, kind in arr:
            t = tcp_seg(peer, HOST, sport, 80, (start + a) & M32, (y + 1) & M32, 0x18 if b == P else 0x10, b"",
                        data[a:b].tobytes(), wnd=65535)
            d = bytearray(ipv4(peer, HOST, 6, bytes(t), ident))
            ident += 1
            if kind == 1:
                d[len(d) - 1 - int(rng.integers(0, b - a))] ^= 1 << int(rng.integers(8))
            elif kind == 2:
                d[8] ^= 0x08                                          # the TTL: only the header checksum sees it
            frames.append(bytes(d))
            rx(eth(bytes(d)))
            R.rr_tick(2)
            acks += [f for f in taken() if int.from_bytes(f[22:24], "big") == sport and f[33] & 0x10]
        R.rr_tick(4)
        acks += [f for f in taken() if int.from_bytes(f[22:24], "big") == sport and f[33] & 0x10]
        after = int.from_bytes(acks[-1][28:32], "big") if acks else start
        want = (after - start) & M32
        assert want <= P
        got = np.zeros(max(want, 1), np.uint8)
        n = R.pico_socket_read(child, got.ctypes.data, want) if want else 0
        assert n == want, (c, n, want)
        cases.append((frames, start, int(c % len(OPTS) in SACK_OPTS), after, got[:want].tobytes(), data.tobytes()))
    R.rr_tx_capture(None, 0, None, 0)
    return cases


def pack(cases):
    frames = [f for c in cases for f in c[0]]
    buf = np.frombuffer(b"".join(frames), np.uint8)
    ln = np.array([len(f) for f in frames], np.uint32)
    off = np.concatenate([[0], np.cumsum(ln[:-1].astype(np.int64))]).astype(np.uint64)
    cnt = np.array([len(c[0]) for c in cases], np.uint32)
    group = np.stack([np.concatenate([[0], np.cumsum(cnt[:-1])]).astype(np.uint32), cnt], axis=1)
    return dict(buf=buf, off=off, len=ln, group=group, rcv_before=np.array([c[1] for c in cases], np.uint32),
                sack_ok=np.array([c[2] for c in cases], np.uint8), rcv_after=np.array([c[3] for c in cases], np.uint32),
                read=np.frombuffer(b"".join(c[4] for c in cases), np.uint8),
                read_len=np.array([len(c[4]) for c in cases], np.uint32))


def main() -> None:
    cases = capture()
    arrays = pack(cases)
    save(os.path.join(OUT, "ref_tcprx_cases.npz"), **arrays)
    print(f"ref_tcprx_cases.npz: {len(cases)} connections, {arrays['len'].size} segments, {arrays['buf'].size} bytes, "
          f"{arrays['read'].size} bytes read")


if __name__ == "__main__":
    main()
