#!/usr/bin/env python3
"""Golden interleaved TCP burst: which socket of the compiled reference stack each segment reaches.

Run where the reference is compiled (oracle/_ref):
    make -C oracle refrx && python tests/golden/make_ref_flowgroup.py

One fresh reference stack (oracle/_ref/libref_rx.so, as tests/golden/make_ref_tcprx.py drives it) with
two listening sockets (ports 80 and 81) and 8 accepted connections whose tuples are near misses of one
another: pairs that differ only in source port, pairs that differ only in source address, and a pair
with one source address and port that reaches the two listening ports.  Every connection's in-order
data segments are then injected INTERLEAVED in a seeded order (each connection's own order kept, each
injection followed by rr_tick), and pico_socket_read is called on every child: the bytes a child
returns are the payloads of exactly the segments pico_socket_tcp_deliver (modules/pico_socket_tcp.c:
125-226) matched to it.  This pins the flow grouping's TCP key to the reference's lookup.

Output (data only): ref_flowgroup_cases.npz
  buf uint8[] (the injected IPv4 datagrams back to back, in injection order, without Ethernet header),
  off uint64[n], len uint32[n], owner uint32[n] (the connection each datagram was built for),
  src uint8[m, 4], dst uint8[m, 4], sport uint16[m], dport uint16[m] (host integers),
  rcv_before uint32[m], sack_ok uint8[m], rcv_after uint32[m] (from the stack's last ACK to that peer),
  read uint8[] (the bytes pico_socket_read returned per child, back to back), read_len uint32[m]
"""
from __future__ import annotations

import ctypes
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)

from tests.golden.make_ref_tcpseg import save  # noqa: E402
from tests.golden.make_ref_tcprx import SACK_OPTS  # noqa: E402
from tests.golden.make_ref_tx import HOST, MAC, OPTS, a32, be16, eth, ipv4, ref_lib, tcp_seg  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
M32 = 0xFFFFFFFF
# (peer's last address byte, source port, listening port)
TUPLES = ((100, 41000, 80), (100, 41001, 80),      # differ only in source port
          (101, 41000, 80),                        # from the first only in source address
          (100, 41000, 81),                        # the first's address and port, the other listening port
          (102, 42000, 80), (102, 42001, 80),      # source port again
          (103, 42000, 81), (104, 42000, 81))      # source address again


def capture(seed: int = 9):
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

    listeners = {port: R.rr_socket(6, a32(HOST), be16(port), 1) for port in (80, 81)}
    assert all(listeners.values())
    ident = 1
    conns = []
    for c, (last, sport, dport) in enumerate(TUPLES):
        peer = bytes([192, 168, 7, last])
        x = int(rng.integers(0, 1 << 32))
        rx(eth(ipv4(peer, HOST, 6, bytes(tcp_seg(peer, HOST, sport, dport, x, 0, 0x02, OPTS[c % len(OPTS)])), ident)))
        ident += 1
        R.rr_tick(2)
        synack = [f for f in taken() if (f[33] & 0x12) == 0x12][-1]
        y = int.from_bytes(synack[24:28], "big")
        rx(eth(ipv4(peer, HOST, 6, bytes(tcp_seg(peer, HOST, sport, dport, (x + 1) & M32, (y + 1) & M32, 0x10, wnd=65535)), ident)))
        ident += 1
        R.rr_tick(2)
        child = R.rr_accept(listeners[dport])
        assert child
        taken()
        P = int(rng.integers(1500, 4000))
        per = max(100, P // int(rng.integers(4, 9)))
        conns.append(dict(peer=peer, sport=sport, dport=dport, child=child, start=(x + 1) & M32, ack=(y + 1) & M32, P=P,
                          data=rng.integers(0, 256, P, dtype=np.uint8), cuts=[(a, min(a + per, P)) for a in range(0, P, per)],
                          sack=int(c % len(OPTS) in SACK_OPTS), after=(x + 1) & M32))
    owner = np.repeat(np.arange(len(conns)), [len(k["cuts"]) for k in conns])
    owner = owner[rng.permutation(owner.size)]              # the interleaving: each connection's own order kept
    nxt = [0] * len(conns)
    frames = []

    def note_acks():
        for f in taken():
            if not f[33] & 0x10:
                continue
            for k in conns:
                if f[16:20] == k["peer"] and int.from_bytes(f[22:24], "big") == k["sport"] and \
                        int.from_bytes(f[20:22], "big") == k["dport"]:
                    k["after"] = int.from_bytes(f[28:32], "big")

    for c in owner:
        k = conns[c]
        a, b = k["cuts"][nxt[c]]
        nxt[c] += 1
        t = tcp_seg(k["peer"], HOST, k["sport"], k["dport"], (k["start"] + a) & M32, k["ack"], 0x18 if b == k["P"] else 0x10,
                    b"", k["data"][a:b].tobytes(), wnd=65535)
        d = bytes(ipv4(k["peer"], HOST, 6, bytes(t), ident))
        ident += 1
        frames.append(d)
        rx(eth(d))
        R.rr_tick(2)
        note_acks()
    R.rr_tick(4)
    note_acks()
    for k in conns:
        want = (k["after"] - k["start"]) & M32
        assert want == k["P"], (k["sport"], want, k["P"])   # in order and intact: everything is acknowledged
        got = np.zeros(want, np.uint8)
        assert R.pico_socket_read(k["child"], got.ctypes.data, want) == want
        assert (got == k["data"]).all()                     # the stack delivered this connection's own bytes
        k["read"] = got.tobytes()
    R.rr_tx_capture(None, 0, None, 0)
    return conns, frames, owner


def main() -> None:
    conns, frames, owner = capture()
    ln = np.array([len(f) for f in frames], np.uint32)
    arrays = dict(buf=np.frombuffer(b"".join(frames), np.uint8),
                  off=np.concatenate([[0], np.cumsum(ln[:-1].astype(np.int64))]).astype(np.uint64), len=ln,
                  owner=owner.astype(np.uint32),
                  src=np.array([list(k["peer"]) for k in conns], np.uint8),
                  dst=np.array([list(HOST)] * len(conns), np.uint8),
                  sport=np.array([k["sport"] for k in conns], np.uint16), dport=np.array([k["dport"] for k in conns], np.uint16),
                  rcv_before=np.array([k["start"] for k in conns], np.uint32),
                  sack_ok=np.array([k["sack"] for k in conns], np.uint8),
                  rcv_after=np.array([k["after"] for k in conns], np.uint32),
                  read=np.frombuffer(b"".join(k["read"] for k in conns), np.uint8),
                  read_len=np.array([len(k["read"]) for k in conns], np.uint32))
    save(os.path.join(OUT, "ref_flowgroup_cases.npz"), **arrays)
    print(f"ref_flowgroup_cases.npz: {len(conns)} connections, {ln.size} segments, {arrays['buf'].size} bytes")


if __name__ == "__main__":
    main()
