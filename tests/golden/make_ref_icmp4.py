#!/usr/bin/env python3
"""Golden ICMPv4 answers: what the compiled reference stack itself sends for the datagrams that call for one.

Run where the reference is compiled (oracle/_ref/libref_rx.so, oracle/Makefile `refrx`):
    make -C oracle refrx && python tests/golden/make_ref_icmp4.py

One fresh stack (a private copy of the library: pico_icmp4_process_in's statics start at firstpkt = 1)
takes the datagrams below through rr_stack_rx, in order, with the real transport layer on
(rr_real_transport) and rr_tx_capture collecting every datagram the stack hands to pico_datalink_send:
  * echo requests of T = 8, 9, 10, 11, 64, 65, 1479, 1480 transport bytes, DF set and clear in turn;
  * an echo request whose ICMP checksum is wrong (answered, with a valid checksum);
  * an immediate repeat of (id, seq) from the same source and one from another source (no answer), and a
    repeat with another request in between (answered);
  * an ICMP echo reply and an ICMP unreachable coming in (no answer);
  * a UDP datagram to a closed port (3 / 3), a datagram of an unknown protocol (3 / 2), a datagram routed on
    with ttl 1 (11 / 0) and one for which there is no route (3 / 1).
Each becomes one record of pico_icmp4_reply_batch_dev: the datagram AS IT LIES when the stack answers it
(the routed one with the ttl pico_ipv4_pre_forward_checks left, modules/pico_ipv4.c:1548), the record's
type / code (0 / 0 for everything that reaches pico_icmp4_process_in), and src / id read off the captured
answer.  The assertions at the end hold the numpy restatement (tests/icmp4_ref.py) to every captured
answer byte for byte, and to "no answer" where the stack sent none.

Output (data only): ref_icmp4_cases.npz
  buf uint8[] (the datagrams back to back), off uint64[n], len uint32[n], req (src, id, type, code)[n],
  ans uint8[] (the captured answers back to back), ans_len uint32[n] (0: none), name <U[n]
"""
from __future__ import annotations

import os
import struct
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import make_ref_tx as TX  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import icmp4_ref as I  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
HOST = TX.HOST
ECHO_T = (8, 9, 10, 11, 64, 65, 1479, 1480)


def ipv4(src: bytes, dst: bytes, proto: int, payload: bytes, ident: int, frag: int = 0, ttl: int = 64) -> bytes:
    h = bytearray(TX.ipv4(src, dst, proto, payload, ident)[:20])
    h[6:8], h[8] = frag.to_bytes(2, "big"), ttl
    h[10:12] = b"\0\0"
    h[10:12] = O.checksum(np.frombuffer(bytes(h), np.uint8)).to_bytes(2, "big")
    return bytes(h) + payload


def icmp(typ: int, code: int, rest: bytes, bad_crc: bool = False) -> bytes:
    m = bytearray(bytes([typ, code, 0, 0]) + rest)
    c = O.checksum(np.frombuffer(bytes(m), np.uint8)) ^ (0x0100 if bad_crc else 0)
    m[2:4] = c.to_bytes(2, "big")
    return bytes(m)


def echo(ident: int, seq: int, T: int, rng, typ: int = 8, bad_crc: bool = False) -> bytes:
    return icmp(typ, 0, struct.pack("!HH", ident, seq) + rng.integers(0, 256, T - 8, dtype=np.uint8).tobytes(), bad_crc)


def traffic(seed: int = 11):
    """(name, incoming datagram, the datagram as it lies when answered, type, code) per record, in order."""
    rng = np.random.default_rng(seed)
    peer = lambda k: bytes([192, 168, 7, k])
    cases, ident = [], [0x2000]

    def add(name, d, typ=0, code=0, lies=None):
        cases.append((name, d, d if lies is None else lies, typ, code))
        ident[0] += 1

    for k, T in enumerate(ECHO_T):
        add(f"echo T={T} {'DF' if k % 2 == 0 else 'no DF'}",
            ipv4(peer(50 + k), HOST, 1, echo(0x100 + k, k, T, rng), ident[0], frag=0x4000 if k % 2 == 0 else 0))
    add("echo, wrong ICMP checksum", ipv4(peer(60), HOST, 1, echo(0x200, 1, 40, rng, bad_crc=True), ident[0]))
    rep = echo(0x300, 7, 33, rng)
    add("echo P", ipv4(peer(61), HOST, 1, rep, ident[0]))
    add("repeat of P, same source", ipv4(peer(61), HOST, 1, rep, ident[0]))
    add("repeat of P, another source", ipv4(peer(62), HOST, 1, echo(0x300, 7, 21, rng), ident[0]))
    add("echo Q", ipv4(peer(61), HOST, 1, echo(0x300, 8, 12, rng), ident[0]))
    add("repeat of P behind Q", ipv4(peer(61), HOST, 1, rep, ident[0]))
    add("echo reply coming in", ipv4(peer(63), HOST, 1, echo(0x400, 1, 24, rng, typ=0), ident[0]))
    quoted = ipv4(HOST, peer(64), 17, struct.pack("!HHHH", 5555, 6666, 12, 0) + b"abcd", 0x77)[:28]
    add("unreachable coming in", ipv4(peer(64), HOST, 1, icmp(3, 3, b"\0\0\0\0" + quoted), ident[0]))
    udp = struct.pack("!HHHH", 4000, 4001, 8 + 19, 0) + rng.integers(0, 256, 19, dtype=np.uint8).tobytes()
    add("UDP to a closed port", ipv4(peer(65), HOST, 17, udp, ident[0]), 3, 3)
    add("unknown protocol", ipv4(peer(66), HOST, 200, rng.integers(0, 256, 31, dtype=np.uint8).tobytes(), ident[0]), 3, 2)
    d = ipv4(peer(67), peer(99), 17, udp, ident[0], ttl=1)
    add("routed on with ttl 1", d, 11, 0, lies=d[:8] + b"\0" + d[9:])
    add("no route", ipv4(peer(68), bytes([10, 9, 9, 9]), 17, udp, ident[0]), 3, 1)
    return cases


def capture(seed: int = 11):
    """Drive one fresh reference stack; returns [(name, datagram as answered, type, code, [answers])]."""
    R = TX.ref_lib()
    assert R.rr_init() == 0 and R.rr_eth_init(TX.MAC) == 0
    assert R.rr_ipv4_link(TX.a32(HOST)) == 0
    R.rr_real_transport(1)
    cap = np.zeros(1 << 20, np.uint8)
    lens = np.zeros(256, np.uint32)
    R.rr_tx_capture(cap.ctypes.data, cap.size, lens.ctypes.data, lens.size)
    got = []
    for name, d, lies, typ, code in traffic(seed):
        b = np.frombuffer(TX.eth(d), np.uint8).copy()
        R.rr_stack_rx(b.ctypes.data, b.size)
        R.rr_tick(2)
        n = R.rr_tx_capture(cap.ctypes.data, cap.size, lens.ctypes.data, lens.size)     # (restarts the buffer)
        o = np.concatenate([[0], np.cumsum(lens[:n].astype(np.int64))])
        frames = [bytes(cap[o[i]:o[i + 1]]) for i in range(n)]
        got.append((name, lies, typ, code, [f for f in frames if f[0] >> 4 == 4]))     # (the ticks' IPv6 router solicitations go too)
    R.rr_tx_capture(None, 0, None, 0)
    return got


def arrays(got):
    """The fixture's arrays of a capture; asserts at most one answer a record, each an ICMPv4 datagram."""
    n = len(got)
    req = np.zeros(n, I.REQ_DTYPE)
    ans, ans_len = [], np.zeros(n, np.uint32)
    for i, (name, d, typ, code, frames) in enumerate(got):
        assert len(frames) <= 1, (name, len(frames))
        req["type"][i], req["code"][i] = typ, code
        req["src"][i] = TX.a32(HOST)
        if frames:
            a = frames[0]
            assert a[0] == 0x45 and a[9] == 1 and a[16:20] == d[12:16], name
            req["src"][i], req["id"][i] = int.from_bytes(a[12:16], "little"), int.from_bytes(a[4:6], "big")
            ans.append(a)
            ans_len[i] = len(a)
    lens = np.array([len(g[1]) for g in got], np.uint32)
    off = np.concatenate([[0], np.cumsum(lens[:-1].astype(np.int64))]).astype(np.uint64)
    return dict(buf=np.frombuffer(b"".join(g[1] for g in got), np.uint8), off=off, len=lens, req=req,
                ans=np.frombuffer(b"".join(ans), np.uint8), ans_len=ans_len, name=np.array([g[0] for g in got]))


def check(a) -> None:
    """The generator's own assertions: the cases the fixture must hold, what the stack answered and what it
    did not, and the restatement against every answer."""
    name = [str(x) for x in a["name"]]
    answered = a["ans_len"] > 0
    want = {n: True for n in name}
    for n in ("repeat of P, same source", "repeat of P, another source", "echo reply coming in", "unreachable coming in"):
        want[n] = False
    assert [bool(x) for x in answered] == [want[n] for n in name], dict(zip(name, answered.tolist()))
    for T in ECHO_T:
        assert any(n.startswith(f"echo T={T} ") for n in name)
    o = np.concatenate([[0], np.cumsum(a["ans_len"].astype(np.int64))])
    st = I.state()
    desc = np.zeros(len(name), I.DESC_DTYPE)
    desc["off"], desc["len"] = a["off"], a["len"]
    od = np.zeros(len(name), I.DESC_DTYPE)
    od["off"], od["len"] = np.arange(len(name)) * 2048, 2048
    out = np.full(len(name) * 2048, 0xEE, np.uint8)
    v, oa = I.reply_batch(a["buf"], desc, a["req"], st, out, od)
    for i, n in enumerate(name):
        ref = bytes(a["ans"][o[i]:o[i + 1]])
        got = bytes(out[2048 * i:2048 * i + int(oa["len"][i])])
        assert got == ref, f"{n}: restated {got.hex()} reference {ref.hex()}"
        assert (v[i] == I.V_ACCEPT) == bool(ref), (n, int(v[i]))
        if ref:                                                     # tos 0, ttl 64: what send_tos / send_ttl of a received frame give
            assert ref[1] == 0 and ref[8] == 64, n
    bad = name.index("echo, wrong ICMP checksum")
    ref = a["ans"][o[bad]:o[bad + 1]]
    assert O.checksum(ref[20:]) == 0 and O.checksum(ref[:20]) == 0         # a corrupted request, a valid reply
    rq = a["buf"][int(a["off"][bad]):][:int(a["len"][bad])]
    assert O.checksum(rq[20:]) != 0


def main() -> None:
    a = arrays(capture())
    check(a)
    np.savez_compressed(os.path.join(OUT, "ref_icmp4_cases.npz"), **a)
    print(f"ref_icmp4_cases.npz: {a['len'].size} records, {int((a['ans_len'] > 0).sum())} answered, "
          f"{a['buf'].size} + {a['ans'].size} bytes")
    for n, k, r in zip(a["name"], a["ans_len"], a["req"]):
        print(f"  {str(n):32s} type {int(r['type']):2d} code {int(r['code']):2d} -> {int(k)} bytes")


if __name__ == "__main__":
    main()
