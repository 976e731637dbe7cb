#!/usr/bin/env python3
"""Golden ICMPv6 answers: what the compiled reference stack itself sends for the datagrams that call for one.

Run where the reference is compiled (oracle/_ref/libref_rx.so, oracle/Makefile `refrx`):
    make -C oracle refrx && python tests/golden/make_ref_icmp6.py

One fresh stack (a private copy of the library) with the links 2001:db8:0:1::1/64 and 2001:db8:0:2::1/64
(rr_ipv6_link) takes the datagrams below through rr_stack_rx, in order, with the real transport layer on
(rr_real_transport) and rr_tx_capture collecting every datagram the stack hands to pico_datalink_send.  The
stack also sends router and neighbour solicitations of its own; only frames from one of the host's addresses
with ICMPv6 type 129, 1, 2, 3 or 4 are kept.  The traffic, from a peer on the first /64:
  * echo requests of T = 8, 9, 10, 11, 64, 65, 1232, 1233, 1460 transport bytes;
  * an echo request whose ICMPv6 checksum is wrong (answered, with a valid checksum);
  * the same (id, seq) twice (both answered: pico_icmp6_process_in keeps no statics);
  * an echo request behind a hop-by-hop header with PadN (answered without it);
  * an echo request to ff02::1 (delivered in this harness; answered from the link's address);
  * an ICMPv6 echo reply and an ICMPv6 unreachable coming in (no answer);
  * UDP to a closed port with 19 and 1400 payload bytes (1 / 4; the second quote capped at 1232 bytes), a
    datagram with next header 200 (4 / 1, pointer 6), one for which there is no route (1 / 3), and one
    towards the second prefix with hop limit 1 (3 / 0);
  * "echo with a trailer": an echo request with 7 bytes behind the datagram in its frame.  DOCUMENTED
    DIFFERENCE 1: the reference takes T from the frame's length (modules/pico_icmp6.c:110) and echoes the
    trailer; the batch stops at the datagram's end.  The row is flagged `differs`; check() holds the
    restatement to the reference's answer up to the datagram's end and the reference to the trailer.
Each becomes one record of pico_icmp6_reply_batch_dev: the datagram as it lies when the stack answers it
(the routed one with the hop limit the forwarding step left), the record's type / code / arg (0 for
everything that reaches pico_icmp6_process_in), and src / hop read off the captured answer (src = the
link's address where no answer was captured).  The assertions at the end hold the
numpy restatement (tests/icmp6_ref.py) to every captured answer byte for byte, and to "no answer" where the
stack sent none.  Every row here was captured; Packet Too Big (type 2) is not in the fixture: the reference
never sends it (documented difference 2), it is pinned by the restatement alone.

Output (data only): ref_icmp6_cases.npz
  buf uint8[] (the datagrams back to back, a trailer included), off uint64[n], len uint32[n] (the bytes of
  the frame from the IPv6 header on), req (src, arg, type, code, hop, rsvd)[n], ans uint8[] (the captured
  answers back to back), ans_len uint32[n] (0: none), differs uint8[n], name <U[n]
"""
from __future__ import annotations

import ctypes
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import make_ref_tx as TX  # noqa: E402
from oracle import oracle as O  # noqa: E402
from picotcp_amd import synth  # noqa: E402
from tests import icmp6_ref as I  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
HOST = bytes.fromhex("20010db8000000010000000000000001")
HOST2 = bytes.fromhex("20010db8000000020000000000000001")
PEER = bytes.fromhex("20010db8000000010000000000000099")
ALL_NODES = bytes.fromhex("ff020000000000000000000000000001")
ECHO_T = (8, 9, 10, 11, 64, 65, 1232, 1233, 1460)
TRAILER = b"TRAILER"
UNANSWERED = ("echo reply coming in", "unreachable coming in")


def traffic(seed: int = 13):
    """(name, the incoming frame's bytes from the IPv6 header on, the same as they lie when answered, type,
    code, arg) per record, in order."""
    rng = np.random.default_rng(seed)
    cases = []

    def add(name, d, typ=0, code=0, arg=0, lies=None):
        d = bytes(np.asarray(d, np.uint8))
        cases.append((name, d, d if lies is None else lies(d), typ, code, arg))

    for k, T in enumerate(ECHO_T):
        add(f"echo T={T}", synth.icmp6_echo_request(rng, T, 0x100 + k, k, PEER, HOST))
    add("echo, wrong ICMPv6 checksum", synth.icmp6_echo_request(rng, 40, 0x200, 1, PEER, HOST, bad_crc=True))
    rep = synth.icmp6_echo_request(rng, 33, 0x300, 7, PEER, HOST)
    add("echo P", rep)
    add("repeat of P", rep)
    add("echo behind hop-by-hop PadN", synth.icmp6_echo_request(rng, 24, 0x400, 2, PEER, HOST, hbh=True))
    add("echo to ff02::1", synth.icmp6_echo_request(rng, 27, 0x500, 3, PEER, ALL_NODES))
    add("echo reply coming in", synth.icmp6_echo_request(rng, 24, 0x600, 1, PEER, HOST, icmp_type=129))
    un = synth.ipv6_datagram(rng, 58, np.concatenate([np.frombuffer(bytes([1, 4, 0, 0, 0, 0, 0, 0]), np.uint8),
                                                      synth.udp6_datagram(rng, 4, src=HOST, dst=PEER)]), PEER, HOST)
    c = synth._csum16_v6(un[8:24], un[24:40], 58, un[40:])
    un[42], un[43] = c >> 8, c & 0xFF
    add("unreachable coming in", un)
    add("UDP to a closed port, 19 bytes", synth.udp6_datagram(rng, 19, src=PEER, dst=HOST), 1, 4)
    add("UDP to a closed port, 1400 bytes", synth.udp6_datagram(rng, 1400, src=PEER, dst=HOST), 1, 4)
    add("next header 200", synth.ipv6_datagram(rng, 200, rng.integers(0, 256, 31, dtype=np.uint8), PEER, HOST), 4, 1, 6)
    add("no route", synth.udp6_datagram(rng, 19, src=PEER, dst=bytes.fromhex("20010db8000000090000000000000001")), 1, 3)
    far = bytes.fromhex("20010db8000000020000000000000077")
    add("hop limit 1 towards the second prefix", synth.ipv6_datagram(rng, 17, synth.udp6_datagram(rng, 19)[40:], PEER, far, hop=1), 3, 0,
        lies=lambda d: d[:7] + b"\0" + d[8:])              # (quoted with the hop limit the forwarding step left)
    add("echo with a trailer", np.concatenate([synth.icmp6_echo_request(rng, 16, 0x700, 4, PEER, HOST), np.frombuffer(TRAILER, np.uint8)]))
    return cases


def eth6(payload: bytes) -> bytes:
    return TX.MAC + bytes.fromhex("02aabbccdd01") + b"\x86\xdd" + payload


def capture(seed: int = 13):
    """Drive one fresh reference stack; returns [(name, frame bytes from the IPv6 header, type, code, arg, [answers])]."""
    R = TX.ref_lib()
    R.rr_ipv6_link.argtypes = [ctypes.c_char_p]
    assert R.rr_init() == 0 and R.rr_eth_init(TX.MAC) == 0
    assert R.rr_ipv6_link(HOST) == 0 and R.rr_ipv6_link(HOST2) == 0
    R.rr_real_transport(1)
    cap = np.zeros(1 << 20, np.uint8)
    lens = np.zeros(256, np.uint32)
    R.rr_tx_capture(cap.ctypes.data, cap.size, lens.ctypes.data, lens.size)
    got = []
    for name, d, lies, typ, code, arg in traffic(seed):
        b = np.frombuffer(eth6(d), np.uint8).copy()
        R.rr_stack_rx(b.ctypes.data, b.size)
        R.rr_tick(2)
        n = R.rr_tx_capture(cap.ctypes.data, cap.size, lens.ctypes.data, lens.size)     # (restarts the buffer)
        o = np.concatenate([[0], np.cumsum(lens[:n].astype(np.int64))])
        frames = [bytes(cap[o[i]:o[i + 1]]) for i in range(n)]
        # (the stack's own router and neighbour solicitations go)
        keep = [f for f in frames if len(f) >= 48 and f[0] >> 4 == 6 and f[8:24] in (HOST, HOST2) and f[6] == 58 and f[40] in (129, 1, 2, 3, 4)]
        got.append((name, lies, typ, code, arg, keep))
    R.rr_tx_capture(None, 0, None, 0)
    return got


def arrays(got):
    """The fixture's arrays of a capture; asserts at most one answer a record, each an ICMPv6 datagram to the asker."""
    n = len(got)
    req = np.zeros(n, I.REQ_DTYPE)
    ans, ans_len = [], np.zeros(n, np.uint32)
    for i, (name, d, typ, code, arg, frames) in enumerate(got):
        assert len(frames) <= 1, (name, len(frames))
        req["type"][i], req["code"][i], req["arg"][i] = typ, code, arg
        req["src"][i] = np.frombuffer(HOST, np.uint8)
        if frames:
            a = frames[0]
            assert a[24:40] == d[8:24], name
            req["src"][i], req["hop"][i] = np.frombuffer(a[8:24], np.uint8), a[7]
            ans.append(a)
            ans_len[i] = len(a)
    lens = np.array([len(g[1]) for g in got], np.uint32)
    off = np.concatenate([[0], np.cumsum(lens[:-1].astype(np.int64))]).astype(np.uint64)
    name = np.array([g[0] for g in got])
    return dict(buf=np.frombuffer(b"".join(g[1] for g in got), np.uint8), off=off, len=lens, req=req,
                ans=np.frombuffer(b"".join(ans), np.uint8), ans_len=ans_len,
                differs=(name == "echo with a trailer").astype(np.uint8), name=name)


def valid_crc(a: bytes) -> bool:
    """An answer's ICMPv6 checksum over its pseudo header sums to zero."""
    ps = a[8:40] + (len(a) - 40).to_bytes(4, "big") + b"\0\0\0\x3a"
    return O.dualbuffer_checksum(np.frombuffer(ps, np.uint8), np.frombuffer(a[40:], np.uint8)) == 0


def check(a) -> None:
    """The generator's own assertions: the cases the fixture must hold, what the stack answered and what it
    did not, and the restatement against every answer."""
    name = [str(x) for x in a["name"]]
    n = len(name)
    answered = a["ans_len"] > 0
    assert [bool(x) for x in answered] == [nm not in UNANSWERED for nm in name], dict(zip(name, answered.tolist()))
    for T in ECHO_T:
        assert f"echo T={T}" in name
    o = np.concatenate([[0], np.cumsum(a["ans_len"].astype(np.int64))])
    desc = np.zeros(n, I.DESC_DTYPE)
    desc["off"], desc["len"] = a["off"], a["len"]
    od = np.zeros(n, I.DESC_DTYPE)
    od["off"], od["len"] = np.arange(n) * 2048, 2048
    out = np.full(n * 2048, 0xEE, np.uint8)
    v, oa = I.reply_batch(a["buf"], desc, a["req"], out, od)
    for i, nm in enumerate(name):
        ref = bytes(a["ans"][o[i]:o[i + 1]])
        got = bytes(out[2048 * i:2048 * i + int(oa["len"][i])])
        assert (v[i] == I.V_ACCEPT) == bool(ref), (nm, int(v[i]))
        if ref:
            assert valid_crc(ref) and valid_crc(got), nm
        if a["differs"][i]:
            # documented difference 1: the reference echoes the trailer too, the batch stops at the datagram's end
            k = len(TRAILER)
            assert len(ref) == len(got) + k and ref[-k:] == TRAILER, nm
            assert got[:4] == ref[:4] and got[6:42] == ref[6:42] and got[44:] == ref[44:-k], nm
            continue
        assert got == ref, f"{nm}: restated {got.hex()} reference {ref.hex()}"
    by = {nm: bytes(a["ans"][o[i]:o[i + 1]]) for i, nm in enumerate(name)}
    bad = name.index("echo, wrong ICMPv6 checksum")
    rq = bytes(a["buf"][int(a["off"][bad]):][:int(a["len"][bad])])
    ps = rq[8:40] + (len(rq) - 40).to_bytes(4, "big") + b"\0\0\0\x3a"
    assert O.dualbuffer_checksum(np.frombuffer(ps, np.uint8), np.frombuffer(rq[40:], np.uint8)) != 0   # a corrupted request, a valid reply
    assert by["echo P"] and by["repeat of P"] and by["echo P"][44:] == by["repeat of P"][44:]           # repeats are answered
    assert len(by["echo behind hop-by-hop PadN"]) == 40 + 24 and by["echo behind hop-by-hop PadN"][6] == 58
    assert by["echo to ff02::1"][8:24] == HOST
    assert len(by["UDP to a closed port, 19 bytes"]) == 115 and len(by["UDP to a closed port, 1400 bytes"]) == 1280
    assert by["next header 200"][40:48] == bytes([4, 1]) + by["next header 200"][42:44] + b"\0\0\0\x06"
    assert by["no route"][40:42] == b"\x01\x03" and by["hop limit 1 towards the second prefix"][40:42] == b"\x03\x00"


def main() -> None:
    a = arrays(capture())
    check(a)
    np.savez_compressed(os.path.join(OUT, "ref_icmp6_cases.npz"), **a)
    print(f"ref_icmp6_cases.npz: {a['len'].size} records, {int((a['ans_len'] > 0).sum())} answered, "
          f"{a['buf'].size} + {a['ans'].size} bytes")
    for n, k, r in zip(a["name"], a["ans_len"], a["req"]):
        print(f"  {str(n):40s} type {int(r['type'])} code {int(r['code'])} hop {int(r['hop'])} -> {int(k)} bytes")


if __name__ == "__main__":
    main()
