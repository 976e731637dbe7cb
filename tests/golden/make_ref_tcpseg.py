#!/usr/bin/env python3
"""Golden TCP data segments: what the compiled reference stack itself emits for a pico_socket_write.

Run where the reference is compiled (oracle/_ref):
    make -C oracle refrx && python tests/golden/make_ref_tcpseg.py

oracle/_ref/libref_rx.so is the reference stack compiled unmodified (oracle/Makefile `refrx`); its
driver records every IPv4 datagram the stack hands to pico_datalink_send (rr_tx_capture).  Per
connection: a SYN with one of make_ref_tx.py's option sets (OPTS[c % 6]: none, MSS, MSS + window
scale, MSS + SACK-permitted + timestamp + window scale, SACK-permitted, MSS 536 + timestamp), the
ACK, rr_accept, ONE rr_write, then rr_tick(2) / take the captured frames / a pure ACK of the last
byte seen, until a tick emits nothing.  pico_socket_xmit (stack/pico_socket.c:1322-1358) cuts the
write into frames of `space` bytes, pico_tcp_push (modules/pico_tcp.c:3127-3157) numbers them,
tcp_send (:968-985) and pico_ipv4_frame_push (modules/pico_ipv4.c:1039-1079) finish them.  A
write is accepted up to the socket's queue (14 560 / 14 440 bytes): lengths stay at or below 14 000.

The clock: pico_tcp_output (:2938) calls tcp_add_options_frame (:633-660) per segment as it sends
it, and that sets tsval = TCP_TIME = PICO_TIME_MS(), the wall clock in milliseconds.  One write
leaves over several ticks with an ACK between them, so on a connection with the timestamp option
(OPTS 3 and 5) a millisecond boundary may fall inside a write, and the segments after it carry a
later tsval.  `capture` asserts what holds whatever the clock does: a write's segments differ from
its first only in IPv4 len / id / crc, TCP seq / crc, the payload and tsval, and tsval does not run
backwards.  tests/test_ref_tcpseg.py cuts a write into send units where the option bytes change.
The stack also draws its initial sequence numbers and first id from pico_rand, which it feeds with
the wall clock: a second run gives the same lengths, split and payload bytes (the payload generator
is seeded) but other values in those fields, in tsval and in the checksums over them.  The file
itself is written with fixed member timestamps (`save`).

Output (data only): ref_tcpseg_cases.npz
  buf uint8[] (the captured data segments back to back), off uint64[n], len uint32[n],
  group uint32[n] (the write each belongs to), written uint32[m] (the bytes each write passed)
"""
from __future__ import annotations

import io
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)

from tests.golden.make_ref_tx import HOST, MAC, OPTS, a32, be16, eth, ipv4, ref_lib, tcp_seg  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
# 1 byte, per - 1, per, per + 1 (per 1456: no timestamp option), exact multiples (2 x 1456 + 1 ... 9 x
# 1456 = 13104; 3 x 1456 = 4368 on a timestamp connection), odd tails, the 520-byte MSS (connections 5, 11)
LENGTHS = [1, 1455, 1456, 1457, 2913, 5001, 14000, 13104, 7, 4368, 9999, 12345]
M32 = 0xFFFFFFFF


def capture(lengths, seed: int = 3):
    """Drive one fresh reference stack; returns [(written bytes, [data segments as bytes])] per write."""
    rng = np.random.default_rng(seed)
    R = ref_lib()
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
    writes = []
    for c, ln in enumerate(lengths):
        peer = bytes([192, 168, 7, 100 + c])
        sport, x = 40000 + c, int(rng.integers(0, 1 << 32))

        def send(seq, ack, flags, opts=b"", wnd=8192):
            nonlocal ident
            rx(eth(ipv4(peer, HOST, 6, bytes(tcp_seg(peer, HOST, sport, 80, seq & M32, ack & M32, flags, opts, wnd=wnd)), ident)))
            ident += 1

        send(x, 0, 0x02, OPTS[c % len(OPTS)])
        R.rr_tick(2)
        synack = [f for f in taken() if (f[33] & 0x12) == 0x12][-1]
        y = int.from_bytes(synack[24:28], "big")
        send(x + 1, y + 1, 0x10, wnd=65535)
        R.rr_tick(2)
        child = R.rr_accept(lst)
        assert child
        data = rng.integers(0, 256, int(ln), dtype=np.uint8)
        assert R.rr_write(child, data.ctypes.data, int(ln)) == ln          # accepted whole
        segs = []
        while True:
            R.rr_tick(2)
            got = taken()
            if not got:
                break
            segs += got
            f = got[-1]
            send(x + 1, int.from_bytes(f[24:28], "big") + len(f) - 20 - (f[32] >> 4) * 4, 0x10, wnd=65535)
        thl = (segs[0][32] >> 4) * 4
        assert b"".join(f[20 + thl:] for f in segs) == data.tobytes()
        # per segment: IPv4 len, id, crc; TCP seq, crc; with the timestamp option (a 36-byte header:
        # window scale, kind, length, tsval, tsecr) tsval at 45..48.  Every other header byte is segment 0's.
        own = {2, 3, 4, 5, 10, 11, 24, 25, 26, 27, 36, 37} | ({45, 46, 47, 48} if thl == 36 else set())
        same = [i for i in range(20 + thl) if i not in own]
        for k, f in enumerate(segs):                                       # ids and seqs are consecutive
            assert int.from_bytes(f[4:6], "big") == (int.from_bytes(segs[0][4:6], "big") + k) & 0xFFFF
            assert int.from_bytes(f[24:28], "big") == (int.from_bytes(segs[0][24:28], "big")
                                                       + sum(len(s) - 20 - thl for s in segs[:k])) & M32
            assert bytes(f[i] for i in same) == bytes(segs[0][i] for i in same)
            assert f[6:8] == b"\x40\x00" and f[33] == 0x18                  # DF; PSH|ACK on every segment
            if thl == 36 and k:                                            # tsval: the clock, never backwards
                assert (int.from_bytes(f[45:49], "big") - int.from_bytes(segs[k - 1][45:49], "big")) & M32 < 1 << 31
        writes.append((data.tobytes(), segs))
    R.rr_tx_capture(None, 0, None, 0)
    return writes


def pack(writes):
    frames = [f for _, fr in writes for f in fr]
    group = np.array([g for g, (_, fr) in enumerate(writes) for _ in fr], np.uint32)
    buf = np.frombuffer(b"".join(frames), np.uint8)
    ln = np.array([len(f) for f in frames], np.uint32)
    off = np.concatenate([[0], np.cumsum(ln[:-1].astype(np.int64))]).astype(np.uint64)
    return buf, off, ln, group, np.array([len(d) for d, _ in writes], np.uint32)


def save(path: str, **arrays) -> None:
    """An .npz np.load reads, with fixed member timestamps: the same arrays give the same file."""
    with zipfile.ZipFile(path, "w") as z:
        for name, a in arrays.items():
            b = io.BytesIO()
            np.lib.format.write_array(b, np.ascontiguousarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, b.getvalue())


def main() -> None:
    buf, off, ln, group, written = pack(capture(LENGTHS))
    save(os.path.join(OUT, "ref_tcpseg_cases.npz"), buf=buf, off=off, len=ln, group=group, written=written)
    print(f"ref_tcpseg_cases.npz: {written.size} writes, {ln.size} segments, {buf.size} bytes")


if __name__ == "__main__":
    main()
