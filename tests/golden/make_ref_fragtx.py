#!/usr/bin/env python3
"""Golden TX fragments: what the compiled reference stack itself emits for an oversized UDP sendto.

Run where the reference is compiled (oracle/_ref):
    make -C oracle refrx && python tests/golden/make_ref_fragtx.py

oracle/_ref/libref_rx.so is the reference stack compiled unmodified with PICO_SUPPORT_IPV4FRAG
(oracle/Makefile `refrx`); its driver records every IPv4 datagram the stack hands to
pico_datalink_send (rr_tx_capture).  A UDP socket sends payloads larger than the device MTU (1500):
pico_socket_xmit_fragments (stack/pico_socket.c:1131-1251) copies each into MTU-sized frames and
pico_udp_push / pico_ipv4_frame_push (modules/pico_ipv4.c:1039-1079) give every frame its len, the
datagram's id, frag and header checksum.  The first sendto of a fresh socket runs before s->dev is
set and splits by PICO_MIN_MSS 1280 (misplacing the second fragment: frag = (written + 8) >> 3 is
only right when mtu - 20 is a multiple of 8): one warm-up sendto is made and its output discarded.

Output (data only): ref_fragtx_cases.npz
  buf uint8[] (the captured fragments back to back), off uint64[n], len uint32[n],
  group uint32[n] (the sendto each belongs to), payload uint32[m] (the bytes each sendto passed)
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)

from tests.golden.make_ref_tx import HOST, MAC, a32, be16, ref_lib  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
FIXED = [1473, 1480, 1481, 2952, 2953, 4000, 9000, 65507]


def capture(lengths, seed: int = 1):
    """Drive one fresh reference stack; returns [(payload bytes, [fragments as bytes])] per sendto."""
    rng = np.random.default_rng(seed)
    R = ref_lib()
    assert R.rr_init() == 0 and R.rr_eth_init(MAC) == 0
    assert R.rr_ipv4_link(a32(HOST)) == 0
    R.rr_real_transport(1)
    cap = np.zeros(1 << 20, np.uint8)
    lens = np.zeros(1024, np.uint32)
    R.rr_tx_capture(cap.ctypes.data, cap.size, lens.ctypes.data, lens.size)

    def taken():
        n = R.rr_tx_capture(cap.ctypes.data, cap.size, lens.ctypes.data, lens.size)   # (restarts the buffer)
        out, o = [], 0
        for i in range(n):
            out.append(bytes(cap[o:o + lens[i]]))
            o += int(lens[i])
        return out

    s = R.rr_socket(17, a32(HOST), be16(5000), 0)
    assert s
    warm = np.zeros(1472, np.uint8)
    R.rr_sendto(s, warm.ctypes.data, warm.size, a32(bytes([192, 168, 7, 99])), be16(6999))   # s->dev unset: discarded
    R.rr_tick(2)
    taken()
    sends = []
    for i, ln in enumerate(lengths):
        data = rng.integers(0, 256, int(ln), dtype=np.uint8)
        R.rr_sendto(s, data.ctypes.data, int(ln), a32(bytes([192, 168, 7, 100 + i % 100])), be16(7000 + i))
        R.rr_tick(2)
        sends.append((data.tobytes(), [f for f in taken() if f[0] >> 4 == 4 and f[9] == 17]))
    R.rr_tx_capture(None, 0, None, 0)
    return sends


def lengths(seed: int = 1, extra: int = 10):
    rng = np.random.default_rng(seed ^ 0x5EED)
    return FIXED + [int(x) for x in rng.integers(1473, 12001, extra)]


def pack(sends):
    frames = [f for _, fr in sends for f in fr]
    group = np.array([g for g, (_, fr) in enumerate(sends) for _ in fr], np.uint32)
    buf = np.frombuffer(b"".join(frames), np.uint8)
    ln = np.array([len(f) for f in frames], np.uint32)
    off = np.concatenate([[0], np.cumsum(ln[:-1].astype(np.int64))]).astype(np.uint64)
    return buf, off, ln, group, np.array([len(d) for d, _ in sends], np.uint32)


def main() -> None:
    buf, off, ln, group, payload = pack(capture(lengths()))
    np.savez_compressed(os.path.join(OUT, "ref_fragtx_cases.npz"), buf=buf, off=off, len=ln, group=group, payload=payload)
    print(f"ref_fragtx_cases.npz: {payload.size} sendto calls, {ln.size} fragments, {buf.size} bytes")


if __name__ == "__main__":
    main()
