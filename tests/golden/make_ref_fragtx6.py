#!/usr/bin/env python3
"""Golden IPv6 TX fragments, pinned to the reference's own receiver.

Run where the reference is compiled (oracle/_ref):
    make -C oracle all refrx && python tests/golden/make_ref_fragtx6.py

The reference cannot fragment IPv6 when it sends (pico_socket_xmit_fragments: "Can't fragment
IPv6", stack/pico_socket.c:1179-1185), so there are no reference fragments to capture as
make_ref_fragtx.py does for IPv4.  Its receiver does reassemble them: the fragments that the
restatement of pico_ipv6_fragment_batch_dev's contract (tests/fragtx6_ref.py) cuts, with F_WRITE,
are fed in a shuffled arrival order through rr_reasm(1, ...) of oracle/_ref/libref_rx.so (the
reference stack compiled unmodified; pico_ipv6_extension_headers, then pico_ipv6_process_frag,
modules/pico_fragments.c:432-498, as in make_ref_reasm.py).  Asserted here for every fragmented
row: the reference hands on a datagram of the input's transport length and transport bytes (the
crc field holding the batch's value), and for TCP / UDP pico_transport_crc_check accepts it.  The
source address's second byte is the protocol: the reference's check dispatches on header byte 9.

A datagram that fits the MTU goes out whole: it is no fragment and goes through no reassembly, so
those rows are pinned by the restatement alone (pinned = 0); so is the crc check of a fragmented
TCP row whose transport is shorter than a TCP header (no checksum is computed: its bytes are still
pinned).

Datagrams: TCP / UDP / ICMPv6 in turn, T from 1 to 6000 transport bytes around every edge of the
split, at MTU 1280, 1500 and 72 (per = 24: many fragments, the TCP crc in fragment 0's last bytes).

Output (data only): ref_fragtx6_cases.npz, per MTU m in (1280, 1500, 72), prefix "m<mtu>_":
  buf uint8[], off uint64[n], len uint32[n], id uint32[n], proto uint8[n], groups uint32[n, 2],
  out_off uint64[n], out_cap uint32[n], out_size, stride, exp_out uint8[out_size] (canary 0xA5),
  slot_off uint64[n_frag], slot_len uint32[n_frag], count uint32[n], transport uint16[n],
  pinned uint8[n]
"""
from __future__ import annotations

import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from picotcp_amd import batch, synth  # noqa: E402
from tests import fragtx6_ref as R  # noqa: E402
from tests.golden.make_ref_reasm import REF_RX, ref_lib  # noqa: E402

CANARY = 0xA5
# (mtu, stride, region offset mod 16)
MTUS = ((1280, 1280, 0), (1500, 1504, 8), (72, 72, 3))


def lengths(mtu: int):
    per = (mtu - 48) & ~7
    if mtu == 72:
        return [1, 17, 24, 32, 33, 47, 48, 49, 72, 100, 333, 600]
    return [1, 8, 100, mtu - 41, mtu - 40, mtu - 39, per, per + 1, 2 * per - 1, 2 * per, 2 * per + 1, 3 * per, 3000, 4001, 6000]


def case(mtu: int, stride: int, out_off: int, seed: int):
    """One batch of the restatement at `mtu`: the arrays of the fixture."""
    T = np.array(lengths(mtu))
    proto = np.array([6, 17, 58])[np.arange(T.size) % 3]
    buf, off, dlen, ids, groups, ooff, cap, n_frag, out_size = synth.ipv6_oversized(
        T, mtu=mtu, stride=stride, seed=seed, proto=proto, align=np.arange(T.size) * 7 % 16, out_off=out_off, b9_proto=True)
    out = np.full(out_size, CANARY, np.uint8)
    v, cnt, l4, of = R.fragment(buf, batch.make_desc(off, dlen, ids), mtu, groups, n_frag, out,
                                batch.make_desc(ooff, cap), stride, R.F_WRITE)
    assert (v == R.V_ACCEPT).all()
    return dict(buf=buf, off=off, len=dlen, id=ids, proto=proto.astype(np.uint8), groups=groups, out_off=ooff, out_cap=cap,
                out_size=np.array([out_size], np.uint64), stride=np.array([stride], np.uint32), exp_out=out,
                slot_off=of["off"].copy(), slot_len=of["len"].copy(), count=cnt, transport=l4)


def pin(Rx, c, rng) -> np.ndarray:
    """Every fragmented row of case c through the reference's reassembly; returns the pinned column."""
    n = c["len"].size
    pinned = np.zeros(n, np.uint8)
    out = c["exp_out"]
    for g in range(n):
        cnt, first = int(c["count"][g]), int(c["groups"][g, 0])
        if cnt < 2:
            continue                                    # sent whole: no fragment, no reassembly
        order = rng.permutation(cnt)
        offs = np.ascontiguousarray(c["slot_off"][first:first + cnt][order])
        lens = np.ascontiguousarray(c["slot_len"][first:first + cnt][order])
        rout = np.zeros(70000, np.uint8)
        rl, rm, rc = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_int(0)
        ok = Rx.rr_reasm(1, out.ctypes.data, offs.ctypes.data, lens.ctypes.data, cnt, rout.ctypes.data, rout.size,
                         ctypes.byref(rl), ctypes.byref(rm), ctypes.byref(rc))
        o, ln, pr = int(c["off"][g]), int(c["len"][g]), int(c["proto"][g])
        T = ln - 40
        assert ok == 1 and rl.value == T and rm.value == pr, (g, ok, rl.value, T, rm.value)
        want = c["buf"][o + 40:o + ln].copy()
        at = R.CRC_AT[pr]
        if T >= R.MIN_HDR[pr]:
            want[at], want[at + 1] = int(c["transport"][g]) >> 8, int(c["transport"][g]) & 0xFF
        assert np.array_equal(rout[40:40 + T], want), g
        if pr in (6, 17) and T >= R.MIN_HDR[pr]:
            assert rc.value > 0, (g, pr, rc.value)      # pico_transport_crc_check accepts
        pinned[g] = 1
    return pinned


def build(Rx, seed: int = 20261021):
    rng = np.random.default_rng(seed)
    arrays = {}
    for k, (mtu, stride, out_off) in enumerate(MTUS):
        c = case(mtu, stride, out_off, 70 + k)
        c["pinned"] = pin(Rx, c, rng)
        for name, a in c.items():
            arrays[f"m{mtu}_{name}"] = a
    return arrays


def main() -> None:
    if not os.path.exists(REF_RX):
        sys.exit(f"{REF_RX} missing: run `make -C oracle refrx` first")
    arrays = build(ref_lib())
    np.savez_compressed(os.path.join(HERE, "ref_fragtx6_cases.npz"), **arrays)
    rows = sum(arrays[f"m{m}_len"].size for m, _, _ in MTUS)
    pinned = sum(int(arrays[f"m{m}_pinned"].sum()) for m, _, _ in MTUS)
    frags = sum(int(arrays[f"m{m}_count"].sum()) for m, _, _ in MTUS)
    print(f"ref_fragtx6_cases.npz: {rows} datagrams, {frags} fragments; {pinned} rows reassembled by the reference, "
          f"{rows - pinned} pinned by the restatement alone (sent whole)")


if __name__ == "__main__":
    main()
