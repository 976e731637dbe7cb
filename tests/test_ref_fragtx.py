"""The TX fragmentation contract pinned to the fragments the compiled reference stack itself emits.

tests/golden/ref_fragtx_cases.npz (tests/golden/make_ref_fragtx.py): every IPv4 datagram the
unmodified reference stack handed to pico_datalink_send for UDP sendto calls larger than its MTU
of 1500 (pico_socket_xmit_fragments, stack/pico_socket.c:1131-1251; pico_ipv4_frame_push,
modules/pico_ipv4.c:1039-1079).  Here (no GPU): tests/fragtx_ref.py, the restatement the GPU tests
check the kernel against, reproduces those fragments byte for byte from the unfragmented datagram,
and its fragments reassemble (oracle.ipv4_reassemble) into that datagram again."""
from __future__ import annotations

import os

import numpy as np
import pytest

from oracle import oracle as O
from picotcp_amd import batch, synth
from tests import fragtx_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def fixture():
    c = np.load(os.path.join(GOLDEN, "ref_fragtx_cases.npz"))
    return c["buf"], c["off"].astype(np.int64), c["len"].astype(np.int64), c["group"], c["payload"]


def datagrams(buf, off, ln, group, seed=3):
    """Per captured group: (input datagram = the first fragment's header with len / frag / crc
    scrambled + the concatenated payloads, the captured fragments in order)."""
    rng = np.random.default_rng(seed)
    out = []
    for g in range(int(group.max()) + 1):
        idx = np.nonzero(group == g)[0]
        frs = [buf[off[i]:off[i] + ln[i]] for i in idx]
        h = frs[0][:20].copy()
        h[[2, 3, 6, 7, 10, 11]] = rng.integers(0, 256, 6)
        out.append((np.concatenate([h] + [f[20:] for f in frs]), frs))
    return out


def run_ref(dgrams, mtu, stride, flags=0, out_off=12):
    """The restatement over a list of datagrams packed back to back; returns (out, out_frag, groups,
    out_desc, verdict, count, transport)."""
    lens = np.array([d.size for d in dgrams], np.int64)
    offs = np.concatenate([[0], np.cumsum(lens[:-1])])
    base = np.concatenate(dgrams)
    cnt = np.array([synth.fragtx_count(int(x), mtu) for x in lens], np.uint32)
    first = np.concatenate([[0], np.cumsum(cnt[:-1])]).astype(np.uint32)
    groups = np.stack([first, cnt], axis=1)
    cap = cnt.astype(np.int64) * stride
    ooff = out_off + np.concatenate([[0], np.cumsum(cap[:-1] + 16)])
    out = np.full(int(ooff[-1] + cap[-1] + 16), 0xA5, np.uint8)
    od = batch.make_desc(ooff, cap)
    v, c, l4, of = R.fragment(base, batch.make_desc(offs, lens), mtu, groups, int(cnt.sum()), out, od, stride, flags)
    return out, of, groups, od, v, c, l4


def test_fixture_shape():
    buf, off, ln, group, payload = fixture()
    assert set([1473, 1480, 1481, 2952, 2953, 4000, 9000, 65507]) <= set(payload.tolist()) and payload.size >= 18
    counts = np.bincount(group)
    np.testing.assert_array_equal(counts, -(-(payload.astype(np.int64) + 8) // 1480))
    assert counts.max() == 45


def test_restatement_reproduces_reference_fragments():
    dg = datagrams(*fixture()[:4])
    out, of, groups, od, v, c, l4 = run_ref([d for d, _ in dg], 1500, 1504)
    assert (v == R.V_ACCEPT).all()
    for g, (_, frs) in enumerate(dg):
        assert c[g] == len(frs)
        ids = {bytes(f[4:6]) for f in frs}
        assert len(ids) == 1
        for k, f in enumerate(frs):
            d = of[groups[g, 0] + k]
            assert (int(d["len"]), int(d["seed"])) == (f.size, 0)
            np.testing.assert_array_equal(out[int(d["off"]):int(d["off"]) + f.size], f, err_msg=f"group {g} fragment {k}")
            assert O.checksum(f[:20]) == 0
            fr = (int(f[6]) << 8) | int(f[7])
            assert fr == (k * 1480 >> 3) | (0x2000 if k + 1 < len(frs) else 0)     # MF but the last, DF never


def test_single_frame_is_df():
    """A payload that fits goes out as one datagram with frag = 0x4000 (pico_ipv4.c:1059): the UDP rows
    of ref_tx_cases.npz."""
    c = np.load(os.path.join(GOLDEN, "ref_tx_cases.npz"))
    buf, off, ln, proto = c["buf"], c["off"].astype(np.int64), c["len"].astype(np.int64), c["proto"]
    rows = np.nonzero(proto == 17)[0]
    assert rows.size >= 20
    rng = np.random.default_rng(4)
    dgs = []
    for i in rows:
        d = buf[off[i]:off[i] + ln[i]].copy()
        assert (int(d[6]) << 8 | int(d[7])) == 0x4000
        d[[2, 3, 6, 7, 10, 11]] = rng.integers(0, 256, 6)
        dgs.append(d)
    out, of, groups, od, v, cnt, l4 = run_ref(dgs, 1500, 1504)
    assert (v == R.V_ACCEPT).all() and (cnt == 1).all()
    for g, i in enumerate(rows):
        o = int(od["off"][g])
        np.testing.assert_array_equal(out[o:o + ln[i]], buf[off[i]:off[i] + ln[i]])


def test_fragments_reassemble_to_the_datagram():
    """The restatement's fragments (F_WRITE) through oracle.ipv4_reassemble: the datagram again,
    header normalised, its UDP checksum verifying (0)."""
    dg = [d for d, _ in datagrams(*fixture()[:4])]
    for mtu, stride in ((1500, 1504), (1280, 1280), (576, 576)):
        out, of, groups, od, v, c, l4 = run_ref(dg, mtu, stride, flags=R.F_WRITE)
        assert (v == R.V_ACCEPT).all() and (l4 != 0).any()
        cap = np.array([d.size for d in dg], np.int64)
        ro = 12 + np.concatenate([[0], np.cumsum((cap[:-1] + 31) // 16 * 16)])      # (regions on 12 mod 16)
        rout = np.zeros(int(ro[-1] + cap[-1] + 16), np.uint8)
        ol, rl4, rv = O.ipv4_reassemble(out, of, groups, rout, batch.make_desc(ro, cap))
        assert (rv == R.V_ACCEPT).all() and (rl4 == 0).all()
        for g, d in enumerate(dg):
            assert ol[g] == d.size - 20
            got = rout[int(ro[g]):int(ro[g]) + d.size]
            want = d.copy()
            want[[2, 3, 6, 7, 10, 11]] = got[[2, 3, 6, 7, 10, 11]]       # the first fragment's own len / frag / crc
            want[26], want[27] = l4[g] >> 8, l4[g] & 0xFF                # UDP crc
            np.testing.assert_array_equal(got, want)


REF_RX = os.path.join(os.path.dirname(GOLDEN), "..", "oracle", "_ref", "libref_rx.so")


@pytest.mark.skipif(not os.path.exists(REF_RX), reason="oracle/_ref/libref_rx.so not built here")
def test_restatement_on_live_reference_capture():
    """A fresh capture of the live reference stack (its ids and the random lengths differ run to
    run): the restatement rebuilds every fragment it emits."""
    from tests.golden import make_ref_fragtx as M
    rng = np.random.default_rng(int.from_bytes(os.urandom(4), "little"))
    lengths = [1473, 65507] + [int(x) for x in rng.integers(1473, 20000, 6)]
    buf, off, ln, group, payload = M.pack(M.capture(lengths, seed=int(rng.integers(1 << 30))))
    np.testing.assert_array_equal(payload, lengths)
    dg = datagrams(buf, off.astype(np.int64), ln.astype(np.int64), group)
    out, of, groups, od, v, c, l4 = run_ref([d for d, _ in dg], 1500, 1536)
    assert (v == R.V_ACCEPT).all()
    for g, (_, frs) in enumerate(dg):
        assert c[g] == len(frs) == -(-(lengths[g] + 8) // 1480)
        for k, f in enumerate(frs):
            o = int(of[groups[g, 0] + k]["off"])
            np.testing.assert_array_equal(out[o:o + f.size], f, err_msg=f"send {g} fragment {k}")
