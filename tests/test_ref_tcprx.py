"""The restatement of pico_tcp_coalesce_batch_dev's contract (tests/tcprx_ref.py) pinned to the compiled
reference stack: tests/golden/ref_tcprx_cases.npz (tests/golden/make_ref_tcprx.py) holds 24
connections' received bursts -- reordered, duplicated, resegmented, with holes and corrupted frames --
with the rcv_nxt the stack acknowledged afterwards and the bytes pico_socket_read returned.  Here (no
GPU): the restatement reproduces both on every connection; tests/test_gpu_tcprx.py checks the kernel
against the restatement and against this fixture.  Not pinned by a reference run: IPv6 (the frozen
driver has no IPv6 TCP path), overlapping segments that disagree, and groups beyond the reference's
input queue."""
from __future__ import annotations

import os

import numpy as np
import pytest

from picotcp_amd import batch, synth
from tests import tcprx_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REF_RX = os.path.join(os.path.dirname(GOLDEN), "..", "oracle", "_ref", "libref_rx.so")
M32 = 0xFFFFFFFF
_fixture = None


def fixture():
    """The fixture's arrays (loaded once, shared, read-only)."""
    global _fixture
    if _fixture is None:
        c = np.load(os.path.join(GOLDEN, "ref_tcprx_cases.npz"))
        _fixture = {k: c[k] for k in c.files}
        for a in _fixture.values():
            a.setflags(write=False)
    return _fixture


def batch_of(a, slack: int = 64, out_off: int = 0):
    """The fixture as the batch's arguments: (buf, seg DESC, groups, conn, out DESC, out_size); every
    region holds the reference's delivery + slack."""
    n = a["group"].shape[0]
    cap = ((a["rcv_after"].astype(np.int64) - a["rcv_before"].astype(np.int64)) & M32) + slack
    ooff = np.zeros(n, np.uint64)
    pos = 0
    for g in range(n):
        pos += (out_off - pos) % 16
        ooff[g] = pos
        pos += int(cap[g])
    conn = np.stack([a["rcv_before"], a["sack_ok"].astype(np.uint32)], axis=1).astype(np.uint32)
    return a["buf"], batch.make_desc(a["off"], a["len"]), a["group"], conn, batch.make_desc(ooff, cap), pos + 16


def check_against_reference(a, v, ol, sv, out, od, note=""):
    """Results (of the restatement or of the kernel) against what the reference stack did."""
    assert (v == R.V_ACCEPT).all(), note
    want = (a["rcv_after"].astype(np.int64) - a["rcv_before"].astype(np.int64)) & M32
    np.testing.assert_array_equal(ol, want, err_msg=note)                # rcv_nxt after, from the stack's ACKs
    np.testing.assert_array_equal(a["read_len"], want, err_msg=note)
    ro = np.concatenate([[0], np.cumsum(a["read_len"].astype(np.int64))])
    for g in range(want.size):
        o = int(od["off"][g])
        np.testing.assert_array_equal(out[o:o + int(want[g])], a["read"][ro[g]:ro[g + 1]], err_msg=f"connection {g} {note}")


def corrupted(a):
    """(indices of frames whose IPv4 header checksum fails, indices whose TCP checksum fails), found
    with the oracle's own sums."""
    from oracle import oracle as O
    net, l4 = [], []
    for i, (o, n) in enumerate(zip(a["off"].astype(np.int64), a["len"].astype(np.int64))):
        f = a["buf"][o:o + n]
        if O.checksum(f[:20]) != 0:
            net.append(i)
        elif O.dualbuffer_checksum(np.concatenate([f[12:20], np.array([0, 6, (n - 20) >> 8, (n - 20) & 0xFF], np.uint8)]), f[20:]) != 0:
            l4.append(i)
    return net, l4


def test_restatement_reproduces_the_reference_fixture():
    a = fixture()
    assert a["group"].shape[0] >= 24 and int(a["sack_ok"].sum()) >= 8 and (a["sack_ok"] == 0).sum() >= 8
    buf, sd, groups, conn, od, out_size = batch_of(a)
    out = np.full(out_size, 0xA5, np.uint8)
    v, ol, sv = R.coalesce(buf, sd, groups, conn, out, od)
    check_against_reference(a, v, ol, sv, out, od)
    # the corrupted frames: every flipped IPv4 header is NET_BAD; a flipped payload is L4_BAD where the
    # chain reached it and is never delivered
    net, l4 = corrupted(a)
    assert len(net) >= 12 and len(l4) >= 12
    assert (sv[net] == R.V_NET_BAD).all()
    assert set(sv[l4].tolist()) <= {R.V_L4_BAD, R.V_TCP_HELD, R.V_TCP_OLD} and (sv[l4] == R.V_L4_BAD).sum() >= 6
    assert set(sv.tolist()) >= {R.V_ACCEPT, R.V_NET_BAD, R.V_L4_BAD, R.V_TCP_OLD, R.V_TCP_HELD}
    # the region is the window: with exactly the delivered bytes as capacity nothing changes
    buf, sd, groups, conn, od0, out_size = batch_of(a, slack=0)
    out0 = np.full(out_size, 0xA5, np.uint8)
    v0, ol0, sv0 = R.coalesce(buf, sd, groups, conn, out0, od0)
    np.testing.assert_array_equal(ol0, ol)
    np.testing.assert_array_equal(sv0, sv)


@pytest.mark.skipif(not os.path.exists(REF_RX), reason="oracle/_ref/libref_rx.so not built here")
def test_restatement_on_live_reference_capture():
    """A fresh run of the committed generator against the live reference stack (its initial sequence
    numbers come from pico_rand, so the frames' ack fields and checksums differ run to run): the same
    bursts, the same deliveries as the fixture, and the restatement reproduces them."""
    from tests.golden import make_ref_tcprx as M
    live = M.pack(M.capture())
    a = fixture()
    for k in ("off", "len", "group", "sack_ok", "read", "read_len"):
        np.testing.assert_array_equal(live[k], a[k], err_msg=k)
    np.testing.assert_array_equal((live["rcv_after"] - live["rcv_before"]) & M32, (a["rcv_after"] - a["rcv_before"]) & M32)
    buf, sd, groups, conn, od, out_size = batch_of(live)
    out = np.full(out_size, 0xA5, np.uint8)
    v, ol, sv = R.coalesce(buf, sd, groups, conn, out, od)
    check_against_reference(live, v, ol, sv, out, od, "(live)")


# ---------------------------------------------------------------- restatement self-checks

def run(conns, **kw):
    buf, off, ln, groups, conn, ooff, cap, out_size = synth.tcp_rx_pack(conns, **kw)
    od = batch.make_desc(ooff, cap)
    out = np.full(out_size, 0xA5, np.uint8)
    v, ol, sv = R.coalesce(buf, batch.make_desc(off, ln), groups, conn, out, od)
    return v, ol, sv, out, od


def frames_of(rng, rcv, data, per, family=4):
    return [synth.tcp_rx_frame(rng, (rcv + a) & M32, data[a:a + per], family, 32) for a in range(0, data.size, per)]


@pytest.mark.parametrize("family", [4, 6])
def test_sack_against_no_sack_on_the_same_shuffled_group(family):
    """With SACK a shuffled group delivers the whole stream; without, exactly the segments that arrive
    in sequence, one behind the other -- and both stop at the same byte when the group is in order."""
    rng = np.random.default_rng(7 + family)
    data = synth.random_bytes(8, 8 * 500)
    f = frames_of(rng, 99, data, 500, family)
    order = [2, 0, 3, 1, 4, 7, 5, 6]
    sh = [f[i] for i in order]
    v, ol, sv, out, od = run([(sh, 99, True, data.size), (sh, 99, False, data.size), (f, 99, True, data.size),
                              (f, 99, False, data.size)], align=3, out_off=5)
    assert list(ol) == [4000, 1000, 4000, 4000]
    assert list(sv[:8]) == [R.V_ACCEPT] * 8
    # no SACK: 0 (arrival 1) then 1 (arrival 3); 2 arrived before them and is HELD, like everything behind
    assert list(sv[8:16]) == [R.V_TCP_HELD, R.V_ACCEPT, R.V_TCP_HELD, R.V_ACCEPT] + [R.V_TCP_HELD] * 4
    for g in (0, 2, 3):
        o = int(od["off"][g])
        np.testing.assert_array_equal(out[o:o + 4000], data)
    o = int(od["off"][1])
    np.testing.assert_array_equal(out[o:o + 1000], data[:1000])
    assert (out[o + 1000:o + 4000] == 0xA5).all()


def test_seq_wraps_across_2_32():
    rng = np.random.default_rng(9)
    data = synth.random_bytes(10, 3000)
    rcv = M32 - 1200
    f = frames_of(rng, rcv, data, 1000)
    assert int.from_bytes(bytes(f[2][24:28]), "big") == 799            # the third segment's seq has wrapped
    old = synth.tcp_rx_frame(rng, (rcv - 10) & M32, data[:5])
    ahead = synth.tcp_rx_frame(rng, (rcv + 3500) & M32, data[:5])
    v, ol, sv, out, od = run([([f[2], old, f[1], ahead, f[0]], rcv, True, 3000)])
    assert list(ol) == [3000] and list(sv) == [R.V_ACCEPT, R.V_TCP_OLD, R.V_ACCEPT, R.V_TCP_HELD, R.V_ACCEPT]
    np.testing.assert_array_equal(out[:3000], data)
    assert R.seq_before(M32, 5) and not R.seq_before(5, M32) and not R.seq_before(7, 7)
    assert R.seq_before(0x80000000, 0) and not R.seq_before(0, 0x80000000)   # pico_seq_compare at 2^31 apart


@pytest.mark.parametrize("sack", [True, False])
def test_struck_member_replaced_by_a_later_copy(sack):
    """A member whose TCP checksum fails is struck (L4_BAD); a later retransmission of its seq -- here
    with another split -- takes its place, and the delivered bytes are the good ones."""
    rng = np.random.default_rng(11)
    data = synth.random_bytes(12, 3000)
    f = frames_of(rng, 500, data, 1000)
    bad = f[1].copy()
    bad[-7] ^= 0x20
    re = [synth.tcp_rx_frame(rng, 1500, data[1000:1600]), synth.tcp_rx_frame(rng, 2100, data[1600:2000])]
    v, ol, sv, out, od = run([([f[0], bad, f[2]] + re, 500, sack, 3000), ([f[0], bad, f[2]], 500, sack, 3000)])
    # with SACK f[2], which arrived before the repair, closes the stream; without, it is lost to this call
    assert list(ol) == [3000 if sack else 2000, 1000]
    assert list(sv[:5]) == [R.V_ACCEPT, R.V_L4_BAD, R.V_ACCEPT if sack else R.V_TCP_HELD, R.V_ACCEPT, R.V_ACCEPT]
    assert list(sv[5:]) == [R.V_ACCEPT, R.V_L4_BAD, R.V_TCP_HELD]
    np.testing.assert_array_equal(out[:int(ol[0])], data[:int(ol[0])])
