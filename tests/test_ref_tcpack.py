"""The restatement of pico_tcp_ack_batch_dev's contract (tests/tcpack_ref.py) pinned to the compiled
reference stack: tests/golden/ref_tcpack_cases.npz (tests/golden/make_ref_tcpack.py) holds 18
connections' bursts with the ACK frame the stack itself sent to each burst's last arrival.  Here (no
GPU): the restatement, fed by tcprx_ref.coalesce, reproduces every frame byte for byte -- the ack
number, rwnd, the WS byte, thl, the option layout, the SACK block, the lengths and both checksums;
tests/test_gpu_tcpack.py checks the kernel against the restatement and against this fixture.  Pinned
by the restatement alone, not by a reference run: shift > 0 (it needs more than 64 KiB of receive
space, the reference's queue is 16 KiB) and IPv6 (the frozen driver has no IPv6 TCP path); and, since
the reference's next_segment follows one contiguous run, no reference run yields two blocks."""
from __future__ import annotations

import os

import numpy as np

from picotcp_amd import batch, synth
from tests import tcpack_ref as A
from tests import tcprx_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
M32 = 0xFFFFFFFF
REGION = 100
_fixture = None


def fixture():
    """The fixture's arrays (loaded once, shared, read-only)."""
    global _fixture
    if _fixture is None:
        c = np.load(os.path.join(GOLDEN, "ref_tcpack_cases.npz"))
        _fixture = {k: c[k] for k in c.files}
        for a in _fixture.values():
            a.setflags(write=False)
    return _fixture


def batch_of(a):
    """The fixture as the two batches' arguments: (buf, seg DESC, groups, conn, rx out DESC, rx out size,
    template buffer, template DESC, ack records, ack out DESC, ack out size)."""
    m = a["group"].shape[0]
    conn = np.stack([a["rcv_before"], a["sack_ok"].astype(np.uint32)], axis=1).astype(np.uint32)
    ak = np.zeros(m, A.ACK_DTYPE)
    ak["space"], ak["tsval"], ak["tsecr"], ak["aflags"] = a["space"], a["tsval"], a["tsecr"], a["ts_ok"]
    return (a["buf"], batch.make_desc(a["off"], a["len"]), a["group"], conn,
            batch.make_desc(np.arange(m) * 4096, np.full(m, 4096)), m * 4096,
            np.ascontiguousarray(a["tmpl"]).reshape(-1), batch.make_desc(np.arange(m) * 40, np.full(m, 40)), ak,
            batch.make_desc(np.arange(m) * REGION, np.full(m, REGION)), m * REGION)


def reference_frames(a):
    o = np.concatenate([[0], np.cumsum(a["ack_len"].astype(np.int64))])
    return [bytes(a["ack"][o[g]:o[g + 1]]) for g in range(a["ack_len"].size)]


def check_against_reference(a, v, oa, out, note=""):
    """Frames (of the restatement or of the kernel) against the reference stack's own, in full."""
    assert (v == A.V_ACCEPT).all(), note
    for g, want in enumerate(reference_frames(a)):
        assert int(oa["off"][g]) == REGION * g and int(oa["len"][g]) == len(want) and int(oa["seed"][g]) == 0, (g, note)
        assert bytes(out[REGION * g:REGION * g + len(want)]) == want, f"connection {g} {note}"


def restated(a):
    buf, seg, grp, conn, rod, rsize, tb, td, ak, fd, fsize = batch_of(a)
    _, ol, sv = R.coalesce(buf, seg, grp, conn, np.zeros(rsize, np.uint8), rod)
    out = np.full(fsize, 0xEE, np.uint8)
    v, oa, sv2 = A.ack_batch(buf, seg, grp, conn, ol, sv, tb, td, ak, out, fd)
    return v, oa, sv, sv2, out


def test_restatement_reproduces_every_reference_frame():
    a = fixture()
    v, oa, _, _, out = restated(a)
    check_against_reference(a, v, oa, out)
    for g in range(v.size):                                 # nothing behind a frame is written
        assert (out[REGION * g + int(oa["len"][g]):REGION * (g + 1)] == 0xEE).all()


def test_fixture_covers_the_cases():
    a = fixture()
    _, _, sv, sv2, _ = restated(a)
    frames = reference_frames(a)
    assert len(frames) == 18
    blocks = []
    for g, f in enumerate(frames):
        thl = 4 * (f[32] >> 4)
        assert len(f) == 20 + thl and f[33] == 0x10
        o = f[40:]
        k = 13 if a["ts_ok"][g] else 3
        blocks.append((o[k + 1] - 2) // 8 if o[k] == 5 else 0)
        first, cnt = (int(x) for x in a["group"][g])
        if a["sack_ok"][g]:                                 # the last arrival is a verified held segment
            assert sv2[first + cnt - 1] == R.V_TCP_HELD
        else:
            assert blocks[-1] == 0
    assert set(blocks) == {0, 1}
    assert {int(t) for t, s in zip(a["ts_ok"], a["sack_ok"]) if s} == {0, 1}          # option sets 3 and 4
    assert (a["sack_ok"] == 0).sum() >= 3
    # corrupted held / old segments: judged here, not by the coalescing
    changed = sv != sv2
    assert changed.sum() >= 4 and set(sv[changed].tolist()) == {R.V_TCP_HELD, R.V_TCP_OLD} and (sv2[changed] == R.V_L4_BAD).all()
    # a stream across 2^32: a block whose right edge wrapped, and held segments skipped by the raw compare
    wrapped = [g for g, f in enumerate(frames) if blocks[g] and int.from_bytes(f[-9:-5], "big") > int.from_bytes(f[-5:-1], "big")]
    assert wrapped, "no block across 2^32"
    assert any(a["sack_ok"][g] and not blocks[g] for g in range(len(frames)))


def test_sack_prepare_quirks():
    """tcp_sack_prepare as the reference has it: one contiguous run from the first segment."""
    assert A.sack_prepare([], 100) == []
    assert A.sack_prepare([(200, 50), (250, 50), (400, 10)], 100) == [(200, 300)]          # the walk ends at the gap
    assert A.sack_prepare([(200, 50), (260, 50)], 100) == [(200, 250)]
    assert A.sack_prepare([(0, 50)], 0) == []                                               # left == 0: no open block
    assert A.sack_prepare([(0, 50), (50, 50)], 0) == [(50, 100)]                            # the run loses its first segment
    assert A.sack_prepare([(50, 10), (60, 10)], 0xFFFFFF00) == []                           # raw compare past the wrap
    assert A.sack_prepare([(0xFFFFFFF0, 0x20), (0x10, 0x10)], 0xFFFFFF00) == [(0xFFFFFFF0, 0x10)]   # 0x10 < rcv': not added


def test_window_and_options():
    assert A.window(16384, 1000, 500) == (14884, 0)
    assert A.window(1000, 1500, 0) == (0, 0)                # space < out_len clamps to 0
    assert A.window(0x20000, 0, 0) == (0x8000, 2)
    assert A.window(0x1FFFF, 0, 0) == (0xFFFF, 1)
    assert A.window(0x7FFFF, 0, 0) == (0xFFFF, 3)
    assert A.options(0, False, 0, 0, []) == bytes([3, 3, 0, 0])
    assert A.options(2, True, 1, 2, []) == bytes([3, 3, 2, 8, 10, 0, 0, 0, 1, 0, 0, 0, 2, 1, 1, 0])
    o = A.options(0, True, 1, 2, [(1, 2), (3, 4), (5, 6)])
    assert len(o) == 40 and o[13:15] == bytes([5, 26]) and o[-1] == 0
    assert len(A.options(0, False, 0, 0, [(1, 2)])) == 16


def test_synth_inputs_and_ipv6_restated():
    """synth.tcp_ack_inputs' templates pass the family checks for both families, and the restated frames
    verify: IPv4 header checksum and both families' TCP checksum sum to zero."""
    from oracle import oracle as O
    conns, _ = synth.tcp_rx_bursts(8, seed=3, family=[4, 6] * 4, per=300, max_bytes=3000)
    buf, off, ln, grp, conn, ooff, cap, osize = synth.tcp_rx_pack(conns)
    tb, toff, tln, ak, foff, fcap, fsize = synth.tcp_ack_inputs(conns, space=[16384, 0x40000] * 4)
    seg = batch.make_desc(off, ln)
    _, ol, sv = R.coalesce(buf, seg, grp, conn, np.zeros(osize, np.uint8), batch.make_desc(ooff, cap))
    out = np.zeros(fsize, np.uint8)
    v, oa, _ = A.ack_batch(buf, seg, grp, conn, ol, sv, tb, batch.make_desc(toff, tln), ak, out, batch.make_desc(foff, fcap))
    assert (v == A.V_ACCEPT).all() and (oa["len"] > 0).all()
    for g in range(8):
        f = out[int(oa["off"][g]):int(oa["off"][g]) + int(oa["len"][g])]
        n = 40 if g % 2 else 20
        tl = f.size - n
        if n == 20:
            assert O.checksum(f[:20]) == 0
            ph = np.concatenate([f[12:20], np.array([0, 6, tl >> 8, tl & 0xFF], np.uint8)])
        else:
            ph = np.concatenate([f[8:40], np.array([0, 0, tl >> 8, tl & 0xFF, 0, 0, 0, 6], np.uint8)])
        assert O.dualbuffer_checksum(ph, f[n:]) == 0
        assert int(f[n + 22]) == (2 if g % 2 else 0)        # the WS option's shift
