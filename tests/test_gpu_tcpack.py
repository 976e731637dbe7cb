"""GPU: the burst's ACKs (pico_tcp_ack_batch_dev) behind the coalescing, against the numpy restatement of
its contract (tests/tcpack_ref.py, pinned to the compiled reference stack by tests/test_ref_tcpack.py)
and against that stack's own ACK frames (tests/golden/ref_tcpack_cases.npz).  Every case runs the
coalescing on the device first (checked against tests/tcprx_ref.py) and hands its device outputs on as
they are.  Every comparison is over the WHOLE output buffer, pre-filled with a canary: the frames' bytes
and every byte around them -- before and behind each region, and behind each frame inside its region
-- are compared exactly.  Segment verdicts: only TCP_OLD / TCP_HELD may change, and only to L4_BAD
(asserted in every case).  The launcher has two launch shapes: four waves per connection (every test
but one) and one wave per connection (test_large_batch_one_wave_per_connection)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from picotcp_amd import batch, synth
from tests import flowgroup_ref as FG
from tests import tcpack_ref as A
from tests import tcprx_ref as R
from tests import test_ref_tcpack as RF
from tests.gpu_util import DEV, pairs_dev, replay_captured, to_dev

pytestmark = pytest.mark.gpu

CANARY = 0xA5
OK, LB, MF, CT, OL, HE = R.V_ACCEPT, R.V_L4_BAD, R.V_MALFORMED, R.V_TCP_CTRL, R.V_TCP_OLD, R.V_TCP_HELD
M32 = 0xFFFFFFFF
BAD = 100000                        # piece index + BAD: that piece with a flipped payload bit


def dev_desc(d):
    return to_dev(d.view(np.uint8)) if d.size else torch.zeros(16, dtype=torch.uint8, device=DEV)


def run_arrays(buf, sd, groups, conn, rx_size, rod, tb, td, ak, fsize, fd, base=None):
    """Coalescing then ACKs on the device, each against its restatement, everything compared.  Returns the
    restated (verdict, out_ack, seg verdicts before, seg verdicts after, out_len, frames' buffer) and the
    device tensors (out, out_ack)."""
    want_rx = np.full(rx_size, CANARY, np.uint8)
    wv, wl, ws = R.coalesce(buf, sd, groups, conn, want_rx, rod)
    base = to_dev(buf) if base is None else base
    d_sd, d_grp, d_conn = dev_desc(sd), pairs_dev(groups), pairs_dev(conn)
    rx = torch.full((rx_size,), CANARY, dtype=torch.uint8, device=DEV)
    sv0 = torch.zeros(max(sd.size, 1), dtype=torch.uint8, device=DEV)
    n = len(wv)
    v, ol, sv = batch.tcp_coalesce_batch(base, d_sd, sd.size, d_grp, d_conn, rx, dev_desc(rod),
                                         results=(torch.empty(n, dtype=torch.uint8, device=DEV),
                                                  torch.empty(n, dtype=torch.int32, device=DEV), sv0))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(v.cpu().numpy(), wv)
    np.testing.assert_array_equal(ol.cpu().numpy().view(np.uint32), wl)
    np.testing.assert_array_equal(sv.cpu().numpy()[:sd.size], ws)

    want = np.full(fsize, CANARY, np.uint8)
    av, aoa, asv = A.ack_batch(buf, sd, groups, conn, wl, ws, tb, td, ak, want, fd)
    out = torch.full((fsize,), CANARY, dtype=torch.uint8, device=DEV)
    gv, goa = batch.tcp_ack_batch(base, d_sd, sd.size, d_grp, d_conn, ol, sv, to_dev(tb), dev_desc(td),
                                  to_dev(ak.view(np.uint8)), out, dev_desc(fd))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(gv.cpu().numpy(), av)
    got_oa = goa.cpu().numpy().view(R.DESC_DTYPE)
    for k in ("off", "len", "seed"):
        np.testing.assert_array_equal(got_oa[k], aoa[k], err_msg=k)
    np.testing.assert_array_equal(sv.cpu().numpy()[:sd.size], asv)
    bad = np.flatnonzero(out.cpu().numpy() != want)
    assert bad.size == 0, f"{bad.size} bytes differ, first at {bad[:8].tolist()}"
    ch = ws != asv
    assert np.isin(ws[ch], (OL, HE)).all() and (asv[ch] == LB).all()
    return (av, aoa, ws, asv, wl, want), (out, goa)


def run(conns, align=0, rx_off=0, out_off=0, region=100, t_align=0, **kw):
    buf, off, ln, groups, conn, ooff, cap, rx_size = synth.tcp_rx_pack(conns, align=align, out_off=rx_off)
    tb, toff, tln, ak, foff, fcap, fsize = synth.tcp_ack_inputs(conns, region=region, out_off=out_off, align=t_align, **kw)
    return run_arrays(buf, batch.make_desc(off, ln), groups, conn, rx_size, batch.make_desc(ooff, cap), tb,
                      batch.make_desc(toff, tln), ak, fsize, batch.make_desc(foff, fcap))


def conn_of(rng, rcv, per, pieces, sack, family=4, thl=20, cap=None, seed=0):
    """A connection whose stream is cut into pieces of `per` bytes: arrivals = piece indexes (+ BAD: the
    last payload byte with a flipped bit), seq = rcv + index * per."""
    npieces = max(p % BAD for p in pieces) + 1
    data = synth.random_bytes(7919 * seed + per, per * npieces)
    frames = []
    for p in pieces:
        i = p % BAD
        f = synth.tcp_rx_frame(rng, (rcv + i * per) & M32, data[i * per:(i + 1) * per], family, thl, 0x10)
        if p >= BAD:
            f = f.copy()
            f[-1] ^= 0x40
        frames.append(f)
    return (frames, rcv & M32, sack, per * npieces if cap is None else cap)


def blocks_of(frame: np.ndarray, n: int):
    """The SACK blocks of an ACK frame (n = network header bytes)."""
    o = bytes(frame[n + 20:])
    k = 13 if o[3] == 8 else 3
    if o[k] != 5:
        return []
    return [(int.from_bytes(o[k + 2 + 8 * b:k + 6 + 8 * b], "big"), int.from_bytes(o[k + 6 + 8 * b:k + 10 + 8 * b], "big"))
            for b in range((o[k + 1] - 2) // 8)]


def frame_of(res, g):
    av, aoa, _, _, _, want = res
    return want[int(aoa["off"][g]):int(aoa["off"][g]) + int(aoa["len"][g])]


# ---------------------------------------------------------------- the reference's own frames

@pytest.mark.parametrize("out_off", [0, 6])
def test_reference_fixture(out_off):
    """The 18 bursts the compiled reference stack received: the kernel writes the ACK the stack itself
    sent to each burst's last arrival, byte for byte."""
    a = RF.fixture()
    buf, sd, grp, conn, rod, rsize, tb, td, ak, fd, fsize = RF.batch_of(a)
    fd = fd.copy()
    fd["off"] += out_off
    (av, aoa, _, _, _, want), _ = run_arrays(buf, sd, grp, conn, rsize, rod, tb, td, ak, fsize + 16, fd)
    assert (av == OK).all()
    for g, f in enumerate(RF.reference_frames(a)):
        o = int(aoa["off"][g])
        assert o == RF.REGION * g + out_off and bytes(want[o:o + int(aoa["len"][g])]) == f, g


# ---------------------------------------------------------------- group sizes

def test_group_sizes():
    """Groups of 1, 2, 7, 64, 65, 512 and 513 segments (513: MALFORMED), each once complete and shuffled
    (all delivered) and once behind a hole (all held: with SACK one block over the whole run, and a
    corrupted member that splits it)."""
    rng = np.random.default_rng(300)
    conns = []
    for n in (1, 2, 7, 64, 65, 512, 513):
        conns.append(conn_of(rng, 1000 * n, 9, [int(i) for i in rng.permutation(n)], True, seed=n))
        held = [int(i) + 1 for i in rng.permutation(n)]
        if n in (7, 65):
            held[held.index(3)] = 3 + BAD
        conns.append(conn_of(rng, 5 + n, 9, held, True, family=6 if n % 2 else 4, seed=n + 1))
    res, _ = run(conns, align=3, out_off=5, ts_ok=[1, 0] * 7)
    av, aoa, ws, asv = res[:4]
    assert list(av) == [OK] * 12 + [MF, MF] and list(aoa["len"][12:]) == [0, 0]
    for k, n in enumerate((1, 2, 7, 64, 65, 512)):
        g = 2 * k + 1
        fam_n = 40 if n % 2 else 20
        rcv = 5 + n
        want = [(rcv + 9, rcv + 9 * 3)] if n in (7, 65) else [(rcv + 9, rcv + 9 * (n + 1))]
        assert blocks_of(frame_of(res, g), fam_n) == want, n
    assert (asv == LB).sum() == 2


# ---------------------------------------------------------------- held runs, families, options

@pytest.mark.parametrize("family", [4, 6])
def test_held_runs_options_and_families(family):
    """0 to 5 held runs behind a delivered prefix, x sack on / off x timestamps on / off: the block is the
    lowest run's (the reference's next_segment ends the walk at the first gap), without sack_ok there is
    none and the held bytes do not count against the window."""
    rng = np.random.default_rng(310 + family)
    runs = [[], [2, 3], [2, 5, 6], [3, 5, 7], [2, 3, 6, 8, 9, 11], [2, 4, 6, 8, 10]]
    conns, ts = [], []
    for k, held in enumerate(runs):
        for sack in (True, False):
            for t in (0, 1):
                order = [0] + [int(x) for x in rng.permutation(held)]
                conns.append(conn_of(rng, int(rng.integers(1 << 32)), 50 + k, order, sack, family, 20 + 12 * t, seed=k))
                ts.append(t)
    res, _ = run(conns, align=11, out_off=9, t_align=7, ts_ok=ts, space=16384)
    av, aoa, ws, asv, wl, _ = res
    N = 40 if family == 6 else 20
    assert (av == OK).all() and (aoa["len"] > 0).all()
    for g, c in enumerate(conns):
        k, sack, t = g // 4, not (g // 2) % 2, g % 2
        per, rcv = 50 + k, (c[1] + 50 + k) & M32
        f = frame_of(res, g)
        want = []
        if sack and runs[k]:
            first = runs[k][0]
            ln = 2 if runs[k][:2] == [first, first + 1] else 1
            want = [((rcv + (first - 1) * per) & M32, (rcv + (first - 1 + ln) * per) & M32)]
        assert blocks_of(f, N) == want, g
        assert (f[N + 23] == 8) == bool(t)
        assert int.from_bytes(bytes(f[N + 8:N + 12]), "big") == rcv
        held_bytes = per * len(runs[k]) if sack else 0
        assert int.from_bytes(bytes(f[N + 14:N + 16]), "big") == 16384 - per - held_bytes
        assert f.size == N + 20 + ((4 + 10 * t + (10 if want else 0) + 3) & ~3)


# ---------------------------------------------------------------- payload lengths and alignments

def test_payload_lengths_and_alignments():
    """Held and old payloads of 1, 15, 16, 17, 31, 1448 and 1460 bytes at every source alignment mod 16:
    per connection a delivered segment, its duplicate (old), a held one -- good, or with a flipped bit in
    the payload's LAST byte (held) or FIRST byte (old), which only a sum over exactly the payload sees."""
    rng = np.random.default_rng(320)
    conns, aligns = [], []
    for li, pl in enumerate((1, 15, 16, 17, 31, 1448, 1460)):
        for a in range(16):
            fam = (4, 6)[(a + li) % 2]
            c = conn_of(rng, int(rng.integers(1 << 32)), pl, [0, 0, 2 + (BAD if a % 3 == 0 else 0)], True, fam,
                        (20, 32, 60)[(a + li) % 3], seed=16 * li + a)
            if a % 3 == 1:
                c[0][1] = c[0][1].copy()
                c[0][1][c[0][1].size - pl] ^= 0x01          # the old duplicate's first payload byte
            conns.append(c)
            aligns += [a, (a + 7) % 16, a]
    res, _ = run(conns, align=aligns, out_off=13)
    av, aoa, ws, asv = res[:4]
    assert (av == OK).all() and (aoa["len"] > 0).all()
    assert list(ws[:3]) == [OK, OL, HE]
    for g in range(len(conns)):
        want = [OK, LB if g % 16 % 3 == 1 else OL, LB if g % 16 % 3 == 0 else HE]
        assert list(asv[3 * g:3 * g + 3]) == want, g


def test_segment_at_the_end_of_base():
    """A held segment whose buffer ends at the last byte of base_len, at every alignment of that end: the
    batch's base is a view of a larger allocation whose following bytes would break every sum if one of
    them were added (0xFF), so nothing behind base_len contributes."""
    rng = np.random.default_rng(330)
    for end in range(16):
        conns = [conn_of(rng, 77, 33 + end, [0, 0, 2], True, (4, 6)[end % 2], seed=end)]
        buf, off, ln, groups, conn, ooff, cap, rx_size = synth.tcp_rx_pack(conns, align=end)
        size = int(off[-1] + ln[-1])                       # the last frame ends the buffer
        buf = buf[:size]
        big = torch.full((size + 64,), 0xFF, dtype=torch.uint8, device=DEV)
        big[:size] = to_dev(buf)
        tb, toff, tln, ak, foff, fcap, fsize = synth.tcp_ack_inputs(conns)
        res, _ = run_arrays(buf, batch.make_desc(off, ln), groups, conn, rx_size, batch.make_desc(ooff, cap), tb,
                            batch.make_desc(toff, tln), ak, fsize, batch.make_desc(foff, fcap), base=big[:size])
        assert list(res[3]) == [OK, OL, HE] and res[1]["len"][0] > 0


# ---------------------------------------------------------------- the window

def test_window():
    """space giving shift 0, 1 and 3, a zero window and space < out_len (clamped to 0); the held bytes
    count with sack_ok only."""
    rng = np.random.default_rng(340)
    spaces = [16384, 0x1FFFF + 400, 0x7FFFF + 400, 300, 299, 400, 0, 500]
    conns = [conn_of(rng, 9000 + g, 100, [0, 1, 2, 4], g != 7, seed=g) for g in range(8)]
    res, _ = run(conns, space=spaces, ts_ok=0, out_off=2)
    want = [(16384 - 400, 0), (0xFFFF, 1), (0xFFFF, 3), (0, 0), (0, 0), (0, 0), (0, 0), (200, 0)]
    for g in range(8):
        f = frame_of(res, g)
        assert (int.from_bytes(bytes(f[34:36]), "big"), int(f[42])) == want[g], g
        assert bytes(f[40:42]) == b"\x03\x03"


# ---------------------------------------------------------------- 2^32 and seq 0

def test_wrap_and_seq_zero():
    """Streams across 2^32 and a held seq of exactly 0, with tcp_sack_prepare's quirks as the reference
    has them: the raw `seq < rcv_nxt` compare skips held segments past the wrap (a held seq of 0 always
    is: the held bytes still count against the window)."""
    rng = np.random.default_rng(350)
    per = 400
    conns = [
        conn_of(rng, M32 - 1499, per, [0, 2, 3], True, seed=1),       # block [2, 3]: right edge wraps
        conn_of(rng, M32 - 1499, per, [0, 5, 6], True, seed=2),       # both behind the wrap: below rcv' raw, no block
        conn_of(rng, M32 - 99, per, [0, 1, 3], True, seed=3),         # rcv' itself wrapped: ordinary
        conn_of(rng, M32 + 1 - 2 * per, per, [0, 2], True, seed=4),   # a held seq of exactly 0: below every rcv' raw
        conn_of(rng, M32 + 1 - 2 * per, per, [0, 2, 3], True, seed=5),   # ... and so is its successor
        conn_of(rng, M32 + 1 - 2 * per, per, [0, 2, 3], False, seed=6),
    ]
    res, _ = run(conns, ts_ok=0, align=4)
    got = [blocks_of(frame_of(res, g), 20) for g in range(6)]
    a = M32 - 1499
    assert got[0] == [((a + 2 * per) & M32, (a + 4 * per) & M32)] and got[0][0][1] < got[0][0][0]
    assert got[1] == []
    assert got[2] == [((M32 - 99 + 3 * per) & M32, (M32 - 99 + 4 * per) & M32)]
    assert got[3] == [] and got[4] == [] and got[5] == []
    assert [int(x) for x in res[4]] == [per, per, 2 * per, per, per, per]


# ---------------------------------------------------------------- no ACK due

def test_no_ack_due():
    """Groups with only TCP_CTRL segments, only segments with a bad checksum (IPv4 header: NET_BAD by the
    coalescing; a held payload: L4_BAD by this batch) or only malformed ones: no ACK, {0, 0, 0}, the
    region untouched, the connection ACCEPT."""
    rng = np.random.default_rng(360)
    data = synth.random_bytes(361, 64)
    ctrl = [synth.tcp_rx_frame(rng, 5, data[:0], 4, 20, 0x11), synth.tcp_rx_frame(rng, 5, data, 4, 20, 0x12)]
    net = synth.tcp_rx_frame(rng, 5, data)
    net[8] ^= 0x10
    short = synth.tcp_rx_frame(rng, 5, data)[:30]
    conns = [(ctrl, 5, True, 64), ([net], 5, True, 64), conn_of(rng, 5, 64, [1 + BAD, 2 + BAD], True, seed=1),
             ([short], 5, False, 64), conn_of(rng, 5, 64, [1 + BAD, 2], True, seed=2), conn_of(rng, 5, 64, [0 + BAD], False, seed=3)]
    res, _ = run(conns, out_off=1)
    av, aoa, ws, asv = res[:4]
    assert (av == OK).all()
    assert list(aoa["len"] > 0) == [False, False, False, False, True, False]
    assert list(asv) == [CT, CT, R.V_NET_BAD, LB, LB, MF, LB, HE, LB]


# ---------------------------------------------------------------- MALFORMED

def test_malformed_causes():
    """Every MALFORMED cause beside accepted neighbours: nothing of the region is written, {0, 0, 0}, and
    the group's segment verdicts stay as they came -- a corrupted held segment included."""
    rng = np.random.default_rng(370)
    conns = [conn_of(rng, 100 * g, 40, [0, 2 + BAD, 3], True, (4, 6)[g % 2], seed=g) for g in range(16)]
    buf, off, ln, groups, conn, ooff, cap, rx_size = synth.tcp_rx_pack(conns, align=2)
    tb, toff, tln, ak, foff, fcap, fsize = synth.tcp_ack_inputs(conns, ts_ok=1, out_off=4)
    sd, rod, td, fd = batch.make_desc(off, ln), batch.make_desc(ooff, cap), batch.make_desc(toff, tln), batch.make_desc(foff, fcap)
    groups, conn, ak, tb = groups.copy(), conn.copy(), ak.copy(), tb.copy()
    groups[1, 1] = 0                                   # 1: an empty group
    groups[2, 0] = sd.size - 1                         # 2: a group past n_seg
    conn[3, 1] = 3                                     # 3: reserved cflags
    ak["aflags"][4] = 2                                # 4: reserved aflags
    td["off"][5] = tb.size - 30                        # 5: a template past tmpl_len
    tb[int(td["off"][6])] = 0x55                       # 6: version 5
    tb[int(td["off"][7])] = 0x65                       # 7 (IPv6 group, IPv4-sized check): fine -- version 6 reads nxthdr
    tb[int(td["off"][7]) + 6] = 17                     #    ... nxthdr 17
    tb[int(td["off"][8])] = 0x46                       # 8: IHL 6
    tb[int(td["off"][10]) + 9] = 17                    # 10: proto 17
    td["len"][12] = 39                                 # 12: the template ends inside the TCP header
    fd["off"][13] = fsize - 50                         # 13: a region past out_len
    fd["len"][14] = 20 + 20 + 24 - 1                   # 14: a region one byte smaller than the frame (ts + one block)
    td["len"][9] = 59                                  # 9 (IPv6): the template ends inside the TCP header
    res, _ = run_arrays(buf, sd, groups, conn, rx_size, rod, tb, td, ak, fsize, fd)
    av, aoa, ws, asv = res[:4]
    bad = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 13, 14}
    assert [int(x) for x in av] == [MF if g in bad else OK for g in range(16)]
    assert all(int(aoa["len"][g]) == (0 if g in bad else (40 if g % 2 else 20) + 20 + 24) for g in range(16))
    for g in range(16):
        mine = slice(3 * g, 3 * g + 3)
        if g in (1, 2, 3):                             # (the coalescing refused these itself)
            continue
        assert list(asv[mine]) == ([OK, HE, HE] if g in bad else [OK, LB, HE]), g


def test_null_outputs_and_empty_batch():
    conns, _ = synth.tcp_rx_bursts(6, seed=380, family=[4, 6] * 3, per=200, max_bytes=2000)
    buf, off, ln, groups, conn, ooff, cap, rx_size = synth.tcp_rx_pack(conns, align=1)
    tb, toff, tln, ak, foff, fcap, fsize = synth.tcp_ack_inputs(conns)
    sd, rod, td, fd = batch.make_desc(off, ln), batch.make_desc(ooff, cap), batch.make_desc(toff, tln), batch.make_desc(foff, fcap)
    (av, aoa, ws, asv, wl, want), _ = run_arrays(buf, sd, groups, conn, rx_size, rod, tb, td, ak, fsize, fd)
    args = (to_dev(buf), dev_desc(sd), sd.size, pairs_dev(groups), pairs_dev(conn), to_dev(wl.view(np.int32)))
    tail = (to_dev(tb), dev_desc(td), to_dev(ak.view(np.uint8)))
    for res in ((None, None), (None, torch.zeros(96, dtype=torch.uint8, device=DEV)), (torch.zeros(6, dtype=torch.uint8, device=DEV), None)):
        out = torch.full((fsize,), CANARY, dtype=torch.uint8, device=DEV)
        sv = to_dev(ws)
        v, oa = batch.tcp_ack_batch(*args, sv, *tail, out, dev_desc(fd), results=res)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(out.cpu().numpy(), want)
        np.testing.assert_array_equal(sv.cpu().numpy(), asv)
        if v is not None:
            np.testing.assert_array_equal(v.cpu().numpy(), av)
        if oa is not None:
            np.testing.assert_array_equal(oa.cpu().numpy().view(R.DESC_DTYPE)["len"], aoa["len"])
    out = torch.full((64,), CANARY, dtype=torch.uint8, device=DEV)
    e32, e8 = torch.zeros(0, dtype=torch.int32, device=DEV), torch.zeros(0, dtype=torch.uint8, device=DEV)
    v, oa = batch.tcp_ack_batch(args[0], e8, 0, e32, e32, e32, e8, tail[0], e8, e8, out, e8)
    torch.cuda.synchronize()
    assert v.numel() == 0 and (out.cpu().numpy() == CANARY).all()


# ---------------------------------------------------------------- the two launch shapes

def test_large_batch_one_wave_per_connection():
    """Batches of 3072 connections or more with at most 16 segments a connection on average run one
    wave per connection (every other test here: four waves): 3100 generated bursts of small segments,
    both families, beside one connection of 150 held segments on the one wave -- and the same
    connections in a batch of 3000 (four waves) give the same frames and verdicts."""
    rng = np.random.default_rng(390)
    n = 3100
    conns, _ = synth.tcp_rx_bursts(n, seed=391, family=rng.choice([4, 6], n), thl=rng.choice([20, 32], n),
                                   per=rng.choice([24, 40, 57], n), max_bytes=200)
    conns[7] = conn_of(rng, 31, 9, [int(i) + 1 for i in rng.permutation(150)], True, seed=9)
    m = sum(len(c[0]) for c in conns)
    assert m <= 16 * n
    buf, off, ln, groups, conn, ooff, cap, rx_size = synth.tcp_rx_pack(conns, align=rng.integers(0, 16, m))
    tb, toff, tln, ak, foff, fcap, fsize = synth.tcp_ack_inputs(conns, out_off=3)
    sd, rod, td, fd = batch.make_desc(off, ln), batch.make_desc(ooff, cap), batch.make_desc(toff, tln), batch.make_desc(foff, fcap)
    one, _ = run_arrays(buf, sd, groups, conn, rx_size, rod, tb, td, ak, fsize, fd)
    assert (one[0] == OK).all() and {OK, LB, OL, HE} <= set(one[3].tolist())
    assert blocks_of(frame_of(one, 7), 20) == [(31 + 9, 31 + 9 * 151)]
    k = 3000
    m4 = sum(len(c[0]) for c in conns[:k])
    four, _ = run_arrays(buf, sd[:m4], groups[:k], conn[:k], rx_size, rod[:k], tb, td[:k], ak[:k], fsize, fd[:k])
    np.testing.assert_array_equal(four[3], one[3][:m4])
    np.testing.assert_array_equal(four[1]["len"], one[1]["len"][:k])
    end = int(fd["off"][k])
    np.testing.assert_array_equal(four[5][:end], one[5][:end])


# ---------------------------------------------------------------- the frames through the other batches

@pytest.mark.parametrize("family", [4, 6])
def test_frames_verify_in_the_rx_batches(family):
    """The emitted ACKs, d_out and d_out_ack as they are, through pico_ipv4_checksum_batch_dev /
    pico_ipv6_checksum_batch_dev in RX mode: every frame ACCEPT with both results 0; and through
    pico_tcp_coalesce_batch_dev: every frame TCP_CTRL."""
    conns, _ = synth.tcp_rx_bursts(40, seed=400 + family, family=family, per=300, max_bytes=3000)
    res, (out, goa) = run(conns, out_off=family, space=0x30000)
    due = np.flatnonzero(res[1]["len"] > 0)
    assert due.size >= 30
    d = to_dev(res[1][due].view(np.uint8))
    if family == 4:
        net, l4, v = batch.ipv4_checksum_batch(out, d, due.size)
        assert (net.cpu().numpy() == 0).all()
    else:
        l4, v = batch.ipv6_checksum_batch(out, d, due.size, flags=batch.F_NXTHDR_DISPATCH)
    torch.cuda.synchronize()
    assert (l4.cpu().numpy() == 0).all() and (v.cpu().numpy() == OK).all()
    grp = np.stack([np.arange(due.size), np.ones(due.size)], axis=1).astype(np.uint32)
    conn = np.zeros((due.size, 2), np.uint32)
    rx = torch.zeros(64, dtype=torch.uint8, device=DEV)
    cv, col, csv = batch.tcp_coalesce_batch(out, d, due.size, pairs_dev(grp), pairs_dev(conn), rx,
                                            to_dev(batch.make_desc(np.zeros(due.size), np.zeros(due.size)).view(np.uint8)))
    torch.cuda.synchronize()
    assert (csv.cpu().numpy() == CT).all() and (col.cpu().numpy() == 0).all()


# ---------------------------------------------------------------- one graph

def test_grouping_coalescing_and_acks_in_one_graph():
    """pico_flow_group_batch_dev + pico_tcp_coalesce_batch_dev + pico_tcp_ack_batch_dev captured into one
    graph and replayed on two different bursts: the reference fixture's frames interleaved, and the same
    connections in another arrival order with three segments corrupted.  Each replay gives the restatement's frames;
    the first one's are the reference stack's own."""
    a = RF.fixture()
    buf, sd, grp, conn, rod, rsize, tb, td, ak, fd, fsize = RF.batch_of(a)
    m, n = grp.shape[0], sd.size
    known = FG.make_known([(4, bytes(buf[int(sd["off"][f]) + 12:][:4]), bytes(buf[int(sd["off"][f]) + 16:][:4]),
                            int.from_bytes(bytes(buf[int(sd["off"][f]) + 20:][:2]), "big"), 80) for f in grp[:, 0]])
    bursts = []
    for seed, hit in ((41, ()), (42, (int(grp[0, 0]) + 1, int(grp[4, 0]) + 3, int(grp[13, 0]) + 3))):
        arr, _ = synth.interleave_groups(sd, grp, seed=seed)
        b = np.array(buf, copy=True)
        for f in hit:                                                   # a flipped bit in the frame's last payload byte
            b[int(sd["off"][f]) + int(sd["len"][f]) - 1] ^= 0x40
        # the expectation: the restatements on the burst connection by connection (the grouping keeps each one's order)
        _, wl, ws = R.coalesce(b, sd, grp, conn, np.zeros(rsize, np.uint8), rod)
        want = np.full(fsize, CANARY, np.uint8)
        av, aoa, _ = A.ack_batch(b, sd, grp, conn, wl, ws, tb, td, ak, want, fd)
        bursts.append((arr, av, aoa, want, b))
    assert (bursts[0][3] != bursts[1][3]).any()

    base, d_desc = to_dev(buf), torch.zeros(16 * n, dtype=torch.uint8, device=DEV)
    d_known = to_dev(known.view(np.uint8))
    scratch = torch.zeros(batch.flow_group_scratch_bytes(n, m), dtype=torch.uint8, device=DEV)
    fg = (torch.zeros(16 * n, dtype=torch.uint8, device=DEV), torch.zeros(n, dtype=torch.int32, device=DEV),
          torch.zeros(2 * (n + m), dtype=torch.int32, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV))
    d_conn, d_rod, rx = pairs_dev(conn), dev_desc(rod), torch.zeros(rsize, dtype=torch.uint8, device=DEV)
    rxres = (torch.zeros(m, dtype=torch.uint8, device=DEV), torch.zeros(m, dtype=torch.int32, device=DEV),
             torch.zeros(n, dtype=torch.uint8, device=DEV))
    d_tb, d_td, d_ak, d_fd = to_dev(tb), dev_desc(td), to_dev(ak.view(np.uint8)), dev_desc(fd)
    out = torch.full((fsize,), CANARY, dtype=torch.uint8, device=DEV)
    ares = (torch.zeros(m, dtype=torch.uint8, device=DEV), torch.zeros(16 * m, dtype=torch.uint8, device=DEV))

    def call(s):
        batch.flow_group_batch(base, d_desc, n, batch.FLOW_TCP, known=d_known, n_known=m, scratch=scratch, stream=s, results=fg)
        groups = fg[2][:2 * m]                              # the table's groups, in table order
        batch.tcp_coalesce_batch(base, fg[0], n, groups, d_conn, rx, d_rod, stream=s, results=rxres)
        batch.tcp_ack_batch(base, fg[0], n, groups, d_conn, rxres[1], rxres[2], d_tb, d_td, d_ak, out, d_fd, stream=s,
                            results=ares)

    d_desc.copy_(dev_desc(bursts[0][0]))
    call(None)                                              # warm (eager)
    torch.cuda.synchronize()
    assert fg[3].tolist() == [m, n] and (rxres[0] == OK).all() and (ares[0] == OK).all()
    turn = [0]

    def reset():
        d_desc.copy_(dev_desc(bursts[turn[0]][0]))
        base.copy_(to_dev(bursts[turn[0]][4]))
        out.fill_(CANARY)
        for t in ares + rxres + fg:
            t.zero_()
        torch.cuda.synchronize()                            # the replay starts from finished copies

    def check():
        _, av, aoa, want, _ = bursts[turn[0]]
        assert fg[3].tolist() == [m, n], f"replay {turn[0]}"
        assert (rxres[0] == OK).all()
        np.testing.assert_array_equal(ares[0].cpu().numpy(), av)
        np.testing.assert_array_equal(ares[1].cpu().numpy().view(R.DESC_DTYPE)["len"], aoa["len"])
        np.testing.assert_array_equal(out.cpu().numpy(), want)
        if turn[0] == 0:
            RF.check_against_reference(a, av, aoa, out.cpu().numpy(), "in the graph")
        turn[0] += 1

    replay_captured(call, reset, check, times=2)
