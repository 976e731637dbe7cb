"""The TCP segmentation contract pinned to the data segments the compiled reference stack itself emits.

tests/golden/ref_tcpseg_cases.npz (tests/golden/make_ref_tcpseg.py): every data segment the
unmodified reference stack handed to pico_datalink_send for twelve pico_socket_write calls on twelve
connections (six SYN option sets: TCP headers of 24 and 36 bytes, segment payloads of 1456, 1444 and
520 bytes).  Here (no GPU): tests/tcpseg_ref.py, the restatement the GPU tests check the kernel
against, reproduces those segments byte for byte from a send unit's first header, its concatenated
payload and its first segment's payload length.

A send unit is a run of a write's segments that carry the same option bytes.  The reference stamps
the timestamp option of every segment with the wall-clock millisecond at the moment it sends it
(tcp_add_options_frame: tsval = TCP_TIME), the batch copies the template's options to every segment:
a write whose segments all left within one millisecond, or whose connection has no timestamp option,
is one unit; a millisecond boundary inside a write starts another.  `units` cuts there, so these
tests hold whatever the clock did during a capture."""
from __future__ import annotations

import os

import numpy as np
import pytest

from oracle import oracle as O
from picotcp_amd import batch, synth
from tests import tcpseg_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LENGTHS = [1, 1455, 1456, 1457, 2913, 5001, 14000, 13104, 7, 4368, 9999, 12345]
UNREAD = [2, 3, 6, 7, 10, 11, 36, 37]       # IPv4 len, frag, crc; TCP crc (the header is 20 bytes)
PER_SEGMENT = [2, 3, 4, 5, 10, 11, 24, 25, 26, 27, 36, 37]     # IPv4 len, id, crc; TCP seq, crc
TSVAL = range(45, 49)                       # a 36-byte TCP header: window scale (3), kind, length, tsval, tsecr


def fixture():
    c = np.load(os.path.join(GOLDEN, "ref_tcpseg_cases.npz"))
    return c["buf"], c["off"].astype(np.int64), c["len"].astype(np.int64), c["group"], c["written"]


def writes(buf, off, ln, group):
    """Per captured write: its data segments in order."""
    return [[buf[off[i]:off[i] + ln[i]] for i in np.nonzero(group == g)[0]] for g in range(int(group.max()) + 1)]


def units(segs):
    """A write's segments cut at every change of the option bytes."""
    H = 20 + 4 * (int(segs[0][32]) >> 4)
    out = [[segs[0]]]
    for f in segs[1:]:
        if bytes(f[40:H]) == bytes(out[-1][0][40:H]):
            out[-1].append(f)
        else:
            out.append([f])
    return out


def streams(buf, off, ln, group, seed=5):
    """Per send unit of every captured write: (stream = the unit's first H bytes with the fields the
    batch does not read scrambled + the concatenated segment payloads, per = the first segment's
    payload when the unit has more than one segment, else something >= P, the captured segments in
    order).  Only a write's last segment is short, so a unit's first segment is a full one whenever
    another follows it."""
    rng = np.random.default_rng(seed)
    out = []
    for w in writes(buf, off, ln, group):
        for segs in units(w):
            H = 20 + 4 * (int(segs[0][32]) >> 4)
            h = segs[0][:H].copy()
            h[UNREAD] = rng.integers(0, 256, len(UNREAD))
            P = sum(s.size - H for s in segs)
            per = segs[0].size - H if len(segs) > 1 else P + int(rng.integers(0, 3000))
            out.append((np.concatenate([h] + [s[H:] for s in segs]), per, segs))
    return out


def run_ref(strms, pers, stride, out_off=12):
    """The restatement over a list of streams packed back to back; returns (out, out_seg, groups,
    out_desc, verdict, count)."""
    lens = np.array([s.size for s in strms], np.int64)
    offs = np.concatenate([[0], np.cumsum(lens[:-1])])
    base = np.concatenate(strms)
    cnt = np.array([synth.tcpseg_count(int(x) - 20 - 4 * (int(s[32]) >> 4), int(p)) for x, s, p in zip(lens, strms, pers)],
                   np.uint32)
    first = np.concatenate([[0], np.cumsum(cnt[:-1])]).astype(np.uint32)
    groups = np.stack([first, cnt], axis=1)
    cap = cnt.astype(np.int64) * stride
    ooff = out_off + np.concatenate([[0], np.cumsum(cap[:-1] + 16)])
    out = np.full(int(ooff[-1] + cap[-1] + 16), 0xA5, np.uint8)
    od = batch.make_desc(ooff, cap)
    v, c, of = R.segment(base, batch.make_desc(offs, lens, pers), groups, int(cnt.sum()), out, od, stride)
    return out, of, groups, od, v, c


def check_against(st, stride=1504, note=""):
    out, of, groups, od, v, c = run_ref([s for s, _, _ in st], [p for _, p, _ in st], stride)
    assert (v == R.V_ACCEPT).all(), note
    for g, (_, _, segs) in enumerate(st):
        assert c[g] == len(segs), f"unit {g} {note}"
        for k, f in enumerate(segs):
            d = of[groups[g, 0] + k]
            assert (int(d["len"]), int(d["seed"])) == (f.size, 0), f"unit {g} segment {k} {note}"
            np.testing.assert_array_equal(out[int(d["off"]):int(d["off"]) + f.size], f, err_msg=f"unit {g} segment {k} {note}")
    return out


def check_capture(buf, off, ln, group, note=""):
    """What every capture of the reference shows, whatever its clock did: per write, DF and PSH|ACK
    and a good header checksum on every segment, consecutive ids, and segments that differ from the
    write's first only in IPv4 len / id / crc, TCP seq / crc, the payload and -- on a connection
    with the timestamp option -- tsval, which never runs backwards."""
    for g, segs in enumerate(writes(buf, off, ln, group)):
        t = 4 * (int(segs[0][32]) >> 4)
        same = np.setdiff1d(np.arange(20 + t), PER_SEGMENT + (list(TSVAL) if t == 36 else []))
        ts = [int.from_bytes(bytes(f[45:49]), "big") for f in segs]
        for k, f in enumerate(segs):
            where = f"write {g} segment {k} {note}"
            assert bytes(f[6:8]) == b"\x40\x00" and f[33] == 0x18, where
            assert O.checksum(f[:20]) == 0, where
            assert bytes(f[same]) == bytes(segs[0][same]), where
            assert (int(f[4]) << 8 | int(f[5])) == ((int(segs[0][4]) << 8 | int(segs[0][5])) + k) & 0xFFFF, where
            assert t != 36 or k == 0 or (ts[k] - ts[k - 1]) & 0xFFFFFFFF < 1 << 31, where


def test_fixture_shape():
    buf, off, ln, group, written = fixture()
    np.testing.assert_array_equal(written, LENGTHS)
    assert ln.size == 73 and buf.size == 69798
    check_capture(buf, off, ln, group)
    ws = writes(buf, off, ln, group)
    thl = [4 * (int(segs[0][32]) >> 4) for segs in ws]
    assert set(thl) == {24, 36}
    assert {segs[0].size - 20 - t for segs, t in zip(ws, thl) if len(segs) > 1} == {1456, 1444, 520}
    st = streams(buf, off, ln, group)
    assert sum(len(segs) for _, _, segs in st) == 73 and len(st) >= len(ws)


def test_restatement_reproduces_reference_segments():
    check_against(streams(*fixture()[:4]))


def test_unread_template_fields_change_nothing():
    """Another scramble of the template's IPv4 len / frag / crc and TCP crc: the same output."""
    fx = fixture()[:4]
    a = check_against(streams(*fx, seed=5), stride=1536)
    b = check_against(streams(*fx, seed=6), stride=1536)
    np.testing.assert_array_equal(a, b)


def test_a_millisecond_boundary_inside_a_write_starts_a_unit():
    """The fixture with the clock set by hand: on every timestamp write of four segments or more
    tsval is segment 0's on segments 0 and 1, 1 ms later on segment 2 and 3 ms later from segment 3
    on (TCP checksums redone with the oracle), as the reference does when milliseconds pass between
    the segments of a write.  Such a write is three units, and the restatement still rebuilds every
    segment."""
    buf, off, ln, group, _ = fixture()
    buf = buf.copy()
    ws = writes(buf, off, ln, group)                  # views into the copy
    moved = 0
    for segs in ws:
        if 4 * (int(segs[0][32]) >> 4) != 36 or len(segs) < 4:
            continue
        moved += 1
        ts0 = int.from_bytes(bytes(segs[0][45:49]), "big")
        for k, f in enumerate(segs):
            ts = (ts0 + (0, 0, 1)[k] if k < 3 else ts0 + 3) & 0xFFFFFFFF
            f[45:49] = np.frombuffer(ts.to_bytes(4, "big"), np.uint8)
            f[36] = f[37] = 0
            tl = f.size - 20
            c = O.dualbuffer_checksum(np.concatenate([f[12:20], np.array([0, 6, tl >> 8, tl & 0xFF], np.uint8)]), f[20:])
            f[36], f[37] = c >> 8, c & 0xFF
        assert [len(u) for u in units(segs)] == [2, 1, len(segs) - 3]
    assert moved >= 2
    check_capture(buf, off, ln, group)
    st = streams(buf, off, ln, group)
    assert len(st) == sum(len(units(w)) for w in ws) >= len(ws) + 2 * moved
    assert sum(len(segs) for _, _, segs in st) == 73
    check_against(st)


REF_RX = os.path.join(os.path.dirname(GOLDEN), "..", "oracle", "_ref", "libref_rx.so")


@pytest.mark.skipif(not os.path.exists(REF_RX), reason="oracle/_ref/libref_rx.so not built here")
def test_restatement_on_live_reference_capture():
    """A fresh capture of the live reference stack (its initial sequence numbers and ids come from
    pico_rand, its timestamps from the wall clock, so they differ run to run, and a millisecond may
    pass inside a write): the restatement rebuilds every segment it emits, unit by unit."""
    from tests.golden import make_ref_tcpseg as M
    seed = int.from_bytes(os.urandom(4), "little")
    rng = np.random.default_rng(seed)
    lengths = [1, 1456, 14000] + [int(x) for x in rng.integers(1, 14001, 9)]
    note = f"(seed {seed}, lengths {lengths})"
    print(note)
    buf, off, ln, group, written = M.pack(M.capture(lengths, seed=int(rng.integers(1 << 30))))
    np.testing.assert_array_equal(written, lengths, err_msg=note)
    off, ln = off.astype(np.int64), ln.astype(np.int64)
    check_capture(buf, off, ln, group, note)
    check_against(streams(buf, off, ln, group), note=note)
