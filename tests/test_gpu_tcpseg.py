"""GPU: TCP send segmentation (pico_tcp_segment_batch_dev) against the numpy restatement of its contract
(tests/tcpseg_ref.py, pinned to the compiled reference stack's own data segments by
tests/test_ref_tcpseg.py) and against those segments themselves (tests/golden/ref_tcpseg_cases.npz).
Every comparison is over the WHOLE output buffer, pre-filled with a canary: a byte the contract does
not write -- outside a region, between two frames, anywhere in a MALFORMED stream's region -- must
keep it.  The launcher has two launch shapes: four waves per stream (every test but one) and one wave
per stream (test_large_batch_one_wave_per_stream)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from oracle import oracle as O
from picotcp_amd import batch, synth
from tests import tcpseg_ref as R
from tests import test_ref_tcpseg as RF
from tests.gpu_util import DEV, pairs_dev as grp_dev, replay_captured, to_dev

pytestmark = pytest.mark.gpu

CANARY = 0xA5


def gpu_segment(base, sd, groups, n_seg, out_size, od, stride):
    out = torch.full((out_size,), CANARY, dtype=torch.uint8, device=DEV)
    of = torch.zeros(16 * max(n_seg, 1), dtype=torch.uint8, device=DEV)
    v, c = batch.tcp_segment_batch(to_dev(base), to_dev(sd.view(np.uint8)), grp_dev(groups), n_seg, out,
                                   to_dev(od.view(np.uint8)), stride, out_seg=of)
    torch.cuda.synchronize()
    return v.cpu().numpy(), c.cpu().numpy().view(np.uint32), of.cpu().numpy().view(R.DESC_DTYPE)[:n_seg], out.cpu().numpy()


def check(base, sd, groups, n_seg, out_size, od, stride):
    """GPU == restatement on every output and on every byte of the output buffer."""
    want_out = np.full(out_size, CANARY, np.uint8)
    wv, wc, wof = R.segment(base, sd, groups, n_seg, want_out, od, stride)
    gv, gc, gof, got_out = gpu_segment(base, sd, groups, n_seg, out_size, od, stride)
    np.testing.assert_array_equal(gv, wv)
    np.testing.assert_array_equal(gc, wc)
    np.testing.assert_array_equal(gof, wof)
    bad = np.flatnonzero(got_out != want_out)
    assert bad.size == 0, f"{bad.size} bytes differ, first at {bad[:8].tolist()}"
    return wv, wc, wof, got_out


def synth_case(lengths, stride, seed, **kw):
    buf, off, slen, per, groups, ooff, cap, n_seg, out_size = synth.tcp_streams(lengths, stride=stride, seed=seed, **kw)
    return buf, batch.make_desc(off, slen, per), groups, n_seg, out_size, batch.make_desc(ooff, cap)


def test_reference_fixture():
    """All 73 data segments the compiled reference stack emitted for its twelve writes, byte for byte."""
    st = RF.streams(*RF.fixture()[:4])
    lens = np.array([s.size for s, _, _ in st], np.int64)
    offs = np.concatenate([[0], np.cumsum(lens[:-1])])
    base = np.concatenate([s for s, _, _ in st])
    cnt = np.array([len(segs) for _, _, segs in st], np.uint32)
    groups = np.stack([np.concatenate([[0], np.cumsum(cnt[:-1])]).astype(np.uint32), cnt], axis=1)
    cap = cnt.astype(np.int64) * 1504
    ooff = 12 + np.concatenate([[0], np.cumsum(cap[:-1])])
    od = batch.make_desc(ooff, cap)
    sd = batch.make_desc(offs, lens, [p for _, p, _ in st])
    wv, wc, wof, out = check(base, sd, groups, int(cnt.sum()), int(ooff[-1] + cap[-1] + 16), od, 1504)
    assert (wv == batch.V_ACCEPT).all() and int(cnt.sum()) == 73
    np.testing.assert_array_equal(wc, cnt)
    for g, (_, _, segs) in enumerate(st):
        for k, f in enumerate(segs):
            d = wof[groups[g, 0] + k]
            assert int(d["len"]) == f.size
            np.testing.assert_array_equal(out[int(d["off"]):int(d["off"]) + f.size], f, err_msg=f"write {g} segment {k}")


THLS = np.array([20, 24, 36, 60])


@pytest.mark.parametrize("stride", [1500, 1504, 1536])
@pytest.mark.parametrize("out_off", [12, 4, 1, 2, 3, 11])
def test_edge_lengths_and_alignments(out_off, stride):
    """Payloads of 0, 1, per - 1, per, per + 1, 2 per, 2 per + 1 and 45 per + 3 bytes, both families,
    every source alignment 0..15 with every TCP header length 20 / 24 / 36 / 60, for output regions at
    out_off mod 16 and the three strides (1500: the source / destination shift changes from segment
    to segment).  per = 1500 - H: full frames are 1500 bytes, as on the wire."""
    fam, thl, per, lengths, align = [], [], [], [], []
    for f in (4, 6):
        for li in range(8):
            for a in range(16):
                t = int(THLS[(a + li + f // 6) % 4])
                p = 1500 - (20 if f == 4 else 40) - t
                fam.append(f), thl.append(t), per.append(p), align.append(a)
                lengths.append([0, 1, p - 1, p, p + 1, 2 * p, 2 * p + 1, 45 * p + 3][li])
    buf, sd, groups, n_seg, out_size, od = synth_case(lengths, stride, 60, family=fam, thl=thl, per=per, align=align,
                                                      out_off=out_off)
    wv, wc, *_ = check(buf, sd, groups, n_seg, out_size, od, stride)
    assert (wv == batch.V_ACCEPT).all() and wc.max() == 46 and wc.min() == 1


def test_odd_and_tiny_segment_sizes():
    """per = 1, 5, 519, 1455 mixed in one batch, both families: an odd per puts every other segment's
    payload at an odd source offset while its sum pairs bytes from its own start (100 bytes at per 5
    are 20 segments; 37 at per 1 are 37 one-byte segments)."""
    per = np.array([1, 5, 519, 1455, 5, 1, 1455, 519, 7, 3] * 2)
    lengths = np.array([37, 100, 519 * 3 + 1, 1455 * 2 + 7, 101, 2, 1455 * 5, 518, 64, 0] * 2)
    fam = np.repeat([4, 6], 10)
    buf, sd, groups, n_seg, out_size, od = synth_case(lengths, 1536, 61, family=fam, thl=np.tile([20, 32], 10), per=per,
                                                      align=np.arange(20) * 7 % 16, out_off=9)
    wv, wc, *_ = check(buf, sd, groups, n_seg, out_size, od, 1536)
    assert (wv == batch.V_ACCEPT).all() and wc[0] == 37 and wc[1] == 20


def test_seq_and_id_wrap():
    """Template seq 0xFFFFF000 and id 0xFFFE over 5 segments: both wrap (mod 2^32, mod 2^16)."""
    buf, sd, groups, n_seg, out_size, od = synth_case([6000, 6000], 1536, 62, family=[4, 6], thl=32, per=1448,
                                                      seq=0xFFFFF000, ident=0xFFFE)
    wv, wc, wof, out = check(buf, sd, groups, n_seg, out_size, od, 1536)
    assert (wc == 5).all()
    o = wof["off"].astype(np.int64)
    ids = [int(out[o[k] + 4]) << 8 | int(out[o[k] + 5]) for k in range(5)]
    assert ids == [0xFFFE, 0xFFFF, 0, 1, 2]
    for g, N in ((0, 20), (1, 40)):
        seqs = [int.from_bytes(bytes(out[o[5 * g + k] + N + 4:o[5 * g + k] + N + 8]), "big") for k in range(5)]
        assert seqs == [(0xFFFFF000 + 1448 * k) & 0xFFFFFFFF for k in range(5)] and seqs[3] < seqs[2]


def test_one_mebibyte_stream():
    """1 MiB of payload at per 1448 (725 segments: source offsets past 2^16 and 2^20, 64-bit
    k * seg_stride) beside a 1-byte stream in the same batch."""
    buf, sd, groups, n_seg, out_size, od = synth_case([1 << 20, 1], 1504, 63, family=[4, 6], thl=[32, 20], per=1448,
                                                      align=[3, 0])
    wv, wc, *_ = check(buf, sd, groups, n_seg, out_size, od, 1504)
    np.testing.assert_array_equal(wc, [725, 1])


@pytest.mark.parametrize("family", [4, 6])
def test_round_trip_through_the_rx_batch(family):
    """d_out and d_out_seg as they are into the RX verify batch of the family (IPv6 with
    F_NXTHDR_DISPATCH: the default dispatch reads the source address's byte 9): every frame ACCEPT,
    header and transport checksums 0, and the oracle's RX results on the copied-back buffer agree."""
    rng = np.random.default_rng(64 + family)
    n = 160
    lengths = rng.integers(0, 12000, n)
    lengths[:4] = [0, 1, 1448, 14000]
    thl = rng.choice([20, 24, 32, 36, 60], n)
    per = rng.choice([536, 1220, 1400, 1401], n)
    buf, sd, groups, n_seg, out_size, od = synth_case(lengths, 1504, 65, family=family, thl=thl, per=per,
                                                      align=rng.integers(0, 16, n), out_off=12)
    out = torch.full((out_size,), CANARY, dtype=torch.uint8, device=DEV)
    of = torch.zeros(16 * n_seg, dtype=torch.uint8, device=DEV)
    v, c = batch.tcp_segment_batch(to_dev(buf), to_dev(sd.view(np.uint8)), grp_dev(groups), n_seg, out,
                                   to_dev(od.view(np.uint8)), 1504, out_seg=of)
    if family == 4:
        net, l4, rv = batch.ipv4_checksum_batch(out, of, n_seg)
    else:
        l4, rv = batch.ipv6_checksum_batch(out, of, n_seg, flags=batch.F_NXTHDR_DISPATCH)
    torch.cuda.synchronize()
    assert (v.cpu().numpy() == batch.V_ACCEPT).all() and int(c.cpu().numpy().sum()) == n_seg
    assert (rv.cpu().numpy() == batch.V_ACCEPT).all() and (l4.cpu().numpy() == 0).all()
    h_out, h_of = out.cpu().numpy(), of.cpu().numpy().view(R.DESC_DTYPE)
    if family == 4:
        assert (net.cpu().numpy() == 0).all()
        wn, wl, wv = O.batch_ipv4(h_out, h_of, tx=False)
        assert (wn == 0).all()
    else:
        wl, wv = O.batch_ipv6(h_out, h_of, nxthdr_dispatch=True)
    assert (wv == batch.V_ACCEPT).all() and (wl == 0).all()


def test_malformed():
    """Every MALFORMED cause beside accepted neighbours: the verdicts, counts and slots of the
    restatement, and not one byte changed in a MALFORMED stream's region or outside the regions --
    slots past n_seg included (no slot of that group is written)."""
    n = 26
    fam = np.full(n, 4)
    fam[[5, 8, 10, 15, 22, 24]] = 6
    lengths, per = np.full(n, 4000), np.full(n, 1448)
    lengths[[14, 15, 23, 24]] = 70000
    per[[14, 23]], per[[15, 24]] = 65495, 65515        # IPv4 len / IPv6 payload length = 65535: the largest that fit
    stride = 65600
    buf, sd, groups, n_seg, out_size, od = synth_case(lengths, stride, 66, family=fam, thl=20, per=per,
                                                      align=np.arange(n) % 16, spare=1)
    sd, groups, od = sd.copy(), groups.copy(), od.copy()
    off = sd["off"].astype(np.int64)
    buf = buf[:int(off[25]) + int(sd["len"][25]) - 1]  # 25 (the last): runs 1 byte past base_len
    sd["off"][1] = buf.size + 5                        # 1: starts past base_len
    sd["len"][2] = 0                                   # 2: len < 1
    buf[off[3]] = 0x55                                 # 3: version 5
    sd["len"][4] = 19                                  # 4: IPv4, len < 20
    sd["len"][5] = 39                                  # 5: IPv6, len < 40
    buf[off[6]] = 0x46                                 # 6: IHL 6
    buf[off[7] + 9] = 17                               # 7: IPv4 proto 17
    buf[off[8] + 6] = 17                               # 8: IPv6 nxthdr 17
    sd["len"][9] = 39                                  # 9: IPv4, len < N + 20
    sd["len"][10] = 59                                 # 10: IPv6, len < N + 20
    buf[off[11] + 32] = 0x40                           # 11: thl 16
    buf[off[12] + 32] = 0xF0                           # 12: thl 60 in 20 + 59 bytes
    sd["len"][12] = 79
    sd["seed"][13] = 0                                 # 13: per 0
    sd["seed"][14] = 65496                             # 14: IPv4 len 65536
    sd["seed"][15] = 65516                             # 15: IPv6 payload length 65536
    groups[17, 1] = 2                                  # 17: fewer reserved slots than its 3 segments
    groups[18, 0] = n_seg - 2                          # 18: slots past n_seg
    od["len"][19] -= 1                                 # 19: region 1 byte too small
    od["off"][20] = out_size - 100                     # 20: region past out_len
    od["off"][21] = out_size + 1                       # 21: region starts past out_len
    wv, wc, wof, out = check(buf, sd, groups, n_seg, out_size, od, stride)
    ok = [0, 16, 22, 23, 24]                           # (seg_stride's own bound: the test below)
    want = np.full(n, 8)
    want[ok] = 1
    np.testing.assert_array_equal(wv, want)
    np.testing.assert_array_equal(wc[ok], [3, 3, 3, 2, 2])
    assert (np.delete(wc, ok) == 0).all()
    touched = np.zeros(out_size, bool)
    for d in wof[wof["len"] > 0]:
        touched[int(d["off"]):int(d["off"]) + int(d["len"])] = True
    assert int((wof["len"] > 0).sum()) == 13 and (out[~touched] == CANARY).all()
    assert int(out[int(od["off"][23]) + 2]) << 8 | int(out[int(od["off"][23]) + 3]) == 65535


def test_stride_bounds_the_longest_frame_only():
    """H + min(per, P) against seg_stride: per = 1461 at stride 1500 is MALFORMED for a payload of 1461
    bytes or more (a 1501-byte frame), but not for the 1460 bytes that fit one frame."""
    buf, sd, groups, n_seg, out_size, od = synth_case([1460, 1460, 1460], 1500, 67, family=4, thl=20, per=1460)
    sd = sd.copy()
    sd["seed"][0] = 1461                               # one frame of 1500 bytes: min(per, P) = 1460
    sd["seed"][1] = 1461                               # 1: one byte more payload -> a frame of 1501
    sd["len"][1] += 1
    wv, wc, *_ = check(buf, sd, groups, n_seg, out_size, od, 1500)
    np.testing.assert_array_equal(wv, [1, 8, 1])


def test_null_outputs_and_empty_batch():
    lengths = np.array([4000, 100, 9000, 0])
    buf, sd, groups, n_seg, out_size, od = synth_case(lengths, 1504, 68, family=[4, 6, 4, 6], thl=[20, 36, 60, 24], per=1400)
    wv, wc, wof, want_out = check(buf, sd, groups, n_seg, out_size, od, 1504)
    args = (to_dev(buf), to_dev(sd.view(np.uint8)), grp_dev(groups), n_seg)
    d_od = to_dev(od.view(np.uint8))
    for skip in (0, 1, 2, 3):                          # 3: all three optional outputs NULL
        out = torch.full((out_size,), CANARY, dtype=torch.uint8, device=DEV)
        of = None if skip >= 2 else torch.zeros(16 * n_seg, dtype=torch.uint8, device=DEV)
        res = [torch.full((4,), 77, dtype=dt, device=DEV) for dt in (torch.uint8, torch.int32)]
        if skip < 2:
            res[skip] = None
        if skip == 3:
            res = [None, None]
        v, c = batch.tcp_segment_batch(*args, out, d_od, 1504, out_seg=of, results=tuple(res))
        torch.cuda.synchronize()
        np.testing.assert_array_equal(out.cpu().numpy(), want_out)
        for t, w in ((v, wv), (c, wc.view(np.int32))):
            if t is not None:
                np.testing.assert_array_equal(t.cpu().numpy(), w)
        if of is not None:
            np.testing.assert_array_equal(of.cpu().numpy().view(R.DESC_DTYPE), wof)
    # n_stream == 0: nothing runs, nothing is written
    out = torch.full((64,), CANARY, dtype=torch.uint8, device=DEV)
    empty = torch.zeros(0, dtype=torch.int32, device=DEV)
    v, c = batch.tcp_segment_batch(args[0], torch.zeros(0, dtype=torch.uint8, device=DEV), empty, 0, out,
                                   torch.zeros(0, dtype=torch.uint8, device=DEV), 1504)
    torch.cuda.synchronize()
    assert v.numel() == 0 and (out.cpu().numpy() == CANARY).all()


def test_graph_replay():
    """One call captured into a graph and replayed twice: the eager result each time."""
    lengths = np.array([4000, 65000, 100, 9000, 1449])
    buf, sd, groups, n_seg, out_size, od = synth_case(lengths, 1536, 69, family=[4, 6, 4, 6, 4], thl=32, per=1448)
    wv, wc, wof, want_out = check(buf, sd, groups, n_seg, out_size, od, 1536)
    args = (to_dev(buf), to_dev(sd.view(np.uint8)), grp_dev(groups), n_seg)
    d_od = to_dev(od.view(np.uint8))
    out = torch.full((out_size,), CANARY, dtype=torch.uint8, device=DEV)
    of = torch.zeros(16 * n_seg, dtype=torch.uint8, device=DEV)
    res = batch.tcp_segment_batch(*args, out, d_od, 1536, out_seg=of)      # warm (eager)
    torch.cuda.synchronize()

    def call(s):
        batch.tcp_segment_batch(*args, out, d_od, 1536, out_seg=of, stream=s, results=res)

    def reset():
        out.fill_(CANARY)
        of.zero_()
        for r in res:
            r.zero_()

    def same():
        np.testing.assert_array_equal(out.cpu().numpy(), want_out)
        np.testing.assert_array_equal(of.cpu().numpy().view(R.DESC_DTYPE), wof)
        np.testing.assert_array_equal(res[0].cpu().numpy(), wv)
        np.testing.assert_array_equal(res[1].cpu().numpy().view(np.uint32), wc)

    replay_captured(call, reset, same)


def test_large_batch_one_wave_per_stream():
    """Batches of 3072 streams or more that reserve at most 16 slots a stream on average run one wave
    per stream (every other test here: four waves): 3200 mixed streams of 1 .. 4 segments, both
    families, every header length and source alignment, beside 4 one-byte-per-segment streams of 30
    segments (15 pairs on the one wave)."""
    rng = np.random.default_rng(70)
    n = 3200
    lengths = rng.integers(0, 5601, n)
    lengths[:8] = [0, 1, 1399, 1400, 1401, 2800, 2801, 5600]
    per = np.full(n, 1400)
    lengths[8:12], per[8:12] = 30, 1
    buf, sd, groups, n_seg, out_size, od = synth_case(lengths, 1504, 71, family=rng.choice([4, 6], n),
                                                      thl=rng.choice(THLS, n), per=per, align=rng.integers(0, 16, n), out_off=5)
    assert n_seg <= 16 * n
    wv, wc, *_ = check(buf, sd, groups, n_seg, out_size, od, 1504)
    assert (wv == batch.V_ACCEPT).all() and wc.max() == 30 and wc.min() == 1


def test_large_batch_of_long_streams_keeps_four_waves():
    """3072 streams or more that reserve MORE than 16 slots a stream on average stay on the
    four-wave shape: 3072 streams of 17 segments (per 64)."""
    n = 3072
    buf, sd, groups, n_seg, out_size, od = synth_case(np.full(n, 17 * 64 - 3), 200, 72, family=np.arange(n) % 2 * 2 + 4,
                                                      thl=24, per=64, align=np.arange(n) % 16, out_off=0)
    assert n_seg == 17 * n
    wv, wc, *_ = check(buf, sd, groups, n_seg, out_size, od, 200)
    assert (wv == batch.V_ACCEPT).all() and (wc == 17).all()
