"""GPU: the header word rules of the three batches that write finished frames -- a lane per 32-bit header
word, its halves summed, the word stored whole or byte by byte, the TCP/IP template's check and word sums,
wherever the kernels keep them -- pinned through their entry points:
pico_tcp_segment_batch_dev, pico_tcp_ack_batch_dev behind pico_tcp_coalesce_batch_dev, and
pico_icmp4_reply_batch_dev, each against its numpy restatement (tests/tcpseg_ref.py, tests/tcpack_ref.py
behind tests/tcprx_ref.py, tests/icmp4_ref.py), over the WHOLE output buffer, pre-filled with a canary,
with the verdicts and the output descriptors.  Every case is valid: ACCEPT is asserted for all of them,
in the restatement and on the device, before anything is compared, so none drops out of the comparison.

The cells, the smallest shapes at which a header word rule can go wrong:
  * send segments: family 4 / 6 x TCP header 20 / 32 / 60 bytes (H = 40 .. 100: up to all 25 word lanes)
    x the frame's address mod 16 = 0..15 (the region's offset; stride 1504 keeps every segment on that
    place, 1500 moves it by 12 a segment) x 1, 2 or 3 segments of per = 8 bytes before the tail (a lone A
    member, a pair, a pair and a lone one) x a tail of 1..11 bytes (9..11: the tail is itself a whole
    segment and 1..3 bytes, so a stream has up to 4 segments).  3168 streams launch the one-wave shape;
    every third (1056) in a launch of its own takes the four-wave shape;
  * ACKs: family 4 / 6 x timestamps off / on x no SACK block / one x the frame's address mod 16 = 0..15:
    TCP headers of 24, 36 and 44 bytes, every length this kernel writes with at most one block.  A
    connection has 2 or 3 segments.  The 128 connections run as they are (four waves) and tiled 24
    times, 3072 connections, on the one-wave shape;
  * ICMPv4 answers: notices 3 / 11 / 12 x the answer's address mod 16 x a quoted datagram of total length
    20..29 (the quote's last word whole, 1, 2 or 3 bytes long, or cut at 28), echoes x the address x a
    transport of 8, 9 and 12 bytes; the batch on both sides of its launch-shape threshold (the buffer one
    byte short of 1024 bytes a record, and exactly that long)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from picotcp_amd import batch, synth
from tests import icmp4_ref, tcpack_ref, tcprx_ref, tcpseg_ref
from tests.gpu_util import DEV, pairs_dev, to_dev

pytestmark = pytest.mark.gpu

CANARY = 0xA5
OK = batch.V_ACCEPT
PER = 8
SEG_CELLS = [(fam, thl, a, m, tail) for fam in (4, 6) for thl in (20, 32, 60) for a in range(16) for m in (1, 2, 3)
             for tail in range(1, 12)]
SEG_SHAPES = {"one_wave": SEG_CELLS, "four_waves": SEG_CELLS[::3]}       # 3168 streams: >= 3072; 1056: below
ACK_CELLS = [(fam, ts, blk, a) for fam in (4, 6) for ts in (0, 1) for blk in (0, 1) for a in range(16)]
ACK_TILES = {"four_waves": 1, "one_wave": 24}                           # 128 connections; 3072
ICMP_CELLS = [(typ, a, tot) for typ in (3, 11, 12) for a in range(16) for tot in range(20, 30)] + \
             [(0, a, T) for a in range(16) for T in (8, 9, 12)]


def dev_desc(d):
    return to_dev(d.view(np.uint8))


def same_desc(got, want):
    for k in ("off", "len", "seed"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


def same_bytes(got: np.ndarray, want: np.ndarray):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} bytes differ, first at {bad[:8].tolist()}"


# ---------------------------------------------------------------- pico_tcp_segment_batch_dev

def segment_case(cells, stride):
    """(base, stream desc, groups, n_seg, out size, out desc, segments a stream) for tcp_segment_batch; the
    input buffer ends with the last stream's last payload byte."""
    buf, off, slen, per, groups, ooff, cap, n_seg, out_size = synth.tcp_streams(
        [PER * (m - 1) + tail for fam, thl, a, m, tail in cells], family=[c[0] for c in cells], thl=[c[1] for c in cells],
        per=PER, stride=stride, seed=74, align=[(5 * a + m + tail) % 16 for fam, thl, a, m, tail in cells],
        out_off=[c[2] for c in cells])
    assert all(int(o) % 16 == c[2] for o, c in zip(ooff, cells))
    return (buf[:int(off[-1]) + int(slen[-1])], batch.make_desc(off, slen, per), groups, n_seg, out_size,
            batch.make_desc(ooff, cap), [m + (tail > PER) for fam, thl, a, m, tail in cells])


@pytest.mark.parametrize("stride", [1504, 1500])
@pytest.mark.parametrize("shape", SEG_SHAPES)
def test_segment(shape, stride):
    base, sd, groups, n_seg, out_size, od, count = segment_case(SEG_SHAPES[shape], stride)
    want_out = np.full(out_size, CANARY, np.uint8)
    wv, wc, wof = tcpseg_ref.segment(base, sd, groups, n_seg, want_out, od, stride)
    out = torch.full((out_size,), CANARY, dtype=torch.uint8, device=DEV)
    of = torch.zeros(16 * n_seg, dtype=torch.uint8, device=DEV)
    v, c = batch.tcp_segment_batch(to_dev(base), dev_desc(sd), pairs_dev(groups), n_seg, out, dev_desc(od), stride, out_seg=of)
    torch.cuda.synchronize()
    assert (wv == OK).all() and (v.cpu().numpy() == OK).all()
    np.testing.assert_array_equal(wc, count)
    np.testing.assert_array_equal(c.cpu().numpy().view(np.uint32), wc)
    same_desc(of.cpu().numpy().view(tcpseg_ref.DESC_DTYPE), wof)
    same_bytes(out.cpu().numpy(), want_out)


# ---------------------------------------------------------------- pico_tcp_ack_batch_dev

def ack_case(tiles):
    """The arrays of tcp_coalesce_batch and tcp_ack_batch for ACK_CELLS tiled `tiles` times, and each
    connection's expected frame length.  A connection: segment 0 and, without a block, segment 1 delivered
    in order; with one, segments 2 and 3 held behind the hole at 1 (sack_ok: one block over both).  rcv_nxt
    stays below 2^31, so tcp_sack_prepare's raw compare never skips a held segment."""
    rng = np.random.default_rng(75)
    conns, ts, out_off, flen = [], [], [], []
    for t in range(tiles):
        for k, (fam, tsok, blk, a) in enumerate(ACK_CELLS):
            per, rcv = 9 + (k + t) % 23, int(rng.integers(1, 1 << 31))
            data = synth.random_bytes(7 * k + t, 4 * per)
            frames = [synth.tcp_rx_frame(rng, rcv + i * per, data[i * per:(i + 1) * per], fam, (20, 32)[k % 2], 0x10)
                      for i in ((0, 2, 3) if blk else (0, 1))]
            conns.append((frames, rcv, True, 4 * per))
            ts.append(tsok)
            out_off.append((a + t) % 16)
            flen.append((40 if fam == 6 else 20) + 20 + ((3 + 10 * tsok + 1 + 10 * blk + 3) & ~3))
    m = sum(len(c[0]) for c in conns)
    buf, off, ln, groups, conn, ooff, cap, rx_size = synth.tcp_rx_pack(conns, align=np.arange(m) * 7 % 16, seed=75)
    tb, toff, tln, ak, foff, fcap, fsize = synth.tcp_ack_inputs(conns, seed=76, ts_ok=ts, out_off=out_off,
                                                                align=np.arange(len(conns)) * 3 % 16)
    assert all(int(o) % 16 == x for o, x in zip(foff, out_off))
    return (buf, batch.make_desc(off, ln), groups, conn, rx_size, batch.make_desc(ooff, cap), tb, batch.make_desc(toff, tln), ak,
            fsize, batch.make_desc(foff, fcap), np.array(flen, np.uint32))


@pytest.mark.parametrize("shape", ACK_TILES)
def test_ack(shape):
    buf, sd, groups, conn, rx_size, rod, tb, td, ak, fsize, fd, flen = ack_case(ACK_TILES[shape])
    n = groups.shape[0]
    assert (n >= 3072) == (shape == "one_wave") and sd.size <= 4 * n
    want_rx, want = np.full(rx_size, CANARY, np.uint8), np.full(fsize, CANARY, np.uint8)
    wv, wl, ws = tcprx_ref.coalesce(buf, sd, groups, conn, want_rx, rod)
    av, aoa, asv = tcpack_ref.ack_batch(buf, sd, groups, conn, wl, ws, tb, td, ak, want, fd)
    base, d_sd, d_grp, d_conn = to_dev(buf), dev_desc(sd), pairs_dev(groups), pairs_dev(conn)
    rx = torch.full((rx_size,), CANARY, dtype=torch.uint8, device=DEV)
    out = torch.full((fsize,), CANARY, dtype=torch.uint8, device=DEV)
    v, ol, sv = batch.tcp_coalesce_batch(base, d_sd, sd.size, d_grp, d_conn, rx, dev_desc(rod))
    torch.cuda.synchronize()
    sv0 = sv.cpu().numpy().copy()
    gv, goa = batch.tcp_ack_batch(base, d_sd, sd.size, d_grp, d_conn, ol, sv, to_dev(tb), dev_desc(td), to_dev(ak.view(np.uint8)),
                                  out, dev_desc(fd))
    torch.cuda.synchronize()
    assert (wv == OK).all() and (av == OK).all() and (v.cpu().numpy() == OK).all() and (gv.cpu().numpy() == OK).all()
    np.testing.assert_array_equal(aoa["len"], flen)
    np.testing.assert_array_equal(ol.cpu().numpy().view(np.uint32), wl)
    np.testing.assert_array_equal(sv0, ws)
    np.testing.assert_array_equal(sv.cpu().numpy(), asv)
    same_desc(goa.cpu().numpy().view(tcpack_ref.DESC_DTYPE), aoa)
    same_bytes(rx.cpu().numpy(), want_rx)
    same_bytes(out.cpu().numpy(), want)


# ---------------------------------------------------------------- pico_icmp4_reply_batch_dev

def icmp_case():
    """(buffer, desc, req, out desc, out size) for icmp4_reply_batch over ICMP_CELLS: tight regions, every
    echo request with its own (id, seq), a notice's datagram cut at its total length."""
    rng = np.random.default_rng(77)
    dgrams = []
    for k, (typ, a, x) in enumerate(ICMP_CELLS):
        if typ == 0:
            dgrams.append(synth.icmp4_echo_request(rng, x, ident=k, seq=k))
        else:
            d = synth.icmp4_echo_request(rng, max(x - 20, 8))[:x].copy()
            d[2], d[3] = x >> 8, x & 0xFF
            dgrams.append(d)
    n = len(ICMP_CELLS)
    buf, off, ln, req, ooff, cap, osize = synth.icmp4_burst(dgrams, [c[0] for c in ICMP_CELLS], codes=np.arange(n) * 5 % 256, seed=77,
                                                            align=np.arange(n) * 7 % 16, out_off=[c[1] for c in ICMP_CELLS])
    assert all(int(o) % 16 == c[1] for o, c in zip(ooff, ICMP_CELLS)) and buf.size < 1024 * n - 1
    return buf, batch.make_desc(off, ln), req, batch.make_desc(ooff, cap), osize


@pytest.mark.parametrize("shape", ["pair", "lone"])
def test_icmp4(shape):
    buf, desc, req, od, osize = icmp_case()
    n = desc.size
    size = 1024 * n - (shape == "pair")                     # a wave takes two records below 1024 bytes a record
    buf = np.concatenate([buf, synth.random_bytes(size, size - buf.size)])
    want = np.full(osize, CANARY, np.uint8)
    wv, woa = icmp4_ref.reply_batch(buf, desc, req, None, want, od)
    out = torch.full((osize,), CANARY, dtype=torch.uint8, device=DEV)
    gv, goa = batch.icmp4_reply_batch(to_dev(buf), dev_desc(desc), n, to_dev(req.view(np.uint8)), out, dev_desc(od), state=None)
    torch.cuda.synchronize()
    assert (wv == OK).all() and (gv.cpu().numpy() == OK).all()
    np.testing.assert_array_equal(woa["len"], [20 + c[2] if c[0] == 0 else 28 + min(c[2], 28) for c in ICMP_CELLS])
    same_desc(goa.cpu().numpy().view(icmp4_ref.DESC_DTYPE), woa)
    same_bytes(out.cpu().numpy(), want)
