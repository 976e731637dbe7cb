"""GPU: what the three scatter / gather batches share -- the 16-byte unit mover of pico_csum_dev.h
(unit_pair_move) -- pinned through their entry points: pico_ipv4_fragment_batch_dev,
pico_tcp_segment_batch_dev and pico_tcp_coalesce_batch_dev, each against its numpy restatement
(tests/fragtx_ref.py, tests/tcpseg_ref.py, tests/tcprx_ref.py), over the WHOLE output buffer,
pre-filled with a canary.

One batch per entry point, its groups the cross product of
  * members a group: 1, 2, 3;
  * payload bytes L = 1..48: the only member's; in a longer group every member before the last has
    48 (fragments: per = 48 at MTU 68, the batch's one MTU) or L (segments: per = L), and the last
    1..48 (fragments) or 1..L (segments) -- so a member's units run from one partial unit to three
    whole ones, with and without partial first and last units;
  * the first payload byte's place in its 16-byte output line, 0..15 (fragments / send segments:
    through the region's offset, at strides 1504 -- every member on that place -- and 1500 -- the
    place moves by 12 a member; received segments: through the region's offset, the later members'
    by seq - rcv_nxt);
  * the payload's source address, even and odd.
The input buffer ends with the last item's last payload byte: that item's last unit is read byte by
byte with nothing readable behind it.  Every group is valid: ACCEPT is asserted for all of them
before anything is compared, so none drops out of the comparison.  4608 groups launch the one-wave
shape; every third group (1536) in a launch of its own takes the four-wave shape."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from picotcp_amd import batch, synth
from tests import fragtx_ref, tcprx_ref, tcpseg_ref
from tests.gpu_util import DEV, pairs_dev, to_dev

pytestmark = pytest.mark.gpu

CANARY = 0xA5
ITEMS = [(m, L, o, par) for m in (1, 2, 3) for L in range(1, 49) for o in range(16) for par in (0, 1)]
SHAPES = {"one_wave": ITEMS, "four_waves": ITEMS[::3]}      # 4608 groups: >= 3072; 1536: below
FRAG_PER = 48


def last_of(L, o, par):
    """The last member's payload in a group of L-byte members: 1..L."""
    return 1 + (5 * o + 3 * par + L) % L


def header_align(L, o, par):
    """The header's address mod 16: all of 0..15, its parity (and so the payload's: the headers
    are 20 and 40 bytes) the item's."""
    return par + 2 * ((L + o) % 8)


def regions(cap, first_payload_at, hdr):
    """Output regions back to back, region g's first payload byte (hdr bytes in) at
    first_payload_at[g] mod 16.  Returns (offsets uint64, buffer size)."""
    ooff, pos = np.zeros(len(cap), np.uint64), 0
    for g, c in enumerate(cap):
        pos += (first_payload_at[g] - hdr - pos) % 16
        ooff[g] = pos
        pos += int(c)
    return ooff, pos + 16


def same_bytes(got: np.ndarray, want: np.ndarray):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} bytes differ, first at {bad[:8].tolist()}"


def fragment_case(items, stride):
    """(base, dgram desc, mtu, groups, n_frag, out size, out desc) for ipv4_fragment_batch."""
    tl = [FRAG_PER * (m - 1) + L for m, L, o, par in items]
    buf, off, dlen, groups, _, cap, n_frag, _ = synth.ipv4_oversized(
        tl, mtu=20 + FRAG_PER, stride=stride, seed=71, proto=[(6, 17, 1)[i % 3] for i in range(len(items))],
        align=[header_align(L, o, par) for m, L, o, par in items])
    ooff, out_size = regions(cap, [o for m, L, o, par in items], 20)
    return (buf[:int(off[-1]) + int(dlen[-1])], batch.make_desc(off, dlen), 20 + FRAG_PER, groups, n_frag, out_size,
            batch.make_desc(ooff, cap))


def segment_case(items, stride):
    """(base, stream desc, groups, n_seg, out size, out desc) for tcp_segment_batch: IPv4, thl 20."""
    P = [L * (m - 1) + (L if m == 1 else last_of(L, o, par)) for m, L, o, par in items]
    buf, off, slen, per, groups, _, cap, n_seg, _ = synth.tcp_streams(
        P, per=[L for m, L, o, par in items], stride=stride, seed=72, align=[header_align(L, o, par) for m, L, o, par in items])
    ooff, out_size = regions(cap, [o for m, L, o, par in items], 40)
    return buf[:int(off[-1]) + int(slen[-1])], batch.make_desc(off, slen, per), groups, n_seg, out_size, batch.make_desc(ooff, cap)


def coalesce_case(items):
    """(base, seg desc, groups, conn, out size, out desc, stream bytes) for tcp_coalesce_batch: per
    group its members in order, IPv4, thl 20, every frame's descriptor ending with its payload; the
    region holds exactly the stream."""
    rng = np.random.default_rng(73)
    conns, aligns, total = [], [], []
    for m, L, o, par in items:
        lens = [L] * (m - 1) + [L if m == 1 else last_of(L, o, par)]
        rcv = int(rng.integers(0, 1 << 32))
        frames, seq = [], rcv
        for k, pl in enumerate(lens):
            frames.append(synth.tcp_rx_frame(rng, seq & 0xFFFFFFFF, rng.integers(0, 256, pl, dtype=np.uint8)))
            aligns.append((header_align(L, o, par) + 2 * k) % 16)
            seq += pl
        conns.append((frames, rcv, False, sum(lens)))
        total.append(sum(lens))
    buf, off, ln, groups, conn, _, cap, _ = synth.tcp_rx_pack(conns, align=aligns, seed=73)
    ooff, out_size = regions(cap, [o for m, L, o, par in items], 0)
    assert buf.size == int(off[-1]) + int(ln[-1])
    return buf, batch.make_desc(off, ln), groups, conn, out_size, batch.make_desc(ooff, cap), np.array(total, np.uint32)


@pytest.mark.parametrize("stride", [1504, 1500])
@pytest.mark.parametrize("shape", SHAPES)
def test_fragment(shape, stride):
    items = SHAPES[shape]
    base, dd, mtu, groups, n_frag, out_size, od = fragment_case(items, stride)
    want_out = np.full(out_size, CANARY, np.uint8)
    wv, wc, w4, wof = fragtx_ref.fragment(base, dd, mtu, groups, n_frag, want_out, od, stride, batch.F_WRITE)
    out = torch.full((out_size,), CANARY, dtype=torch.uint8, device=DEV)
    of = torch.zeros(16 * n_frag, dtype=torch.uint8, device=DEV)
    v, c, l4 = batch.ipv4_fragment_batch(to_dev(base), to_dev(dd.view(np.uint8)), mtu, pairs_dev(groups), n_frag, out,
                                         to_dev(od.view(np.uint8)), stride, flags=batch.F_WRITE, out_frag=of)
    torch.cuda.synchronize()
    assert (v.cpu().numpy() == batch.V_ACCEPT).all() and (wv == batch.V_ACCEPT).all()
    np.testing.assert_array_equal(c.cpu().numpy().view(np.uint32), [m for m, *_ in items])
    np.testing.assert_array_equal(c.cpu().numpy().view(np.uint32), wc)
    np.testing.assert_array_equal(l4.cpu().numpy().view(np.uint16), w4)
    np.testing.assert_array_equal(of.cpu().numpy().view(fragtx_ref.DESC_DTYPE), wof)
    same_bytes(out.cpu().numpy(), want_out)


@pytest.mark.parametrize("stride", [1504, 1500])
@pytest.mark.parametrize("shape", SHAPES)
def test_segment(shape, stride):
    items = SHAPES[shape]
    base, sd, groups, n_seg, out_size, od = segment_case(items, stride)
    want_out = np.full(out_size, CANARY, np.uint8)
    wv, wc, wof = tcpseg_ref.segment(base, sd, groups, n_seg, want_out, od, stride)
    out = torch.full((out_size,), CANARY, dtype=torch.uint8, device=DEV)
    of = torch.zeros(16 * n_seg, dtype=torch.uint8, device=DEV)
    v, c = batch.tcp_segment_batch(to_dev(base), to_dev(sd.view(np.uint8)), pairs_dev(groups), n_seg, out,
                                   to_dev(od.view(np.uint8)), stride, out_seg=of)
    torch.cuda.synchronize()
    assert (v.cpu().numpy() == batch.V_ACCEPT).all() and (wv == batch.V_ACCEPT).all()
    np.testing.assert_array_equal(c.cpu().numpy().view(np.uint32), [m for m, *_ in items])
    np.testing.assert_array_equal(c.cpu().numpy().view(np.uint32), wc)
    np.testing.assert_array_equal(of.cpu().numpy().view(tcpseg_ref.DESC_DTYPE), wof)
    same_bytes(out.cpu().numpy(), want_out)


@pytest.mark.parametrize("shape", SHAPES)
def test_coalesce(shape):
    items = SHAPES[shape]
    base, sd, groups, conn, out_size, od, total = coalesce_case(items)
    want_out = np.full(out_size, CANARY, np.uint8)
    wv, wl, ws = tcprx_ref.coalesce(base, sd, groups, conn, want_out, od)
    out = torch.full((out_size,), CANARY, dtype=torch.uint8, device=DEV)
    v, ol, sv = batch.tcp_coalesce_batch(to_dev(base), to_dev(sd.view(np.uint8)), sd.shape[0], pairs_dev(groups),
                                         pairs_dev(conn), out, to_dev(od.view(np.uint8)))
    torch.cuda.synchronize()
    assert (v.cpu().numpy() == batch.V_ACCEPT).all() and (sv.cpu().numpy() == batch.V_ACCEPT).all()
    assert (wv == batch.V_ACCEPT).all() and (ws == batch.V_ACCEPT).all()
    np.testing.assert_array_equal(ol.cpu().numpy().view(np.uint32), total)
    np.testing.assert_array_equal(ol.cpu().numpy().view(np.uint32), wl)
    same_bytes(out.cpu().numpy(), want_out)
