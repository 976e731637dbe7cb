"""What the reassembly batches (pico_ipv4_reassemble_batch_dev, pico_ipv6_reassemble_batch_dev) may and
may not write, stated once, and the batches that hold them to it: a plain module, no fixtures, no GPU.

include/pico_csum.h: "The bytes of an output region are unspecified when its datagram is not
reassembled [...] and past the reassembled datagram's end [...]; no byte outside the region is
written."  unspecified_mask is that sentence; every other byte of the output buffer is the oracle's or
the canary the buffer was filled with (same_outside).

The batches are lists of Dgram -- fragment frames in arrival order, each frame's source address mod
16, the place of the first transport byte in its 16-byte output line, the region's capacity --
packed by build(): output regions TIGHT (capacity = header + length exactly, unless the datagram
says otherwise) and back to back, 0-15 canary pad bytes between them, 64 canary guard bytes behind
the last.  grid_dgrams is the unit grid (tests/test_gpu_unit_mover.py's, for the one gather that keeps
its own unit mover), neighbour_dgrams the datagrams that are not reassembled, or reassembled short of
what arrived, each between two reassembled ones.  tests/test_frag_regions_cases.py runs them through
the oracle alone, tests/test_gpu_frag_regions.py through the device."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

from oracle import oracle as O
from tests import golden_data as G

CANARY = 0xA5
GUARD = 64
MALFORMED = 8
MF = 0x2000


def hdr_of(v6: bool) -> int:
    return 40 if v6 else 20


def unspecified_mask(out_size: int, od: np.ndarray, verdict, out_len, hdr: int) -> np.ndarray:
    """bool[out_size]: True exactly for a reassembled (verdict != MALFORMED) datagram's
    [off + hdr + len, off + od.len) and a not-reassembled datagram's [off, off + od.len), each clipped
    to the buffer.  Every other byte is specified."""
    mask = np.zeros(out_size, bool)
    for g in range(od.shape[0]):
        off = int(od["off"][g])
        lo = off if verdict[g] == MALFORMED else off + hdr + int(out_len[g])
        lo, hi = min(lo, out_size), min(off + int(od["len"][g]), out_size)
        if hi > lo:
            mask[lo:hi] = True
    return mask


def same_bytes(got: np.ndarray, want: np.ndarray, what: str = "bytes"):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} {what} differ, first at {bad[:8].tolist()}"


def same_outside(got: np.ndarray, want: np.ndarray, mask: np.ndarray):
    """Every specified byte of the whole buffer: the oracle's where it wrote, else the canary."""
    assert got.size == want.size == mask.size
    bad = np.flatnonzero((got != want) & ~mask)
    assert bad.size == 0, f"{bad.size} specified bytes differ, first at {bad[:8].tolist()}"


# ---- frames ----------------------------------------------------------------------------------------

def frame4(data: np.ndarray, off: int, mf: bool, proto: int, ident: int) -> np.ndarray:
    """An IPv4 fragment: 20-byte header (tot = 20 + payload, the fragment field) + payload (the model:
    frame() of tests/test_frag_oracle.py)."""
    n = data.size
    h = np.zeros(20, np.uint8)
    frag = (off >> 3) | (MF if mf else 0)
    h[0], h[2], h[3], h[4], h[5], h[6], h[7], h[8], h[9] = (0x45, (20 + n) >> 8, (20 + n) & 0xFF, (ident >> 8) & 0xFF,
                                                             ident & 0xFF, frag >> 8, frag & 0xFF, 64, proto)
    h[12:20] = [10, 0, ident & 0xFF, 1, 10, 0, 0, 2]
    return np.concatenate([h, data])


def frame6(data: np.ndarray, off: int, mf: bool, proto: int, ident: int, hbh: bool = False, b9: int | None = None) -> np.ndarray:
    """Its IPv6 twin: 40-byte fixed header, an 8-byte hop-by-hop header (PadN) when `hbh`, the 8-byte
    fragment header (next = proto, offset | M), payload.  b9 = header byte 9, which the reference's
    TCP / UDP dispatch reads on the copied header (the protocol unless given)."""
    n = data.size
    ext = 16 if hbh else 8
    h = np.zeros(40 + ext, np.uint8)
    h[0], h[4], h[5], h[6], h[7] = 0x60, (ext + n) >> 8, (ext + n) & 0xFF, (0 if hbh else 44), 64
    h[8:24] = [0x20, proto if b9 is None else b9, 0x0d, 0xb8] + [0] * 10 + [(ident >> 8) & 0xFF, ident & 0xFF]
    h[24:40] = [0x20, 1, 0x0d, 0xb8] + [0] * 11 + [2]
    f = 40
    if hbh:
        h[40:48] = [44, 0, 1, 4, 0, 0, 0, 0]
        f = 48
    om = off | (1 if mf else 0)
    h[f:f + 8] = [proto, 0, om >> 8, om & 0xFF, 0, 0, (ident >> 8) & 0xFF, ident & 0xFF]
    return np.concatenate([h, data])


def make_frame(v6: bool, data, off, mf, proto, ident, hbh=False, b9=None) -> np.ndarray:
    return frame6(data, off, mf, proto, ident, hbh, b9) if v6 else frame4(data, off, mf, proto, ident)


# ---- batches ---------------------------------------------------------------------------------------

@dataclass
class Dgram:
    frames: list                       # arrival order
    aligns: list                       # each frame's header address mod 16
    place: int                         # the first transport byte's place in its 16-byte output line: 0, 4, 8, 12
    length: int | None                 # out_len when reassembled, None when not
    cap: int | None = None             # od.len; None = tight: hdr + length
    shift: int = 0                     # added to od.off after the place is set (2: a misaligned region)
    cut: dict = field(default_factory=dict)   # frame index -> bytes taken off its descriptor's len
    past: bool = False                 # the group (n_frag - 1, 5): past the descriptor array
    what: str = ""


@dataclass
class Case:
    buf: np.ndarray                    # ends with the last frame's last payload byte
    d: np.ndarray                      # fragment descriptors
    grp: np.ndarray
    od: np.ndarray
    size: int                          # the output buffer: the regions, the last one's end
    length: np.ndarray                 # int64: the expected out_len, -1 = not reassembled
    tight: np.ndarray                  # bool: od.len == hdr + length
    what: list


def build(dgrams, v6: bool, seed: int = 7) -> Case:
    """Frames packed in arrival order, each header at its address mod 16 (the 0-15 gap bytes random),
    the buffer ending with the last frame; regions back to back, each at the next address that puts its
    transport at `place`."""
    rng = np.random.default_rng(seed)
    hdr = hdr_of(v6)
    offs, lens, parts, grp, pos = [], [], [], [], 0
    for dg in dgrams:
        grp.append([len(offs), len(dg.frames)])
        for k, (f, a) in enumerate(zip(dg.frames, dg.aligns)):
            gap = (a - pos) % 16
            parts.append(rng.integers(0, 256, gap, dtype=np.uint8))
            offs.append(pos + gap)
            lens.append(f.size - dg.cut.get(k, 0))
            parts.append(f)
            pos += gap + f.size
    for g, dg in enumerate(dgrams):
        if dg.past:
            grp[g] = [len(offs) - 1, 5]
    ooff, ocap, pos = [], [], 0
    for dg in dgrams:
        assert dg.place in (0, 4, 8, 12)
        pos += (dg.place - hdr - pos) % 16
        cap = hdr + dg.length if dg.cap is None else dg.cap
        ooff.append(pos + dg.shift)
        ocap.append(cap)
        pos += dg.shift + cap
    length = np.array([-1 if dg.length is None else dg.length for dg in dgrams], np.int64)
    od = G.ipv4_desc(np.array(ooff, np.uint64), np.array(ocap, np.uint32))
    return Case(np.concatenate(parts), G.ipv4_desc(np.array(offs, np.uint64), np.array(lens, np.uint32)),
                np.array(grp, np.uint32).reshape(-1, 2), od, pos, length,
                (length >= 0) & (od["len"].astype(np.int64) == hdr + length), [dg.what for dg in dgrams])


def run_oracle(case: Case, v6: bool, od: np.ndarray | None = None):
    """(out_len, out_transport, verdict, the output buffer WITH its guard) of the oracle; the buffer
    pre-filled with the canary.  od: other output descriptors than the case's (the oracle knows no
    out_len: a region past it is stated as od.len = 0)."""
    out = np.full(case.size + GUARD, CANARY, np.uint8)
    fn = O.ipv6_reassemble if v6 else O.ipv4_reassemble
    wl, w4, wv = fn(case.buf, case.d, case.grp, out, case.od if od is None else od)
    return wl, w4, wv, out


def flanked(case: Case, verdict) -> bool:
    """Every not-reassembled datagram stands between two reassembled ones in tight regions."""
    ok = (np.asarray(verdict) != MALFORMED) & case.tight
    bad = np.flatnonzero(np.asarray(verdict) == MALFORMED)
    return bool(bad.size and bad.min() > 0 and bad.max() < ok.size - 1 and ok[bad - 1].all() and ok[bad + 1].all())


# ---- the unit grid ---------------------------------------------------------------------------------

PAYLOADS = (8, 16, 24, 32, 40, 48)
ITEMS = [(m, P, L, place, par) for m in (1, 2, 3) for P in (PAYLOADS if m > 1 else PAYLOADS[:1])
         for L in range(1, 49) for place in (0, 4, 8, 12) for par in (0, 1)]
PROTOS = {False: (6, 17, 1), True: (6, 17, 58)}


def item_length(item) -> int:
    m, P, L, place, par = item
    return P * (m - 1) + L


def grid_dgrams(items, v6: bool, seed: int = 81) -> list:
    """Item (m, P, L, place, par): m fragments, every one but the last of P bytes, the last of L; the
    transport at `place`; the first arrival's header at par + 2 ((L + place / 4) % 8) mod 16 -- all of
    0..15, of parity par -- and each later arrival 2 further; arrival in order or reversed by the parity
    of L + place / 4; the protocol cycling; IPv6 with a hop-by-hop header on half of the items whose L is
    a multiple of 8 (behind one the reference drops a payload length that is not) and the protocol in
    byte 9 on three of four.  Transport bytes random, checksums not fixed up."""
    rng = np.random.default_rng(seed + v6)
    out = []
    for i, (m, P, L, place, par) in enumerate(items):
        proto = PROTOS[v6][i % 3]
        t = rng.integers(0, 256, P * (m - 1) + L, dtype=np.uint8)
        frames = [make_frame(v6, t[k * P:k * P + (P if k < m - 1 else L)], k * P, k < m - 1, proto, i & 0xFFFF,
                             hbh=L % 8 == 0 and bool((par ^ (place // 4)) & 1), b9=None if i % 4 else 0x0d) for k in range(m)]
        q = L + place // 4
        if q & 1:
            frames.reverse()
        a = par + 2 * (q % 8)
        out.append(Dgram(frames, [(a + 2 * k) % 16 for k in range(m)], place, t.size, what=f"item {i}"))
    return out


# ---- neighbours of what is not reassembled ---------------------------------------------------------

def _chain(v6, rng, sizes, proto, ident, order=None, hbh=False):
    """(frames, transport): a valid fragmentation into `sizes`, arrival in `order`."""
    t = rng.integers(0, 256, sum(sizes), dtype=np.uint8)
    at = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    frames = [make_frame(v6, t[at[k]:at[k + 1]], at[k], k < len(sizes) - 1, proto, ident, hbh) for k in range(len(sizes))]
    if order is not None:
        frames = [frames[k] for k in order]
    return frames, t


def neighbour_dgrams(v6: bool, seed: int = 91) -> list:
    """flank, special, flank, special, ..., flank: the specials of the issue's list in its order, the
    flanks two-fragment datagrams in tight regions at every place."""
    rng = np.random.default_rng(seed + v6)
    hdr = hdr_of(v6)
    protos = PROTOS[v6]
    n = [0]

    def ident():
        n[0] += 1
        return 0x4000 + n[0]

    def rnd(k):
        return rng.integers(0, 256, k, dtype=np.uint8)

    def mk(data, off, mf, idn, proto=17, hbh=False):
        return make_frame(v6, data, off, mf, proto, idn, hbh)

    def aligns(k, cnt):
        return [(5 * k + 3 * j) % 16 for j in range(cnt)]

    sp = []

    def add(frames, length, what, **kw):
        k = len(sp)
        sp.append(Dgram(frames, aligns(k, len(frames)), (4 * k + 8) % 16, length, what=what, **kw))

    # 1. incomplete: a hole, fragments on both sides of it present
    i = ident()
    add([mk(rnd(32), 0, True, i), mk(rnd(32), 96, False, i), mk(rnd(32), 64, True, i)], None, "hole", cap=hdr + 128)
    # 2. region too small
    for cap, what in ((hdr + 40 - 1, "cap short by 1"), (hdr + 40 - 8, "cap short by 8"), (hdr, "cap 0"),
                      (hdr - 4, "od.len = HDR - 4"), (0, "od.len = 0")):
        fr, _ = _chain(v6, rng, [24, 16], 6, ident(), order=[1, 0])
        add(fr, None, what, cap=cap)
    # 3. a fragment behind the completing one
    for far in (64, 8191 * 8):
        i = ident()
        add([mk(rnd(32), 0, True, i), mk(rnd(32), far, False, i), mk(rnd(32), 32, False, i)], None,
            f"fragment behind the last, at {far}", cap=hdr + 64)
    # 4. a repeated last offset, the later arrival longer -- and the other way round
    i = ident()
    add([mk(rnd(32), 0, True, i), mk(rnd(8), 32, False, i), mk(rnd(48), 32, False, i)], 40, "repeated last offset, later longer")
    i = ident()
    add([mk(rnd(48), 32, False, i), mk(rnd(32), 0, True, i), mk(rnd(8), 32, False, i)], 80, "repeated last offset, later shorter")
    # 5. a repeated offset, the same length, other bytes
    i = ident()
    add([mk(rnd(32), 0, True, i), mk(rnd(32), 0, True, i), mk(rnd(16), 32, False, i)], 48, "repeated offset, other bytes")
    # 6. an overlap at offset 8 into a 32-byte fragment
    i = ident()
    add([mk(rnd(32), 0, True, i), mk(rnd(32), 8, True, i), mk(rnd(16), 32, False, i)], None, "overlap", cap=hdr + 48)
    # 7. a payload one byte past desc.len
    fr, _ = _chain(v6, rng, [24, 17], 17, ident())
    add(fr, None, "truncated descriptor", cap=hdr + 41, cut={1: 1})
    # 8. HDR + len = 65536, fragments of 1480 bytes
    total = 65536 - hdr
    sizes = [1480] * (total // 1480) + [total % 1480]
    fr, _ = _chain(v6, rng, sizes, 17, ident(), order=rng.permutation(len(sizes)).tolist())
    add(fr, None, "HDR + len = 65536", cap=65536)
    # 9. bad groups and regions
    add([], None, "empty group", cap=hdr + 64)
    add([], None, "group past n_frag", cap=hdr + 64, past=True)
    fr, _ = _chain(v6, rng, [8] * 513, 6, ident(), order=rng.permutation(513).tolist())
    add(fr, None, "513 fragments", cap=hdr + 8 * 513)
    fr, _ = _chain(v6, rng, [24, 16], 6, ident())
    add(fr, None, "region at off = 2 mod 4", cap=hdr + 40, shift=2)
    # 10. reassembled: 9 .. 512 fragments of 8 bytes (the last of 8, or of 1-3)
    for cnt in (9, 64, 65, 128, 129, 512):
        sizes = [8] * (cnt - 1) + [8 if cnt & 1 else (cnt // 64) % 8 + 1]
        fr, t = _chain(v6, rng, sizes, protos[cnt % 3], ident(), order=rng.permutation(cnt).tolist(), hbh=bool(cnt & 1))
        add(fr, t.size, f"{cnt} fragments")

    def flank(k):
        P, L = (8, 16, 24)[k % 3], 1 + (7 * k) % 48
        fr, t = _chain(v6, rng, [P, L], protos[k % 3], ident(), order=[1, 0] if k & 1 else None, hbh=L % 8 == 0)
        return Dgram(fr, [(3 * k + 1) % 16, (3 * k + 6) % 16], (4 * k) % 16, t.size, what=f"flank {k}")

    out = [flank(0)]
    for k, s in enumerate(sp):
        out += [s, flank(k + 1)]
    return out


@functools.lru_cache(maxsize=None)
def grid_case(v6: bool, every: int = 1) -> Case:
    return build(grid_dgrams(ITEMS[::every], v6), v6)


@functools.lru_cache(maxsize=None)
def neighbour_case(v6: bool, with_grid: bool = False) -> Case:
    return build((grid_dgrams(ITEMS, v6) if with_grid else []) + neighbour_dgrams(v6), v6)


@functools.lru_cache(maxsize=None)
def oracle_of(name: str, v6: bool, arg=None):
    """The oracle's results on a cached case, computed once and shared (treat as read-only)."""
    case = grid_case(v6, arg or 1) if name == "grid" else neighbour_case(v6, bool(arg))
    return run_oracle(case, v6)
