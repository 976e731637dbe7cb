"""Seeded synthetic frame batches.

Byte source: splitmix64 (Steele, Lea, Flood 2014): state_i = seed + (i+1)*0x9E3779B97F4A7C15,
z = mix(state_i), little-endian bytes of z concatenated.  Same definition in the
golden-fixture generator (tests/golden/make_golden.py), so fixtures store only
seeds and expected outputs.
"""
from __future__ import annotations

import numpy as np

GAMMA = np.uint64(0x9E3779B97F4A7C15)
M1 = np.uint64(0xBF58476D1CE4E5B9)
M2 = np.uint64(0x94D049BB133111EB)


def splitmix64(seed: int, count: int, start: int = 0) -> np.ndarray:
    with np.errstate(over="ignore"):
        i = np.arange(start + 1, start + count + 1, dtype=np.uint64)
        z = np.uint64(seed & 0xFFFFFFFFFFFFFFFF) + i * GAMMA
        z = (z ^ (z >> np.uint64(30))) * M1
        z = (z ^ (z >> np.uint64(27))) * M2
        return z ^ (z >> np.uint64(31))


def random_bytes(seed: int, nbytes: int) -> np.ndarray:
    words = splitmix64(seed, (nbytes + 7) // 8)
    return words.view(np.uint8)[:nbytes].copy()


def uniform_batch(n: int, length: int, stride: int | None = None, seed: int = 1) -> np.ndarray:
    """C1/C3/C4: n frames of `length` random bytes at `stride` (default packed)."""
    stride = length if stride is None else stride
    total = (n - 1) * stride + length if n else 0
    return random_bytes(seed, total)


SIMPLE_IMIX = ((64, 7), (576, 4), (1500, 1))


def imix_lengths(n: int, seed: int, mix=SIMPLE_IMIX) -> np.ndarray:
    """C2: frame sizes in the simple-IMIX ratio 7:4:1, seeded shuffle."""
    sizes = np.concatenate([np.full(w, s, dtype=np.uint32) for s, w in mix])
    reps = -(-n // sizes.size)
    lens = np.tile(sizes, reps)[:n]
    perm = np.argsort(splitmix64(seed ^ 0x5EED, n), kind="stable")
    return lens[perm]


def ipv4_batch(lengths: np.ndarray, seed: int = 2, proto: int = 6, eth: bool = True, ihl: int = 5,
               frag=None, slot: int = 0):
    """IPv4 datagrams of the given total lengths, packed back to back, each with a
    valid header (vhl = 0x40|ihl, len, ttl 64, proto, random id/addresses/ports/payload)
    and a transport header (TCP 20 B, UDP 8 B, ICMP 8 B).  frag = the flags / offset field
    (host order) of every datagram, or an array cycled over them; default DF (0x4000).
    Every crc field is zero:
    make them valid with the TX kernel (PICO_CSUM_F_TX | F_WRITE) or a host checker.
    eth=True puts a 14-byte Ethernet header in front of each datagram (pico_ethernet.c:183),
    so the IPv4 headers are 2-byte aligned as in the reference RX path.
    slot > 0: frame k starts at k * slot instead (a driver's ring of fixed slots; the rest of each
    slot holds random bytes).
    Returns (buffer uint8, net offsets uint64, available bytes uint32)."""
    lengths = np.asarray(lengths, dtype=np.uint32)
    n = lengths.size
    pre = 14 if eth else 0
    frame_len = lengths.astype(np.uint64) + pre
    starts = np.zeros(n, dtype=np.uint64)
    if slot:
        assert int(frame_len.max(initial=0)) <= slot, "frame larger than its slot"
        starts = np.arange(n, dtype=np.uint64) * np.uint64(slot)
        total = n * slot
    else:
        if n:
            starts[1:] = np.cumsum(frame_len)[:-1]
        total = int(frame_len.sum())
    buf = random_bytes(seed, total)
    net = starts + np.uint64(pre)
    hl = 4 * ihl
    rnd = splitmix64(seed ^ 0xABCDEF, n).view(np.uint8).reshape(n, 8)
    idx = net.astype(np.int64)

    def put(off, vals):
        buf[idx + off] = vals

    if eth:
        e = starts.astype(np.int64)
        buf[e + 12] = 0x08
        buf[e + 13] = 0x00
    put(0, np.uint8(0x40 | ihl))
    put(1, 0)
    put(2, (lengths >> 8).astype(np.uint8))
    put(3, (lengths & 0xFF).astype(np.uint8))
    put(4, rnd[:, 0]); put(5, rnd[:, 1])
    if frag is None:
        put(6, 0x40); put(7, 0)
    else:
        fr = np.resize(np.asarray(frag, dtype=np.uint16), n) if n else np.zeros(0, np.uint16)
        put(6, (fr >> 8).astype(np.uint8)); put(7, (fr & 0xFF).astype(np.uint8))
    put(8, 64)
    put(9, np.uint8(proto))
    put(10, 0); put(11, 0)
    # src 10.x.y.z / dst 192.168.y.z from the random word
    put(12, 10); put(13, rnd[:, 2]); put(14, rnd[:, 3]); put(15, rnd[:, 4])
    put(16, 192); put(17, 168); put(18, rnd[:, 5]); put(19, rnd[:, 6])
    for o in range(20, hl):               # options: NOP padding
        put(o, 1)
    t = idx + hl
    if proto == 6:
        buf[t + 12] = 0x50                  # data offset 5
        buf[t + 13] = 0x18                  # PSH|ACK
        buf[t + 16] = 0
        buf[t + 17] = 0
    elif proto == 17:
        ul = (lengths - hl).astype(np.uint32)
        buf[t + 4] = (ul >> 8).astype(np.uint8)
        buf[t + 5] = (ul & 0xFF).astype(np.uint8)
        buf[t + 6] = 0
        buf[t + 7] = 0
    elif proto == 1:
        buf[t + 0] = 8                      # echo request
        buf[t + 1] = 0
        buf[t + 2] = 0
        buf[t + 3] = 0
    avail = lengths.copy()
    return buf, net, avail


def ipv6_batch(lengths: np.ndarray, seed: int = 3, proto: int = 6, eth: bool = True, hbh: bool = False,
               icmp_type: int = 128, frag=None, destopt: bool = False, walked: bool = False):
    """IPv6 datagrams of the given total lengths (40-byte header + optional 8-byte extension
    headers + transport), packed back to back, crc fields zero.  proto 6 / 17 / 58 (ICMPv6 of
    `icmp_type`).  Extension headers, in RFC 8200 order: hop-by-hop (PadN) when `hbh`, a
    destination-options header (PadN) when `destopt`, a fragment header carrying `frag` (the
    offset / M field, host order; scalar or an array cycled over the datagrams) when frag is not
    None.  Returns (buffer, net offsets, available bytes, descriptor seeds): seed =
    net_len | proto << 16 when extension headers are present and not `walked` (what
    pico_ipv6_extension_headers leaves in the frame), else 0 (the kernel walks them)."""
    lengths = np.asarray(lengths, dtype=np.uint32)
    n = lengths.size
    pre = 14 if eth else 0
    frame_len = lengths.astype(np.uint64) + pre
    starts = np.zeros(n, dtype=np.uint64)
    if n:
        starts[1:] = np.cumsum(frame_len)[:-1]
    buf = random_bytes(seed, int(frame_len.sum()))
    net = starts + np.uint64(pre)
    idx = net.astype(np.int64)
    chain = (["hbh"] if hbh else []) + (["dst"] if destopt else []) + (["frag"] if frag is not None else [])
    net_len = 40 + 8 * len(chain)
    plen = (lengths - 40).astype(np.uint32)
    if eth:
        e = starts.astype(np.int64)
        buf[e + 12] = 0x86
        buf[e + 13] = 0xDD
    code = {"hbh": 0, "dst": 60, "frag": 44}
    buf[idx + 0] = 0x60
    buf[idx + 4] = (plen >> 8).astype(np.uint8)
    buf[idx + 5] = (plen & 0xFF).astype(np.uint8)
    buf[idx + 6] = code[chain[0]] if chain else proto
    buf[idx + 7] = 255 if proto == 58 else 64
    for k, c in enumerate(chain):
        o = idx + 40 + 8 * k
        buf[o] = code[chain[k + 1]] if k + 1 < len(chain) else proto   # next header
        if c == "frag":
            fr = np.resize(np.asarray(frag, dtype=np.uint16), n) if n else np.zeros(0, np.uint16)
            buf[o + 1] = 0
            buf[o + 2] = (fr >> 8).astype(np.uint8)
            buf[o + 3] = (fr & 0xFF).astype(np.uint8)
        else:
            buf[o + 1] = 0            # length: 8 bytes
            buf[o + 2] = 1            # PadN
            buf[o + 3] = 4
            for q in range(4, 8):
                buf[o + q] = 0
    t = idx + net_len
    if proto == 6:
        buf[t + 12] = 0x50
        buf[t + 13] = 0x18
        buf[t + 16] = 0
        buf[t + 17] = 0
    elif proto == 17:
        ul = (lengths - net_len).astype(np.uint32)
        buf[t + 4] = (ul >> 8).astype(np.uint8)
        buf[t + 5] = (ul & 0xFF).astype(np.uint8)
        buf[t + 6] = 0
        buf[t + 7] = 0
    elif proto == 58:
        buf[t + 0] = icmp_type
        buf[t + 1] = 0
        buf[t + 2] = 0
        buf[t + 3] = 0
    seeds = np.full(n, (net_len | (proto << 16)) if chain and not walked else 0, dtype=np.uint32)
    return buf, net, lengths.copy(), seeds


ETH_KINDS = ("ipv4_tcp", "ipv4_udp", "ipv4_icmp", "ipv6_tcp", "ipv6_udp", "ipv6_icmp", "ipv6_hbh_tcp", "arp",
             "lldp", "ipv4_bad_version", "ipv4_opt_tcp", "ipv4_opt_udp", "ipv4_frag", "ipv4_evil", "ipv6_frag",
             "ipv6_dst_tcp")


def interleave(parts, kinds: np.ndarray):
    """One burst from several packed ones: parts[k] = (buffer, frame starts, frame bytes); frame i of
    the result is the next unused frame of parts[kinds[i]], back to back.  Returns (buffer, starts
    uint64, bytes uint32)."""
    kinds = np.asarray(kinds)
    n = kinds.size
    lens = np.zeros(n, np.int64)
    src = np.zeros(n, np.int64)                      # source start, in the concatenated parts
    base = 0
    for k, (b, st, ln) in enumerate(parts):
        sel = np.flatnonzero(kinds == k)
        assert sel.size <= st.size
        lens[sel] = np.asarray(ln, np.int64)[:sel.size]
        src[sel] = np.asarray(st, np.int64)[:sel.size] + base
        base += b.size
    cat = np.concatenate([b for b, _, _ in parts])
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
    seg = np.repeat(np.arange(n), lens)
    idx = (src - starts)[seg] + np.arange(int(lens.sum()))
    return cat[idx], starts.astype(np.uint64), lens.astype(np.uint32)


def eth_batch(n: int, seed: int = 11, mac: bytes = bytes.fromhex("02005e0a0b0c")):
    """A mixed Ethernet burst as a TAP / pico_device RX ring delivers it: n frames, each
    with a 14-byte Ethernet header, of the kinds in ETH_KINDS (IPv4 / IPv6 datagrams in
    IMIX sizes, ARP, an unknown ethertype, an IPv4 ethertype carrying version 6), in seeded
    order with 0-3 byte gaps (every alignment), and destination MACs drawn from {mac,
    broadcast, 01:00:5e IPv4 multicast, 33:33 IPv6 multicast, a foreign unicast}.  Transport
    crc fields are zero (TX input).  IPv4 fragments (first / middle / last) and evil-bit
    datagrams, IPv6 datagrams behind a fragment or a destination-options header left for the
    kernel to walk (seed 0).  Returns (buffer, frame offsets uint64, frame bytes uint32,
    descriptor seeds uint32 (IPv6 net_len | proto << 16 behind a hop-by-hop header, else 0),
    kind index uint8 into ETH_KINDS)."""
    rng = np.random.default_rng(seed)
    kind = rng.integers(0, len(ETH_KINDS), n).astype(np.uint8)
    frames, seeds = [], np.zeros(n, dtype=np.uint32)
    lens = imix_lengths(n, seed ^ 0x33)
    for i in range(n):
        k = ETH_KINDS[kind[i]]
        s = seed * 7919 + i
        if k.startswith("ipv4"):
            proto = {"ipv4_tcp": 6, "ipv4_udp": 17, "ipv4_icmp": 1, "ipv4_bad_version": 6, "ipv4_opt_tcp": 6,
                     "ipv4_opt_udp": 17, "ipv4_frag": 6, "ipv4_evil": 17}[k]
            ihl = int(rng.integers(6, 16)) if "opt" in k else 5
            fr = None
            if k == "ipv4_frag":       # first / middle / last fragments
                fr = int(rng.choice([0x2000, 0x2000 | int(rng.integers(1, 0x1FFF)), int(rng.integers(1, 0x1FFF))]))
            elif k == "ipv4_evil":
                fr = 0x8000 | 0x4000
            b, _, _ = ipv4_batch(np.array([max(int(lens[i]), 4 * ihl + 28)], np.uint32), seed=s, proto=proto, eth=True,
                                 ihl=ihl, frag=fr)
            if k == "ipv4_bad_version":
                b[14] = 0x65
        elif k.startswith("ipv6"):
            proto = 6 if ("tcp" in k or k == "ipv6_frag") else 17 if "udp" in k else 58
            fr = (int(rng.integers(0, 200)) << 3) | int(rng.integers(0, 2)) if k == "ipv6_frag" else None
            b, _, _, sd = ipv6_batch(np.array([max(int(lens[i]) + 20, 68)], np.uint32), seed=s, proto=proto,
                                     eth=True, hbh="hbh" in k, icmp_type=int(rng.choice([128, 129, 135, 136, 143])),
                                     frag=fr, destopt=k == "ipv6_dst_tcp", walked=k in ("ipv6_frag", "ipv6_dst_tcp"))
            seeds[i] = sd[0]
            if proto != 58 and rng.random() < 0.6:
                b[14 + 9] = proto        # the byte pico_transport_crc_check dispatches on (pico_socket.c:1923)
        elif k == "arp":
            b = random_bytes(s, 60)
            b[12], b[13] = 0x08, 0x06
        else:
            b = random_bytes(s, int(rng.integers(60, 300)))
            b[12], b[13] = 0x88, 0xCC
        d = int(rng.integers(0, 10))
        dst = (mac if d < 5 else b"\xff" * 6 if d == 5 else bytes([0x01, 0x00, 0x5e, 1, 2, 3]) if d == 6
               else bytes([0x33, 0x33, 0, 0, 0, 1]) if d == 7 else bytes([0x02, 0x11, 0x22, 0x33, 0x44, 0x55]))
        b[0:6] = np.frombuffer(dst, np.uint8)
        frames.append(b)
    gaps = rng.integers(0, 4, n)
    off = np.zeros(n, dtype=np.uint64)
    pos = 0
    for i in range(n):
        pos += int(gaps[i])
        off[i] = pos
        pos += frames[i].size
    buf = random_bytes(seed ^ 0xE7, pos + 16)
    for i in range(n):
        buf[int(off[i]):int(off[i]) + frames[i].size] = frames[i]
    flen = np.array([f.size for f in frames], dtype=np.uint32)
    return buf, off, flen, seeds, kind


def _ones_sum(data: np.ndarray, seed: int = 0) -> int:
    """pico_checksum_adder over data (LE 16-bit words, odd trailing byte low), mod 2^32."""
    n = data.size
    s = int(data[: n & ~1].view("<u2").astype(np.uint64).sum()) if n >= 2 else 0
    if n & 1:
        s += int(data[-1])
    return (seed + s) & 0xFFFFFFFF


def _finalize(s: int) -> int:
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    c = ~s & 0xFFFF
    return ((c >> 8) | (c << 8)) & 0xFFFF


def ipv4_fragments(lengths, seed: int = 21, proto: int = 17, frag_payload: int = 1480, shuffle: bool = True,
                   valid: bool = True):
    """IPv4 datagrams of the given TRANSPORT lengths, each split into fragments of
    `frag_payload` bytes (a multiple of 8; the last one shorter) as a sender's
    pico_ipv4_fragment / an MTU-1500 path produces them, every fragment an IPv4 frame
    (14-byte Ethernet gap, 20-byte header: tot = 20 + payload, frag = MF | offset/8, same
    id / src / dst / proto).  With `valid` the transport carries a correct TCP / UDP
    checksum over the whole datagram.  Fragments of a datagram are placed in the buffer
    (and listed) in a seeded arrival order when `shuffle`.
    Returns (buffer, frag offsets uint64 (-> IPv4 header), frag bytes uint32, groups
    uint32[n, 2] = (first descriptor, count) per datagram)."""
    lengths = np.asarray(lengths, dtype=np.uint32)
    assert frag_payload % 8 == 0 and frag_payload > 0
    rng = np.random.default_rng(seed)
    pieces, groups = [], []
    for g, L in enumerate(lengths.tolist()):
        t = random_bytes(seed * 1000003 + g, L)
        src = bytes([10, int(rng.integers(256)), int(rng.integers(256)), 1])
        dst = bytes([192, 168, int(rng.integers(256)), 2])
        if proto == 6 and L >= 20:
            t[12], t[13], t[16], t[17] = 0x50, 0x18, 0, 0
        if proto == 17 and L >= 8:
            t[4], t[5], t[6], t[7] = (L >> 8) & 0xFF, L & 0xFF, 0, 0
        if valid and proto in (6, 17) and L >= (20 if proto == 6 else 8):
            ph = np.frombuffer(src + dst + bytes([0, proto, (L >> 8) & 0xFF, L & 0xFF]), np.uint8)
            c = _finalize(_ones_sum(t, _ones_sum(ph)))
            x = 16 if proto == 6 else 6
            t[x], t[x + 1] = c >> 8, c & 0xFF
        ident = int(rng.integers(1, 65536))
        offs = list(range(0, max(L, 1), frag_payload)) if L else [0]
        frs = []
        for o in offs:
            pl = min(frag_payload, L - o)
            h = np.zeros(20, np.uint8)
            h[0], h[2], h[3] = 0x45, ((20 + pl) >> 8) & 0xFF, (20 + pl) & 0xFF
            h[4], h[5], h[8], h[9] = ident >> 8, ident & 0xFF, 64, proto
            fr = (o >> 3) | (0x2000 if o + pl < L else 0)
            h[6], h[7] = fr >> 8, fr & 0xFF
            h[12:16] = np.frombuffer(src, np.uint8)
            h[16:20] = np.frombuffer(dst, np.uint8)
            frs.append(np.concatenate([h, t[o:o + pl]]))
        if shuffle:
            frs = [frs[i] for i in rng.permutation(len(frs))]
        groups.append((len(pieces), len(frs)))
        pieces.extend(frs)
    n = len(pieces)
    place = rng.permutation(n) if shuffle else np.arange(n)
    off = np.zeros(n, dtype=np.uint64)
    pos = 0
    for j in place.tolist():
        pos += 14
        off[j] = pos
        pos += pieces[j].size
    buf = random_bytes(seed ^ 0xF4A6, pos + 16)
    for j in range(n):
        buf[int(off[j]):int(off[j]) + pieces[j].size] = pieces[j]
    flen = np.array([p.size for p in pieces], dtype=np.uint32)
    return buf, off, flen, np.array(groups, dtype=np.uint32).reshape(-1, 2)


def ipv6_fragments(lengths, seed: int = 23, proto: int = 6, frag_payload: int = 1448, shuffle: bool = True,
                   valid: bool = True, hbh: bool = False, b9_proto: bool = True):
    """IPv6 datagrams of the given TRANSPORT lengths, each split into fragments of
    `frag_payload` bytes (a multiple of 8; the last one shorter) as pico_ipv6_frag_send / an
    MTU-1500 path produces them: every fragment an IPv6 frame (14-byte Ethernet gap, 40-byte
    header, an optional 8-byte hop-by-hop header (PadN) when `hbh`, the 8-byte fragment header:
    next header = proto, offset | M, a per-datagram id; payload length = the rest), same src /
    dst.  With `valid` the transport carries a correct TCP / UDP / ICMPv6 checksum over the whole
    datagram; `b9_proto` puts proto into header byte 9 (the source address's second byte, which
    pico_transport_crc_check dispatches on).  Fragments of a datagram are placed (and listed) in
    a seeded arrival order when `shuffle`.
    Returns (buffer, frag offsets uint64 (-> IPv6 header), frag bytes uint32, groups uint32[n, 2])."""
    lengths = np.asarray(lengths, dtype=np.uint32)
    assert frag_payload % 8 == 0 and frag_payload > 0
    rng = np.random.default_rng(seed)
    pieces, groups = [], []
    for g, L in enumerate(lengths.tolist()):
        t = random_bytes(seed * 1000003 + g, L)
        src = bytearray(random_bytes(seed * 7 + g, 16).tobytes())
        dst = bytes(random_bytes(seed * 11 + g, 16).tobytes())
        if b9_proto:
            src[1] = proto
        src = bytes(src)
        x = {6: 16, 17: 6, 58: 2}.get(proto)
        if proto == 6 and L >= 20:
            t[12], t[13], t[16], t[17] = 0x50, 0x18, 0, 0
        if proto == 17 and L >= 8:
            t[4], t[5], t[6], t[7] = (L >> 8) & 0xFF, L & 0xFF, 0, 0
        if proto == 58 and L >= 4:
            t[0], t[2], t[3] = 128, 0, 0
        if valid and x is not None and L >= x + 2:
            ph = np.frombuffer(src + dst + L.to_bytes(4, "big") + bytes([0, 0, 0, proto]), np.uint8)
            c = _finalize(_ones_sum(t, _ones_sum(ph)))
            t[x], t[x + 1] = c >> 8, c & 0xFF
        ident = int(rng.integers(1, 1 << 32))
        offs = list(range(0, max(L, 1), frag_payload)) if L else [0]
        frs = []
        for o in offs:
            pl = min(frag_payload, L - o)
            ext = 16 if hbh else 8
            h = np.zeros(40 + ext, np.uint8)
            h[0] = 0x60
            plen = ext + pl
            h[4], h[5] = plen >> 8, plen & 0xFF
            h[6], h[7] = (0 if hbh else 44), 64
            h[8:24] = np.frombuffer(src, np.uint8)
            h[24:40] = np.frombuffer(dst, np.uint8)
            f = 40
            if hbh:
                h[40:48] = [44, 0, 1, 4, 0, 0, 0, 0]
                f = 48
            om = o | (1 if o + pl < L else 0)
            h[f:f + 8] = [proto, 0, om >> 8, om & 0xFF, ident >> 24, (ident >> 16) & 0xFF, (ident >> 8) & 0xFF,
                          ident & 0xFF]
            frs.append(np.concatenate([h, t[o:o + pl]]))
        if shuffle:
            frs = [frs[i] for i in rng.permutation(len(frs))]
        groups.append((len(pieces), len(frs)))
        pieces.extend(frs)
    n = len(pieces)
    place = rng.permutation(n) if shuffle else np.arange(n)
    off = np.zeros(n, dtype=np.uint64)
    pos = 0
    for j in place.tolist():
        pos += 14
        off[j] = pos
        pos += pieces[j].size
    buf = random_bytes(seed ^ 0xF6A6, pos + 16)
    for j in range(n):
        buf[int(off[j]):int(off[j]) + pieces[j].size] = pieces[j]
    flen = np.array([p.size for p in pieces], dtype=np.uint32)
    return buf, off, flen, np.array(groups, dtype=np.uint32).reshape(-1, 2)


def fragtx_count(length: int, mtu: int) -> int:
    """Fragments pico_ipv4_fragment_batch_dev emits for a datagram of `length` bytes (header
    included): 1 when it fits the MTU, else ceil(transport / per), per = (mtu - 20) & ~7."""
    per = (mtu - 20) & ~7
    return 1 if length <= mtu else -(-(length - 20) // per)


def ipv4_oversized(lengths, mtu: int = 1500, stride: int = 1504, seed: int = 31, proto=17, align=0, out_off: int = 12,
                   spare: int = 0):
    """Unfragmented IPv4 datagrams of the given TRANSPORT lengths (a 20-byte header, IHL 5, len /
    frag / crc fields arbitrary: the fragmentation batch does not read them) for
    pico_ipv4_fragment_batch_dev, with the arrays that place its output.  proto: one value or one
    per datagram (6 / 17 / 1 get a plausible transport header with an arbitrary crc field);
    align: the header's address mod 16 in the buffer, one value or one per datagram.  Output
    regions are laid out back to back, each starting at out_off mod 16 and holding exactly the
    fragments at `stride`; every group reserves its fragment count + `spare` slots.
    Returns (buffer, dgram offsets uint64, dgram bytes uint32, groups uint32[n, 2] = (first slot,
    slots reserved), out offsets uint64, out capacities uint32, n_frag, out_len)."""
    lengths = np.asarray(lengths, dtype=np.uint32)
    n = lengths.size
    protos = np.broadcast_to(np.asarray(proto, dtype=np.uint8), (n,))
    aligns = np.broadcast_to(np.asarray(align, dtype=np.uint32), (n,))
    rng = np.random.default_rng(seed)
    per = (mtu - 20) & ~7
    off = np.zeros(n, np.uint64)
    pos = 0
    pieces = []
    for g, L in enumerate(lengths.tolist()):
        pr = int(protos[g])
        h = rng.integers(0, 256, 20, dtype=np.uint8)
        h[0], h[8], h[9] = 0x45, 64, pr
        h[12:16] = [10, int(rng.integers(256)), int(rng.integers(256)), 1]
        h[16:20] = [192, 168, int(rng.integers(256)), 2]
        t = random_bytes(seed * 1000003 + g, L)
        if pr == 6 and L >= 20:
            t[12], t[13] = 0x50, 0x18
        if pr == 17 and L >= 8:
            t[4], t[5] = (L >> 8) & 0xFF, L & 0xFF
        if pr == 1 and L >= 8:
            t[0], t[1] = 8, 0
        pos += (int(aligns[g]) - pos) % 16
        off[g] = pos
        pieces.append(np.concatenate([h, t]))
        pos += 20 + L
    buf = random_bytes(seed ^ 0x7F4A, pos + 16)
    for g in range(n):
        buf[int(off[g]):int(off[g]) + pieces[g].size] = pieces[g]
    dlen = lengths + 20
    cnt = np.array([fragtx_count(int(x), mtu) for x in dlen.tolist()], np.uint32)
    reserved = cnt + np.uint32(spare)
    first = np.concatenate([[0], np.cumsum(reserved[:-1])]).astype(np.uint32)
    groups = np.stack([first, reserved], axis=1).astype(np.uint32)
    last = np.where(cnt == 1, dlen, 20 + (lengths - (cnt - 1) * per)).astype(np.int64)
    cap = ((cnt.astype(np.int64) - 1) * stride + last).astype(np.uint32)
    ooff = np.zeros(n, np.uint64)
    pos = 0
    for g in range(n):
        pos += (out_off - pos) % 16
        ooff[g] = pos
        pos += int(cap[g])
    return buf, off, dlen.astype(np.uint32), groups, ooff, cap, int(reserved.sum()), pos + 16


def fragtx6_count(length: int, mtu: int) -> int:
    """Fragments pico_ipv6_fragment_batch_dev emits for a datagram of `length` bytes (the 40-byte
    header included): 1 when it fits the MTU, else ceil(transport / per), per = (mtu - 48) & ~7."""
    per = (mtu - 48) & ~7
    return 1 if length <= mtu else -(-(length - 40) // per)


def ipv6_oversized(lengths, mtu: int = 1500, stride: int = 1504, seed: int = 61, proto=17, align=0, out_off: int = 0,
                   spare: int = 0, b9_proto: bool = False):
    """Unfragmented IPv6 datagrams of the given TRANSPORT lengths (the 40-byte fixed header, no
    extension headers, the payload-length field arbitrary: the fragmentation batch does not read
    it) for pico_ipv6_fragment_batch_dev, with the arrays that place its output.  proto: one value or
    one per datagram (6 / 17 / 58 get a plausible transport header with an arbitrary crc field);
    align: the header's address mod 16 in the buffer, one value or one per datagram; b9_proto puts
    proto into header byte 9 (the source address's second byte, which the reference's
    pico_transport_crc_check dispatches on).  Output regions are laid out back to back, each
    starting at out_off mod 16 and holding exactly the fragments at `stride`; every group reserves
    its fragment count + `spare` slots.
    Returns (buffer, dgram offsets uint64, dgram bytes uint32, ids uint32 (the descriptors' seed),
    groups uint32[n, 2] = (first slot, slots reserved), out offsets uint64, out capacities uint32,
    n_frag, out_len)."""
    lengths = np.asarray(lengths, dtype=np.uint32)
    n = lengths.size
    protos = np.broadcast_to(np.asarray(proto, dtype=np.uint8), (n,))
    aligns = np.broadcast_to(np.asarray(align, dtype=np.uint32), (n,))
    rng = np.random.default_rng(seed)
    per = (mtu - 48) & ~7
    off = np.zeros(n, np.uint64)
    pos = 0
    pieces = []
    for g, L in enumerate(lengths.tolist()):
        pr = int(protos[g])
        t = random_bytes(seed * 1000003 + g, L)
        if pr == 6 and L >= 20:
            t[12], t[13] = 0x50, 0x18
        if pr == 17 and L >= 8:
            t[4], t[5] = (L >> 8) & 0xFF, L & 0xFF
        if pr == 58 and L >= 4:
            t[0], t[1] = 128, 0
        f = ipv6_datagram(rng, pr, t, hop=255 if pr == 58 else 64)
        f[4:6] = rng.integers(0, 256, 2, dtype=np.uint8)
        if b9_proto:
            f[9] = pr
        pos += (int(aligns[g]) - pos) % 16
        off[g] = pos
        pieces.append(f)
        pos += 40 + L
    buf = random_bytes(seed ^ 0x7F6A, pos + 16)
    for g in range(n):
        buf[int(off[g]):int(off[g]) + pieces[g].size] = pieces[g]
    ids = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    dlen = lengths + 40
    cnt = np.array([fragtx6_count(int(x), mtu) for x in dlen.tolist()], np.uint32)
    reserved = cnt + np.uint32(spare)
    first = np.concatenate([[0], np.cumsum(reserved[:-1])]).astype(np.uint32)
    groups = np.stack([first, reserved], axis=1).astype(np.uint32)
    last = np.where(cnt == 1, dlen, 48 + (lengths - (cnt - 1) * per)).astype(np.int64)
    cap = ((cnt.astype(np.int64) - 1) * stride + last).astype(np.uint32)
    ooff = np.zeros(n, np.uint64)
    pos = 0
    for g in range(n):
        pos += (out_off - pos) % 16
        ooff[g] = pos
        pos += int(cap[g])
    return buf, off, dlen.astype(np.uint32), ids, groups, ooff, cap, int(reserved.sum()), pos + 16


def tcpseg_count(payload: int, per: int) -> int:
    """Segments pico_tcp_segment_batch_dev emits for `payload` bytes at `per` bytes a segment:
    max(1, ceil(payload / per)) -- no payload is one bare-header frame."""
    return max(1, -(-payload // per))


def tcp_streams(lengths, family=4, thl=20, per=1448, stride: int = 1504, seed: int = 51, align=0, out_off=12,
                spare: int = 0, seq=None, ident=None):
    """Send units for pico_tcp_segment_batch_dev: per stream a network header (family 4: IPv4, IHL 5;
    6: IPv6, no extension header), a TCP header of `thl` bytes (PSH|ACK, options arbitrary) and
    `lengths[g]` payload bytes, contiguous; the fields the batch does not read (IPv4 len / frag /
    crc, IPv6 payload length, TCP crc) are arbitrary.  family, thl, per, align (the header's address
    mod 16 in the buffer), seq and ident (template seq / IPv4 id; random when None): one value or one
    per stream.  Output regions are laid out back to back, each starting at out_off mod 16 (one value
    or one per stream) and holding exactly the segments at `stride`; every group reserves its segment
    count + `spare` slots.
    Returns (buffer, stream offsets uint64, stream bytes uint32, per uint32[n], groups uint32[n, 2] =
    (first slot, slots reserved), out offsets uint64, out capacities uint32, n_seg, out_len)."""
    lengths = np.asarray(lengths, dtype=np.int64)
    n = lengths.size
    fam = np.broadcast_to(np.asarray(family, dtype=np.uint32), (n,))
    thls = np.broadcast_to(np.asarray(thl, dtype=np.uint32), (n,))
    pers = np.broadcast_to(np.asarray(per, dtype=np.uint32), (n,)).copy()
    aligns = np.broadcast_to(np.asarray(align, dtype=np.uint32), (n,))
    rng = np.random.default_rng(seed)
    seqs = rng.integers(0, 1 << 32, n, dtype=np.uint64) if seq is None else np.broadcast_to(np.asarray(seq, np.uint64), (n,))
    ids = rng.integers(0, 1 << 16, n, dtype=np.uint32) if ident is None else np.broadcast_to(np.asarray(ident, np.uint32), (n,))
    off = np.zeros(n, np.uint64)
    hl = np.zeros(n, np.int64)
    pos = 0
    pieces = []
    for g, L in enumerate(lengths.tolist()):
        tl = int(thls[g])
        if int(fam[g]) == 6:
            h = rng.integers(0, 256, 40, dtype=np.uint8)
            h[0], h[6], h[7] = 0x60 | (int(h[0]) & 15), 6, 64
        else:
            h = rng.integers(0, 256, 20, dtype=np.uint8)
            h[0], h[8], h[9] = 0x45, 64, 6
            h[4], h[5] = int(ids[g]) >> 8, int(ids[g]) & 0xFF
            h[12:16] = [10, int(rng.integers(256)), int(rng.integers(256)), 1]
            h[16:20] = [192, 168, int(rng.integers(256)), 2]
        t = rng.integers(0, 256, tl, dtype=np.uint8)
        t[4:8] = [(int(seqs[g]) >> s) & 0xFF for s in (24, 16, 8, 0)]
        t[12], t[13] = (tl // 4) << 4, 0x18
        pos += (int(aligns[g]) - pos) % 16
        off[g] = pos
        hl[g] = h.size + tl
        pieces.append(np.concatenate([h, t, random_bytes(seed * 1000003 + g, L)]))
        pos += pieces[-1].size
    buf = random_bytes(seed ^ 0x7C95, pos + 16)
    for g in range(n):
        buf[int(off[g]):int(off[g]) + pieces[g].size] = pieces[g]
    cnt = np.array([tcpseg_count(int(L), int(p)) for L, p in zip(lengths.tolist(), pers.tolist())], np.int64)
    reserved = (cnt + spare).astype(np.uint32)
    first = np.concatenate([[0], np.cumsum(reserved[:-1])]).astype(np.uint32)
    groups = np.stack([first, reserved], axis=1).astype(np.uint32)
    last = hl + lengths - (cnt - 1) * pers.astype(np.int64)
    cap = ((cnt - 1) * stride + last).astype(np.uint32)
    ooffs = np.broadcast_to(np.asarray(out_off, dtype=np.int64), (n,))
    ooff = np.zeros(n, np.uint64)
    pos = 0
    for g in range(n):
        pos += (int(ooffs[g]) - pos) % 16
        ooff[g] = pos
        pos += int(cap[g])
    return buf, off, (hl + lengths).astype(np.uint32), pers, groups, ooff, cap, int(reserved.sum()), pos + 16


def tcp_rx_frame(rng, seq: int, payload, family: int = 4, thl: int = 20, flags: int = 0x18, ihl: int = 5) -> np.ndarray:
    """One received TCP frame as the wire delivers it, every checksum valid: an IPv4 header of
    4 * ihl bytes (DF, options arbitrary) or a 40-byte IPv6 header (no extension header), a TCP
    header of `thl` bytes (seq, flags; ports, ack, window and options from rng) and the payload."""
    payload = np.asarray(payload, dtype=np.uint8)
    tl = thl + payload.size
    t = rng.integers(0, 256, thl, dtype=np.uint8)
    t[4:8] = [(seq >> s) & 0xFF for s in (24, 16, 8, 0)]
    t[12], t[13], t[16], t[17] = (thl // 4) << 4, flags, 0, 0
    if family == 6:
        h = rng.integers(0, 256, 40, dtype=np.uint8)
        h[0], h[4], h[5], h[6], h[7] = 0x60 | (int(h[0]) & 15), tl >> 8, tl & 0xFF, 6, 64
        ph = np.concatenate([h[8:40], np.array([0, 0, tl >> 8, tl & 0xFF, 0, 0, 0, 6], np.uint8)])
    else:
        h = rng.integers(0, 256, 4 * ihl, dtype=np.uint8)
        tot = 4 * ihl + tl
        h[0], h[2], h[3], h[6], h[7], h[8], h[9], h[10], h[11] = 0x40 | ihl, tot >> 8, tot & 0xFF, 0x40, 0, 64, 6, 0, 0
        h[12:16] = [10, int(rng.integers(256)), int(rng.integers(256)), 1]
        h[16:20] = [192, 168, int(rng.integers(256)), 2]
        c = _finalize(_ones_sum(h))
        h[10], h[11] = c >> 8, c & 0xFF
        ph = np.concatenate([h[12:20], np.array([0, 6, tl >> 8, tl & 0xFF], np.uint8)])
    c = _finalize(_ones_sum(np.concatenate([t, payload]), _ones_sum(ph)))
    t[16], t[17] = c >> 8, c & 0xFF
    return np.concatenate([h, t, payload])


def tcp_rx_pack(conns, align=0, out_off: int = 0, seed: int = 81, slack=0):
    """The arrays of pico_tcp_coalesce_batch_dev for `conns`, a list of (frames, rcv_nxt, sack_ok,
    capacity) with frames in arrival order: the frames laid out one after another, frame i at `align`
    mod 16 (one value or one per frame, in batch order) with desc.len = its size + `slack` (one value
    or one per frame; negative: the descriptor ends inside the frame), output regions back to back,
    each at out_off mod 16.  Returns (buffer, seg offsets uint64, seg bytes uint32, groups uint32[n, 2]
    = (first, count), conn uint32[n, 2] = (rcv_nxt, cflags), out offsets uint64, out capacities
    uint32, out_len)."""
    frames = [f for c in conns for f in c[0]]
    m = len(frames)
    aligns = np.broadcast_to(np.asarray(align, dtype=np.int64), (m,))
    slacks = np.broadcast_to(np.asarray(slack, dtype=np.int64), (m,))
    off, ln = np.zeros(m, np.uint64), np.zeros(m, np.uint32)
    pos = 0
    for i, f in enumerate(frames):
        pos += (int(aligns[i]) - pos) % 16
        off[i] = pos
        ln[i] = f.size + int(slacks[i])
        pos += f.size + max(int(slacks[i]), 0)
    buf = random_bytes(seed ^ 0x3B1D, pos)
    for i, f in enumerate(frames):
        buf[int(off[i]):int(off[i]) + f.size] = f
    cnt = np.array([len(c[0]) for c in conns], np.uint32)
    first = np.concatenate([[0], np.cumsum(cnt[:-1])]).astype(np.uint32)
    groups = np.stack([first, cnt], axis=1).astype(np.uint32)
    conn = np.array([[c[1] & 0xFFFFFFFF, 1 if c[2] else 0] for c in conns], np.uint32).reshape(-1, 2)
    cap = np.array([c[3] for c in conns], np.uint32)
    ooff = np.zeros(len(conns), np.uint64)
    pos = 0
    for g in range(len(conns)):
        pos += (out_off - pos) % 16
        ooff[g] = pos
        pos += int(cap[g])
    return buf, off, ln, groups, conn, ooff, cap, pos + 16


def tcp_rx_bursts(n_conn: int, seed: int = 83, family=4, thl=32, per=1448, max_bytes: int = 12000, corrupt: bool = True):
    """Received-segment groups for pico_tcp_coalesce_batch_dev, each cut from one byte stream (the send
    segmentation's split: `per` payload bytes a segment): per connection an in-order run disturbed by
    swaps, exact duplicates, a retransmission of a byte range with another split, a hole (a segment
    lost: every later one is ahead of rcv_nxt) and, with `corrupt`, a flipped payload bit followed
    later by a good copy and a flipped IPv4 header bit.  family, thl, per: one value or one per
    connection.  Returns (conns for tcp_rx_pack with capacity = the stream's bytes, streams): streams[g]
    = the connection's whole byte stream, whose byte 0 has seq rcv_nxt."""
    rng = np.random.default_rng(seed)
    fam = np.broadcast_to(np.asarray(family), (n_conn,))
    thls = np.broadcast_to(np.asarray(thl), (n_conn,))
    pers = np.broadcast_to(np.asarray(per), (n_conn,))
    conns, streams = [], []
    for g in range(n_conn):
        f, t, p = int(fam[g]), int(thls[g]), int(pers[g])
        P = int(rng.integers(1, max_bytes // 2))
        data = random_bytes(seed * 1000003 + g, P)
        rcv = int(rng.integers(0, 1 << 32)) if g % 5 else (1 << 32) - int(rng.integers(1, P + 1))
        mk = lambda a, b: tcp_rx_frame(rng, (rcv + a) & 0xFFFFFFFF, data[a:b], f, t, 0x18 if (a // p) % 2 else 0x10)
        cuts = [(a, min(a + p, P)) for a in range(0, P, p)]
        frames = [mk(a, b) for a, b in cuts]
        for _ in range(int(rng.integers(0, 3))):                     # swaps
            if len(frames) > 1:
                i = int(rng.integers(0, len(frames) - 1))
                frames[i], frames[i + 1] = frames[i + 1], frames[i]
        for _ in range(int(rng.integers(0, 3))):                     # exact duplicates
            i = int(rng.integers(0, len(frames)))
            frames.insert(int(rng.integers(i, len(frames) + 1)), frames[i].copy())
        if P > 3 and rng.integers(2):                                # a retransmission with another split
            a = int(rng.integers(0, P - 2))
            b = int(rng.integers(a + 1, P + 1))
            q = max(1, (b - a) // int(rng.integers(1, 4)))
            at = int(rng.integers(0, len(frames) + 1))
            for k, x in enumerate(range(a, b, q)):
                frames.insert(at + k, mk(x, min(x + q, b)))
        if len(cuts) > 2 and rng.integers(3) == 0:                   # a hole: the first copy of a segment is lost
            frames.pop(int(rng.integers(1, len(frames))))
        if corrupt and rng.integers(2):                              # a flipped payload bit, a good copy later
            i = int(rng.integers(0, len(frames)))
            bad = frames[i].copy()
            bad[-1 - int(rng.integers(0, min(8, bad.size - (40 if f == 6 else 20) - t)))] ^= 1 << int(rng.integers(8))
            good = frames[i]
            frames[i] = bad
            frames.insert(int(rng.integers(i + 1, len(frames) + 1)), good)
        if corrupt and f == 4 and rng.integers(2):                   # a flipped IPv4 header bit
            i = int(rng.integers(0, len(frames)))
            frames[i] = frames[i].copy()
            frames[i][8] ^= 0x10                                     # (the TTL: only the header checksum sees it)
        conns.append((frames, rcv, bool(rng.integers(2)), P))
        streams.append(data)
    return conns, streams


def tcp_ack_inputs(conns, seed: int = 89, space=16384, ts_ok=None, region: int = 100, out_off=0, align=0):
    """What pico_tcp_ack_batch_dev takes beside the coalescing's arrays, for `conns` (tcp_rx_bursts' /
    tcp_rx_pack's list): per connection a header template answering its first frame -- the network
    header with the addresses swapped (IPv4: IHL 5, its own id, ttl 64; IPv6: no extension header) and
    a 20-byte TCP header with the ports swapped, a random seq (snd_nxt) and random bytes in the fields
    the batch does not read -- at `align` mod 16 (one value or one per connection), and a
    pico_csum_tcp_ack record (space: one value or one per connection; ts_ok: likewise, None = seeded).
    Output regions of `region` bytes back to back, each at out_off mod 16 (one value or one per
    connection).  Returns (template buffer,
    template offsets uint64, template bytes uint32, ack records as a structured array (space, tsval,
    tsecr, aflags), out offsets uint64, out capacities uint32, out_len)."""
    rng = np.random.default_rng(seed)
    n = len(conns)
    aligns = np.broadcast_to(np.asarray(align, dtype=np.int64), (n,))
    spaces = np.broadcast_to(np.asarray(space, dtype=np.uint32), (n,))
    tss = rng.integers(0, 2, n) if ts_ok is None else np.broadcast_to(np.asarray(ts_ok, dtype=np.int64), (n,))
    ack = np.zeros(n, np.dtype([("space", "<u4"), ("tsval", "<u4"), ("tsecr", "<u4"), ("aflags", "<u4")]))
    ack["space"], ack["aflags"] = spaces, tss
    ack["tsval"] = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    ack["tsecr"] = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    pieces, off, ln = [], np.zeros(n, np.uint64), np.zeros(n, np.uint32)
    pos = 0
    for g, c in enumerate(conns):
        f = np.asarray(c[0][0], dtype=np.uint8)
        if int(f[0]) >> 4 == 6:
            h = f[:40].copy()
            h[8:24], h[24:40] = f[24:40], f[8:24]
            h[4:6] = rng.integers(0, 256, 2, dtype=np.uint8)          # (payload length: not read)
            t0 = 40
        else:
            h = rng.integers(0, 256, 20, dtype=np.uint8)              # (len, frag, crc: not read)
            h[0], h[1], h[8], h[9] = 0x45, f[1], 64, 6
            h[12:16], h[16:20] = f[16:20], f[12:16]
            t0 = 4 * (int(f[0]) & 15)
        t = rng.integers(0, 256, 20, dtype=np.uint8)                  # (ack, thl, flags, rwnd, crc: not read)
        t[0:2], t[2:4] = f[t0 + 2:t0 + 4], f[t0:t0 + 2]
        pos += (int(aligns[g]) - pos) % 16
        off[g], ln[g] = pos, h.size + 20
        pieces.append(np.concatenate([h, t]))
        pos += pieces[-1].size
    buf = random_bytes(seed ^ 0x51C3, pos + 16)
    for g in range(n):
        buf[int(off[g]):int(off[g]) + pieces[g].size] = pieces[g]
    ooffs = np.broadcast_to(np.asarray(out_off, dtype=np.int64), (n,))
    ooff = np.zeros(n, np.uint64)
    pos = 0
    for g in range(n):
        pos += (int(ooffs[g]) - pos) % 16
        ooff[g] = pos
        pos += region
    return buf, off, ln, ack, ooff, np.full(n, region, np.uint32), pos + 16


def icmp4_echo_request(rng, T: int, ident: int = 0, seq: int = 0, ihl: int = 5, frag: int = 0x4000, src=None, dst=None,
                       icmp_type: int = 8, bad_crc: bool = False) -> np.ndarray:
    """One IPv4 datagram with an ICMP message of T >= 8 transport bytes (type 8: an echo request) behind
    4 * ihl header bytes (options: random bytes), both checksums valid unless bad_crc flips a bit of the
    ICMP one."""
    hl = 4 * ihl
    f = np.zeros(hl + T, np.uint8)
    f[0], f[1], f[8], f[9] = 0x40 | ihl, int(rng.integers(256)), int(rng.integers(1, 256)), 1
    f[2], f[3] = (hl + T) >> 8, (hl + T) & 0xFF
    f[4:6] = rng.integers(0, 256, 2, dtype=np.uint8)
    f[6], f[7] = frag >> 8, frag & 0xFF
    f[12:16] = rng.integers(1, 224, 4, dtype=np.uint8) if src is None else np.frombuffer(bytes(src), np.uint8)
    f[16:20] = rng.integers(1, 224, 4, dtype=np.uint8) if dst is None else np.frombuffer(bytes(dst), np.uint8)
    f[20:hl] = rng.integers(0, 256, hl - 20, dtype=np.uint8)
    c = _csum16(f[:hl])
    f[10], f[11] = c >> 8, c & 0xFF
    t = f[hl:]
    t[8:] = rng.integers(0, 256, T - 8, dtype=np.uint8)
    t[0], t[1] = icmp_type, 0
    t[4], t[5], t[6], t[7] = ident >> 8, ident & 0xFF, seq >> 8, seq & 0xFF
    c = _csum16(t)
    t[2], t[3] = c >> 8, c & 0xFF
    if bad_crc:
        t[3] ^= 0x10
    return f


def _csum16(b: np.ndarray) -> int:
    """The Internet checksum of b as the big-endian field value (numpy; the builders' own, not the oracle's)."""
    a = np.asarray(b, dtype=np.uint8)
    if a.size & 1:
        a = np.concatenate([a, np.zeros(1, np.uint8)])
    s = int((a[0::2].astype(np.uint64) << 8).sum() + a[1::2].astype(np.uint64).sum())
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return ~s & 0xFFFF


def icmp4_burst(dgrams, types, codes=0, seed: int = 97, align=0, slack=0, out_off=0, region=None, local=(10, 0, 0, 1)):
    """The inputs of pico_icmp4_reply_batch_dev for the datagrams `dgrams` (uint8 arrays, the IPv4 header
    first): record i answers datagram i with types[i] (0: echo; 3 / 11 / 12: that notice, codes[i]).  The
    datagrams lie in one buffer at `align` mod 16 each with `slack` readable bytes behind (desc.len =
    bytes + slack; a negative slack cuts the descriptor short), the answers' regions back to back at
    `out_off` mod 16 each, `region` bytes or -- None -- exactly the answer's size (tight).  align, slack,
    out_off, codes: one value or one per record.  Returns (buffer, offsets uint64, lengths uint32, req
    records (src, id, type, code), out offsets uint64, out capacities uint32, out_len = 16 bytes past the last region)."""
    n = len(dgrams)
    rng = np.random.default_rng(seed)
    bc = lambda x: np.broadcast_to(np.asarray(x, dtype=np.int64), (n,))
    aligns, slacks, ooffs, cds, tps = bc(align), bc(slack), bc(out_off), bc(codes), bc(types)
    off, ln = np.zeros(n, np.uint64), np.zeros(n, np.uint32)
    pos = 0
    for i, f in enumerate(dgrams):
        pos += (int(aligns[i]) - pos) % 16
        off[i], ln[i] = pos, len(f) + int(slacks[i])
        pos += len(f) + max(int(slacks[i]), 0)
    buf = random_bytes(seed ^ 0x1C3F, pos)
    for i, f in enumerate(dgrams):
        buf[int(off[i]):int(off[i]) + len(f)] = f
    req = np.zeros(n, np.dtype([("src", "<u4"), ("id", "<u2"), ("type", "u1"), ("code", "u1")]))
    req["src"] = int.from_bytes(bytes(local), "little")
    req["id"] = (int(rng.integers(0, 1 << 16)) + np.arange(n)) & 0xFFFF
    req["type"], req["code"] = tps, cds
    cap = np.zeros(n, np.uint32)
    for i, f in enumerate(dgrams):
        tot = (int(f[2]) << 8 | int(f[3])) if len(f) >= 4 else 0
        need = 20 + max(tot - 4 * (int(f[0]) & 15), 0) if tps[i] == 0 else 28 + min(tot, 28)
        cap[i] = need if region is None else region
    ooff = np.zeros(n, np.uint64)
    pos = 0
    for i in range(n):
        pos += (int(ooffs[i]) - pos) % 16
        ooff[i] = pos
        pos += int(cap[i])
    return buf, off, ln, req, ooff, cap, pos + 16


def _csum16_v6(src, dst, nxt: int, t: np.ndarray) -> int:
    """The Internet checksum of transport t behind the IPv6 pseudo header (src, dst, long_be(len), 0 0 0, nxt)."""
    ps = np.concatenate([np.asarray(src, np.uint8), np.asarray(dst, np.uint8),
                         np.frombuffer(int(t.size).to_bytes(4, "big") + bytes([0, 0, 0, nxt]), np.uint8)])
    return _csum16(np.concatenate([ps, t]))             # (the 40 pseudo bytes keep t's 16-bit pairing)


def ipv6_datagram(rng, nxt: int, transport: np.ndarray, src=None, dst=None, hbh: bool = False, hop: int = 64,
                  ext: bytes = b"", first: int | None = None) -> np.ndarray:
    """One IPv6 datagram: the 40-byte header, an 8-byte hop-by-hop header (PadN) when `hbh` -- or the raw
    extension headers `ext`, the fixed header naming `first` as its next one --, then `transport` as it is."""
    if hbh:
        ext, first = bytes([nxt, 0, 1, 4, 0, 0, 0, 0]), 0
    f = np.zeros(40 + len(ext) + transport.size, np.uint8)
    f[0] = 0x60
    f[1:4] = rng.integers(0, 256, 3, dtype=np.uint8) & np.array([0x0F, 0xFF, 0xFF], np.uint8)
    f[4], f[5] = (f.size - 40) >> 8, (f.size - 40) & 0xFF
    f[6], f[7] = (nxt if first is None else first), hop
    for k, a in ((8, src), (24, dst)):
        f[k:k + 16] = rng.integers(0, 256, 16, dtype=np.uint8) if a is None else np.frombuffer(bytes(a), np.uint8)
        if a is None:
            f[k] = 0x20                                   # (global unicast: never multicast by chance)
    f[40:40 + len(ext)] = np.frombuffer(bytes(ext), np.uint8)
    f[40 + len(ext):] = transport
    return f


def icmp6_echo_request(rng, T: int, ident: int = 0, seq: int = 0, src=None, dst=None, hbh: bool = False,
                       icmp_type: int = 128, bad_crc: bool = False) -> np.ndarray:
    """One IPv6 datagram with an ICMPv6 message of T >= 8 transport bytes (type 128: an echo request), behind
    a hop-by-hop header when `hbh`; the checksum over the pseudo header is valid unless bad_crc flips a bit."""
    t = np.zeros(T, np.uint8)
    t[8:] = rng.integers(0, 256, T - 8, dtype=np.uint8)
    t[0] = icmp_type
    t[4], t[5], t[6], t[7] = ident >> 8, ident & 0xFF, seq >> 8, seq & 0xFF
    f = ipv6_datagram(rng, 58, t, src, dst, hbh)
    c = _csum16_v6(f[8:24], f[24:40], 58, t)
    f[f.size - T + 2], f[f.size - T + 3] = c >> 8, (c & 0xFF) ^ (0x10 if bad_crc else 0)
    return f


def udp6_datagram(rng, payload: int, sport: int = 4000, dport: int = 4001, src=None, dst=None) -> np.ndarray:
    """One IPv6 datagram carrying UDP with `payload` random bytes and a valid checksum (a closed port's burst)."""
    t = np.zeros(8 + payload, np.uint8)
    t[0:6] = np.frombuffer(bytes([sport >> 8, sport & 0xFF, dport >> 8, dport & 0xFF, t.size >> 8, t.size & 0xFF]), np.uint8)
    t[8:] = rng.integers(0, 256, payload, dtype=np.uint8)
    f = ipv6_datagram(rng, 17, t, src, dst)
    c = _csum16_v6(f[8:24], f[24:40], 17, t) or 0xFFFF
    f[46], f[47] = c >> 8, c & 0xFF
    return f


def icmp6_answer_len(f, typ: int) -> int:
    """The answer pico_icmp6_reply_batch_dev writes for datagram f with record type typ, taking f as well
    formed: an echo's 40 + T behind 8 (hdr ext len + 1)-byte headers 0 / 43 / 60, a notice's 48 + min(40 +
    len field, 1232)."""
    plen = (int(f[4]) << 8 | int(f[5])) if len(f) >= 6 else 0
    if typ != 0:
        return 48 + min(40 + plen, 1232)
    nx, o = int(f[6]) if len(f) >= 7 else 58, 40
    while nx in (0, 43, 60) and o + 2 <= len(f):
        nx, o = int(f[o]), o + 8 * (int(f[o + 1]) + 1)
    return 40 + max(40 + plen - o, 0)


def icmp6_burst(dgrams, types, codes=0, args=0, hop=64, seed: int = 101, align=0, slack=0, out_off=0, region=None,
                local=bytes.fromhex("20010db8000000010000000000000001")):
    """The inputs of pico_icmp6_reply_batch_dev for the datagrams `dgrams` (uint8 arrays, the IPv6 header
    first): record i answers datagram i with types[i] (0: echo; 1 / 2 / 3 / 4: that notice, codes[i],
    args[i]).  Laid out as icmp4_burst does: the datagrams in one buffer at `align` mod 16 each with `slack`
    readable bytes behind (desc.len = bytes + slack; a negative slack cuts the descriptor short), the
    answers' regions back to back at `out_off` mod 16 each, `region` bytes or -- None -- exactly the answer's
    size (tight).  Returns (buffer, offsets uint64, lengths uint32, req records (src, arg, type, code, hop,
    rsvd), out offsets uint64, out capacities uint32, out_len = 16 bytes past the last region)."""
    n = len(dgrams)
    bc = lambda x: np.broadcast_to(np.asarray(x, dtype=np.int64), (n,))
    aligns, slacks, ooffs, cds, tps, ags, hops = bc(align), bc(slack), bc(out_off), bc(codes), bc(types), bc(args), bc(hop)
    off, ln = np.zeros(n, np.uint64), np.zeros(n, np.uint32)
    pos = 0
    for i, f in enumerate(dgrams):
        pos += (int(aligns[i]) - pos) % 16
        off[i], ln[i] = pos, len(f) + int(slacks[i])
        pos += len(f) + max(int(slacks[i]), 0)
    buf = random_bytes(seed ^ 0x1C6F, pos)
    for i, f in enumerate(dgrams):
        buf[int(off[i]):int(off[i]) + len(f)] = f
    req = np.zeros(n, np.dtype([("src", "u1", 16), ("arg", "<u4"), ("type", "u1"), ("code", "u1"), ("hop", "u1"), ("rsvd", "u1")]))
    req["src"] = np.frombuffer(bytes(local), np.uint8)
    req["arg"], req["type"], req["code"], req["hop"] = ags, tps, cds, hops
    cap = np.array([icmp6_answer_len(f, int(tps[i])) if region is None else region for i, f in enumerate(dgrams)], np.uint32)
    ooff = np.zeros(n, np.uint64)
    pos = 0
    for i in range(n):
        pos += (int(ooffs[i]) - pos) % 16
        ooff[i] = pos
        pos += int(cap[i])
    return buf, off, ln, req, ooff, cap, pos + 16


def interleave_groups(desc, groups, seed: int = 91):
    """A seeded merge of group-contiguous frames into one arrival order that keeps each group's own order
    (what a link delivers when several flows send at once): desc = the frames' descriptors (any array
    indexed by frame), groups = (first, count) pairs.  Returns (desc[perm], perm): arrival i is input
    frame perm[i]; frames no group covers are dropped."""
    groups = np.asarray(groups, dtype=np.int64).reshape(-1, 2)
    owner = np.repeat(np.arange(groups.shape[0]), groups[:, 1])
    rng = np.random.default_rng(seed)
    owner = owner[rng.permutation(owner.size)]              # which group sends at each arrival
    nxt = groups[:, 0].copy()
    perm = np.empty(owner.size, np.int64)
    for i, g in enumerate(owner):
        perm[i] = nxt[g]
        nxt[g] += 1
    return np.asarray(desc)[perm], perm
