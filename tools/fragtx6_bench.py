#!/usr/bin/env python3
"""Measurement aid: the IPv6 TX fragmentation batch (pico_ipv6_fragment_batch_dev, K15) beside the IPv4
batch (K8) at equal transport bytes, beside the copy ceilings and beside the IPv6 reassembly of the
fragments it just produced -- the same process, the legs alternating replay by replay.

Legs, per shape (datagrams of --tl transport bytes, split at --mtu into frames --stride apart):
  fragment6       ipv6_fragment_batch(F_WRITE): scatter + fragment headers + the datagram's checksum
  fragment4       ipv4_fragment_batch(F_WRITE) on IPv4 datagrams of the same transport bytes
                  (tools/fragtx_bench.py's sets): K15 is judged against K8 by fragment6_over_fragment4
  reassemble6     ipv6_reassemble_batch on the fragments just written (the inverse gather)
  bare_scatter_*  tools/gather_ceiling.hip's bare copy of every fragment's payload from its place in
                  the datagram to its place in the output, nothing summed, no headers (4 waves per
                  datagram as the fragment kernel, and flat: one wave per fragment pair)
  seq_copy        the device's contiguous copy of the payload bytes (seq_copy, nt loads and stores)
Without tools/bin/libgather_ceiling.so the bare_scatter legs and seq_copy are left out, with a warning
and a note in the JSON.  The scaffold (graphs, warm-up, timing, summary) is tools/sg_harness.py's.
Each leg runs over --rotate buffer sets; one replay = one pass over every set, captured as a HIP
graph; the figure is the median of --replays (>= 20) replays timed by HIP events, per call.
Before timing, the round trip is checked at the timed size: every datagram ACCEPT on both sides, the
TCP checksum the fragment batch stored verifying (0) in the reassembly, the transport bytes the input's.

  python tools/fragtx6_bench.py [--shape c3|9000|both] [--mtu 1500|1280] [--out profiles/fragtx6/x.json]
"""
from __future__ import annotations

import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fragtx_bench as F4  # noqa: E402
import sg_harness as SG  # noqa: E402
from picotcp_amd import batch, synth  # noqa: E402


def make_set(n, tl, mtu, stride, dev, seed):
    """n TCP datagrams of tl transport bytes, 8 mod 16 into 16-byte lines (the transport on a line),
    random payload; output regions at 0 mod 16."""
    per = (mtu - 48) & ~7
    cnt = synth.fragtx6_count(40 + tl, mtu)
    hb = 48 if cnt > 1 else 40
    pitch = (40 + tl + 8 + 15) // 16 * 16
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    buf = torch.randint(0, 256, (n * pitch + 16,), dtype=torch.uint8, device=dev, generator=g)
    off = 8 + np.arange(n, dtype=np.int64) * pitch
    hdr = np.zeros((n, 40), np.uint8)
    hdr[:, 0], hdr[:, 6], hdr[:, 7] = 0x60, 6, 64
    hdr[:, 8:40] = np.frombuffer(bytes.fromhex("20010db8000000010000000000000001" "20010db8000000020000000000000002"), np.uint8)
    idx = torch.from_numpy((off[:, None] + np.arange(40)[None, :]).reshape(-1)).to(dev)
    buf[idx] = torch.from_numpy(hdr.reshape(-1)).to(dev)
    cap = cnt * stride
    ooff = np.arange(n, dtype=np.int64) * cap
    groups = np.stack([np.arange(n) * cnt, np.full(n, cnt)], axis=1).astype(np.uint32)
    out = torch.zeros(int(ooff[-1] + cap + 16), dtype=torch.uint8, device=dev)
    rout = torch.zeros(n * pitch + 16, dtype=torch.uint8, device=dev)
    k = np.tile(np.arange(cnt, dtype=np.int64), n)
    gi = np.repeat(np.arange(n, dtype=np.int64), cnt)
    f_src = (off[gi] + 40 + k * per).astype(np.uint64)
    f_dst = (ooff[gi] + k * stride + hb).astype(np.uint64)
    f_len = np.minimum(per, tl - k * per).astype(np.uint32) if cnt > 1 else np.full(n, tl, np.uint32)
    dv = lambda x: torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x.view(np.int32)).to(dev)   # noqa: E731
    return dict(buf=buf, dd=batch.desc_to_device(batch.make_desc(off, np.full(n, 40 + tl), 1 + np.arange(n)), dev),
                grp=torch.from_numpy(groups.reshape(-1).view(np.int32)).to(dev), n_frag=n * cnt, out=out,
                od=batch.desc_to_device(batch.make_desc(ooff, np.full(n, cap)), dev),
                of=torch.zeros(16 * n * cnt, dtype=torch.uint8, device=dev), rout=rout,
                rod=batch.desc_to_device(batch.make_desc(off, np.full(n, 40 + tl)), dev),
                res=(torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
                     torch.empty(n, dtype=torch.int16, device=dev)),
                rres=(torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int16, device=dev),
                      torch.empty(n, dtype=torch.uint8, device=dev)),
                f_src=dv(f_src), f_dst=dv(f_dst), f_len=dv(f_len), cnt=cnt)


def run_shape(name, n, tl, a, dev, lib):
    mtu, stride = a.mtu, a.stride
    sets = [make_set(n, tl, mtu, stride, dev, 900 + i) for i in range(a.rotate)]
    for s, s4 in zip(sets, (F4.make_set(n, tl, mtu, stride, dev, 950 + i) for i in range(a.rotate))):
        s["v4"] = s4
    cnt, cnt4 = sets[0]["cnt"], sets[0]["v4"]["cnt"]
    if cnt < 2:
        raise SystemExit(f"{name}: a {tl}-byte transport fits MTU {mtu}: nothing to fragment")
    stream = torch.cuda.current_stream(dev)

    def fragment6(s, st):
        batch.ipv6_fragment_batch(s["buf"], s["dd"], mtu, s["grp"], s["n_frag"], s["out"], s["od"], stride,
                                  flags=batch.F_WRITE, out_frag=s["of"], stream=st, results=s["res"])

    def fragment4(s, st):
        s = s["v4"]
        batch.ipv4_fragment_batch(s["buf"], s["dd"], mtu, s["grp"], s["n_frag"], s["out"], s["od"], stride,
                                  flags=batch.F_WRITE, out_frag=s["of"], stream=st, results=s["res"])

    def reassemble6(s, st):
        batch.ipv6_reassemble_batch(s["out"], s["of"], s["n_frag"], s["grp"], s["rout"], s["rod"],
                                    flags=batch.F_NXTHDR_DISPATCH, stream=st, results=s["rres"])

    def bare(mode):
        def f(s, st):
            assert lib.gather_ceiling_launch(mode, s["buf"].data_ptr(), s["buf"].numel(), s["f_src"].data_ptr(),
                                             s["f_dst"].data_ptr(), s["f_len"].data_ptr(), s["grp"].data_ptr(), n,
                                             s["n_frag"], s["out"].data_ptr(), s["out"].numel(),
                                             ctypes.c_void_p(st.cuda_stream)) == 0
        return f

    payload = n * tl

    def seq(s, st):
        assert lib.seq_copy_launch(0, 4, 0, s["rout"].data_ptr(), s["buf"].data_ptr(), payload & ~15,
                                   ctypes.c_void_p(st.cuda_stream)) == 0

    # the round trip at the timed size, checked once
    for s in sets:
        fragment6(s, stream)
        reassemble6(s, stream)
        fragment4(s, stream)
    torch.cuda.synchronize(dev)
    s = sets[0]
    ok = bool((s["res"][0] == batch.V_ACCEPT).all() and (s["res"][1] == cnt).all() and (s["rres"][2] == batch.V_ACCEPT).all()
              and (s["rres"][1] == 0).all() and (s["rres"][0] == tl).all()
              and (s["v4"]["res"][0] == batch.V_ACCEPT).all() and (s["v4"]["res"][1] == cnt4).all())
    pitch = (s["buf"].numel() - 16) // n
    a_in = s["buf"][:n * pitch].view(n, pitch)[:, 48:48 + tl]
    a_out = s["rout"][:n * pitch].view(n, pitch)[:, 48:48 + tl]
    same = a_in != a_out
    same[:, 16:18] = False                                   # the TCP crc the fragment batch stored
    ok = ok and not bool(same.any())
    if not ok:
        raise SystemExit(f"{name}: the fragment / reassemble round trip does not check out at the timed size")

    # the legs take turns in this order, replay by replay
    # (the bare scatter rounds its stores up past a fragment's end, into the next header: the
    # fragment6 leg, which rewrites every header, always runs between it and the reassembly)
    legs = {"fragment6": fragment6, "reassemble6": reassemble6, "fragment4": fragment4}
    if lib is not None:
        legs.update({"bare_scatter_4waves": bare(2), "bare_scatter_flat": bare(3), "seq_copy": seq})
    times = SG.time_legs(legs, sets, dev, stream, a.warmup, a.replays, a.rotate)
    for s in sets:                                           # the timed replays worked on good data
        if not bool((s["res"][0] == batch.V_ACCEPT).all() and (s["rres"][2] == batch.V_ACCEPT).all()
                    and (s["v4"]["res"][0] == batch.V_ACCEPT).all()):
            raise SystemExit(f"{name}: a timed replay did not accept every datagram")
    # bytes the algorithm needs, from the shapes: read = datagrams + their descriptors / groups /
    # out descriptors; written = fragments (headers + payload) + fragment descriptors + results
    read_b = n * (40 + tl) + n * (16 + 8 + 16)
    written_b = n * (cnt * 48 + tl) + 16 * n * cnt + n * (1 + 4 + 2)
    read4 = n * (20 + tl) + n * (16 + 8 + 16)
    written4 = n * (cnt4 * 20 + tl) + 16 * n * cnt4 + n * (1 + 4 + 2)
    r = {"shape": name, "datagrams": n, "transport_bytes": tl, "mtu": mtu, "frag_stride": stride, "fragments": cnt,
         "fragments_ipv4": cnt4, "rotate": a.rotate, "replays": a.replays,
         "working_set_bytes_per_set": int(sets[0]["buf"].numel() + sets[0]["out"].numel()),
         "payload_bytes": payload, "algorithmic_bytes_read": read_b, "algorithmic_bytes_written": written_b,
         "round_trip_checked": ok}
    SG.summarise(r, times, {"fragment6": read_b + written_b, "reassemble6": read_b + written_b, "fragment4": read4 + written4},
                 payload)
    r["fragment6_over_fragment4"] = round(r["fragment6_us"] / r["fragment4_us"], 3)
    r["fragment6_over_reassemble6"] = round(r["fragment6_us"] / r["reassemble6_us"], 3)
    if lib is None:
        r["ceiling_legs"] = SG.CEILING_NOT_MEASURED
    else:
        r["fragment6_over_bare_scatter_4waves"] = round(r["fragment6_us"] / r["bare_scatter_4waves_us"], 3)
        r["fragment6_over_seq_copy"] = round(r["fragment6_us"] / r["seq_copy_us"], 3)
    return r


if __name__ == "__main__":
    SG.main("fragtx6_bench.py", "datagrams", (("--mtu", 1500),), ("c3_fragtx6", "fragtx6_9000"), run_shape)
