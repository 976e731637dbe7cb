#!/usr/bin/env python3
"""Measurement aid: the TCP segmentation batch (pico_tcp_segment_batch_dev) beside the IPv4
fragmentation batch on the same bytes and beside the copy ceilings -- the same process, the legs
alternating replay by replay.

Legs, per shape (streams of --payload bytes behind an IPv4 header and a 32-byte TCP header, cut into
segments of --per bytes, frames --stride apart):
  segment         tcp_segment_batch: scatter + every frame's IPv4 header checksum and TCP checksum
  fragment        ipv4_fragment_batch(F_WRITE) on the same buffer, each stream read as one IPv4 / TCP
                  datagram of 20 + 32 + payload bytes at MTU 1500 (per 1480: one frame fewer when the
                  payload fills 45 segments; one checksum per datagram, not per frame) -- the yardstick
  bare_scatter_*  tools/gather_ceiling.hip's bare copy of every segment's payload from its place in
                  the stream to its place in the output, nothing summed, no headers (4 waves per stream
                  as the segment kernel, and flat: one wave per segment pair).  It stores whole 16-byte
                  units non-temporally, rounding past a segment's end; the segment and fragment
                  kernels store through the cache and to the byte, so a ratio to this leg crosses two
                  store paths.  Without tools/bin/libgather_ceiling.so these legs and seq_copy are
                  left out, with a warning and a note in the JSON
  seq_copy       the device's contiguous copy of the payload bytes (seq_copy, nt loads and stores)
Each leg runs over --rotate buffer sets (the working set of one set already exceeds the 256 MiB
Infinity Cache at the default shapes); one replay = one pass over every set, captured as a HIP
graph; the figure is the median of --replays (>= 20) replays timed by HIP events, per call.
Before timing, the segments are checked at the timed size: every stream ACCEPT and every frame
ACCEPT with both checksums verifying (0) in the IPv4 RX batch.

  python tools/tcpseg_bench.py [--shape c3|9000|both] [--replays 24] [--out profiles/tcpseg/x.json]
"""
from __future__ import annotations

import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sg_harness as SG  # noqa: E402
from picotcp_amd import batch, synth  # noqa: E402

H = 52                  # 20 + a 32-byte TCP header (timestamp option, padded)
MTU = 1500


def make_set(n, P, per, stride, dev, seed):
    """n IPv4 / TCP streams of P payload bytes, 12 mod 16 into 16-byte lines (the payload on a line),
    random payload."""
    cnt = synth.tcpseg_count(P, per)
    fcnt = synth.fragtx_count(H + P, MTU)
    pitch = (H + P + 12 + 15) // 16 * 16
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    buf = torch.randint(0, 256, (n * pitch + 16,), dtype=torch.uint8, device=dev, generator=g)
    off = 12 + np.arange(n, dtype=np.int64) * pitch
    hdr = np.zeros((n, H), np.uint8)
    hdr[:, 0], hdr[:, 8], hdr[:, 9] = 0x45, 64, 6
    hdr[:, 4:6] = (np.arange(n) * cnt).astype(np.uint16).byteswap().view(np.uint8).reshape(n, 2)
    hdr[:, 12:20] = [10, 1, 2, 3, 192, 168, 7, 2]
    hdr[:, 20:24] = [0, 80, 0x9C, 0x40]
    hdr[:, 24:28] = (np.arange(n, dtype=np.uint32) * 2654435761).astype(np.uint32).byteswap().view(np.uint8).reshape(n, 4)
    hdr[:, 32], hdr[:, 33], hdr[:, 34] = 0x80, 0x18, 0x20
    hdr[:, 40:52] = [1, 1, 8, 10, 0, 1, 2, 3, 0, 4, 5, 6]
    idx = torch.from_numpy((off[:, None] + np.arange(H)[None, :]).reshape(-1)).to(dev)
    buf[idx] = torch.from_numpy(hdr.reshape(-1)).to(dev)
    cap = cnt * stride
    ooff = 12 + np.arange(n, dtype=np.int64) * cap
    groups = np.stack([np.arange(n) * cnt, np.full(n, cnt)], axis=1).astype(np.uint32)
    fgroups = np.stack([np.arange(n) * fcnt, np.full(n, fcnt)], axis=1).astype(np.uint32)
    out = torch.zeros(int(ooff[-1] + cap + 16), dtype=torch.uint8, device=dev)
    k = np.tile(np.arange(cnt, dtype=np.int64), n)
    gi = np.repeat(np.arange(n, dtype=np.int64), cnt)
    f_src = (off[gi] + H + k * per).astype(np.uint64)
    f_dst = (ooff[gi] + k * stride + H).astype(np.uint64)
    f_len = np.minimum(per, P - k * per).astype(np.uint32)
    dv = lambda x: torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x.view(np.int32)).to(dev)   # noqa: E731
    return dict(buf=buf, sd=batch.desc_to_device(batch.make_desc(off, np.full(n, H + P), np.full(n, per)), dev),
                dd=batch.desc_to_device(batch.make_desc(off, np.full(n, H + P)), dev),
                grp=torch.from_numpy(groups.reshape(-1).view(np.int32)).to(dev), n_seg=n * cnt,
                fgrp=torch.from_numpy(fgroups.reshape(-1).view(np.int32)).to(dev), n_frag=n * fcnt, out=out,
                od=batch.desc_to_device(batch.make_desc(ooff, np.full(n, cap)), dev),
                of=torch.zeros(16 * n * cnt, dtype=torch.uint8, device=dev),
                ff=torch.zeros(16 * n * fcnt, dtype=torch.uint8, device=dev), copy=torch.empty(n * P + 16, dtype=torch.uint8, device=dev),
                res=(torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.int32, device=dev)),
                fres=(torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
                      torch.empty(n, dtype=torch.int16, device=dev)),
                f_src=dv(f_src), f_dst=dv(f_dst), f_len=dv(f_len), cnt=cnt, fcnt=fcnt)


def run_shape(name, n, P, a, dev, lib):
    per, stride = a.per, a.stride
    sets = [make_set(n, P, per, stride, dev, 900 + i) for i in range(a.rotate)]
    cnt, fcnt = sets[0]["cnt"], sets[0]["fcnt"]
    stream = torch.cuda.current_stream(dev)

    def segment(s, st):
        batch.tcp_segment_batch(s["buf"], s["sd"], s["grp"], s["n_seg"], s["out"], s["od"], stride, out_seg=s["of"],
                                stream=st, results=s["res"])

    def fragment(s, st):
        batch.ipv4_fragment_batch(s["buf"], s["dd"], MTU, s["fgrp"], s["n_frag"], s["out"], s["od"], stride,
                                  flags=batch.F_WRITE, out_frag=s["ff"], stream=st, results=s["fres"])

    def bare(mode):
        def f(s, st):
            assert lib.gather_ceiling_launch(mode, s["buf"].data_ptr(), s["buf"].numel(), s["f_src"].data_ptr(),
                                             s["f_dst"].data_ptr(), s["f_len"].data_ptr(), s["grp"].data_ptr(), n,
                                             s["n_seg"], s["out"].data_ptr(), s["out"].numel(),
                                             ctypes.c_void_p(st.cuda_stream)) == 0
        return f

    payload = n * P

    def seq(s, st):
        assert lib.seq_copy_launch(0, 4, 0, s["copy"].data_ptr(), s["buf"].data_ptr(), payload & ~15,
                                   ctypes.c_void_p(st.cuda_stream)) == 0

    # the segments at the timed size, checked once through the RX verify batch
    ok = True
    for s in sets:
        segment(s, stream)
        net, l4, rv = batch.ipv4_checksum_batch(s["out"], s["of"], s["n_seg"])
        torch.cuda.synchronize(dev)
        ok = ok and bool((s["res"][0] == batch.V_ACCEPT).all() and (s["res"][1] == cnt).all() and (rv == batch.V_ACCEPT).all()
                         and (net == 0).all() and (l4 == 0).all())
        del net, l4, rv
    if not ok:
        raise SystemExit(f"{name}: the segments do not verify in the RX batch at the timed size")

    legs = {"segment": segment, "fragment": fragment}
    if lib is not None:
        legs.update({"bare_scatter_4waves": bare(2), "bare_scatter_flat": bare(3), "seq_copy": seq})
    times = SG.time_legs(legs, sets, dev, stream, a.warmup, a.replays, a.rotate)
    for s in sets:                                           # the timed replays worked on good data
        if not bool((s["res"][0] == batch.V_ACCEPT).all() and (s["fres"][0] == batch.V_ACCEPT).all()):
            raise SystemExit(f"{name}: a timed replay did not accept every stream")
    # bytes the algorithm needs, from the shapes: read = streams + their descriptors / groups / out
    # descriptors; written = frames (headers + payload) + frame descriptors + results
    moved = {"segment": n * (H + P) + n * 40 + n * (cnt * H + P) + 16 * n * cnt + n * 5,
             "fragment": n * (H + P) + n * 40 + n * (fcnt * 20 + 32 + P) + 16 * n * fcnt + n * 7}
    r = {"shape": name, "streams": n, "payload_bytes_per_stream": P, "per": per, "seg_stride": stride, "segments": cnt,
         "fragments_of_the_fragment_leg": fcnt, "rotate": a.rotate, "replays": a.replays,
         "working_set_bytes_per_set": int(sets[0]["buf"].numel() + sets[0]["out"].numel()), "payload_bytes": payload,
         "algorithmic_bytes_segment": moved["segment"], "algorithmic_bytes_fragment": moved["fragment"],
         "segments_verified_in_rx_batch": ok}
    SG.summarise(r, times, moved, payload)
    r["segment_over_fragment"] = round(r["segment_us"] / r["fragment_us"], 3)
    if lib is not None:
        r["segment_over_bare_scatter_4waves"] = round(r["segment_us"] / r["bare_scatter_4waves_us"], 3)
        r["segment_over_bare_scatter_flat"] = round(r["segment_us"] / r["bare_scatter_flat_us"], 3)
        r["segment_over_seq_copy"] = round(r["segment_us"] / r["seq_copy_us"], 3)
        # the bare scatter stores non-temporally and in whole 16-byte units past a segment's end; the segment
        # and fragment kernels store through the cache, to the byte: these ratios cross two store paths
        r["ceiling_store_path"] = "non-temporal whole-unit stores; segment and fragment legs use cached stores"
    else:
        r["ceiling_legs"] = SG.CEILING_NOT_MEASURED
    return r


if __name__ == "__main__":
    SG.main("tcpseg_bench.py", "streams", (("--per", 1448),), ("tcpseg_64512", "tcpseg_9000"), run_shape)
