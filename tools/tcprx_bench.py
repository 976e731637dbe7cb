#!/usr/bin/env python3
"""Measurement aid: the TCP coalescing batch (pico_tcp_coalesce_batch_dev) on the send segmentation's
own output, beside the IPv4 reassembly of the same byte count, the segmentation itself and the copy
ceilings -- the same process, the legs alternating replay by replay.

Legs, per shape (tools/tcpseg_bench.py's: streams of --payload bytes behind an IPv4 header and a
32-byte TCP header, segments of --per bytes, frames --stride apart):
  coalesce        tcp_coalesce_batch on tcp_segment_batch's d_out / d_out_seg as they are (in order,
                  no SACK): every frame's IPv4 header checksum and TCP checksum verified, the payload
                  gathered into one region per connection (16-byte aligned)
  reassemble      ipv4_reassemble_batch on ipv4_fragment_batch's output for the same streams (each read
                  as one IPv4 / TCP datagram of 20 + 32 + payload bytes at MTU 1500: per 1480, one
                  checksum per datagram, no per-fragment verification) -- the yardstick, the c3_reasm shape
  segment         tcp_segment_batch, the inverse, on the same streams
  bare_gather_*   tools/gather_ceiling.hip's bare copy of every segment's payload from its frame to its
                  place in the region, nothing parsed, nothing summed (4 waves per connection as the
                  coalescing kernel, and flat: one wave per segment pair).  It stores whole 16-byte units
                  non-temporally, rounding past a segment's end; the coalescing kernel stores through the
                  cache and to the byte, so a ratio to this leg crosses two store paths
  seq_copy        the device's contiguous copy of the payload bytes (nt loads and stores)
Each leg runs over --rotate buffer sets (one set's working set already exceeds the 256 MiB Infinity
Cache at the default shapes); one replay = one pass over every set, captured as a HIP graph; the
figure is the median of --replays (>= 20) replays timed by HIP events, per call.  Before timing,
every connection's output is verified at the timed size: out_len == payload, every verdict ACCEPT,
and the delivered bytes equal the stream's payload.

  python tools/tcprx_bench.py [--shape c3|9000|both] [--replays 24] [--out profiles/tcprx/x.json]
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
from picotcp_amd import batch  # noqa: E402
from tcpseg_bench import H, MTU, make_set as make_stream_set  # noqa: E402  (the sets are the segmentation tool's)


def make_set(n, P, per, stride, dev, seed):
    """tools/tcpseg_bench.py's set, segmented and fragmented once, with the arrays of the RX legs."""
    s = make_stream_set(n, P, per, stride, dev, seed)
    cnt, fcnt = s["cnt"], s["fcnt"]
    s["fout"] = torch.zeros_like(s["out"])                                  # the fragments (the reassembly's input)
    batch.tcp_segment_batch(s["buf"], s["sd"], s["grp"], s["n_seg"], s["out"], s["od"], stride, out_seg=s["of"], results=s["res"])
    batch.ipv4_fragment_batch(s["buf"], s["dd"], MTU, s["fgrp"], s["n_frag"], s["fout"], s["od"], stride, flags=batch.F_WRITE,
                              out_frag=s["ff"], results=s["fres"])
    torch.cuda.synchronize(dev)
    assert bool((s["res"][0] == batch.V_ACCEPT).all() and (s["fres"][0] == batch.V_ACCEPT).all())
    RP = (P + 15) // 16 * 16                                                # a connection's region, on a 16-byte line
    DP = (20 + 32 + P + 12 + 15) // 16 * 16                                 # a reassembled datagram's, transport on a line
    s["RP"], s["DP"] = RP, DP
    s["rbuf"] = torch.zeros(n * RP + 16, dtype=torch.uint8, device=dev)
    s["rod"] = batch.desc_to_device(batch.make_desc(np.arange(n, dtype=np.int64) * RP, np.full(n, P)), dev)
    seq0 = (np.arange(n, dtype=np.uint32) * 2654435761).astype(np.uint32)   # the templates' seq (make_stream_set)
    s["conn"] = torch.from_numpy(np.stack([seq0, np.zeros(n, np.uint32)], axis=1).reshape(-1).view(np.int32)).to(dev)
    s["rres"] = (torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
                 torch.empty(n * cnt, dtype=torch.uint8, device=dev))
    s["dbuf"] = torch.zeros(n * DP + 16, dtype=torch.uint8, device=dev)
    s["dod"] = batch.desc_to_device(batch.make_desc(12 + np.arange(n, dtype=np.int64) * DP, np.full(n, DP - 12)), dev)
    s["dres"] = (torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int16, device=dev),
                 torch.empty(n, dtype=torch.uint8, device=dev))
    # the bare gather: frame payload -> region
    k = np.tile(np.arange(cnt, dtype=np.int64), n)
    gi = np.repeat(np.arange(n, dtype=np.int64), cnt)
    g_src = (12 + gi * cnt * stride + k * stride + H).astype(np.uint64)
    g_dst = (gi * RP + k * per).astype(np.uint64)
    s["g_src"] = torch.from_numpy(g_src.view(np.int64)).to(dev)
    s["g_dst"] = torch.from_numpy(g_dst.view(np.int64)).to(dev)
    return s


def run_shape(name, n, P, a, dev, lib):
    per, stride = a.per, a.stride
    sets = [make_set(n, P, per, stride, dev, 900 + i) for i in range(a.rotate)]
    cnt, fcnt = sets[0]["cnt"], sets[0]["fcnt"]
    stream = torch.cuda.current_stream(dev)

    def coalesce(s, st):
        batch.tcp_coalesce_batch(s["out"], s["of"], s["n_seg"], s["grp"], s["conn"], s["rbuf"], s["rod"], stream=st,
                                 results=s["rres"])

    def reassemble(s, st):
        batch.ipv4_reassemble_batch(s["fout"], s["ff"], s["n_frag"], s["fgrp"], s["dbuf"], s["dod"], stream=st,
                                    results=s["dres"])

    def segment(s, st):
        batch.tcp_segment_batch(s["buf"], s["sd"], s["grp"], s["n_seg"], s["out"], s["od"], stride, out_seg=s["of"],
                                stream=st, results=s["res"])

    def bare(mode):
        def f(s, st):
            assert lib.gather_ceiling_launch(mode, s["out"].data_ptr(), s["out"].numel(), s["g_src"].data_ptr(),
                                             s["g_dst"].data_ptr(), s["f_len"].data_ptr(), s["grp"].data_ptr(), n,
                                             s["n_seg"], s["rbuf"].data_ptr(), s["rbuf"].numel(),
                                             ctypes.c_void_p(st.cuda_stream)) == 0
        return f

    payload = n * P

    def seq(s, st):
        assert lib.seq_copy_launch(0, 4, 0, s["copy"].data_ptr(), s["buf"].data_ptr(), payload & ~15,
                                   ctypes.c_void_p(st.cuda_stream)) == 0

    def verified(s):
        """Every connection's output at the timed size: verdicts, out_len and the delivered bytes."""
        pitch = (H + P + 12 + 15) // 16 * 16
        want = torch.as_strided(s["buf"], (n, P), (pitch, 1), 12 + H)
        got = torch.as_strided(s["rbuf"], (n, P), (s["RP"], 1), 0)
        v, ol, sv = s["rres"]
        return bool((v == batch.V_ACCEPT).all() and (ol == P).all() and (sv == batch.V_ACCEPT).all() and torch.equal(want, got))

    for s in sets:
        s["rbuf"].zero_()
        coalesce(s, stream)
        reassemble(s, stream)
        torch.cuda.synchronize(dev)
        if not verified(s):
            raise SystemExit(f"{name}: the coalesced streams do not equal the payload at the timed size")
        if not bool((s["dres"][2] == batch.V_ACCEPT).all() and (s["dres"][0] == 32 + P).all()):
            raise SystemExit(f"{name}: the reassembly leg does not accept every datagram")

    legs = {"coalesce": coalesce, "reassemble": reassemble, "segment": segment}
    if lib is not None:
        legs.update({"bare_gather_4waves": bare(2), "bare_gather_flat": bare(3), "seq_copy": seq})
    times = SG.time_legs(legs, sets, dev, stream, a.warmup, a.replays, a.rotate)
    for s in sets:                                           # the timed replays worked on good data (the bare
        coalesce(s, stream)                                  # gather's rounded stores last wrote the regions)
        torch.cuda.synchronize(dev)
        if not verified(s):
            raise SystemExit(f"{name}: a replay after timing does not verify")
    # bytes the algorithm needs, from the shapes: read = frames (headers + payload) + descriptors / groups /
    # conn / out descriptors; written = the stream + results
    moved = {"coalesce": n * (cnt * H + P) + 16 * n * cnt + n * 32 + n * P + n * 5 + n * cnt,
             "reassemble": n * (fcnt * 20 + 32 + P) + 16 * n * fcnt + n * 24 + n * (20 + 32 + P) + n * 7,
             "segment": n * (H + P) + n * 40 + n * (cnt * H + P) + 16 * n * cnt + n * 5}
    r = {"shape": name.replace("tcpseg", "tcprx"), "connections": n, "payload_bytes_per_connection": P, "per": per,
         "seg_stride": stride, "segments": cnt, "fragments_of_the_reassemble_leg": fcnt, "rotate": a.rotate,
         "replays": a.replays, "payload_bytes": payload, "outputs_verified_before_and_after_timing": True}
    SG.summarise(r, times, moved, payload, bytes_key=True)
    r["coalesce_over_reassemble"] = round(r["coalesce_us"] / r["reassemble_us"], 3)
    r["coalesce_over_segment"] = round(r["coalesce_us"] / r["segment_us"], 3)
    if lib is not None:
        r["coalesce_over_bare_gather_4waves"] = round(r["coalesce_us"] / r["bare_gather_4waves_us"], 3)
        r["coalesce_over_bare_gather_flat"] = round(r["coalesce_us"] / r["bare_gather_flat_us"], 3)
        r["coalesce_over_seq_copy"] = round(r["coalesce_us"] / r["seq_copy_us"], 3)
        r["ceiling_store_path"] = "non-temporal whole-unit stores; the coalesce leg uses cached stores, to the byte"
    else:
        r["ceiling_legs"] = SG.CEILING_NOT_MEASURED
    return r


if __name__ == "__main__":
    SG.main("tcprx_bench.py", "connections", (("--per", 1448),), ("tcpseg_64512", "tcpseg_9000"), run_shape)
