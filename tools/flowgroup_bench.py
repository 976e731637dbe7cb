#!/usr/bin/env python3
"""Measurement aid: the flow grouping (pico_flow_group_batch_dev) on the coalescing tool's burst with its
connections interleaved, beside the coalescing of its output, the two as one graph, and the host pass
the grouping replaces -- the same process, the device legs alternating replay by replay.

The burst (tools/tcprx_bench.py's: streams of --payload bytes behind an IPv4 header and a 32-byte TCP
header, segmented by tcp_segment_batch into frames --stride apart), with a source address and port of
its own per connection, and the segments' descriptors merged into one seeded arrival order that keeps
each connection's own order (synth.interleave_groups).  The connections' tuples are the grouping's
table, so group t is connection t and conn[] / the output regions line up with no host step.

Legs, per shape:
  group           flow_group_batch: descriptors in arrival order -> group-contiguous descriptors + groups
  coalesce        tcp_coalesce_batch on the grouping's out_desc / out_groups as they are
  group_coalesce  the two in ONE graph, back to back on one stream
  host_group      (wall clock, not a graph) what a host does instead: D2H of the descriptors and of the
                  first 64 bytes of every frame (gathered on the device into one array first), a numpy
                  grouping by packed key -- src, dst, ports; np.unique for the group of each frame, groups
                  numbered by first arrival, a stable argsort by group -- and H2D of the permuted descriptors
                  and the groups
The device legs run over --rotate buffer sets, one replay = one pass over every set, captured as a HIP
graph; the figure is the median of --replays (>= 20) replays timed by HIP events, per call.  The host leg
is the median of the same number of runs on one set, between device synchronisations.  Before and after
timing every connection's coalesced stream is verified against its payload, and the host grouping
against the device's.

  python tools/flowgroup_bench.py [--shape c3|9000|both] [--replays 24] [--out profiles/flowgroup/x.json]
"""
from __future__ import annotations

import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sg_harness as SG  # noqa: E402
from picotcp_amd import batch, synth  # noqa: E402
from tcpseg_bench import H, make_set as make_stream_set  # noqa: E402  (the sets are the segmentation tool's)


def make_set(n, P, per, stride, dev, seed):
    s = make_stream_set(n, P, per, stride, dev, seed)
    cnt = s["cnt"]
    pitch = (H + P + 12 + 15) // 16 * 16
    # a tuple of its own per connection: source 10.g2.g1.g0, source port 1024 + g % 50000
    g = np.arange(n)
    tup = np.zeros((n, 6), np.uint8)
    tup[:, 0], tup[:, 1], tup[:, 2], tup[:, 3] = 10, g >> 16 & 255, g >> 8 & 255, g & 255
    sport = 1024 + g % 50000
    tup[:, 4], tup[:, 5] = sport >> 8, sport & 255
    hdr = torch.as_strided(s["buf"], (n, H), (pitch, 1), 12)
    hdr[:, 12:16] = torch.from_numpy(tup[:, :4].copy()).to(dev)
    hdr[:, 20:22] = torch.from_numpy(tup[:, 4:].copy()).to(dev)
    batch.tcp_segment_batch(s["buf"], s["sd"], s["grp"], s["n_seg"], s["out"], s["od"], stride, out_seg=s["of"], results=s["res"])
    torch.cuda.synchronize(dev)
    assert bool((s["res"][0] == batch.V_ACCEPT).all())
    n_seg = s["n_seg"]
    desc = s["of"].cpu().numpy().view(batch.DESC_DTYPE)
    groups = np.stack([np.arange(n) * cnt, np.full(n, cnt)], axis=1)
    arr, perm = synth.interleave_groups(desc, groups, seed=seed)
    s["arr"] = batch.desc_to_device(arr, dev)
    s["perm"] = torch.from_numpy(perm).to(dev)
    known = np.zeros(n, batch.FLOW_KEY_DTYPE)
    known["family"] = 4
    known["src"][:, :4] = tup[:, :4]
    known["dst"][:, :4] = [192, 168, 7, 2]
    known["sport"] = (sport >> 8) | ((sport & 255) << 8)                    # as stored: network byte order
    known["dport"] = 0x9C | (0x40 << 8)
    s["known"] = torch.from_numpy(known.view(np.uint8).reshape(-1).copy()).to(dev)
    s["scratch"] = torch.empty(batch.flow_group_scratch_bytes(n_seg, n), dtype=torch.uint8, device=dev)
    s["gres"] = (torch.zeros(16 * n_seg, dtype=torch.uint8, device=dev), torch.zeros(n_seg, dtype=torch.int32, device=dev),
                 torch.zeros(2 * (n_seg + n), dtype=torch.int32, device=dev), torch.zeros(2, dtype=torch.int32, device=dev))
    RP = (P + 15) // 16 * 16
    s["RP"], s["pitch"] = RP, pitch
    s["rbuf"] = torch.zeros(n * RP + 16, dtype=torch.uint8, device=dev)
    s["rod"] = batch.desc_to_device(batch.make_desc(np.arange(n, dtype=np.int64) * RP, np.full(n, P)), dev)
    seq0 = (np.arange(n, dtype=np.uint32) * 2654435761).astype(np.uint32)   # the templates' seq (make_stream_set)
    s["conn"] = torch.from_numpy(np.stack([seq0, np.zeros(n, np.uint32)], axis=1).reshape(-1).view(np.int32)).to(dev)
    s["rres"] = (torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
                 torch.empty(n_seg, dtype=torch.uint8, device=dev))
    # the frames in segmentation order, 64 bytes each (the host leg gathers them in arrival order)
    s["heads"] = torch.as_strided(s["out"], (n_seg, 64), (stride, 1), 12)
    return s


def host_group(s, dev):
    """The host pass: (permuted descriptors, groups uint32[m, 2]) on the device, from the burst on the device."""
    heads = s["heads"].index_select(0, s["perm"]).cpu().numpy()             # D2H: 64 bytes a frame, arrival order
    desc = s["arr"].cpu().numpy().view(batch.DESC_DTYPE)                    # D2H: the descriptors
    ihl = (heads[:, 0] & 15).astype(np.int64) * 4
    key = np.concatenate([heads[:, 12:20], np.take_along_axis(heads, ihl[:, None] + np.arange(4)[None, :], axis=1)], axis=1)
    _, first, inv = np.unique(np.ascontiguousarray(key).view("V12").reshape(-1), return_index=True, return_inverse=True)
    rank = np.empty(first.size, np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(first.size)          # groups by first arrival
    gid = rank[inv.reshape(-1)]
    order = np.argsort(gid, kind="stable")
    cnt = np.bincount(gid, minlength=first.size)
    groups = np.stack([np.concatenate([[0], np.cumsum(cnt)[:-1]]), cnt], axis=1).astype(np.uint32)
    d = batch.desc_to_device(desc[order], dev)                              # H2D
    g = torch.from_numpy(groups.reshape(-1).view(np.int32)).to(dev)
    torch.cuda.synchronize(dev)
    return d, g, order, groups


def run_shape(name, n, P, a, dev, lib):
    per, stride = a.per, a.stride
    sets = [make_set(n, P, per, stride, dev, 900 + i) for i in range(a.rotate)]
    cnt, n_seg = sets[0]["cnt"], sets[0]["n_seg"]
    stream = torch.cuda.current_stream(dev)

    def group(s, st):
        batch.flow_group_batch(s["out"], s["arr"], n_seg, batch.FLOW_TCP, known=s["known"], n_known=n, hash_seed=0x5EED,
                               scratch=s["scratch"], stream=st, results=s["gres"])

    def coalesce(s, st):
        batch.tcp_coalesce_batch(s["out"], s["gres"][0], n_seg, s["gres"][2][:2 * n], s["conn"], s["rbuf"], s["rod"],
                                 stream=st, results=s["rres"])

    def both(s, st):
        group(s, st)
        coalesce(s, st)

    def verified(s):
        want = torch.as_strided(s["buf"], (n, P), (s["pitch"], 1), 12 + H)
        got = torch.as_strided(s["rbuf"], (n, P), (s["RP"], 1), 0)
        v, ol, sv = s["rres"]
        counts = s["gres"][3].cpu().numpy()
        return bool(counts[0] == n and counts[1] == n_seg and (v == batch.V_ACCEPT).all() and (ol == P).all() and
                    (sv == batch.V_ACCEPT).all() and torch.equal(want, got))

    for s in sets:
        s["rbuf"].zero_()
        both(s, stream)
        torch.cuda.synchronize(dev)
        if not verified(s):
            raise SystemExit(f"{name}: grouping + coalescing does not deliver every connection's payload at the timed size")
    # the host grouping finds the same groups (numbered by first arrival; the device's by the table)
    s0 = sets[0]
    _, _, order, hgroups = host_group(s0, dev)
    oi = s0["gres"][1].cpu().numpy().view(np.uint32)
    og = s0["gres"][2].cpu().numpy().view(np.uint32).reshape(-1, 2)[:n]
    dev_groups = {tuple(oi[f:f + c]) for f, c in og}
    if {tuple(order[f:f + c]) for f, c in hgroups} != dev_groups:
        raise SystemExit(f"{name}: the host grouping and the device grouping disagree")

    times = SG.time_legs({"group": group, "coalesce": coalesce, "group_coalesce": both}, sets, dev, stream, a.warmup,
                         a.replays, a.rotate)
    host = []
    for _ in range(a.replays):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        host_group(s0, dev)
        host.append((time.perf_counter() - t0) * 1e6)
    times["host_group"] = host
    for s in sets:
        s["rbuf"].zero_()
        both(s, stream)
        torch.cuda.synchronize(dev)
        if not verified(s):
            raise SystemExit(f"{name}: a replay after timing does not verify")
    payload = n * P
    # bytes the grouping needs: descriptors + verdict-free headers (24 bytes of a 64-byte line) + table read;
    # descriptors, indexes, groups written
    moved = {"group": n_seg * (16 + 64) + 40 * n + n_seg * (16 + 4) + 8 * (n_seg + n),
             "coalesce": n * (cnt * H + P) + 16 * n * cnt + n * 32 + n * P + n * 5 + n * cnt,
             "host_group": n_seg * (16 + 64) + n_seg * 16 + 8 * n}
    moved["group_coalesce"] = moved["group"] + moved["coalesce"]
    r = {"shape": name.replace("tcpseg", "flowgroup"), "connections": n, "payload_bytes_per_connection": P, "per": per,
         "seg_stride": stride, "frames": n_seg, "table_keys": n, "rotate": a.rotate, "replays": a.replays,
         "scratch_bytes": int(s0["scratch"].numel()), "payload_bytes": payload,
         "outputs_verified_before_and_after_timing": True, "host_group_is_wall_clock_on_one_set": True}
    SG.summarise(r, times, moved, payload, bytes_key=True)
    r["host_group_over_group"] = round(r["host_group_us"] / r["group_us"], 2)
    r["group_over_coalesce"] = round(r["group_us"] / r["coalesce_us"], 3)
    r["group_coalesce_over_sum"] = round(r["group_coalesce_us"] / (r["group_us"] + r["coalesce_us"]), 3)
    r["frames_per_second_group"] = round(n_seg / (r["group_us"] * 1e-6))
    return r


if __name__ == "__main__":
    SG.main("flowgroup_bench.py", "connections", (("--per", 1448),), ("tcpseg_64512", "tcpseg_9000"), run_shape)
