#!/usr/bin/env python3
"""Measurement aid: the ACK batch (pico_tcp_ack_batch_dev) behind the TCP coalescing batch, on the burst
tools/tcprx_bench.py measures (streams of --payload bytes behind an IPv4 header and a 32-byte TCP
header, segments of --per bytes), beside the coalescing itself and the host pass the batch replaces --
the same process, the device legs alternating replay by replay.

Two bursts per shape:
  in order    every segment ACCEPT: the ACK batch reads verdicts and writes one frame per connection;
              there is no TCP_OLD / TCP_HELD payload to sum
  disturbed   in --disturb percent of the connections (SACK on) the middle segment is lost and the one
              before it arrives twice: one TCP_OLD segment and every segment behind the hole TCP_HELD,
              about half of those connections' bytes, which the ACK batch sums
Legs:
  coalesce      tcp_coalesce_batch alone (the yardstick, unchanged by the ACK batch)
  ack           tcp_ack_batch alone on the coalescing's outputs (restored before every call: the batch
                updates the segment verdicts in place -- the restoring copy of n_seg bytes is in the leg)
  coalesce_ack  the two behind each other, one graph
  host_pass     what the ACK batch replaces, in numpy on a host copy of the burst: D2H of out_len and
                the verdicts, the held / old segments found, their headers re-read and their checksums
                summed, the blocks, windows, options and both checksums of every frame, H2D of the
                frames.  Wall clock, the median of --host-reps; vectorised numpy, not a C stack.
Before timing, the device's frames are compared with the host pass's, byte for byte, on every set.

  python tools/tcpack_bench.py [--shape c3|9000|both] [--replays 24] [--out profiles/tcpack/x.json]
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
from picotcp_amd import batch  # noqa: E402
from tcprx_bench import make_set as make_rx_set  # noqa: E402  (the sets are the coalescing tool's)

REGION = 64                  # an ACK's region: 20 + 20 + 24 bytes at most here (timestamps, one block)
SPACE = 1 << 20


def make_set(n, P, per, stride, dev, seed, disturb):
    s = make_rx_set(n, P, per, stride, dev, seed)
    cnt = s["cnt"]
    of = s["of"].cpu().numpy().view(batch.DESC_DTYPE).copy()
    conn = s["conn"].cpu().numpy().view(np.uint32).reshape(n, 2).copy()
    hit = np.zeros(n, bool)
    if disturb and cnt >= 4:
        hit[:n * disturb // 100] = True
        np.random.default_rng(seed).shuffle(hit)
        k = cnt // 2
        of[np.flatnonzero(hit) * cnt + k] = of[np.flatnonzero(hit) * cnt + k - 1]       # k lost, k - 1 twice
        conn[hit, 1] = 1
        s["of"] = batch.desc_to_device(of, dev)
        s["conn"] = torch.from_numpy(conn.reshape(-1).view(np.int32)).to(dev)
    s["h_of"], s["h_conn"], s["hit"] = of, conn, hit
    s["h_out"] = s["out"].cpu().numpy()                                     # the host's copy of the burst
    first = s["h_out"][of["off"][::cnt].astype(np.int64)[:, None] + np.arange(40)]
    tmpl = first.copy()
    tmpl[:, 12:16], tmpl[:, 16:20] = first[:, 16:20], first[:, 12:16]
    tmpl[:, 20:22], tmpl[:, 22:24] = first[:, 22:24], first[:, 20:22]
    tmpl[:, 24:28] = (np.arange(n, dtype=np.uint32) * 40503).astype(">u4").view(np.uint8).reshape(n, 4)
    s["h_tmpl"] = tmpl
    s["tmpl"] = torch.from_numpy(tmpl.reshape(-1).copy()).to(dev)
    s["td"] = batch.desc_to_device(batch.make_desc(np.arange(n) * 40, np.full(n, 40)), dev)
    ak = np.zeros(n, batch.TCP_ACK_DTYPE)
    ak["space"], ak["tsval"], ak["tsecr"], ak["aflags"] = SPACE, 1000 + np.arange(n), 7 * np.arange(n), 1
    s["h_ack"] = ak
    s["ack"] = torch.from_numpy(ak.view(np.uint8).copy()).to(dev)
    s["abuf"] = torch.zeros(n * REGION + 16, dtype=torch.uint8, device=dev)
    s["aod"] = batch.desc_to_device(batch.make_desc(np.arange(n) * REGION, np.full(n, REGION)), dev)
    s["ares"] = (torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(16 * n, dtype=torch.uint8, device=dev))
    s["sv0"] = torch.empty_like(s["rres"][2])
    return s


def be_sum(rows: np.ndarray) -> np.ndarray:
    """Per row: the sum of its big-endian 16-bit words (an odd last byte padded with 0)."""
    if rows.shape[1] & 1:
        rows = np.concatenate([rows, np.zeros((rows.shape[0], 1), np.uint8)], axis=1)
    return np.ascontiguousarray(rows).view(">u2").astype(np.uint64).sum(axis=1)


def fold(s: np.ndarray) -> np.ndarray:
    s = (s & 0xFFFF) + (s >> 16)
    s = (s & 0xFFFF) + (s >> 16)
    return (~s & 0xFFFF).astype(np.uint16)


def host_pass(s, n, cnt, dev):
    """The host's ACK generation for the set: returns the frames' buffer (host) after the H2D copy."""
    ol = s["rres"][1].cpu().numpy().view(np.uint32)                         # D2H
    sv = s["rres"][2].cpu().numpy().copy()
    buf, of, conn, ak = s["h_out"], s["h_of"], s["h_conn"], s["h_ack"]
    rcv = conn[:, 0] + ol
    need = np.flatnonzero((sv == batch.V_TCP_OLD) | (sv == batch.V_TCP_HELD))
    good = np.ones(sv.size, bool)
    seq = np.zeros(sv.size, np.uint32)
    pl = np.zeros(sv.size, np.int64)
    for ln in np.unique(of["len"][need]):                                   # (the frames here: IHL 5, thl 32)
        idx = need[of["len"][need] == ln]
        rows = buf[of["off"][idx].astype(np.int64)[:, None] + np.arange(int(ln))]
        seq[idx] = rows[:, 24:28].copy().view(">u4").reshape(-1)
        pl[idx] = int(ln) - 52
        ps = be_sum(rows[:, 12:20]) + 6 + (int(ln) - 20)
        good[idx] = fold(ps + be_sum(rows[:, 20:])) == 0
    sv[need[~good[need]]] = batch.V_L4_BAD
    due = np.zeros(n, bool)
    np.logical_or.at(due, np.arange(sv.size) // cnt, np.isin(sv, (batch.V_ACCEPT, batch.V_TCP_OLD, batch.V_TCP_HELD)))
    held = np.zeros(n, np.int64)
    left, right = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    for g in np.unique(need // cnt):                                        # tcp_sack_prepare per connection with held segments
        if not conn[g, 1] & 1:
            continue
        q = {}
        for j in range(g * cnt, (g + 1) * cnt):
            if sv[j] == batch.V_TCP_HELD and int(seq[j]) not in q:
                q[int(seq[j])] = int(pl[j])
        held[g] = sum(q.values())
        order = sorted(q, key=lambda x: (x - int(rcv[g])) & 0xFFFFFFFF)
        if order and order[0] >= int(rcv[g]):                               # one contiguous run from the first segment
            a = b = order[0]
            while b in q:
                b = (b + q[b]) & 0xFFFFFFFF
            left[g], right[g] = a, b
    space = np.maximum(0, ak["space"].astype(np.int64) - ol - held)
    shift = np.zeros(n, np.uint8)
    while (space > 0xFFFF).any():
        big = space > 0xFFFF
        space[big] >>= 1
        shift[big] += 1
    blk = left != 0
    frames = np.full((n, REGION), 0xA5, np.uint8)
    for has in (False, True):
        g = np.flatnonzero(due & (blk == has))
        if not g.size:
            continue
        thl = 44 if has else 36
        f = np.zeros((g.size, 20 + thl), np.uint8)
        f[:, :40] = s["h_tmpl"][g]
        f[:, 2:4] = [(20 + thl) >> 8, (20 + thl) & 0xFF]
        f[:, 6:8], f[:, 10:12] = [0x40, 0], 0
        f[:, 10:12] = fold(be_sum(f[:, :20])).astype(">u2").view(np.uint8).reshape(-1, 2)
        f[:, 28:32] = rcv[g].astype(">u4").view(np.uint8).reshape(-1, 4)
        f[:, 32] = (thl << 2) | (f[:, 32] & 0x0F)
        f[:, 33] = 0x10
        f[:, 34:36] = space[g].astype(">u2").view(np.uint8).reshape(-1, 2)
        f[:, 36:38] = 0
        f[:, 40:] = 1
        f[:, 40], f[:, 41], f[:, 42] = 3, 3, shift[g]
        f[:, 43], f[:, 44] = 8, 10
        f[:, 45:49] = ak["tsval"][g].astype(">u4").view(np.uint8).reshape(-1, 4)
        f[:, 49:53] = ak["tsecr"][g].astype(">u4").view(np.uint8).reshape(-1, 4)
        if has:
            f[:, 53], f[:, 54] = 5, 10
            f[:, 55:59] = left[g].astype(">u4").view(np.uint8).reshape(-1, 4)
            f[:, 59:63] = right[g].astype(">u4").view(np.uint8).reshape(-1, 4)
        f[:, -1] = 0
        f[:, 36:38] = fold(be_sum(f[:, 12:20]) + 6 + thl + be_sum(f[:, 20:])).astype(">u2").view(np.uint8).reshape(-1, 2)
        frames[g, :20 + thl] = f
    dev_frames = torch.from_numpy(frames.reshape(-1)).to(dev)               # H2D
    torch.cuda.synchronize(dev)
    return frames, dev_frames


def run_burst(name, n, P, a, dev, disturb):
    per, stride = a.per, a.stride
    sets = [make_set(n, P, per, stride, dev, 900 + i, disturb) for i in range(a.rotate)]
    cnt = sets[0]["cnt"]
    stream = torch.cuda.current_stream(dev)

    def coalesce(s, st):
        batch.tcp_coalesce_batch(s["out"], s["of"], s["n_seg"], s["grp"], s["conn"], s["rbuf"], s["rod"], stream=st,
                                 results=s["rres"])

    def ack_only(s, st, sv=None):
        batch.tcp_ack_batch(s["out"], s["of"], s["n_seg"], s["grp"], s["conn"], s["rres"][1], s["rres"][2] if sv is None else sv,
                            s["tmpl"], s["td"], s["ack"], s["abuf"], s["aod"], stream=st, results=s["ares"])

    def ack(s, st):
        with torch.cuda.stream(st):
            s["sv0"].copy_(s["svc"])                        # the verdicts as the coalescing wrote them
        ack_only(s, st, s["sv0"])

    def coalesce_ack(s, st):
        coalesce(s, st)
        ack_only(s, st)

    host_us = []
    for s in sets:
        s["abuf"].fill_(0xA5)
        coalesce(s, stream)
        torch.cuda.synchronize(dev)
        if not bool((s["rres"][0] == batch.V_ACCEPT).all()):
            raise SystemExit(f"{name}: the coalescing does not accept every connection")
        s["svc"] = s["rres"][2].clone()
        want, _ = host_pass(s, n, cnt, dev)
        ack_only(s, stream)
        torch.cuda.synchronize(dev)
        got = s["abuf"].cpu().numpy()[:n * REGION].reshape(n, REGION)
        if not (bool((s["ares"][0] == batch.V_ACCEPT).all()) and np.array_equal(got, want)):
            raise SystemExit(f"{name}: the device's ACK frames do not equal the host pass's")
        s["rres"][2].copy_(s["svc"])
    for _ in range(a.host_reps):
        s = sets[len(host_us) % len(sets)]
        s["rres"][2].copy_(s["svc"])
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        host_pass(s, n, cnt, dev)
        host_us.append((time.perf_counter() - t0) * 1e6)
    times = SG.time_legs({"coalesce": coalesce, "ack": ack, "coalesce_ack": coalesce_ack}, sets, dev, stream, a.warmup,
                         a.replays, a.rotate)
    sv = sets[0]["svc"].cpu().numpy()
    summed = int(np.isin(sv, (batch.V_TCP_OLD, batch.V_TCP_HELD)).sum())
    r = {"shape": name.replace("tcpseg", "tcpack") + ("_disturbed" if disturb else "_in_order"), "connections": n,
         "payload_bytes_per_connection": P, "per": per, "segments": cnt, "disturbed_percent": disturb,
         "old_or_held_segments_summed": summed, "rotate": a.rotate, "replays": a.replays,
         "frames_equal_the_host_pass_before_timing": True}
    frames = n * 56
    moved = {"coalesce": n * (cnt * 52 + P) + 16 * n * cnt + n * 32 + n * P + n * 5 + n * cnt,
             "ack": n * cnt + summed * (52 + per) + n * (8 + 8 + 4 + 16 + 40 + 16 + 16) + frames + n * cnt}
    moved["coalesce_ack"] = moved["coalesce"] + moved["ack"] - n * cnt
    SG.summarise(r, times, moved, n * P, bytes_key=True)
    r["host_pass_us"] = round(float(np.median(host_us)), 1)
    r["host_pass_us_min_max"] = [round(min(host_us), 1), round(max(host_us), 1)]
    r["host_pass_reps"] = a.host_reps
    r["ack_over_coalesce"] = round(r["ack_us"] / r["coalesce_us"], 3)
    r["coalesce_ack_over_sum_of_both"] = round(r["coalesce_ack_us"] / (r["coalesce_us"] + r["ack_us"]), 3)
    r["host_pass_over_ack"] = round(r["host_pass_us"] / r["ack_us"], 1)
    return r


def run_shape(name, n, P, a, dev, lib):
    r = run_burst(name, n, P, a, dev, 0)
    import json
    print(json.dumps(r), flush=True)
    torch.cuda.empty_cache()
    d = run_burst(name, n, P, a, dev, a.disturb)
    d["in_order"] = r
    return d


if __name__ == "__main__":
    SG.main("tcpack_bench.py", "connections", (("--per", 1448), ("--disturb", 25), ("--host-reps", 5)),
            ("tcpseg_64512", "tcpseg_9000"), run_shape)
