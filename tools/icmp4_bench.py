#!/usr/bin/env python3
"""Measurement aid: the ICMPv4 answer batch (pico_icmp4_reply_batch_dev) beside the TCP segmentation batch
on bytes of the same shape, beside the copy ceilings and beside the host pass it replaces -- the same
process, the legs alternating replay by replay (sg_harness.time_legs).

Echo shapes: 262144 x 84-byte datagrams (the 56-byte ping), 29360 x 9000 bytes, 4096 x 64512 bytes; every
request its own (id, seq), the duplicate state carried (four launches a call).  Legs, per shape:
  echo            icmp4_reply_batch: the answers, transport copied and summed in one pass
  segment         tcp_segment_batch on streams of the same byte count, one segment a stream (per = the whole
                  payload): one header a record, as the echo leg -- the nearest existing kernel of the same
                  kind, the yardstick
  bare_scatter_*  tools/gather_ceiling.hip's bare copy of every transport from its place in the request to its
                  place in the answer, nothing summed, no headers (flat: one wave per pair, the echo kernel's
                  shape; 4waves: four waves a datagram).  Non-temporal whole-unit stores: a ratio to these
                  legs crosses two store paths.  Without tools/bin/libgather_ceiling.so these legs and
                  seq_copy are left out, with a warning and a note in the JSON
  seq_copy        the device's contiguous copy of the transport bytes
  host pass       D2H of the burst, the replies built in numpy (vectorised: header, type 0, both checksums),
                  H2D of the answers: wall clock, the median of --host-reps
A fourth shape times 262144 Time Exceeded notices (84-byte datagrams) behind the forwarding batch: the
notices alone, the forwarding batch alone, and both in one graph.  (The forwarding step decrements every
ttl on every replay; its time does not depend on the verdicts.)
Each leg runs over rotating buffer sets whose sum exceeds the 256 MiB Infinity Cache (at least --rotate,
more for the short shape); one replay = one pass over every set, captured as a HIP graph; the figure is the
median of --replays (>= 20) replays timed by HIP events, per call.  Before timing, every answer of every
set is checked at the timed size: ACCEPT with both checksums verifying (0) in the IPv4 RX batch.

  python tools/icmp4_bench.py [--shape 84|9000|64512|notice|all] [--replays 24] [--out profiles/icmp4/x.json]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sg_harness as SG  # noqa: E402
from picotcp_amd import batch  # noqa: E402

H = 52                  # the segment leg's headers: 20 + a 32-byte TCP header
SHAPES = {"84": (262144, 84), "9000": (29360, 9000), "64512": (4096, 64512)}
PAST_CACHE = 768 << 20  # the rotating sets' bytes, in and out, at least


def dv(x, dev):
    return torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x.view(np.int32)).to(dev)


def make_set(n, size, dev, seed, ttl=64, rtype=0):
    """n IPv4 / ICMP echo requests of `size` bytes, 12 mod 16 into 16-byte lines (the transport on a line),
    random payload, (id, seq) = the index; the answers' regions 8 mod 16 (the moved bytes on a line); and
    the segment leg's streams of the same size in a buffer of its own."""
    pitch = (size + 12 + 15) // 16 * 16
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    off = 12 + np.arange(n, dtype=np.int64) * pitch
    idx = np.arange(n, dtype=np.uint32)
    hdr = np.zeros((n, 28), np.uint8)
    hdr[:, 0], hdr[:, 6], hdr[:, 8], hdr[:, 9] = 0x45, 0x40, ttl, 1
    hdr[:, 2], hdr[:, 3] = size >> 8, size & 0xFF
    hdr[:, 4:6] = idx.astype(np.uint16).byteswap().view(np.uint8).reshape(n, 2)
    hdr[:, 12:20] = [192, 168, 7, 2, 10, 1, 2, 3]
    hdr[:, 20] = 8
    hdr[:, 24:28] = idx.byteswap().view(np.uint8).reshape(n, 4)
    at = torch.from_numpy((off[:, None] + np.arange(28)[None, :]).reshape(-1)).to(dev)
    buf = torch.randint(0, 256, (n * pitch + 16,), dtype=torch.uint8, device=dev, generator=g)
    buf[at] = torch.from_numpy(hdr.reshape(-1)).to(dev)
    alen = size if rtype == 0 else 56
    opitch = (alen + 8 + 15) // 16 * 16
    ooff = 8 + np.arange(n, dtype=np.int64) * opitch
    req = np.zeros(n, batch.ICMP4_REQ_DTYPE)
    req["src"], req["id"], req["type"] = int.from_bytes(bytes([10, 1, 2, 3]), "little"), idx & 0xFFFF, rtype
    s = dict(buf=buf, desc=batch.desc_to_device(batch.make_desc(off, np.full(n, size)), dev),
             req=torch.from_numpy(req.view(np.uint8).copy()).to(dev), out=torch.zeros(n * opitch + 16, dtype=torch.uint8, device=dev),
             od=batch.desc_to_device(batch.make_desc(ooff, np.full(n, alen)), dev), state=batch.icmp4_state(dev),
             res=(torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(16 * n, dtype=torch.uint8, device=dev)),
             fv=torch.empty(n, dtype=torch.uint8, device=dev), fst=batch.fwd_state(dev), pitch=pitch, opitch=opitch)
    if rtype:
        return s
    # the segment leg: the same byte count a stream, one segment a stream
    stride = (size + 15) // 16 * 16
    sh = np.zeros((n, H), np.uint8)
    sh[:, 0], sh[:, 8], sh[:, 9] = 0x45, 64, 6
    sh[:, 4:6] = hdr[:, 4:6]
    sh[:, 12:20] = [10, 1, 2, 3, 192, 168, 7, 2]
    sh[:, 20:24] = [0, 80, 0x9C, 0x40]
    sh[:, 32], sh[:, 33], sh[:, 34] = 0x80, 0x18, 0x20
    sh[:, 40:52] = [1, 1, 8, 10, 0, 1, 2, 3, 0, 4, 5, 6]
    sbuf = torch.randint(0, 256, (n * pitch + 16,), dtype=torch.uint8, device=dev, generator=g)
    at = torch.from_numpy((off[:, None] + np.arange(H)[None, :]).reshape(-1)).to(dev)
    sbuf[at] = torch.from_numpy(sh.reshape(-1)).to(dev)
    soff = 12 + np.arange(n, dtype=np.int64) * (stride + 16)
    groups = np.stack([np.arange(n), np.ones(n)], axis=1).astype(np.uint32)
    s.update(sbuf=sbuf, sd=batch.desc_to_device(batch.make_desc(off, np.full(n, size), np.full(n, size - H)), dev),
             grp=torch.from_numpy(groups.reshape(-1).view(np.int32)).to(dev), stride=stride,
             sout=torch.zeros(int(soff[-1] + stride + 16), dtype=torch.uint8, device=dev),
             sod=batch.desc_to_device(batch.make_desc(soff, np.full(n, stride)), dev),
             sres=(torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.int32, device=dev)),
             f_src=dv((off + 24).astype(np.uint64), dev), f_dst=dv((ooff + 24).astype(np.uint64), dev),
             f_len=dv(np.full(n, size - 24, np.uint32), dev), copy=torch.empty(n * (size - 20) + 16, dtype=torch.uint8, device=dev))
    return s


def fold(s):
    s = (s & 0xFFFF) + (s >> 16)
    s = (s & 0xFFFF) + (s >> 16)
    return (~s & 0xFFFF).astype(np.uint16)


def host_pass(s, n, size, stage):
    """What the batch replaces: the burst to the host, every reply built there (numpy over the whole burst),
    the replies back to the device.  Returns the seconds."""
    t0 = time.perf_counter()
    h = s["buf"].cpu().numpy()
    m = h[:n * s["pitch"]].reshape(n, s["pitch"])[:, 12:12 + size]
    a = np.empty((n, size + (size & 1)), np.uint8)
    a[:, size:] = 0
    a[:, 20:size] = m[:, 20:]
    a[:, 20], a[:, 22], a[:, 23] = 0, 0, 0
    a[:, :20] = 0
    a[:, 0], a[:, 8], a[:, 9] = 0x45, 64, 1
    a[:, 2], a[:, 3] = size >> 8, size & 0xFF
    a[:, 4:8] = m[:, 4:8]
    a[:, 12:16], a[:, 16:20] = [10, 1, 2, 3], m[:, 12:16]
    w = a.view("<u2")
    a[:, 22:24] = fold(w[:, 10:].sum(axis=1, dtype=np.uint64)).view(np.uint8).reshape(n, 2)
    a[:, 10:12] = fold(w[:, :10].sum(axis=1, dtype=np.uint64)).view(np.uint8).reshape(n, 2)
    stage.copy_(torch.from_numpy(a))
    torch.cuda.synchronize()
    return time.perf_counter() - t0, a


def run_echo(name, n, size, a, dev, lib):
    per_set = n * ((size + 27) // 16 * 16 + (size + 23) // 16 * 16)
    rotate = max(a.rotate, -(-PAST_CACHE // per_set))
    sets = [make_set(n, size, dev, 700 + i) for i in range(rotate)]
    stream = torch.cuda.current_stream(dev)
    T = size - 20

    def echo(s, st):
        batch.icmp4_reply_batch(s["buf"], s["desc"], n, s["req"], s["out"], s["od"], state=s["state"], stream=st, results=s["res"])

    def segment(s, st):
        batch.tcp_segment_batch(s["sbuf"], s["sd"], s["grp"], n, s["sout"], s["sod"], s["stride"], stream=st, results=s["sres"])

    def bare(mode):
        def f(s, st):
            assert lib.gather_ceiling_launch(mode, s["buf"].data_ptr(), s["buf"].numel(), s["f_src"].data_ptr(),
                                             s["f_dst"].data_ptr(), s["f_len"].data_ptr(), s["grp"].data_ptr(), n, n,
                                             s["out"].data_ptr(), s["out"].numel(), ctypes.c_void_p(st.cuda_stream)) == 0
        return f

    payload = n * T

    def seq(s, st):
        assert lib.seq_copy_launch(0, 4, 0, s["copy"].data_ptr(), s["buf"].data_ptr(), payload & ~15,
                                   ctypes.c_void_p(st.cuda_stream)) == 0

    # every answer at the timed size, checked once through the RX verify batch; the host pass's too
    ok = True
    for s in sets:
        echo(s, stream)
        net, l4, rv = batch.ipv4_checksum_batch(s["out"], s["res"][1], n)
        segment(s, stream)
        torch.cuda.synchronize(dev)
        ok = ok and bool((s["res"][0] == batch.V_ACCEPT).all() and (rv == batch.V_ACCEPT).all() and (net == 0).all()
                         and (l4 == 0).all() and (s["sres"][0] == batch.V_ACCEPT).all())
        del net, l4, rv
    if not ok:
        raise SystemExit(f"{name}: the answers do not verify in the RX batch at the timed size")
    stage = torch.empty((n, size + (size & 1)), dtype=torch.uint8, device=dev)
    host = []
    for k in range(a.host_reps):
        secs, ans = host_pass(sets[0], n, size, stage)
        host.append(secs)
    got = sets[0]["out"][:n * sets[0]["opitch"]].reshape(n, sets[0]["opitch"])[:, 8:8 + size].cpu().numpy()
    host_equal = bool(np.array_equal(got[:, 6:], ans[:, 6:size]))           # (all but the id: the host pass copies the request's)
    del stage, ans, got

    legs = {"echo": echo, "segment": segment}
    if lib is not None:
        legs.update({"bare_scatter_flat": bare(3), "bare_scatter_4waves": bare(2), "seq_copy": seq})
    times = SG.time_legs(legs, sets, dev, stream, a.warmup, a.replays, rotate)
    for s in sets:
        if not bool((s["res"][0] == batch.V_ACCEPT).all() and (s["sres"][0] == batch.V_ACCEPT).all()):
            raise SystemExit(f"{name}: a timed replay did not accept every record")
    # bytes the algorithm needs: read = requests + descriptors, records, regions; written = answers + descriptors + verdicts
    moved = {"echo": n * size + n * 40 + n * size + n * 17, "segment": n * size + n * 40 + n * size + n * 5}
    r = {"shape": name, "records": n, "datagram_bytes": size, "transport_bytes": T, "rotate": rotate, "replays": a.replays,
         "working_set_bytes_per_set": int(sets[0]["buf"].numel() + sets[0]["out"].numel()), "payload_bytes": payload,
         "answers_verified_in_rx_batch": ok, "host_pass_equals_device": host_equal,
         "host_pass_us": round(float(np.median(host)) * 1e6, 1), "host_pass_reps": a.host_reps}
    SG.summarise(r, times, moved, payload, bytes_key=True)
    r["echo_over_segment"] = round(r["echo_us"] / r["segment_us"], 3)
    r["host_pass_over_echo"] = round(r["host_pass_us"] / r["echo_us"], 1)
    if lib is not None:
        for k in ("bare_scatter_flat", "bare_scatter_4waves", "seq_copy"):
            r["echo_over_" + k] = round(r["echo_us"] / r[k + "_us"], 3)
        r["ceiling_store_path"] = "non-temporal whole-unit stores; echo and segment legs use cached stores"
    else:
        r["ceiling_legs"] = SG.CEILING_NOT_MEASURED
    return r


def run_notice(name, n, size, a, dev):
    rotate = max(a.rotate, -(-PAST_CACHE // (n * (96 + 64))))
    sets = [make_set(n, size, dev, 800 + i, ttl=1, rtype=11) for i in range(rotate)]
    stream = torch.cuda.current_stream(dev)

    def notice(s, st):
        batch.icmp4_reply_batch(s["buf"], s["desc"], n, s["req"], s["out"], s["od"], state=None, stream=st, results=s["res"])

    def forward(s, st):
        batch.ipv4_forward_batch(s["buf"], s["desc"], n, state=s["fst"], verdict=s["fv"], stream=st)

    def both(s, st):
        forward(s, st)
        notice(s, st)

    ok = True
    for s in sets:
        both(s, stream)
        net, l4, rv = batch.ipv4_checksum_batch(s["out"], s["res"][1], n)
        torch.cuda.synchronize(dev)
        ok = ok and bool((s["fv"] == batch.V_EXPIRED).all() and (s["res"][0] == batch.V_ACCEPT).all()
                         and (rv == batch.V_ACCEPT).all() and (net == 0).all() and (l4 == 0).all())
        del net, l4, rv
    if not ok:
        raise SystemExit(f"{name}: the notices do not verify in the RX batch at the timed size")
    times = SG.time_legs({"notice": notice, "forward": forward, "forward_notice": both}, sets, dev, stream, a.warmup, a.replays,
                         rotate)
    moved = {"notice": n * 28 + n * 40 + n * 56 + n * 17, "forward": n * 20 + n * 16 + n * 4 + n, "forward_notice": 0}
    moved["forward_notice"] = moved["notice"] + moved["forward"]
    r = {"shape": name, "records": n, "datagram_bytes": size, "rotate": rotate, "replays": a.replays,
         "notices_verified_in_rx_batch": ok}
    SG.summarise(r, times, moved, n * 28, bytes_key=True)
    r["graph_over_sum_of_parts"] = round(r["forward_notice_us"] / (r["forward_us"] + r["notice_us"]), 3)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all", choices=list(SHAPES) + ["notice", "all"])
    ap.add_argument("--n", type=int, default=0, help="records (0: the shape's own count)")
    ap.add_argument("--rotate", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--replays", type=int, default=24)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.replays < 20:
        raise SystemExit("--replays: at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("icmp4_bench.py measures on the GPU: no HIP device here (not measured)")
    dev = torch.device("cuda:0")
    lib = SG.load_ceiling_lib("icmp4_bench.py")
    results = []
    for key in (list(SHAPES) + ["notice"]) if a.shape == "all" else [a.shape]:
        if key == "notice":
            r = run_notice("icmp4_time_exceeded_84", a.n or 262144, 84, a, dev)
        else:
            r = run_echo(f"icmp4_echo_{key}", a.n or SHAPES[key][0], SHAPES[key][1], a, dev, lib)
        print(json.dumps(r), flush=True)
        results.append(r)
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "results": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
