#!/usr/bin/env python3
"""Measurement aid: the ICMPv6 answer batch (pico_icmp6_reply_batch_dev) beside the ICMPv4 answer batch at the
same transport size and beside the copy ceilings -- the same process, the legs alternating replay by replay
(sg_harness.time_legs).  Nothing here is a pass mark.

Shapes: echo requests of 64, 1460 and 9000 transport bytes (262144, 65536 and 29360 records), and a burst of
65536 UDP datagrams of 1500 bytes to a closed port (type 1 code 4: 1232 quoted bytes, an answer of 1280).
Legs, per shape:
  icmp6           icmp6_reply_batch: the answers, the transport / the quote copied and summed in one pass
  icmp4           icmp4_reply_batch (no carried state) on echo requests of the same transport bytes -- for the
                  closed-port shape: of the notice's 1240 transport bytes
  bare_scatter_flat, seq_copy   tools/gather_ceiling.hip's bare copy of those transports from request to
                  answer (one wave per pair, nothing summed, no headers) and the device's contiguous copy of
                  the same byte count, both over the ICMPv4 leg's buffers.  Without
                  tools/bin/libgather_ceiling.so they are left out, with a warning and a note in the JSON
Datagrams and regions start on 16-byte lines (the moved bytes on a line at both ends).  Each leg runs over
rotating buffer sets whose sum exceeds the 256 MiB Infinity Cache; one replay = one pass over every set,
captured as a HIP graph; the figure is the median of --replays (>= 20) replays timed by HIP events, per call.
Before timing, every ICMPv6 answer of every set is checked at the timed size: ACCEPT, and ACCEPT with result
0 in the IPv6 RX batch.

  python tools/icmp6_bench.py [--shape 64|1460|9000|closed_port|all] [--replays 24] [--out profiles/icmp6/x.json]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import icmp4_bench as B4  # noqa: E402
import sg_harness as SG  # noqa: E402
from picotcp_amd import batch  # noqa: E402

SHAPES = {"64": (262144, 64), "1460": (65536, 1460), "9000": (29360, 9000)}
CLOSED_PORT = (65536, 1500)
HOST = bytes.fromhex("20010db8000000010000000000000001")


def make_set6(n, T, dev, seed, rtype):
    """n IPv6 datagrams of 40 + T bytes on 16-byte lines -- ICMPv6 echo requests, (id, seq) = the index, or UDP
    (rtype 1) -- with random payload, and the answers' regions on lines of their own."""
    size = 40 + T
    pitch = (size + 15) // 16 * 16
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    off = np.arange(n, dtype=np.int64) * pitch
    idx = np.arange(n, dtype=np.uint32)
    hdr = np.zeros((n, 48), np.uint8)
    hdr[:, 0], hdr[:, 4], hdr[:, 5], hdr[:, 6], hdr[:, 7] = 0x60, T >> 8, T & 0xFF, 17 if rtype else 58, 64
    hdr[:, 8:24] = np.frombuffer(bytes.fromhex("20010db8000000010000000000000099"), np.uint8)
    hdr[:, 20:24] = idx.byteswap().view(np.uint8).reshape(n, 4)
    hdr[:, 24:40] = np.frombuffer(HOST, np.uint8)
    if rtype:
        hdr[:, 40:48] = [0x0F, 0xA0, 0x0F, 0xA1, T >> 8, T & 0xFF, 0, 0]
    else:
        hdr[:, 40] = 128
        hdr[:, 44:48] = idx.byteswap().view(np.uint8).reshape(n, 4)
    at = torch.from_numpy((off[:, None] + np.arange(48)[None, :]).reshape(-1)).to(dev)
    buf = torch.randint(0, 256, (n * pitch + 16,), dtype=torch.uint8, device=dev, generator=g)
    buf[at] = torch.from_numpy(hdr.reshape(-1)).to(dev)
    alen = 48 + min(size, 1232) if rtype else size
    opitch = (alen + 15) // 16 * 16
    req = np.zeros(n, batch.ICMP6_REQ_DTYPE)
    req["src"], req["type"], req["code"], req["hop"] = np.frombuffer(HOST, np.uint8), rtype, 4 if rtype else 0, 64
    return dict(buf=buf, desc=batch.desc_to_device(batch.make_desc(off, np.full(n, size)), dev),
                req=torch.from_numpy(req.view(np.uint8).copy()).to(dev), out=torch.zeros(n * opitch + 16, dtype=torch.uint8, device=dev),
                od=batch.desc_to_device(batch.make_desc(np.arange(n, dtype=np.int64) * opitch, np.full(n, alen)), dev),
                res=(torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(16 * n, dtype=torch.uint8, device=dev)), alen=alen)


def run_shape(name, n, T, rtype, a, dev, lib):
    T4 = 8 + 1232 if rtype else T                           # the ICMPv4 leg's transport: what the ICMPv6 answer carries
    per_set = n * (2 * (40 + T) + 2 * (20 + T4))
    rotate = max(a.rotate, -(-B4.PAST_CACHE // per_set))
    sets = [dict(v6=make_set6(n, T, dev, 900 + i, rtype), v4=B4.make_set(n, 20 + T4, dev, 950 + i)) for i in range(rotate)]
    stream = torch.cuda.current_stream(dev)

    def icmp6(s, st):
        s = s["v6"]
        batch.icmp6_reply_batch(s["buf"], s["desc"], n, s["req"], s["out"], s["od"], stream=st, results=s["res"])

    def icmp4(s, st):
        s = s["v4"]
        batch.icmp4_reply_batch(s["buf"], s["desc"], n, s["req"], s["out"], s["od"], state=None, stream=st, results=s["res"])

    def bare(s, st):
        s = s["v4"]
        assert lib.gather_ceiling_launch(3, s["buf"].data_ptr(), s["buf"].numel(), s["f_src"].data_ptr(), s["f_dst"].data_ptr(),
                                         s["f_len"].data_ptr(), s["grp"].data_ptr(), n, n, s["out"].data_ptr(), s["out"].numel(),
                                         ctypes.c_void_p(st.cuda_stream)) == 0

    payload = n * T4

    def seq(s, st):
        s = s["v4"]
        assert lib.seq_copy_launch(0, 4, 0, s["copy"].data_ptr(), s["buf"].data_ptr(), payload & ~15, ctypes.c_void_p(st.cuda_stream)) == 0

    ok = True
    for s in sets:
        icmp6(s, stream)
        icmp4(s, stream)
        l4, rv = batch.ipv6_checksum_batch(s["v6"]["out"], s["v6"]["res"][1], n, flags=batch.F_NXTHDR_DISPATCH)
        torch.cuda.synchronize(dev)
        ok = ok and bool((s["v6"]["res"][0] == batch.V_ACCEPT).all() and (rv == batch.V_ACCEPT).all() and (l4 == 0).all()
                         and (s["v4"]["res"][0] == batch.V_ACCEPT).all())
        del l4, rv
    if not ok:
        raise SystemExit(f"{name}: the answers do not verify in the RX batch at the timed size")
    legs = {"icmp6": icmp6, "icmp4": icmp4}
    if lib is not None:
        legs.update({"bare_scatter_flat": bare, "seq_copy": seq})
    times = SG.time_legs(legs, sets, dev, stream, a.warmup, a.replays, rotate)
    alen = sets[0]["v6"]["alen"]
    read6 = n * (min(40 + T, 1232) if rtype else 40 + T)
    # bytes the algorithm needs: read = datagrams (a notice: the quote) + descriptors, records, regions; written = answers + descriptors + verdicts
    moved = {"icmp6": read6 + n * 56 + n * alen + n * 17, "icmp4": n * (20 + T4) + n * 40 + n * (20 + T4) + n * 17}
    r = {"shape": name, "records": n, "transport_bytes": T, "answer_bytes": alen, "icmp4_transport_bytes": T4, "rotate": rotate,
         "replays": a.replays, "answers_verified_in_rx_batch": ok, "launch_shape": "one record a wave" if 40 + T >= 1024 else "two records a wave"}
    SG.summarise(r, times, moved, payload, bytes_key=True)
    r["icmp6_over_icmp4"] = round(r["icmp6_us"] / r["icmp4_us"], 3)
    if lib is not None:
        for k in ("bare_scatter_flat", "seq_copy"):
            r["icmp6_over_" + k] = round(r["icmp6_us"] / r[k + "_us"], 3)
        r["ceiling_store_path"] = "non-temporal whole-unit stores; the icmp6 and icmp4 legs use cached stores"
    else:
        r["ceiling_legs"] = SG.CEILING_NOT_MEASURED
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all", choices=list(SHAPES) + ["closed_port", "all"])
    ap.add_argument("--n", type=int, default=0, help="records (0: the shape's own count)")
    ap.add_argument("--rotate", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--replays", type=int, default=24)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.replays < 20:
        raise SystemExit("--replays: at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("icmp6_bench.py measures on the GPU: no HIP device here (not measured)")
    dev = torch.device("cuda:0")
    lib = SG.load_ceiling_lib("icmp6_bench.py")
    results = []
    for key in (list(SHAPES) + ["closed_port"]) if a.shape == "all" else [a.shape]:
        if key == "closed_port":
            r = run_shape("icmp6_closed_port_1500", a.n or CLOSED_PORT[0], CLOSED_PORT[1] - 40, 1, a, dev, lib)
        else:
            r = run_shape(f"icmp6_echo_{key}", a.n or SHAPES[key][0], SHAPES[key][1], 0, a, dev, lib)
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
