"""The measurement scaffold of the scatter/gather batch tools (fragtx_bench.py, tcpseg_bench.py,
tcprx_bench.py), stated once: the ceiling library's prototypes (gather_ceiling.py loads it here too),
the common arguments, one HIP graph per leg over the rotating buffer sets, the warm-up, the timing
loop that alternates the legs replay by replay under HIP events, the per-leg summary and the JSON
writer.  A tool keeps what is its own: its sets, its legs and their order, its checks before and
after timing, its byte counts and its ratios.
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
HBM_PEAK = 8.0e12       # MI355X HBM3E, bytes / s (datasheet)
CEILING_LIB = os.path.join("tools", "bin", "libgather_ceiling.so")
CEILING_NOT_MEASURED = f"not measured: {CEILING_LIB} is not built"


def load_ceiling_lib(tool):
    """tools/gather_ceiling.hip's library with both prototypes set, or None -- with a warning on stderr
    -- where it is not built."""
    p = os.path.join(ROOT, CEILING_LIB)
    if not os.path.exists(p):
        print(f"{tool}: {CEILING_LIB} is not built (__graft_entry__.build() builds it): the bare copy and seq_copy "
              "legs and their ratios are NOT measured in this run", file=sys.stderr, flush=True)
        return None
    lib = ctypes.CDLL(p)
    lib.seq_copy_launch.restype = ctypes.c_int
    lib.seq_copy_launch.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
                                    ctypes.c_uint64, ctypes.c_void_p]
    lib.gather_ceiling_launch.restype = ctypes.c_int
    lib.gather_ceiling_launch.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64] + [ctypes.c_void_p] * 4 + \
        [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    return lib


def time_legs(legs, sets, dev, stream, warmup, replays, rotate):
    """legs = {name: f(set, stream)}.  One graph per leg, captured on a side stream over all sets; after
    `warmup` rounds, `replays` rounds in which the legs take turns in the order of `legs` -- which is
    therefore the caller's to decide -- each replay between two events.  Returns {name: [us per call]}."""
    graphs = {}
    for nm, f in legs.items():
        gph = torch.cuda.CUDAGraph()
        cs = torch.cuda.Stream(dev)
        cs.wait_stream(stream)
        with torch.cuda.stream(cs):
            with torch.cuda.graph(gph, stream=cs):
                for s in sets:
                    f(s, cs)
        stream.wait_stream(cs)
        graphs[nm] = gph
    for _ in range(warmup):
        for gph in graphs.values():
            gph.replay()
    torch.cuda.synchronize(dev)
    times = {nm: [] for nm in legs}
    for _ in range(replays):                                 # the legs alternate, replay by replay
        for nm, gph in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            gph.replay()
            e1.record(stream)
            torch.cuda.synchronize(dev)
            times[nm].append(e0.elapsed_time(e1) * 1e3 / rotate)
    return times


def summarise(r, times, moved_of, payload, bytes_key=False):
    """Per leg, into r: the median us, min / max, TB/s and the fraction of the HBM peak over the bytes
    moved_of[leg] (a bare copy, not listed there: the payload read and written); bytes_key records
    those bytes too."""
    for nm, v in times.items():
        us = float(np.median(v))
        b = moved_of.get(nm, 2 * payload)
        r[nm + "_us"] = round(us, 2)
        r[nm + "_us_min_max"] = [round(min(v), 2), round(max(v), 2)]
        if bytes_key:
            r[nm + "_algorithmic_bytes"] = b
        r[nm + "_TBs"] = round(b / us / 1e6, 3)
        r[nm + "_fraction_of_8TBs"] = round(b / (us * 1e-6) / HBM_PEAK, 3)


def main(tool, units, extra, names, run_shape):
    """The command line of a tool: `extra` = its own (flag, default) integers, names = its (64512-byte,
    9000-byte) shapes; run_shape(name, n, bytes, args, device, ceiling lib) -> one result, printed as
    a JSON line and collected into --out."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="both", choices=["c3", "9000", "both"])
    ap.add_argument("--n", type=int, default=0, help=f"{units} (0: 4096 x 64512 B, or as many 9000 B ones for the same bytes)")
    for flag, default in extra:
        ap.add_argument(flag, type=int, default=default)
    ap.add_argument("--stride", type=int, default=1504)
    ap.add_argument("--rotate", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--replays", type=int, default=24)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.replays < 20:
        raise SystemExit("--replays: at least 20")
    if not torch.cuda.is_available():
        raise SystemExit(f"{tool} measures on the GPU: no HIP device here (not measured)")
    dev = torch.device("cuda:0")
    lib = load_ceiling_lib(tool)
    shapes = []
    if a.shape in ("c3", "both"):
        shapes.append((names[0], a.n or 4096, 64512))
    if a.shape in ("9000", "both"):
        shapes.append((names[1], a.n or 4096 * 64512 // 9000, 9000))
    results = []
    for name, n, size in shapes:
        r = run_shape(name, n, size, a, dev, lib)
        print(json.dumps(r), flush=True)
        results.append(r)
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "results": results}, f, indent=1)
            f.write("\n")
