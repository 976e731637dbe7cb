"""Device helpers shared by the GPU tests: a plain module, no fixtures."""
from __future__ import annotations

import numpy as np
import torch

DEV = "cuda:0"


def to_dev(a) -> torch.Tensor:
    return torch.from_numpy(np.array(a, copy=True, order="C")).to(DEV)      # (a copy: golden fixtures' arrays are read-only)


def pairs_dev(a) -> torch.Tensor:
    """uint32 pairs per group ((first, count), (rcv_nxt, cflags)) as the batches take them: an int32 tensor of 2*n."""
    return to_dev(np.ascontiguousarray(a, np.uint32).reshape(-1).view(np.int32))


def replay_captured(call, reset, check, times=2):
    """call(stream) captured into a graph on a side stream; then `times` times reset(), one replay, check()."""
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            call(s)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(times):
        reset()
        g.replay()
        torch.cuda.synchronize()
        check()
