"""CPU tests of pico_flow_group_batch_dev's argument checks and of pico_flow_group_scratch_bytes
(include/pico_csum.h): every refusal comes before any device work, so none of this launches anything."""
from __future__ import annotations

import ctypes
import os
import re

import pytest
import torch

from picotcp_amd import _lib, batch

vp = ctypes.c_void_p
HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "pico_csum.h")


def scratch_bytes(n, n_known=0):
    return _lib.load().pico_flow_group_scratch_bytes(n, n_known)


def args(**kw):
    """A well-formed call (fake device addresses), fields replaced by keyword."""
    a = dict(d_base=vp(0x1000), base_len=1 << 20, d_desc=vp(0x2000), n=16, d_verdict_in=vp(0x2800), mode_flags=_lib.FLOW_TCP,
             d_known=vp(0x3000), n_known=4, hash_seed=7, d_out_desc=vp(0x4000), d_out_index=vp(0x5000),
             d_out_groups=vp(0x6000), d_out_counts=vp(0x7000), d_scratch=vp(0x100000), scratch_len=None, stream=None)
    a.update(kw)
    if a["scratch_len"] is None:
        a["scratch_len"] = scratch_bytes(a["n"], a["n_known"])
    return tuple(a.values())


def call(**kw):
    return _lib.load().pico_flow_group_batch_dev(*args(**kw))


def test_symbols_are_exported_and_declared():
    for name in ("pico_flow_group_batch_dev", "pico_flow_group_scratch_bytes"):
        assert name in _lib.EXPORTED
        assert hasattr(_lib.load(), name)
    assert _lib.load().pico_csum_abi_version() == 4          # added entry points: no bump
    assert _lib.ABI_VERSION == 4


def test_header_values():
    src = open(HEADER).read()
    for name, val in (("FLOW_TCP", "1u"), ("FLOW_FRAG4", "2u"), ("FLOW_FRAG6", "3u"), ("FLOW_F_ETH", "0x10u")):
        m = re.search(rf"#define PICO_CSUM_{name}\s+(\w+)", src)
        assert m and m.group(1) == val, name
        assert getattr(_lib, name) == int(val.rstrip("u"), 0)
    assert "#define PICO_CSUM_ABI_VERSION 4" in src
    assert "INADDR_ANY" in src and "struct pico_csum_flow_key" in src
    assert batch.FLOW_KEY_DTYPE.itemsize == 40


@pytest.mark.parametrize("kw", [
    dict(n=0), dict(n=0x00FFFFFF, n_known=1, scratch_len=1 << 40), dict(n=0x01000000, n_known=0, scratch_len=1 << 40),
    dict(n=1, n_known=0x00FFFFFF, scratch_len=1 << 40), dict(n=0xFFFFFFFF, n_known=0xFFFFFFFF, scratch_len=1 << 40),
    dict(mode_flags=0), dict(mode_flags=4), dict(mode_flags=_lib.FLOW_F_ETH), dict(mode_flags=_lib.FLOW_TCP | 0x20),
    dict(mode_flags=_lib.FLOW_TCP | 0x80000000), dict(mode_flags=_lib.FLOW_TCP | _lib.FLOW_FRAG4 | 0x100),
    dict(mode_flags=_lib.FLOW_FRAG4), dict(mode_flags=_lib.FLOW_FRAG6 | _lib.FLOW_F_ETH),       # n_known = 4 in a FRAG mode
    dict(d_known=None),
    dict(d_out_desc=None), dict(d_out_index=None), dict(d_out_groups=None), dict(d_out_counts=None), dict(d_scratch=None),
    dict(d_base=None), dict(d_desc=None),
    dict(d_scratch=vp(0x100008)), dict(d_scratch=vp(0x100001)), dict(d_desc=vp(0x2008)), dict(d_out_desc=vp(0x4008)),
    dict(scratch_len=0), dict(scratch_len=scratch_bytes(16, 4) - 1), dict(scratch_len=scratch_bytes(16, 3)),
], ids=lambda kw: ",".join(f"{k}={getattr(v, 'value', v)}" for k, v in kw.items()))
def test_einval(kw):
    assert call(**kw) == -_lib.EINVAL
    assert _lib.load().pico_csum_last_error().decode() != ""


def test_scratch_formula():
    """0 out of range; 16-byte granular; never smaller for a larger n or n_known."""
    assert scratch_bytes(0, 0) == 0 and scratch_bytes(0, 5) == 0
    assert scratch_bytes(0x00FFFFFF, 1) == 0 and scratch_bytes(0x01000000, 0) == 0 and scratch_bytes(0xFFFFFFFF, 0xFFFFFFFF) == 0
    assert scratch_bytes(0x00FFFFFF, 0) > 0 and scratch_bytes(1, 0x00FFFFFE) > 0
    ns = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4099, 65535, 65536, 65537, 262144,
          (1 << 20) + 1, 0x007FFFFF, 0x00800000]
    ks = [0, 1, 3, 64, 65, 1000, 65536]
    for k in ks:
        sizes = [scratch_bytes(n, k) for n in ns]
        assert all(s > 0 and s % 16 == 0 for s in sizes)
        assert sizes == sorted(sizes), k
    for n in ns:
        sizes = [scratch_bytes(n, k) for k in ks]
        assert sizes == sorted(sizes), n
    assert batch.flow_group_scratch_bytes(4099, 3) == scratch_bytes(4099, 3)
    assert batch.flow_group_scratch_bytes(0) == 0 and batch.flow_group_scratch_bytes(1 << 40) == 0


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-device error path")
def test_enodev_without_a_device():
    """No CPU fallback: well-formed arguments without a HIP device give -ENODEV (also without verdicts
    and without a table, and in the FRAG modes)."""
    assert call() == -_lib.ENODEV
    assert "HIP device" in _lib.load().pico_csum_last_error().decode()
    assert call(d_verdict_in=None, d_known=None, n_known=0) == -_lib.ENODEV
    assert call(mode_flags=_lib.FLOW_FRAG4 | _lib.FLOW_F_ETH, n_known=0) == -_lib.ENODEV
    assert call(mode_flags=_lib.FLOW_FRAG6, n_known=0, d_known=None) == -_lib.ENODEV


def test_python_wrapper_checks_before_the_library():
    base = torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(ValueError):                          # host tensors: the batched path is GPU-only
        batch.flow_group_batch(base, torch.zeros(16, dtype=torch.uint8), 1, _lib.FLOW_TCP)
