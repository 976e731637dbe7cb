"""CPU tests of pico_tcp_ack_batch_dev's argument checks (include/pico_csum.h): every refusal comes
before any device work, so none of this launches anything."""
from __future__ import annotations

import ctypes
import os
import re

import pytest
import torch

from picotcp_amd import _lib, batch

vp = ctypes.c_void_p
HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "pico_csum.h")


def args(**kw):
    """A well-formed call (fake device addresses), fields replaced by keyword."""
    a = dict(d_base=vp(0x1000), base_len=1 << 20, d_seg=vp(0x2000), n_seg=16, d_groups=vp(0x3000), d_conn=vp(0x3800),
             n_conn=4, d_out_len=vp(0x6000), d_seg_verdict=vp(0x7000), d_tmpl_base=vp(0xA000), tmpl_len=1 << 12,
             d_tmpl=vp(0xB000), d_ack=vp(0xC000), d_out=vp(0x4000), out_len=1 << 20, d_out_desc=vp(0x5000),
             d_out_ack=vp(0xD000), d_verdict=vp(0x9000), flags=0, stream=None)
    a.update(kw)
    return tuple(a.values())


def call(**kw):
    return _lib.load().pico_tcp_ack_batch_dev(*args(**kw))


def test_symbol_is_exported_and_declared():
    assert "pico_tcp_ack_batch_dev" in _lib.EXPORTED
    assert hasattr(_lib.load(), "pico_tcp_ack_batch_dev")
    src = open(HEADER).read()
    assert re.search(r"\bint pico_tcp_ack_batch_dev\(", src)
    assert "4 (added, no bump): pico_tcp_ack_batch_dev" in src


def test_abi_version_is_still_4():
    assert _lib.load().pico_csum_abi_version() == _lib.ABI_VERSION == 4          # an added entry point: no bump
    assert "#define PICO_CSUM_ABI_VERSION 4" in open(HEADER).read()


def test_struct_size():
    """struct pico_csum_tcp_ack: four uint32, 16 bytes, in the header and the binding."""
    src = open(HEADER).read()
    m = re.search(r"struct pico_csum_tcp_ack \{(.*?)\};", src, re.S)
    assert m
    fields = re.findall(r"uint32_t\s+([a-z, ]+);", m.group(1))
    assert [f.strip() for g in fields for f in g.split(",")] == ["space", "tsval", "tsecr", "aflags"]
    assert batch.TCP_ACK_DTYPE.itemsize == 16 and batch.TCP_ACK_DTYPE.names == ("space", "tsval", "tsecr", "aflags")


@pytest.mark.parametrize("kw", [
    dict(flags=_lib.F_WRITE), dict(flags=_lib.F_TX), dict(flags=0x4), dict(flags=_lib.F_NXTHDR_DISPATCH),
    dict(flags=0x80000000),                                  # reserved: anything but 0
    dict(d_seg=vp(0x2008)), dict(d_tmpl=vp(0xB008)), dict(d_out_desc=vp(0x5008)), dict(d_out_ack=vp(0xD008)),
    dict(d_groups=vp(0x3002)), dict(d_conn=vp(0x3802)), dict(d_out_len=vp(0x6002)), dict(d_ack=vp(0xC002)),
    dict(d_base=None), dict(d_seg=None), dict(d_groups=None), dict(d_conn=None), dict(d_out_len=None),
    dict(d_seg_verdict=None), dict(d_tmpl_base=None), dict(d_tmpl=None), dict(d_ack=None), dict(d_out=None),
    dict(d_out_desc=None),
], ids=lambda kw: ",".join(f"{k}={getattr(v, 'value', v)}" for k, v in kw.items()))
def test_einval(kw):
    assert call(**kw) == -_lib.EINVAL
    assert _lib.load().pico_csum_last_error().decode() != ""


def test_empty_batch_is_a_no_op():
    assert call(n_conn=0, d_base=None, d_seg=None, d_groups=None, d_conn=None, d_out_len=None, d_seg_verdict=None,
                d_tmpl_base=None, d_tmpl=None, d_ack=None, d_out=None, d_out_desc=None) == 0


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-device error path")
def test_enodev_without_a_device():
    """No CPU fallback: well-formed arguments without a HIP device give -ENODEV (also with every
    optional output NULL)."""
    assert call() == -_lib.ENODEV
    assert "HIP device" in _lib.load().pico_csum_last_error().decode()
    assert call(d_out_ack=None, d_verdict=None) == -_lib.ENODEV
