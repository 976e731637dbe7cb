"""CPU tests of pico_tcp_segment_batch_dev's argument checks (include/pico_csum.h): every refusal
comes before any device work, so none of this launches anything."""
from __future__ import annotations

import ctypes

import pytest
import torch

from picotcp_amd import _lib

vp = ctypes.c_void_p


def args(**kw):
    """A well-formed call (fake device addresses), fields replaced by keyword."""
    a = dict(d_base=vp(0x1000), base_len=1 << 20, d_stream=vp(0x2000), n_stream=4, d_groups=vp(0x3000), n_seg=16,
             d_out=vp(0x4000), out_len=1 << 20, d_out_desc=vp(0x5000), seg_stride=1504, d_out_seg=vp(0x6000),
             d_out_count=vp(0x7000), d_verdict=vp(0x9000), flags=0, stream=None)
    a.update(kw)
    return tuple(a.values())


def call(**kw):
    return _lib.load().pico_tcp_segment_batch_dev(*args(**kw))


def test_symbol_is_exported_and_declared():
    assert "pico_tcp_segment_batch_dev" in _lib.EXPORTED
    assert hasattr(_lib.load(), "pico_tcp_segment_batch_dev")
    assert _lib.load().pico_csum_abi_version() == 4          # an added entry point: no bump


@pytest.mark.parametrize("kw", [
    dict(flags=_lib.F_WRITE), dict(flags=_lib.F_TX), dict(flags=0x4), dict(flags=_lib.F_NXTHDR_DISPATCH),
    dict(flags=0x80000000),                                  # reserved: anything but 0
    dict(d_stream=vp(0x2008)), dict(d_groups=vp(0x3002)), dict(d_out_desc=vp(0x5008)), dict(d_out_seg=vp(0x6008)),
    dict(d_out_count=vp(0x7002)),
    dict(d_base=None), dict(d_out=None), dict(d_stream=None), dict(d_groups=None), dict(d_out_desc=None),
    dict(seg_stride=36), dict(seg_stride=0),                 # below 40, the shortest frame
    dict(seg_stride=1502), dict(seg_stride=41),              # not a multiple of 4
], ids=lambda kw: ",".join(f"{k}={getattr(v, 'value', v)}" for k, v in kw.items()))
def test_einval(kw):
    assert call(**kw) == -_lib.EINVAL
    assert _lib.load().pico_csum_last_error().decode() != ""


def test_empty_batch_is_a_no_op():
    assert call(n_stream=0, d_base=None, d_out=None, d_stream=None, d_groups=None, d_out_desc=None,
                seg_stride=0) == 0


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-device error path")
def test_enodev_without_a_device():
    """No CPU fallback: well-formed arguments without a HIP device give -ENODEV (also with every
    optional output NULL and the smallest stride)."""
    assert call() == -_lib.ENODEV
    assert "HIP device" in _lib.load().pico_csum_last_error().decode()
    assert call(d_out_seg=None, d_out_count=None, d_verdict=None, seg_stride=40) == -_lib.ENODEV
