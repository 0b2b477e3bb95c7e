"""Opt-in LDS (above 64 KB) that GROWS from one launch of a kernel instantiation to the next, on the MI355X: the attribute that permits it
is set once per (kernel, device) by the launch helper (csrc/fz_rt.h, fz_plan::launch_lds), and in csrc/attn_temporal.hip what an
instantiation asks for depends on the head width of the launch.  Each test runs ONE instantiation twice in this process, the smaller
request first: a helper that remembered "set" without "set to how much" fails the second launch with a launch error.
(The same per device on a second GPU is the same table entry indexed by another bit; it needs two GPUs to run.)"""
import pytest

from fatezero_amd import _native
from fatezero_amd import kernels as K

import kernel_cases as KC

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def hip_backend():
    _native.reset_backend()
    assert "hip" in K.version()
    assert _native.loaded_path().endswith("libfatezero_hip.so")
    yield


def test_long_kernel_lds_grows():
    # attn_temporal_long_kernel<8> (256 frames, one head per workgroup): 128 x 264 halves = 67 584 B, then 160 x 264 = 84 480 B
    for d in (128, 160):
        KC.case_attn_temporal(DEV, batch=1, clip=256, heads=1, d=d, tokens=4, seed=d)


def test_stream_kernel_lds_grows():
    # attn_temporal_stream_kernel<1, 5> (288 frames, five 32-channel tiles): 136 x 264 halves = 71 808 B, then 160 x 264 = 84 480 B
    for d in (136, 160):
        KC.case_attn_temporal(DEV, batch=1, clip=288, heads=1, d=d, tokens=4, seed=d)


def test_one_thread_per_query_kernel_lds_grows():
    # attn_temporal_lds_kernel<32> (K and V of one token: 2 x 32 frames x channels): 640 channels = 81 920 B, then 1280 = 163 840 B
    for d in (80, 160):
        KC.case_attn_temporal(DEV, batch=1, clip=32, heads=8, d=d, tokens=2, seed=d)
