"""gsrt_normal_noise on the device against tests/philox_ref.py.

The tolerance. A value is z = r cos(th) or r sin(th) with r = sqrtf(-2 logf(ua)), th = 6.2831855f * ub, ua and ub exact
multiples of 2^-25 in (0, 1]; the reference evaluates the same expressions in float64 from the same words.
  - |r| <= sqrt(2 ln 2^25) < 5.9 (ua >= 2^-25).
  - The float32 angle carries at most 0.5 ulp of 6.28 from the product, about 2.4e-7 rad: at most 5.9 * 2.4e-7 = 1.4e-6
    on z.
  - logf, sinf and cosf are accurate to a few ulp: a few 6e-8 relative on sin and cos (|.| <= 1), i.e. a few 3.5e-7 on z;
    logf's few ulp of |log ua| <= 17.4 move r by (few 1e-6) / r relatively to -2 log, under 1e-6 on z after the root;
    the product by -2 is exact, the root and the final product round once each: 2 * 6e-8 * 5.9 = 7e-7.
  - The total is below 5e-6, and the tolerance of 1e-5 gives about 2x over that.
The moments. Over N = 4 * 65536 values the mean of N unit normals has standard deviation 1 / sqrt(N) and the sample
variance sqrt(2 / N): both are held to five of those. test_reference_moments checks on the CPU that the float64 reference
alone meets both bounds for the seeds used."""
import numpy as np
import pytest

import gsrt
import philox_ref as P
from test_features_gpu import u32

LONG = 4 * 65536 + 2
COUNTS = [0, 1, 3, 4, 5, 255, 256, 257, LONG]
SEEDS = [(2024, 0), (0x9E3779B97F4A7C15, 3)]
TOL = 1e-5
_REF = {}


def reference(seed, stream_id):
    if (seed, stream_id) not in _REF:
        _REF[(seed, stream_id)] = P.normal_f64(seed, stream_id, LONG)
    return _REF[(seed, stream_id)]


def moments_ok(z):
    n = 4 * 65536
    z = np.asarray(z[:n], np.float64)
    return abs(z.mean()) < 5 / np.sqrt(n) and abs(z.var() - 1.0) < 5 * np.sqrt(2.0 / n)


@pytest.mark.parametrize("seed,stream_id", SEEDS)
def test_reference_moments(seed, stream_id):
    """no device: the float64 reference itself meets the moment bounds for the seeds the GPU test uses"""
    z = reference(seed, stream_id)
    assert np.isfinite(z).all() and np.abs(z).max() < 5.9 and moments_ok(z)


@pytest.mark.gpu
@pytest.mark.parametrize("seed,stream_id", SEEDS)
def test_host_pointer_counts_prefix_and_accuracy(ctx, seed, stream_id):
    ref = reference(seed, stream_id)
    long = gsrt.normal_noise(ctx, LONG, seed, stream_id)
    assert long.shape == (LONG,) and long.dtype == np.float32 and np.isfinite(long).all()
    worst = float(np.abs(long.astype(np.float64) - ref).max())
    print(f"normal_noise seed {seed:#x} stream {stream_id}: worst |z - f64| = {worst:.3g} (bound {TOL})")
    assert worst <= TOL
    assert moments_ok(long)
    for count in COUNTS[:-1]:
        got = gsrt.normal_noise(ctx, count, seed, stream_id)
        assert got.shape == (count,) and u32(got).tobytes() == u32(long[:count]).tobytes(), count  # the prefix, bit for bit


@pytest.mark.gpu
def test_device_pointers_aligned_and_offset(ctx):
    import torch

    seed, stream_id = SEEDS[0]
    long = gsrt.normal_noise(ctx, LONG, seed, stream_id)
    for count in COUNTS:
        for off in (0, 1):  # a 16-byte aligned base, and one 4 bytes past it (the dword-store path)
            buf = torch.full((count + 8,), 7.0, dtype=torch.float32, device="cuda:0")
            torch.cuda.synchronize()
            assert buf.data_ptr() % 16 == 0
            gsrt.normal_noise(ctx, count, seed, stream_id, d_out=buf.data_ptr() + 4 * off)
            host = buf.cpu().numpy()
            assert u32(host[off:off + count]).tobytes() == u32(long[:count]).tobytes(), (count, off)
            assert (host[:off] == 7.0).all() and (host[off + count:] == 7.0).all()  # nothing outside [0, count)
    # the async form takes a device pointer only
    out = np.zeros(4, np.float32)
    assert gsrt.lib.gsrt_normal_noise_async(ctx.handle, 4, 0, 0, out.ctypes.data) == gsrt.E_ARG
    assert gsrt.lib.gsrt_normal_noise(ctx.handle, 4, 0, 0, None) == gsrt.E_ARG


@pytest.mark.gpu
def test_seeds_and_streams_differ(ctx):
    a = gsrt.normal_noise(ctx, 257, 1, 0)
    assert not np.array_equal(a, gsrt.normal_noise(ctx, 257, 2, 0))
    assert not np.array_equal(a, gsrt.normal_noise(ctx, 257, 1, 1))
    assert not np.array_equal(a, gsrt.normal_noise(ctx, 257, 1 << 32 | 1, 0))  # the seed's high word is part of the key
    assert u32(a).tobytes() == u32(gsrt.normal_noise(ctx, 257, 1, 0)).tobytes()
