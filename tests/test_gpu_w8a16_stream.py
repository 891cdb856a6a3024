"""GPU parity: gptq_gemm with bit = 8 below 1024 rows on w8a16_gemm_stream_kernel (csrc/w8a16_stream.hip).

Reference: oracle.ref_ops.gptq8_gemm, a float64 product of the T-rounded dequantised weights.  The kernel's
weights are those bit for bit (one rounding to T) and its products are exact in fp32, so only the accumulation order
differs: tests.util.assert_gemm_close at its defaults (one output ulp + 2e-4 max|ref|, at most 5 % of the elements
different).  Inputs as test_gptq_gemm_8bit (scales 1e-4 .. 5e-4, x ~ 0.5 randn, weights U{0..255}) with stored
zeros over the full range 0 .. 255: z = 256 must not wrap in a byte.  Every row asserts its route mask exactly.
The k = 8192 / 7680 rows leave a wave two 128-k stages (8 steps: the ring's steady-state loop runs, the LDS image is
re-staged at MT = 4); the last stream row pins the plan (1 k-part, no split: 32 steps per wave, two images).
"""
import numpy as np
import pytest
import torch

from tests.util import assert_bit_exact, assert_gemm_close, dev

pytestmark = pytest.mark.gpu

from oracle import ref_ops as R  # noqa: E402

STREAM, SUM_SLABS, ANY_8 = 256, 128, 32
DTYPES = [torch.bfloat16, torch.float16]

# (m, k, n, group (-1: per channel), act-order, expected route, MI355X_W8_STREAM_FORCE or None)
ROWS = [(m, 256, 128, 128, False, STREAM, None) for m in (1, 16, 17, 33, 64)] + [   # every MT, row tails, n < 256
    (64, 128, 64, 128, False, STREAM, None),                # one stage, one wave's columns
    (48, 384, 320, 96, False, STREAM, None),                # a group change inside a 128-k stage, n % 256 != 0
    (48, 384, 320, 32, False, STREAM, None),
    (20, 512, 192, -1, False, STREAM, None),                # group == k
    (64, 4096, 64, 128, False, STREAM | SUM_SLABS, None),   # the planner splits K (one stage per wave)
    (64, 8192, 64, 128, False, STREAM | SUM_SLABS, None),   # two stages per wave: the ring loop, MT 4 re-stages
    (1, 8192, 64, 128, False, STREAM | SUM_SLABS, None),    # the ring loop at MT 1 and 2
    (20, 8192, 64, 128, False, STREAM | SUM_SLABS, None),
    (48, 7680, 64, 96, False, STREAM | SUM_SLABS, None),    # group changes inside the loop, across a re-staging
    (33, 1024, 128, 32, False, STREAM, "1,1"),              # pinned: 32 steps per wave, a group per step, 2 images
    (65, 512, 256, 128, False, STREAM, None),               # passes with a tail pass
    (200, 512, 256, 128, False, STREAM, None),
    (40, 512, 128, 128, True, STREAM, None),                # act-order in front of the kernel
    (8, 512, 72, 128, False, ANY_8, None),                  # refused shapes keep the old kernel
    (8, 96, 64, 32, False, ANY_8, None),
]


def ops():
    from vllm_metax_amd import _custom_ops
    return _custom_ops


def make(m, k, n, group, act, dtype, zeros=None, binary=False):
    """The arguments of ops.gptq_gemm (on the GPU) and the oracle's result."""
    g = k if group == -1 else group
    rng = np.random.default_rng(m * 7 + k + n)
    w = rng.integers(0, 256, size=(k, n), dtype=np.uint8)
    if binary:
        w = (w & 1) * np.uint8(255)
    z = rng.integers(0, 256, size=(k // g, n), dtype=np.uint8) if zeros is None else np.full((k // g, n), zeros, np.uint8)
    zb = z.reshape(k // g, n // 4, 4).astype(np.uint32)
    qz = torch.from_numpy((zb[..., 0] | (zb[..., 1] << 8) | (zb[..., 2] << 16) | (zb[..., 3] << 24)).view(np.int32))
    qw = R.gptq8_pack_rows(w)
    sc = (torch.rand(k // g, n, generator=torch.Generator().manual_seed(1)) * 4e-4 + 1e-4).to(dtype)
    x = (torch.randn(m, k, generator=torch.Generator().manual_seed(2)) * 0.5).to(dtype)
    perm = torch.randperm(k, generator=torch.Generator().manual_seed(3)).to(torch.int32) if act else None
    ref = R.gptq8_gemm(x if perm is None else x[:, perm.long()], qw, qz, sc, g)
    d = dev()
    idx = torch.empty(0, dtype=torch.int32, device=d) if perm is None else perm.to(d)
    return (x.to(d), qw.to(d), qz.to(d), sc.to(d), idx, True, 8, group, torch.empty(0), torch.empty(0),
            dtype == torch.bfloat16), ref


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("m,k,n,group,act,route,force", ROWS)
def test_w8a16_stream(m, k, n, group, act, route, force, dtype, monkeypatch):
    assert ops().W8_ROUTE_STREAM == STREAM
    if force:
        monkeypatch.setenv("MI355X_W8_STREAM_FORCE", force)
    args, ref = make(m, k, n, group, act, dtype)
    out = ops().gptq_gemm(*args)
    assert ops().w4a16_last_route() == route
    assert_gemm_close(out, ref, f"gptq 8-bit {m}x{n}x{k} g{group}")
    if route & SUM_SLABS:
        assert_bit_exact(ops().gptq_gemm(*args), out, "split K: a second call")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("zeros", [255, 0])
def test_w8a16_stream_zero_point_edges(zeros, dtype):
    """Stored zeros all 255 (z = 256) or all 0 (z = 1), weights only 0 and 255: the extreme values of q - z."""
    args, ref = make(33, 256, 128, 128, False, dtype, zeros=zeros, binary=True)
    out = ops().gptq_gemm(*args)
    assert ops().w4a16_last_route() == STREAM
    assert_gemm_close(out, ref, f"stored zeros {zeros}")


def test_w8a16_stream_split_k_replays_from_a_graph():
    dtype = torch.bfloat16
    args, ref = make(64, 4096, 64, 128, False, dtype)
    eager = ops().gptq_gemm(*args)
    assert ops().w4a16_last_route() == STREAM | SUM_SLABS
    assert_gemm_close(eager, ref, "eager")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        ops().gptq_gemm(*args)                       # (allocations settle before the capture)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops().gptq_gemm(*args)
    for i in range(3):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert_bit_exact(out, eager, f"replay {i}")
