"""GPU parity: block-scaled fp8 GEMM (one fp32 scale per 128 x 128 weight block, one per token and 128-wide K group)
behind cutlass_scaled_mm, and its activation quantiser per_token_group_quant_fp8.

Reference: the definition of the reference's tests/kernels/quant_utils.py (native_w8a8_block_matmul) restated in
float64 on the CPU — both operands dequantised with their broadcast scales, ONE matmul, the bias, one rounding to the
output type.  Inputs as tests/test_gpu_fp8_gemm.py::_mk; tolerance: tests.util.assert_gemm_close with its defaults and
that file's caps on the fraction of differing elements (3 % bf16, 9 % f16: the fp8 MFMA's internal adder, measured
there).  b_scales is always the .t() of a checkpoint-style [NB, KB] tensor; a_scales alternates between the row-major
and the token-contiguous layout.  Every case asserts the kernel the router took (scaled_mm_block_last_route).

(1, 128, 128) has one block in every direction: its scales are per-token x per-tensor, a form the row-scaled path
already accepts, so by the wrapper's rule it stays there (the same mathematics) and no block route is recorded.
"""
import pytest
import torch

from tests.util import assert_bit_exact, assert_gemm_close, dev

pytestmark = pytest.mark.gpu

FP8 = torch.float8_e4m3fn
DECODE, TILE, SLABS = 1, 2, 4


def ops():
    from vllm_metax_amd import _custom_ops
    return _custom_ops


def _ref(a, b_nk, a_s, b_s_nk, out_dtype, bias=None):
    n = b_nk.shape[0]
    ad = a.double() * a_s.double().repeat_interleave(128, 1)
    bd = b_nk.double() * b_s_nk.double().repeat_interleave(128, 0).repeat_interleave(128, 1)[:n]
    r = ad @ bd.t()
    return (r + bias.double() if bias is not None else r).to(out_dtype)


def _run(a, b_nk, a_s, b_s_nk, bias, out_dtype, a_s_token_contiguous=False):
    d = dev()
    a_sd = a_s.t().contiguous().to(d).t() if a_s_token_contiguous else a_s.to(d)
    out = torch.full((a.shape[0], b_nk.shape[0]), float("nan"), dtype=out_dtype, device=d)
    ops().cutlass_scaled_mm(out, a.to(d), b_nk.to(d).t(), a_sd, b_s_nk.to(d).t(),
                            bias.to(d) if bias is not None else None)
    return out, ops().scaled_mm_block_last_route()


# (m, n, k) -> the route: kernel bit, + SLABS where the plan splits K
SHAPES = {
    (1, 128, 128): None,                      # a single block: the row-scaled path (see the module docstring)
    (16, 272, 256): DECODE,                   # ragged last column block, two k-blocks
    (33, 576, 1024): DECODE,                  # ragged rows, NB = 5
    (64, 1280, 8192): DECODE | SLABS,         # K split through slabs
    (65, 256, 384): DECODE,                   # a second pass of one row
    (320, 512, 512): DECODE,                  # both sides of the router's threshold
    (321, 512, 512): TILE,
    (333, 320, 1152): TILE | SLABS,           # tile kernel with a K split, 9 k-blocks over 2 uneven splits
    (1030, 272, 384): TILE,                   # ragged in m and n, odd number of k-blocks
    (2048, 512, 1024): TILE,
}


@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("m,n,k", list(SHAPES))
def test_block_scaled_mm(m, n, k, bias, out_dtype):
    g = torch.Generator().manual_seed(0)
    a = (torch.randn(m, k, generator=g) * 2).clamp(-448, 448).to(FP8)
    b_nk = (torch.randn(n, k, generator=g) * 2).clamp(-448, 448).to(FP8)
    a_s = torch.rand(m, k // 128, generator=g) * 9e-3 + 1e-3
    b_s_nk = torch.rand((n + 127) // 128, k // 128, generator=g) * 9e-3 + 1e-3
    bi = (torch.rand(n, generator=g) * 2 - 1).to(out_dtype) if bias else None
    out, route = _run(a, b_nk, a_s, b_s_nk, bi, out_dtype, a_s_token_contiguous=bool((m + bias) % 2))
    if SHAPES[m, n, k] is not None:
        assert route == SHAPES[m, n, k], f"{m}x{n}x{k}: route {route}"
    assert_gemm_close(out, _ref(a, b_nk, a_s, b_s_nk, out_dtype, bi), f"block fp8 {m}x{n}x{k}",
                      max_frac=0.09 if out_dtype == torch.float16 else 0.03)


@pytest.mark.parametrize("m,route", [(40, DECODE), (330, TILE), (64, DECODE | SLABS), (333, TILE | SLABS)])
def test_scale_placement_is_exact(m, route):
    """Small integer operands and power-of-two scales that differ per (row, k-block) and per weight block: every
    product and partial sum is exact in fp32, so the result must EQUAL the float64 reference — a scale applied to the
    wrong row, k-block or column block cannot hide inside a tolerance.  A k-block's sum is an integer below 2^9; with
    scale exponents in [-e, e] any partial sum of KB blocks is a multiple of 2^-2e below KB 2^(9 + 2e): 4 blocks and
    e = 3 need 23 bits, 64 blocks and e = 1 need 19."""
    n, k, e = (272, 512, 3) if not route & SLABS else ((1280, 8192, 1) if route & DECODE else (320, 1152, 1))
    g = torch.Generator().manual_seed(m)
    a = torch.randint(-2, 3, (m, k), generator=g).float().to(FP8)
    b_nk = torch.randint(-2, 3, (n, k), generator=g).float().to(FP8)
    a_s = torch.pow(2.0, torch.randint(-e, e + 1, (m, k // 128), generator=g).float())
    b_s_nk = torch.pow(2.0, torch.randint(-e, e + 1, ((n + 127) // 128, k // 128), generator=g).float())
    bi = torch.randint(-8, 9, (n,), generator=g).to(torch.bfloat16)
    out, got_route = _run(a, b_nk, a_s, b_s_nk, bi, torch.bfloat16, m % 2 == 0)
    assert got_route == route
    assert_bit_exact(out, _ref(a, b_nk, a_s, b_s_nk, torch.bfloat16, bi), f"placement m={m}")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("column_major", [False, True])
@pytest.mark.parametrize("tokens,hidden", [(7, 512), (300, 4096)])
def test_per_token_group_quant_fp8(tokens, hidden, column_major, dtype):
    g = torch.Generator().manual_seed(hidden)
    x = (torch.randn(tokens, hidden, generator=g) * torch.rand(tokens, 1, generator=g) * 8).to(dtype)
    x[0, :128] = 0                                                     # an all-zero group: the eps clamp
    q, s = ops().per_token_group_quant_fp8(x.to(dev()), 128, column_major_scales=column_major)
    assert s.shape == (tokens, hidden // 128) and s.stride(0) == (1 if column_major else hidden // 128)
    xg = x.float().view(tokens, hidden // 128, 128)
    want_s = xg.abs().amax(-1).clamp(min=1e-10) / 448.0
    want_q = (xg / want_s[..., None]).clamp(-448, 448).to(FP8).view(tokens, hidden)
    assert_bit_exact(s, want_s, "group scales")
    assert_bit_exact(q, want_q, "group-quantised bytes")


def test_argument_errors_and_untouched_paths():
    d = dev()
    out = torch.empty(16, 256, dtype=torch.bfloat16, device=d)
    ones = lambda *shape: torch.ones(*shape, dtype=torch.float32, device=d)   # noqa: E731
    a = torch.zeros(16, 320, dtype=FP8, device=d)
    b = torch.zeros(256, 320, dtype=FP8, device=d).t()
    with pytest.raises(RuntimeError):                     # k % 128 != 0
        ops().cutlass_scaled_mm(out, a, b, ones(16, 3), ones(3, 2), None)
    a, b = a[:, :256], torch.zeros(256, 256, dtype=FP8, device=d).t()
    with pytest.raises(RuntimeError):                     # neither per-row / per-column nor block shaped
        ops().cutlass_scaled_mm(out, a, b, ones(16, 2), ones(2, 3), None)
    with pytest.raises(RuntimeError, match="only 128"):
        ops().per_token_group_quant_fp8(torch.zeros(4, 256, dtype=torch.bfloat16, device=d), 64)
    assert ops().cutlass_scaled_mm_supports_block_fp8(90) is True
    import vllm_metax_amd._C  # noqa: F401
    assert hasattr(torch.ops._C, "per_token_group_fp8_quant")
    assert torch.ops._C.cutlass_scaled_mm_supports_block_fp8(90) is True
    # a per-row / per-column call stays on the row-scaled path: the oracle's result as before, no block route
    from oracle import ref_ops as R
    g = torch.Generator().manual_seed(1)
    a = (torch.randn(33, 256, generator=g) * 2).to(FP8)
    b = (torch.randn(256, 256, generator=g) * 2).to(FP8).t()
    a_s, b_s = torch.rand(33, 1, generator=g) * 9e-3 + 1e-3, torch.rand(1, 256, generator=g) * 9e-3 + 1e-3
    _run(a[:16], b.t(), torch.ones(16, 2), torch.ones(2, 2), None, torch.bfloat16)    # leaves a block route behind
    out = torch.empty(33, 256, dtype=torch.bfloat16, device=d)
    ops().cutlass_scaled_mm(out, a.to(d), b.t().contiguous().to(d).t(), a_s.to(d), b_s.to(d), None)
    assert_gemm_close(out, R.scaled_mm_fp8(a, b, a_s, b_s, torch.bfloat16), "row-scaled call", max_frac=0.03)
    assert ops().scaled_mm_block_last_route() == DECODE   # still the earlier block call's: this one never got there


def test_apply_fp8_block_linear():
    """quant_config.linear.apply_fp8_block = group quantiser + GEMM on the checkpoint's own tensors (weight [n, k],
    weight_scale_inv [NB, KB]); against the float64 reference on the quantiser's own bytes and scales."""
    from vllm_metax_amd.quant_config import linear
    d = dev()
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 20, 512, generator=g).to(torch.bfloat16).to(d)
    w = (torch.randn(272, 512, generator=g) * 2).to(FP8).to(d)
    ws = (torch.rand(3, 4, generator=g) * 9e-3 + 1e-3).to(d)
    bias = torch.randn(272, generator=g).to(torch.bfloat16).to(d)
    out = linear.apply_fp8_block(x, w, ws, bias)
    assert out.shape == linear.apply_fp8_block_fake(x, w, ws, bias).shape == (2, 20, 272)
    q, s = ops().per_token_group_quant_fp8(x.reshape(-1, 512))
    assert_gemm_close(out.reshape(-1, 272), _ref(q.cpu(), w.cpu(), s.cpu(), ws.cpu(), torch.bfloat16, bias.cpu()),
                      "apply_fp8_block", max_frac=0.03)


def test_graph_replay_of_the_slab_path():
    """The K-split call captured into a HIP graph: three replays give the eager call's bits (nothing in the slab path
    depends on a memset or on what an earlier launch left in the workspace)."""
    m, n, k = 64, 1280, 8192
    d = dev()
    g = torch.Generator().manual_seed(4)
    a = (torch.randn(m, k, generator=g) * 2).to(FP8).to(d)
    b = (torch.randn(n, k, generator=g) * 2).to(FP8).to(d).t()
    a_s = (torch.rand(m, k // 128, generator=g) * 9e-3 + 1e-3).to(d)
    b_s = (torch.rand(n // 128, k // 128, generator=g) * 9e-3 + 1e-3).to(d).t()
    eager = torch.empty(m, n, dtype=torch.bfloat16, device=d)
    ops().cutlass_scaled_mm(eager, a, b, a_s, b_s, None)
    assert ops().scaled_mm_block_last_route() == DECODE | SLABS
    out = torch.empty_like(eager)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops().cutlass_scaled_mm(out, a, b, a_s, b_s, None)      # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops().cutlass_scaled_mm(out, a, b, a_s, b_s, None)
    for _ in range(3):
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert_bit_exact(out, eager, "graph replay")
