"""GPU parity: MX-FP4 (w4a4) GEMM behind cutlass_scaled_mm (e2m1 nibbles, one E8M0 scale byte per 32-wide K group on
both operands, applied inside the scaled MFMA) and its activation quantiser per_token_group_quant_mxfp4.

Reference: the contract restated in float64 on the CPU — nibbles decoded through the 16-entry table, multiplied by the
decoded scales, ONE matmul, the bias, one rounding to the output type.  Tolerance of the random cases:
tests.util.assert_gemm_close with its default `rel` and the caps tests/test_gpu_fp8_gemm.py carries for this MFMA's
internal adder (3 % bf16, 9 % f16; e2m1 products are shorter than e4m3 ones).  Every case asserts the kernel the router
took (scaled_mm_mxfp4_last_route)."""
import pytest
import torch

from tests.util import assert_bit_exact, assert_gemm_close, dev

pytestmark = pytest.mark.gpu

F4, E8 = torch.float4_e2m1fn_x2, torch.float8_e8m0fnu
STREAM, TILE, SLABS = 1, 2, 4
T = 65                                     # the router's threshold: m <= T streams (profiles/mxfp4_gemm.txt)
E2M1 = torch.tensor([0, .5, 1, 1.5, 2, 3, 4, 6, -0., -.5, -1, -1.5, -2, -3, -4, -6], dtype=torch.float64)


def ops():
    from vllm_metax_amd import _custom_ops
    return _custom_ops


def _decode(q, s):
    """bytes [r, k / 2], scale bytes [r, k / 32] -> float64 [r, k]"""
    q = q.view(torch.uint8).long()
    v = torch.stack((E2M1[q & 15], E2M1[q >> 4]), -1).reshape(q.shape[0], -1)
    return v * torch.pow(2.0, s.view(torch.uint8).double() - 127).repeat_interleave(32, 1)


def _ref(a, b_nk, a_s, b_s_nk, out_dtype, bias=None):
    r = _decode(a, a_s) @ _decode(b_nk, b_s_nk).t()
    return (r + bias.double() if bias is not None else r).to(out_dtype)


def _run(a, b_nk, a_s, b_s_nk, bias, out_dtype, op=None):
    d = dev()
    out = torch.full((a.shape[0], b_nk.shape[0]), float("nan"), dtype=out_dtype, device=d)
    (op or ops().cutlass_scaled_mm)(out, a.to(d).view(F4), b_nk.to(d).view(F4).t(), a_s.to(d).view(E8),
                                    b_s_nk.to(d).view(E8).t(), bias.to(d) if bias is not None else None)
    return out, ops().scaled_mm_mxfp4_last_route()


def _nibbles(values, shape, g):
    """random bytes whose two nibbles are drawn from `values` (e2m1 codes)"""
    c = torch.tensor(values, dtype=torch.uint8)
    return c[torch.randint(len(values), shape, generator=g)] | (c[torch.randint(len(values), shape, generator=g)] << 4)


# (m, n, k) -> the route: kernel bit, + SLABS where the plan splits K
SHAPES = {
    (1, 16, 128): STREAM,                     # one k-step: a ragged super-step of r = 1
    (16, 272, 384): STREAM,                   # r = 3, ragged last column block
    (33, 576, 1024): STREAM,                  # ragged rows, two whole super-steps
    (64, 1280, 8192): STREAM | SLABS,         # K split through slabs
    (65, 256, 640): STREAM,                   # a second pass of one row
    (T, 512, 512): STREAM,                    # both sides of the router's threshold
    (T + 1, 512, 512): TILE,
    (333, 320, 1152): TILE | SLABS,           # 9 k-steps over 2 uneven splits: a half stage ends the first
    (1030, 272, 384): TILE,                   # ragged in m and n, odd number of k-steps
}


@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("m,n,k", list(SHAPES))
def test_mxfp4_scaled_mm(m, n, k, bias, out_dtype):
    g = torch.Generator().manual_seed(0)
    a = torch.randint(0, 256, (m, k // 2), generator=g, dtype=torch.uint8)        # all 16 codes, -0 included
    b_nk = torch.randint(0, 256, (n, k // 2), generator=g, dtype=torch.uint8)
    a_s = (127 + torch.randint(-6, 0, (m, k // 32), generator=g)).to(torch.uint8)
    b_s_nk = (127 + torch.randint(-6, 0, (n, k // 32), generator=g)).to(torch.uint8)
    bi = (torch.rand(n, generator=g) * 2 - 1).to(out_dtype) if bias else None
    out, route = _run(a, b_nk, a_s, b_s_nk, bi, out_dtype)
    assert route == SHAPES[m, n, k], f"{m}x{n}x{k}: route {route}"
    assert_gemm_close(out, _ref(a, b_nk, a_s, b_s_nk, out_dtype, bi), f"mxfp4 {m}x{n}x{k}",
                      max_frac=0.09 if out_dtype == torch.float16 else 0.03)


@pytest.mark.parametrize("m,n,k,route", [(40, 272, 640, STREAM), (64, 1280, 8192, STREAM | SLABS),
                                         (T + 10, 272, 640, TILE), (333, 320, 1152, TILE | SLABS)])
def test_scale_placement_is_exact(m, n, k, route):
    """Nibbles from {0, +-0.5, +-1, +-2} and scale bytes 127 + {-1, 0, 1}, independent per (row, group) and per
    (column, group), integer bias: every product is a multiple of 2^-4 and a partial sum stays below 2^17 even at
    K = 8192 (|a b| <= 4 * 4 per element), 21 bits — exact in fp32 in any order, so the result must EQUAL the float64
    reference.  A scale applied to the wrong row, column, group or op_sel byte cannot hide inside a tolerance."""
    g = torch.Generator().manual_seed(m)
    codes = [0, 1, 2, 4, 9, 10, 12]
    a, b_nk = _nibbles(codes, (m, k // 2), g), _nibbles(codes, (n, k // 2), g)
    a_s = (127 + torch.randint(-1, 2, (m, k // 32), generator=g)).to(torch.uint8)
    b_s_nk = (127 + torch.randint(-1, 2, (n, k // 32), generator=g)).to(torch.uint8)
    bi = torch.randint(-8, 9, (n,), generator=g).to(torch.bfloat16)
    out, got_route = _run(a, b_nk, a_s, b_s_nk, bi, torch.bfloat16)
    assert got_route == route
    assert_bit_exact(out, _ref(a, b_nk, a_s, b_s_nk, torch.bfloat16, bi), f"placement m={m}")


def _quant_ref(x):
    """The rule of the contract, restated: (packed nibbles [tokens, hidden / 2], scale bytes [tokens, hidden / 32])"""
    tokens, hidden = x.shape
    xg = x.float().view(tokens, hidden // 32, 32)
    e = ((xg.abs().amax(-1).view(torch.int32) + 0x200000) >> 23) & 0xFF
    s = (e - 2).clamp(0, 254)
    v = (xg.double() * torch.pow(2.0, (127 - s).double())[..., None]).abs()
    code = ((v > 0.25).long() + (v >= 0.75) + (v > 1.25) + (v >= 1.75) + (v > 2.5) + (v >= 3.5) + (v > 5))
    nib = (code + 8 * torch.signbit(xg)).view(tokens, hidden // 2, 2)
    return (nib[..., 0] | (nib[..., 1] << 4)).to(torch.uint8), s.to(torch.uint8)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("tokens,hidden", [(7, 512), (300, 4096)])
def test_per_token_group_quant_mxfp4(tokens, hidden, dtype):
    g = torch.Generator().manual_seed(hidden)
    x = (torch.randn(tokens, hidden, generator=g) * torch.rand(tokens, 1, generator=g) * 8).to(dtype)
    x[0, :32] = 0                                                   # an all-zero group: s = 0, zero nibbles
    x[1, :32] = x[1, :32].clamp(-1, 1)
    x[1, 5] = -1.875                                                # amax mantissa >= 1.75: the carry into e
    x[2, 32:64] = x[2, 32:64].clamp(-1, 1)                          # amax 40 = 5 * 2^3: scale 2^3 and exact ties
    x[2, 32:40] = torch.tensor([40, 2, 6, 20, -10, 14, 28, -2]).to(dtype)
    q, s = ops().per_token_group_quant_mxfp4(x.to(dev()))
    assert q.dtype == F4 and s.dtype == E8 and q.shape == (tokens, hidden // 2) and s.shape == (tokens, hidden // 32)
    want_q, want_s = _quant_ref(x)
    assert want_s[0, 0] == 0 and want_s[1, 0] == 126 and want_s[2, 1] == 130
    assert_bit_exact(s.view(torch.uint8), want_s, "group scale bytes")
    assert_bit_exact(q.view(torch.uint8), want_q, "packed nibbles")


def test_apply_mxfp4_linear_and_torch_ops():
    """quant_config.linear.apply_mxfp4 = group quantiser + GEMM on the checkpoint's own uint8 tensors; against the
    float64 reference on the quantiser's own bytes.  The torch.ops._C forms give the same bits."""
    from vllm_metax_amd.quant_config import linear
    import vllm_metax_amd._C  # noqa: F401
    d = dev()
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 20, 512, generator=g).to(torch.bfloat16).to(d)
    w = torch.randint(0, 256, (272, 256), generator=g, dtype=torch.uint8)
    ws = (127 + torch.randint(-6, 0, (272, 16), generator=g)).to(torch.uint8)
    bias = torch.randn(272, generator=g).to(torch.bfloat16)
    out = linear.apply_mxfp4(x, w.to(d), ws.to(d), bias.to(d))
    assert out.shape == linear.apply_mxfp4_fake(x, w, ws, bias).shape == (2, 20, 272)
    q, s = ops().per_token_group_quant_mxfp4(x.reshape(-1, 512))
    qb, sb = q.view(torch.uint8).cpu(), s.view(torch.uint8).cpu()
    assert_gemm_close(out.reshape(-1, 272), _ref(qb, w, sb, ws, torch.bfloat16, bias), "apply_mxfp4", max_frac=0.03)
    q2, s2 = torch.empty_like(q), torch.empty_like(s)
    torch.ops._C.per_token_group_mxfp4_quant(x.reshape(-1, 512), q2, s2)
    assert_bit_exact(q2.view(torch.uint8), q.view(torch.uint8), "_C quantiser q")
    assert_bit_exact(s2.view(torch.uint8), s.view(torch.uint8), "_C quantiser s")
    out2, route = _run(qb, w, sb, ws, bias, torch.bfloat16, op=torch.ops._C.cutlass_scaled_mm)
    assert route == STREAM
    assert_bit_exact(out2, out.reshape(-1, 272), "_C cutlass_scaled_mm")


def test_graph_replay_of_the_slab_path():
    """The K-split call captured into a HIP graph: three replays give the eager call's bits (nothing in the slab path
    depends on a memset or on what an earlier launch left in the workspace)."""
    m, n, k = 64, 1280, 8192
    d = dev()
    g = torch.Generator().manual_seed(4)
    a = torch.randint(0, 256, (m, k // 2), generator=g, dtype=torch.uint8).to(d).view(F4)
    b = torch.randint(0, 256, (n, k // 2), generator=g, dtype=torch.uint8).to(d).view(F4).t()
    a_s = (127 + torch.randint(-6, 0, (m, k // 32), generator=g)).to(torch.uint8).to(d).view(E8)
    b_s = (127 + torch.randint(-6, 0, (n, k // 32), generator=g)).to(torch.uint8).to(d).view(E8).t()
    eager = torch.empty(m, n, dtype=torch.bfloat16, device=d)
    ops().cutlass_scaled_mm(eager, a, b, a_s, b_s, None)
    assert ops().scaled_mm_mxfp4_last_route() == STREAM | SLABS
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


def test_argument_errors_and_untouched_paths():
    d = dev()
    out = torch.empty(16, 256, dtype=torch.bfloat16, device=d)
    f4 = lambda *shape: torch.zeros(*shape, dtype=torch.uint8, device=d).view(F4)          # noqa: E731
    e8 = lambda *shape: torch.full(shape, 127, dtype=torch.uint8, device=d).view(E8)       # noqa: E731
    a, b = f4(16, 128), f4(256, 128).t()
    for mm in (ops().cutlass_scaled_mm, torch.ops._C.cutlass_scaled_mm):
        with pytest.raises(RuntimeError):                     # k % 128 != 0
            mm(out, f4(16, 160), f4(256, 160).t(), e8(16, 10), e8(256, 10).t(), None)
        with pytest.raises(RuntimeError):                     # a mixed dtype
            mm(out, a, torch.zeros(256, 128, dtype=torch.float8_e4m3fn, device=d).t(), e8(16, 8), e8(256, 8).t(), None)
        with pytest.raises(RuntimeError):                     # a scale shape off by one group
            mm(out, a, b, e8(16, 9), e8(256, 8).t(), None)
        with pytest.raises(RuntimeError):                     # b_scales not contiguous along the K groups
            mm(out, a, b, e8(16, 8), e8(8, 256), None)
    # afterwards a row-scaled e4m3 call gives the oracle's result as before
    from oracle import ref_ops as R
    g = torch.Generator().manual_seed(1)
    a8 = (torch.randn(33, 256, generator=g) * 2).to(torch.float8_e4m3fn)
    b8 = (torch.randn(256, 256, generator=g) * 2).to(torch.float8_e4m3fn).t()
    a_s, b_s = torch.rand(33, 1, generator=g) * 9e-3 + 1e-3, torch.rand(1, 256, generator=g) * 9e-3 + 1e-3
    out = torch.empty(33, 256, dtype=torch.bfloat16, device=d)
    ops().cutlass_scaled_mm(out, a8.to(d), b8.t().contiguous().to(d).t(), a_s.to(d), b_s.to(d), None)
    assert_gemm_close(out, R.scaled_mm_fp8(a8, b8, a_s, b_s, torch.bfloat16), "row-scaled call", max_frac=0.03)
